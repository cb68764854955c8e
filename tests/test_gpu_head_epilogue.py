"""The policy and value softmax of every forward kernel family (want_logits = 0) against an fp64 softmax of the same launch's
logits, relative to each probability's own size (needs a GPU).  Cases, reference, criterion and fault models:
tools/head_epilogue_precision.py; what the criterion catches: tests/test_head_epilogue_host.py.

(a) crafted logits: networks with zero FC weights put out their FC biases as logits in every family; every board of every
    launch is held, and every output entry must be written into NaN-prefilled buffers.
(b) real networks: every algorithm at launch sizes on both sides of its kernel switches, probabilities against the fp64 softmax
    of the logits of the same launch, on all boards - boards of a workgroup have different maxima and sums here.
(c) policy probabilities are the same bits whatever the launch size, also across the two 19x19 heads kernels."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import forward_precision_ladder as fpl  # noqa: E402
import head_epilogue_precision as hep  # noqa: E402

_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _planes(size, name):
    return _memo(("planes", size), lambda: fpl.plane_sets(size))[name]


def _tiled(planes, batch):
    reps = (batch + planes.shape[0] - 1) // planes.shape[0]
    return planes.repeat(reps, 1, 1, 1)[:batch].contiguous()


# ------------------------------------------------------------------------------------------------------ (a) crafted logits
@pytest.mark.parametrize("size,case", [(s, name) for s in hep.SIZES for name in hep.case_names(s)])
def test_crafted_logits_every_family_every_board(size, case):
    """One network per (size, case), every family of the size on it: the logits are the biases, policy and value probabilities
    of every board are within the criterion, and forward_device writes every entry of NaN-prefilled outputs (the same
    criterion, which no NaN passes)."""
    _, row, vrow = next(c for c in hep.cases(size) if c[0] == case)
    net = fpl.make_net(size, hep.zero_fc_state(size, row, vrow))
    planes = _planes(size, "uniform")
    missed = []
    for launch in hep.launches(size):
        fid, batch, algo, shared, exact, want_name = launch
        rec = hep.measure_case(net, size, launch, planes, row, vrow)
        print(f"{fid} {case}: policy err_hip {rec['policy_err_hip']:.3e} err_ref32 {rec['policy_err_ref32']:.3e} bound "
              f"{rec['policy_bound']:.3e}; value err_hip {rec['value_err_hip']:.3e} err_ref32 {rec['value_err_ref32']:.3e}")
        assert rec["kernel"] == want_name, fid
        assert rec["logits_equal_bias"], fid
        if not exact:
            assert rec["range_fallbacks"] == 0 and rec["band_timeouts"] == 0, fid
        pol, val = hep.forward_prefilled(net, _tiled(planes, batch), algo, shared)
        written = hep.within(pol.numpy(), np.broadcast_to(row, pol.shape)) and hep.within(val.numpy(), np.broadcast_to(vrow, val.shape))
        if not (rec["policy_ok"] and rec["value_ok"] and written):
            missed.append((fid, rec["policy_ok"], rec["value_ok"], written, rec["policy_err_hip"], rec["value_err_hip"]))
    assert not missed, missed


# ------------------------------------------------------------------------------------------------------ (b) real networks
REAL_BATCHES = {9: (1, 5, 301), 13: (5,), 19: (3, 100, 513, 529)}


def _algorithms():
    """(size, algo, shared, exact, batches): each distinct (algorithm, shared device) of fpl.FAMILIES once, at the launch sizes
    of its board size; the shared-device family stays at its own batch."""
    seen = {}
    for fid, size, batch, algo, shared, exact, _ in fpl.FAMILIES:
        seen.setdefault((size, algo, shared), (exact, (batch,) if shared else REAL_BATCHES[size]))
    return [(size, algo, shared, exact, batches) for (size, algo, shared), (exact, batches) in seen.items()]


def _real_net(size):
    from oracle.net import make_state_dict
    return _memo(("net", size), lambda: fpl.make_net(size, make_state_dict(size, 7, 1.5)))     # test_gpu_net_precision's base


@pytest.mark.parametrize("plane_set", ["uniform", "feat"])
@pytest.mark.parametrize("size,algo,shared,exact,batches", _algorithms(),
                         ids=[f"{s}-{a or 'default'}{'-shared' if sh else ''}" for s, a, sh, _, _ in _algorithms()])
def test_real_network_probabilities_against_fp64_softmax_of_the_same_launch(size, algo, shared, exact, batches, plane_set):
    """All boards of every launch: inference() against the fp64 softmax of inference_with_policy_logits() of the same
    positions.  A board that used another board's maximum or 1 / sum is off by the ratio of two rows' sums."""
    net = _real_net(size)
    for batch in batches:
        x = _tiled(_planes(size, plane_set), batch)
        logits, val_l, name = hep.forward(net, x, algo, shared, True)
        pol, val, _ = hep.forward(net, x, algo, shared, False)
        assert exact == fpl.is_exact_kernel(name), (batch, name)
        verdict = hep.judge(pol.numpy(), logits.numpy())
        err, ref = hep.worst(verdict)
        print(f"{size} {algo} {plane_set} batch {batch} {name}: err_hip {err:.3e} err_ref32 {ref:.3e} bound {hep.bound(ref):.3e}")
        assert verdict["ok"].all(), (batch, name, err, ref, np.flatnonzero(~verdict["ok"])[:8].tolist())
        assert torch.equal(val, val_l), (batch, name)
        vsum = val.double().sum(dim=1)
        assert float((vsum - 1.0).abs().max()) <= 4 * hep.ULP, (batch, name)
        if not exact:
            assert net.range_fallbacks() == 0 and net.band_timeouts() == 0, (batch, name)


# --------------------------------------------------------------------------------- (c) launch-shape invariance of probabilities
@pytest.mark.parametrize("size,algo,boards,ranges", [
    (9, "w1d", 1000, ((0, 100), (7, 8), (997, 1000))),
    (9, "split16", 1000, ((0, 100), (7, 8), (997, 1000))),
    (19, None, 600, ((0, 40), (77, 78), (300, 500), (597, 600))),
], ids=["9-w1d", "9-split16", "19-default"])
def test_probabilities_do_not_depend_on_the_launch_size(size, algo, boards, ranges):
    """tests/test_gpu_net.py pins logits and value across launch shapes; the search takes probabilities.  A position's policy
    and value probabilities are the same bits alone, in a small launch and inside the big one - at 19x19 across
    dualnet_heads19_fin_kernel (up to 512 boards) and dualnet_heads19_kernel<16> (above), whose sums split the same way."""
    from oracle.net import make_state_dict
    net = _memo(("shape-net", size), lambda: fpl.make_net(size, make_state_dict(size, 5, 1.5)))
    x = torch.from_numpy(np.random.RandomState(3).randint(-1, 2, size=(boards, 6, size, size)).astype(np.float32))
    big = hep.forward(net, x, algo, False, False)
    for lo, hi in ranges:
        part = hep.forward(net, x[lo:hi].contiguous(), algo, False, False)
        assert torch.equal(part[0], big[0][lo:hi]) and torch.equal(part[1], big[1][lo:hi]), (algo, lo, hi)
    assert net.range_fallbacks() == 0 and net.band_timeouts() == 0
