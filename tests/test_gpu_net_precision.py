"""Every forward kernel family against the oracle's fp64 forward at logit level (needs a GPU).

The contract (README; tests/test_gpu_net.py): logits as close to an fp64 forward as the reference's own fp32 path,
err_hip < 4 * err_ref + 1e-6.  Held here for every kernel a launch can reach (tools/forward_precision_ladder.py: FAMILIES,
each asserted by tg_net_kernel_name), on planes that are NOT exact in f16 (the stem's low activation piece is zero on the
randint(-1, 2) planes of the rest of the suite), on recorded feature planes, and on networks whose mid-block channel scales
spread over 2^S inside a layer (oracle.net.rescale_mid_channels: the same function bit for bit, so one fp64 reference and
one err_ref serve every rung).  The API hands out no value logits: the value softmax is held to 1e-4 against the fp64 one.

The fp64 reference of a (size, plane set) is computed once, on 16 positions; larger launches tile them, the first copy is
compared, err_ref is taken over the same positions."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import forward_precision_ladder as fpl  # noqa: E402

_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _base(size):
    from oracle.net import make_state_dict
    return _memo(("sd", size), lambda: make_state_dict(size, 7, 1.5))


def _planes(size, name):
    return _memo(("planes", size), lambda: fpl.plane_sets(size))[name]


def _ref(size, name):
    return _memo(("ref", size, name), lambda: fpl.reference(_base(size), _planes(size, name)))


def _net(size, S):
    """The base network (S = None) or its rescaling at spread 2^S, built once."""
    from oracle.net import rescale_mid_channels
    return _memo(("net", size, S), lambda: fpl.make_net(
        size, _base(size) if S is None else rescale_mid_channels(_base(size), S, seed=1)))


def _check_against_fp64(fid, net, plane_set, what):
    _, size, _, _, _, exact, want_name = fpl.family(fid)
    logits, value, name = fpl.run_family(net, fid, _planes(size, plane_set))
    assert name == want_name, what
    err_hip, err_ref, err_val = fpl.errors(logits, value, _ref(size, plane_set))
    print(f"{fid} {what}: err_hip {err_hip:.3e} err_ref {err_ref:.3e} bound {fpl.bound(err_ref):.3e} value {err_val:.2e}")
    assert err_hip < fpl.bound(err_ref), (what, err_hip, err_ref)
    assert err_val < fpl.VALUE_TOL, (what, err_val)
    if not exact:
        assert net.range_fallbacks() == 0 and net.band_timeouts() == 0, what


@pytest.mark.parametrize("plane_set", ["randint", "uniform", "thirds"])
@pytest.mark.parametrize("fid", fpl.FAMILY_IDS)
def test_every_family_against_fp64_on_f16_exact_and_inexact_planes(fid, plane_set):
    """(a) randint(-1, 2) planes, planes uniform in [0, 1) and planes from {0, 1/3, 2/3, 1}: the last two give the stem a
    non-zero low activation piece."""
    _check_against_fp64(fid, _net(fpl.family(fid)[1], None), plane_set, plane_set)


@pytest.mark.parametrize("fid", fpl.FAMILY_IDS)
def test_every_family_against_fp64_on_recorded_feature_planes(fid):
    """(b) the first 16 positions of tests/golden/feat_s{9,13,19}.npz: sparse 0/1 planes and a constant one."""
    _check_against_fp64(fid, _net(fpl.family(fid)[1], None), "feat", "feat")


@pytest.mark.parametrize("plane_set", ["randint", "uniform", "thirds", "feat"])
@pytest.mark.parametrize("fid", [f for f in fpl.FAMILY_IDS if fpl.family(f)[1] == 19])
def test_every_19x19_family_against_fp64_with_a_live_value_head(fid, plane_set):
    """(a), (b) again on make_state_dict(19, 3, 1.4): the value features of the base network above are all zero behind the ReLU
    on these planes (tests/test_net_magnitude_host.py), so its value FC is held on its biases alone.  This one's reach 28."""
    from oracle.net import make_state_dict
    sd = _memo(("sd-live", 19), lambda: make_state_dict(19, *fpl.BASES[19][1]))
    net = _memo(("net-live", 19), lambda: fpl.make_net(19, sd))
    ref = _memo(("ref-live", 19, plane_set), lambda: fpl.reference(sd, _planes(19, plane_set)))
    _, _, _, _, _, exact, want_name = fpl.family(fid)
    logits, value, name = fpl.run_family(net, fid, _planes(19, plane_set))
    assert name == want_name
    err_hip, err_ref, err_val = fpl.errors(logits, value, ref)
    print(f"{fid} {plane_set}: err_hip {err_hip:.3e} err_ref {err_ref:.3e} bound {fpl.bound(err_ref):.3e} value {err_val:.2e}")
    assert err_hip < fpl.bound(err_ref), (err_hip, err_ref)
    assert err_val < fpl.VALUE_TOL, err_val
    if not exact:
        assert net.range_fallbacks() == 0 and net.band_timeouts() == 0


def _exact_base(size, batch):
    """The base network on the exact kernel that a network the load-time guard keeps off the f16 towers runs on (the Winograd
    kernel; at 13x13 the default one), in a launch of the same size: (logits, value softmax, kernel name)."""
    return _memo(("exact", size, batch), lambda: fpl.run(_net(size, None), batch, None if size == 13 else "wino", False,
                                                         _planes(size, "randint")))


@pytest.mark.parametrize("fid", fpl.FAMILY_IDS)
def test_spread_ladder(fid):
    """(c) rescale_mid_channels(base, S, seed=1) for S in 0, 8, 12, 16, 20 on the randint planes.

    Exact-fp32 kernels (wino, direct, the 13x13 default): logits and value equal the base network's bit for bit at every rung -
    folding gamma / sqrt(var + eps) in double and rounding commutes with a power of two, the Winograd weight transform is
    computed in double from the scaled weights, and every later fp32 operation commutes as well.

    f16 families: the criterion up to 2^12; beyond it no silent breach - the criterion still holds, or the load-time guard
    (tg_net_channel_spread against the limits in csrc/net_forward.hip) has moved the network to an exact kernel, which
    tg_net_kernel_name and tg_net_executed_flops_per_position say, and whose result then equals the base network's on that
    kernel bit for bit.  The f16 range guard stays silent throughout: the exponents only go down."""
    import ctypes
    _, size, batch, algo, _, exact, want_name = fpl.family(fid)
    planes, ref = _planes(size, "randint"), _ref(size, "randint")
    for S in fpl.RUNGS:
        net = _net(size, S)
        logits, value, name = fpl.run_family(net, fid, planes)
        err_hip, err_ref, err_val = fpl.errors(logits, value, ref)
        print(f"{fid} S={S}: {name}: err_hip {err_hip:.3e} err_ref {err_ref:.3e} bound {fpl.bound(err_ref):.3e} value {err_val:.2e}")
        if exact or fpl.is_exact_kernel(name):
            if exact:
                assert name == want_name, S
                want = _memo(("exact-own", fid), lambda: fpl.run_family(_net(size, None), fid, planes))
            else:
                assert S > 12, (S, name)                         # up to 2^12 the f16 kernels are within their contract: they run
                want = _exact_base(size, batch)
                assert name == want[2], (S, name, want[2])
                dtype = ctypes.c_char_p()
                with fpl.environment(TG_FWD_ALGO=algo):
                    net._lib.tg_net_executed_flops_per_position(net.handle, batch, None, ctypes.byref(dtype))
                assert dtype.value == b"f32", (S, dtype.value)
            assert torch.equal(logits, want[0]) and torch.equal(value, want[1]), (S, name)
        else:
            if S == 0:
                assert name == want_name
            assert err_hip < fpl.bound(err_ref), (S, name, err_hip, err_ref)
            assert err_val < fpl.VALUE_TOL, (S, name, err_val)
        assert net.range_fallbacks() == 0 and net.band_timeouts() == 0, S


def test_channel_spread_of_ordinary_networks_and_of_the_rungs():
    """tg_net_channel_spread, what the load-time guard looks at.  make_state_dict networks: every input channel of a layer has
    576 weights uniform in one interval (the one-axis Winograd image folds batch-norm scales of [0.75, 1.25] / sqrt([0.5, 1.5]) =
    at most 2.4x apart into them and halves some sums), so their largest weights lie within 4x of each other - orders of magnitude
    below any limit, those networks keep their kernels and bits.  A rung 2^S: channel 0 is scaled by 2^-S and channel 1 by 1, so
    the spread is 2^S times the ratio of two such maxima - within [2^S / 4, 2^S * 4]."""
    from oracle.net import make_state_dict
    lib = _net(9, None)._lib
    for size, seed, gain in ((9, 0, 1.0), (9, 11, 1.4), (13, 3, 1.4), (19, 6, 1.3)):
        net = fpl.make_net(size, make_state_dict(size, seed, gain))
        for image in (0, 1):
            assert 1.0 <= lib.tg_net_channel_spread(net.handle, image) < 4.0, (size, seed, image)
    for S in fpl.RUNGS[1:]:
        for image in (0, 1):
            spread = lib.tg_net_channel_spread(_net(9, S).handle, image)
            assert 2.0 ** (S - 2) <= spread <= 2.0 ** (S + 2), (S, image, spread)
