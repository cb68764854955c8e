"""Every forward kernel family against the oracle's fp64 forward as activations LEAVE the f16 range (needs a GPU).

tests/test_gpu_net_precision.py holds the kernels where exponents go down; here they go up, one step at a time, past the f16
range guard's limits (tools/forward_precision_ladder.py: GUARDS) and past 65 504 itself:

  tower ladder        oracle.net.scale_tower(base, k): stem and layer outputs x 2^k, the same function bit for bit
  head ladders        oracle.net.scale_head(base, head, k): one head's features x 2^k, the tower untouched, the same function
  one layer, channel  oracle.net.spike_channel: ONE layer output is hot, in one channel (its own reference)
  one point           oracle.net.spike_point: one plane entry of ONE board makes the stem hot in a 3x3 neighbourhood
  one row             oracle.net.spike_last_row: the last layer is hot on the last board row only

The contract of an f16 family at every rung and position: finite outputs, err_hip < 4 * err_ref + 1e-6 on the logits, the value
softmax within 1e-4, the family's own kernel name; a position the placement (fpl.classify, from oracle.net.layer_maxima in
fp64) calls hot carries the bits of the exact Winograd kernel, and the fallback counters say exactly what the placement
predicts at the granularity of the kernel's bitmap (fpl.predicted_redo) - nothing is redone where everything is cold.  A
policy feature between 16 000 and 65 504 may go either way.  tests/test_net_magnitude_host.py shows on the CPU that no chosen
case lies within 2^-10 of a limit and that the criterion catches an unguarded f16 feature path.

Exact-fp32 families: logits and value of every rung equal the base network's bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import forward_precision_ladder as fpl  # noqa: E402

F16 = tuple(fpl.GUARDS)
SMALL = tuple(f for f in F16 if f not in fpl.LARGE)
EXACT = tuple(f[0] for f in fpl.FAMILIES if f[5])
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _base(size, which):
    from oracle.net import make_state_dict
    return _memo(("base", size, which), lambda: make_state_dict(size, *fpl.BASES[size][which]))


def _planes(size):
    return _memo(("planes", size), lambda: fpl.plane_sets(size)["randint"])


class Case:
    """A network on a set of distinct positions: state dict, planes, the fp64 / fp32 reference, the fp64 per-position maxima, the
    device network - each computed once.  `same_as`: a case of the same function bit for bit (its reference serves)."""

    def __init__(self, key, size, make_sd, planes, same_as=None):
        self.key, self.size, self._make_sd, self.planes, self.same_as = key, size, make_sd, planes, same_as

    @property
    def sd(self):
        return _memo(("sd",) + self.key, self._make_sd)

    @property
    def ref(self):
        if self.same_as is not None:
            return self.same_as.ref
        return _memo(("ref",) + self.key, lambda: fpl.reference(self.sd, self.planes))

    @property
    def maxima(self):
        from oracle.net import layer_maxima
        return _memo(("maxima",) + self.key, lambda: layer_maxima(self.sd, self.planes))

    @property
    def net(self):
        return _memo(("net",) + self.key[:-1], lambda: fpl.make_net(self.size, self.sd))     # (the last key entry names the planes)

    def exact(self):
        """The exact Winograd kernel on this network and these positions (logits, value softmax).  9x9, 19x19: TG_FWD_ALGO=wino.
        13x13 has that kernel only behind the guard: the split launch of the same network with its tower x 2^16 - the same
        function bit for bit for an exact kernel, every board beyond every limit, so every board is redone (asserted)."""
        def make():
            n = self.planes.shape[0]
            if self.size != 13:
                logits, value, name = fpl.run(self.net, n, "wino", False, self.planes)
                assert name.startswith("dualnet_fwd_wino8_kernel"), name
                return logits, value
            from oracle.net import scale_tower
            net = fpl.make_net(13, scale_tower(self.sd, 16))
            logits, value, _ = fpl.run(net, n, "split16", False, self.planes)
            assert net.range_fallbacks() == 1 and net.range_fallback_positions() == n
            return logits, value
        return _memo(("exact",) + self.key, make)


def _ladder_case(size, which, ladder, k):
    base = Case(("base", size, which, "randint"), size, lambda: _base(size, which), _planes(size))
    if ladder is None:
        return base
    return Case((ladder, size, which, k, "randint"), size, lambda: fpl.magnitude_net(_base(size, which), ladder, k), _planes(size),
                same_as=base)


def _hold(fid, case, idx, what):
    """One launch of the family, launch position i carrying position idx[i] of the case: the whole contract."""
    _, size, batch, _, _, _, want_name = fpl.family(fid)
    idx = np.asarray(idx)
    assert len(idx) == batch
    must, may = fpl.classify(case.maxima, fid)
    redone, undecided = fpl.predicted_redo(must[idx], may[idx], fid)
    logits, value, name, launches, positions = fpl.run_launch(case.net, fid, case.planes[idx].contiguous())
    l64, v64, l32, _ = case.ref
    err_ref = float((l32 - l64).abs().max())
    err_hip = float((logits.double() - l64[idx]).abs().max())
    err_val = float((value.double() - v64[idx]).abs().max())
    print(f"{fid} {what}: err_hip {err_hip:.3e} err_ref {err_ref:.3e} bound {fpl.bound(err_ref):.3e} value {err_val:.2e}; "
          f"redone {launches} launches / {positions} positions, predicted {int(redone.sum())} (+ up to {int(undecided.sum())})")
    assert name == want_name, what
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(value).all()), what
    assert err_hip < fpl.bound(err_ref), (what, err_hip, err_ref)
    assert err_val < fpl.VALUE_TOL, (what, err_val)
    assert int(redone.sum()) <= positions <= int((redone | undecided).sum()), (what, positions)
    assert launches == (1 if positions else 0), (what, launches, positions)
    if redone.any():
        exact = case.exact()
        hot = torch.from_numpy(redone)
        at = torch.from_numpy(idx[redone])
        assert torch.equal(logits[hot], exact[0][at]) and torch.equal(value[hot], exact[1][at]), what
    assert case.net.band_timeouts() == 0, what


def _tiled(fid, n=fpl.POSITIONS):
    return np.arange(fpl.family(fid)[2]) % n


def _first_rung(fid, size, which, ladder, hot):
    for k in fpl.magnitude_rungs(ladder):
        if hot(_ladder_case(size, which, ladder, k)):
            return k
    raise AssertionError((fid, ladder))


def _rungs(fid, which, ladder):
    """Every rung for the small launches; the large ones take the first rung that trips - the family's tower guard, or, on a head
    ladder, the first with a feature beyond the f16 range."""
    size = fpl.family(fid)[1]
    if fid not in fpl.LARGE:
        return fpl.magnitude_rungs(ladder)
    if ladder == "tower":
        return (_first_rung(fid, size, which, ladder, lambda c: fpl.classify(c.maxima, fid)[0].any()),)
    return (_first_rung(fid, size, which, ladder, lambda c: c.maxima[ladder].max() >= fpl.F16_MAX),)


def _exact_ladder(fid, which, ladder):
    size = fpl.family(fid)[1]
    planes = _planes(size)
    want = fpl.run_family(_ladder_case(size, which, None, 0).net, fid, planes)
    for k in fpl.magnitude_rungs(ladder):
        net = _ladder_case(size, which, ladder, k).net
        before = net.range_fallbacks()                                # (the f16 families' tests run on the same network)
        got = fpl.run_family(net, fid, planes)
        assert got[2] == fpl.family(fid)[6] == want[2], k
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (fid, ladder, k)
        assert net.range_fallbacks() == before, k


def _value_bases(size):
    """The base networks whose value head is alive on the planes (tests/test_net_magnitude_host.py: the 19x19 network of the
    precision suite has none)."""
    return [w for w in range(len(fpl.BASES[size])) if (size, w) != (19, 0)]


@pytest.mark.parametrize("fid", F16 + EXACT)
def test_tower_ladder(fid):
    """scale_tower, k in 0, 4, 6, 7, 8, 9, 10, 12, 16: the layer maxima cross 16 000, 32 752, 60 000 and 65 504 one layer at a time
    (the deepest layers first); at 19x19 on both base networks."""
    size = fpl.family(fid)[1]
    for which in range(len(fpl.BASES[size])):
        if fid in EXACT:
            _exact_ladder(fid, which, "tower")
            continue
        for k in _rungs(fid, which, "tower"):
            _hold(fid, _ladder_case(size, which, "tower", k), _tiled(fid), f"base {which} tower x 2^{k}")


@pytest.mark.parametrize("fid", F16 + EXACT)
def test_policy_head_ladder(fid):
    """scale_head("policy_head", k), k in 4, 8, 12, 13, 14, 16, 20: the tower stays where it is (largest activation about 100), the
    policy features pass 65 504 position by position.  The 9x9 f16 kernels write them as f16 pieces: such a position is redone."""
    size = fpl.family(fid)[1]
    if fid in EXACT:
        return _exact_ladder(fid, 0, "policy_head")
    for k in _rungs(fid, 0, "policy_head"):
        _hold(fid, _ladder_case(size, 0, "policy_head", k), _tiled(fid), f"policy features x 2^{k}")


@pytest.mark.parametrize("fid", F16 + EXACT)
def test_value_head_ladder(fid):
    """scale_head("value_head", k), the same rungs: the value features are fp32 in every family - nothing is redone."""
    size = fpl.family(fid)[1]
    for which in _value_bases(size):
        if fid in EXACT:
            _exact_ladder(fid, which, "value_head")
            continue
        for k in _rungs(fid, which, "value_head"):
            case = _ladder_case(size, which, "value_head", k)
            assert not any(a.any() for a in fpl.classify(case.maxima, fid))
            _hold(fid, case, _tiled(fid), f"base {which} value features x 2^{k}")


@pytest.mark.parametrize("layer", range(12))
@pytest.mark.parametrize("fid", SMALL)
def test_one_layer_one_channel(fid, layer):
    """spike_channel: one tower layer's output, in channel 0 and in channel 63, at twice the family's limit; every other layer
    output, every other channel and both heads are where the base network has them (the host test shows it)."""
    from oracle.net import spike_channel
    size, height = fpl.family(fid)[1], 2.0 * fpl.GUARDS[fid][0]
    for c in (0, 63):
        case = Case(("spike", size, layer, c, height, "randint"), size,
                    lambda: spike_channel(_base(size, 0), layer, c, height), _planes(size))
        assert fpl.classify(case.maxima, fid)[0].all()
        _hold(fid, case, _tiled(fid), f"layer {layer} channel {c} at {height}")


@pytest.mark.parametrize("fid", F16)
def test_only_the_last_board_row_of_the_last_layer(fid):
    """spike_last_row: the tower's last layer passes the limit on the last board row alone, every other layer output and every
    other row stays cold - the one-axis kernels finish the tower's last rows apart from the layer loop, with a range check of
    their own."""
    from oracle.net import spike_last_row
    size, height = fpl.family(fid)[1], 2.0 * fpl.GUARDS[fid][0]
    case = Case(("lastrow", size, height, "randint"), size, lambda: spike_last_row(_base(size, 0), fpl.LAST_ROW_CHANNEL, height),
                _planes(size))
    assert fpl.classify(case.maxima, fid)[0].all()
    _hold(fid, case, _tiled(fid), f"last row of the last layer at {height}")


def _point_case(size, point, height):
    """The 16 positions and, as position 16, position 0 with the point spike."""
    from oracle.net import spike_point

    def planes():
        base = _planes(size)
        return torch.cat([base, spike_point(_base(size, 0), base, 0, point, height)[:1]])
    return Case(("base", size, 0, ("point", point, height)), size, lambda: _base(size, 0), _memo(("pp", size, point, height), planes))


@pytest.mark.parametrize("fid", F16)
def test_one_point(fid):
    """spike_point at the three corners, the centre and the middle of the last row: one hot board in a launch of cold ones - as
    the launch's first and last position and as the first and last board of a three-board group.  The large launches take the
    centre as their last position."""
    from oracle.net import spike_points
    _, size, batch = fpl.family(fid)[:3]
    height = 2.0 * fpl.GUARDS[fid][0]
    points = spike_points(size)
    for point in (points[3:4] if fid in fpl.LARGE else points):
        case = _point_case(size, point, height)
        must, may = fpl.classify(case.maxima, fid)
        assert must[16] and not must[:16].any() and not may.any()
        places = (batch - 1,) if fid in fpl.LARGE else sorted({0, batch - 1, 3 * ((batch - 1) // 3), 2})
        for at in places:
            idx = _tiled(fid)
            idx[at] = 16
            _hold(fid, case, idx, f"point {point} on launch position {at}")
