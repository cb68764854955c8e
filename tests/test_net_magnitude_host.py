"""What tests/test_gpu_net_magnitude.py stands on, shown without a GPU.

  - oracle.net.scale_tower / scale_head leave forward_logits bit-identical in fp32 and in fp64 at every rung and board size;
  - the criterion of the GPU test (finite, err < fpl.bound(err_ref)) catches an f16 feature path without a range check: a numpy
    model of the 9x9 head phase's split-operand policy features (np.float16 pieces, the low piece x 2048, sums in float64, as
    tools/head_epilogue_precision.py restates the epilogue) passes below 65 504, is non-finite above, and passes again with the guard;
  - no chosen (case, position) lies within 2^-10 of a limit: the placement the GPU test predicts the fallback counters from is
    the kernels' as long as their activations are fp32-class (relative error about 1e-6, against a band of 1e-3 and rungs 2x apart);
  - spike_channel, spike_last_row and spike_point do what they say; the networks used have live heads."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import forward_precision_ladder as fpl  # noqa: E402

from oracle.net import (TOWER_LAYERS, forward_logits, layer_maxima, make_state_dict, scale_head, spike_channel,  # noqa: E402
                        spike_last_row, spike_point, spike_points, stem_output, tower_output)

SIZES = (9, 13, 19)
LADDERS = ("tower", "policy_head", "value_head")
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _base(size, which):
    return _memo(("base", size, which), lambda: make_state_dict(size, *fpl.BASES[size][which]))


def _planes(size):
    return _memo(("planes", size), lambda: fpl.plane_sets(size)["randint"])


def _families(size, only=None):
    return [f for f in fpl.GUARDS if fpl.family(f)[1] == size and (only is None or f in only)]


@pytest.mark.parametrize("size", SIZES)
def test_the_transforms_keep_the_bits_in_fp32_and_fp64(size):
    planes = _planes(size)
    for which in range(len(fpl.BASES[size])):
        base = _base(size, which)
        for dtype in (torch.float32, torch.float64):
            def forward(sd):
                with torch.no_grad():
                    return forward_logits({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, planes.to(dtype))
            want = forward(base)
            for ladder in LADDERS:
                for k in fpl.magnitude_rungs(ladder):
                    got = forward(fpl.magnitude_net(base, ladder, k))
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (which, dtype, ladder, k)


@pytest.mark.parametrize("size", SIZES)
def test_the_ladders_move_what_they_say_and_nothing_else(size):
    planes = _planes(size)
    base = _base(size, 0)
    m0 = layer_maxima(base, planes)
    for k in fpl.TOWER_RUNGS:
        m = layer_maxima(fpl.magnitude_net(base, "tower", k), planes)
        for key in ("stem", "layers"):
            assert np.array_equal(m[key], m0[key] * 2.0 ** k), (k, key)
        for key in ("policy_head", "value_head"):
            assert np.allclose(m[key], m0[key], rtol=1e-12), (k, key)
    for head in ("policy_head", "value_head"):
        other = "value_head" if head == "policy_head" else "policy_head"
        for k in fpl.HEAD_RUNGS:
            m = layer_maxima(scale_head(base, head, k), planes)
            assert np.array_equal(m["layers"], m0["layers"]) and np.array_equal(m[other], m0[other])
            assert np.allclose(m[head], m0[head] * 2.0 ** k, rtol=1e-12), (head, k)


# ------------------------------------------------------------------------------------------------------- the fault model
def _pieces(x):
    """The kernels' operand split: high piece f16(x), low piece f16((x - high) * 2048), as float64 arrays (Inf - Inf = NaN kept)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def head_model(sd, planes, guarded):
    """The 9x9 head phase's policy path (run_heads_x32 / run_heads_mfma): fp32 features, split into f16 pieces; the FC weights x
    2^e (their largest below 2^15) as pieces; three partial products summed in float64, the low-order ones / 2048; x 2^-e, +
    bias.  guarded: a position with a feature at or beyond kHeadRangeLimit gets the exact path's logits (the fp32 oracle's) -
    what the exact kernel behind the raised flag writes."""
    x = tower_output(sd, planes)
    with torch.no_grad():
        from oracle.net import EPS_BODY, _bn
        import torch.nn.functional as F
        feat = F.relu(_bn(F.conv2d(x, sd["policy_head.conv_layer.weight"]), sd, "policy_head.bn_layer", EPS_BODY))
        exact = forward_logits(sd, planes)[0].numpy().astype(np.float64)
    feat = feat.reshape(feat.shape[0], -1).numpy()
    w = sd["policy_head.fc_layer.weight"].numpy().astype(np.float64)
    e = 14 - int(np.floor(np.log2(np.abs(w).max())))
    wh, wl = _pieces((w * 2.0 ** e).astype(np.float32))
    fh, fl = _pieces(feat)
    with np.errstate(over="ignore", invalid="ignore"):
        acc = fh @ wh.T + (fh @ wl.T + fl @ wh.T) / 2048.0
    logits = acc * 2.0 ** -e + sd["policy_head.fc_layer.bias"].numpy().astype(np.float64)
    if guarded:
        hot = feat.max(axis=1) >= 60000.0
        logits[hot] = exact[hot]
    return logits, feat.max(axis=1)


def test_the_criterion_catches_an_unguarded_f16_feature_path():
    planes = _planes(9)
    base = _base(9, 0)
    l64, _, l32, _ = fpl.reference(base, planes)
    err_ref = float((l32 - l64).abs().max())
    first_beyond = None
    for k in (0,) + fpl.HEAD_RUNGS:
        sd = scale_head(base, "policy_head", k)
        for guarded in (False, True):
            logits, top = head_model(sd, planes, guarded)
            err = np.abs(logits - l64.numpy())
            inside = top < fpl.F16_MAX
            # a position whose features fit: the model is fp32-class, with or without the guard
            assert np.isfinite(logits[inside]).all() and (err[inside].max() if inside.any() else 0.0) < fpl.bound(err_ref), (k, guarded)
            if guarded:
                assert np.isfinite(logits).all() and err.max() < fpl.bound(err_ref), k
            elif (~inside).any():
                # Inf high piece, -Inf low piece: every logit of the position is lost, and the criterion says so
                assert not np.isfinite(logits[~inside]).any(), k
                first_beyond = first_beyond if first_beyond is not None else k
    assert first_beyond == 12                                    # 24.3 * 2^12 = 99 370: the first rung beyond 65 504


# ----------------------------------------------------------------------------------------------------------- placement
@pytest.mark.parametrize("size", SIZES)
def test_no_ladder_position_lies_inside_a_band(size):
    planes = _planes(size)
    tripped = {f: set() for f in _families(size)}
    for which in range(len(fpl.BASES[size])):
        for ladder in LADDERS:
            for k in fpl.magnitude_rungs(ladder):
                maxima = layer_maxima(fpl.magnitude_net(_base(size, which), ladder, k), planes)
                for fid in _families(size):
                    must, may = fpl.classify(maxima, fid)                     # (raises inside a band)
                    if ladder == "value_head":
                        assert not must.any() and not may.any(), (fid, k)
                    if must.any():
                        tripped[fid].add(ladder)
    for fid in _families(size):
        assert tripped[fid] == ({"tower", "policy_head"} if fpl.GUARDS[fid][2] else {"tower"}), fid
    # the ladders hold mixed launches: some positions of a policy rung are beyond the f16 range, others are not
    if size == 9:
        for k, n_must in ((12, 3), (13, 12), (14, 16)):
            must, _ = fpl.classify(layer_maxima(scale_head(_base(9, 0), "policy_head", k), planes), "9-w1d-1")
            assert int(must.sum()) == n_must, k


def test_predicted_redo_at_each_granularity():
    must = np.zeros(6, bool)
    may = np.zeros(6, bool)
    must[4], may[1] = True, True
    for fid, redone, undecided in (("9-w1d-1", [4], [1]), ("9-split16-1", [0, 1, 2, 3, 4, 5], []), ("19-pair", None, None)):
        batch = fpl.family(fid)[2]
        r, u = fpl.predicted_redo(must[:batch], may[:batch], fid)
        if redone is not None:
            assert list(np.flatnonzero(r)) == redone and list(np.flatnonzero(u)) == undecided, fid
    idx = np.arange(300) % 16
    m16 = np.zeros(16, bool)
    m16[5] = True
    r, u = fpl.predicted_redo(m16[idx], np.zeros(300, bool), "9-w1d-3")
    hot_groups = {i // 3 for i in range(300) if i % 16 == 5}
    assert int(r.sum()) == 3 * len(hot_groups) and all(r[3 * g:3 * g + 3].all() for g in hot_groups) and not u.any()


@pytest.mark.parametrize("size", SIZES)
def test_spike_channel_heats_one_layer_in_one_channel(size):
    planes = _planes(size)
    base = _base(size, 0)
    heights = sorted({2.0 * fpl.GUARDS[f][0] for f in _families(size)})
    for height in heights:
        limit = height / 2.0
        for layer in range(TOWER_LAYERS):
            for c in (0, 63):
                m = layer_maxima(spike_channel(base, layer, c, height), planes)
                ch = m["layer_channels"]
                assert ch[layer, c] >= height and m["layers"][layer].min() >= limit * (1 + fpl.BAND), (layer, c)
                ch = ch.copy()
                ch[layer, c] = 0.0
                assert ch.max() < 200.0 and m["stem"].max() < 200.0, (layer, c, ch.max())       # everything else: where the base has it
                assert max(m["policy_head"].max(), m["value_head"].max()) < 200.0
                for fid in _families(size):
                    if 2.0 * fpl.GUARDS[fid][0] == height and fid not in fpl.LARGE:
                        assert fpl.classify(m, fid)[0].all(), (fid, layer, c)


@pytest.mark.parametrize("size", SIZES)
def test_spike_last_row_heats_the_last_layer_on_the_last_board_row_only(size):
    planes = _planes(size)
    base = _base(size, 0)
    for height in sorted({2.0 * fpl.GUARDS[f][0] for f in _families(size)}):
        limit = height / 2.0
        sd = spike_last_row(base, fpl.LAST_ROW_CHANNEL, height)
        m = layer_maxima(sd, planes)
        assert max(m["stem"].max(), m["layers"][:-1].max()) < limit * (1 - fpl.BAND)          # (layer 10 carries the constant limit / 2)
        assert max(m["policy_head"].max(), m["value_head"].max()) < 200.0
        x = tower_output(sd, planes)
        assert float(x[:, fpl.LAST_ROW_CHANNEL, size - 1, :].min()) >= limit * (1 + fpl.BAND)
        x[:, fpl.LAST_ROW_CHANNEL, size - 1, :] = 0.0
        assert float(x.max()) < 200.0
        for fid in _families(size):
            if 2.0 * fpl.GUARDS[fid][0] == height:
                must, may = fpl.classify(m, fid)
                assert must.all() and not may.any(), fid


@pytest.mark.parametrize("size", SIZES)
def test_spike_point_heats_the_stem_in_a_3x3_neighbourhood_of_one_board(size):
    planes = _planes(size)
    base = _base(size, 0)
    cold = stem_output(base, planes)
    for height in sorted({2.0 * fpl.GUARDS[f][0] for f in _families(size)}):
        for y, x in spike_points(size):
            spiked = spike_point(base, planes, 0, (y, x), height)
            assert int((spiked != planes).sum()) == 1 and torch.equal(spiked[1:], planes[1:])
            hot = stem_output(base, spiked)
            changed = (hot != cold).nonzero()
            assert len(changed) and (changed[:, 0] == 0).all()
            assert ((changed[:, 2] - y).abs() <= 1).all() and ((changed[:, 3] - x).abs() <= 1).all()
            assert float(hot[0].max()) >= height / 2.0 * (1 + fpl.BAND) and float(cold.max()) < 200.0
            both = torch.cat([planes, spiked[:1]])
            maxima = layer_maxima(base, both)
            for fid in _families(size):
                if 2.0 * fpl.GUARDS[fid][0] == height:
                    must, may = fpl.classify(maxima, fid)
                    assert must[16] and not must[:16].any() and not may.any(), (fid, y, x)


# ------------------------------------------------------------------------------------------------------------ liveness
def test_the_networks_have_live_heads_on_the_planes():
    for size in SIZES:
        for which in range(len(fpl.BASES[size])):
            m = layer_maxima(_base(size, which), _planes(size))
            assert (m["policy_channels"] > 1.0).all() and (m["policy_head"] > 1.0).all(), (size, which)
            if (size, which) == (19, 0):
                # the 19x19 network of the precision suite: every value feature is zero behind the ReLU - its value FC is held
                # on its biases alone, which is why the value-head ladder and test_gpu_net_precision take a second 19x19 base
                assert m["value_head"].max() == 0.0
            else:
                assert (m["value_head"] > 1.0).all(), (size, which)
