"""The 9x9 one-axis Winograd forward kernel (TG_FWD_ALGO=w1d) outside its tower: input staging, im2col, stem, the tower's
first / last row, heads (needs a GPU).

Those phases may be re-staged and re-addressed but never re-ordered arithmetically: tests/golden/w1d_bits_s9.npz
(tools/gen_golden_w1d_bits.py, generated with the library of the commit BEFORE the phases were reworked) pins every output
bit for planes that are not f16-exact (the low pieces of the operand split carry information) and for a position that is
non-zero on the corner and edge cells only (every 3x3 tap that crosses the border of the board).  Batches 1, 3, 4, 7 (the
one-board kernel, one to seven workgroups), 260 (the three-board kernel, 87 workgroups of one group each, the last of two
boards) and 1300 (the three-board kernel, 434 groups on 256 workgroups: 178 of them are a workgroup's SECOND group, handed
out by the ticket counter, staged over what the first group left in LDS from planes prefetched behind its tower; the last
group is ragged with ONE board, the border position; no second launch for the tail).  Which kernel a batch runs is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.helpers import load_npz

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden_w1d_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4                                   # tests/test_gpu_net.py: policy / value against the oracle, random planes


@pytest.fixture(scope="module")
def runs():
    """batch -> (planes, probabilities, logits, value) of the kernel under test; computed once, read by every test"""
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    old = os.environ.get("TG_FWD_ALGO")
    os.environ["TG_FWD_ALGO"] = "w1d"
    try:
        net = DualNet(torch.device("cuda:0"), 9)
        net.load_state_dict(make_state_dict(9, gen.SEED, gen.GAIN))
        out = {}
        for b in gen.BATCHES:
            x = gen.planes(b)
            t = torch.from_numpy(x)
            pol, val = net.inference(t)
            lg, val2 = net.inference_with_policy_logits(t)
            out[b] = (x, pol.numpy(), lg.numpy(), val.numpy(), val2.numpy())
        from tamago_amd import lib as tl
        out["kernel"] = {b: tl.load().tg_net_kernel_name(net.handle, b).decode() for b in gen.BATCHES}
        # the positions of the large launches on their own and as a group of three
        parts = {}
        for big, cuts in ((260, ((0, 1), (0, 3), (100, 1), (100, 3), (257, 1), (257, 3), (258, 1), (259, 1))),
                          (1300, ((0, 1), (0, 3), (900, 1), (900, 3), (1296, 3), (1298, 1), (1299, 1)))):
            x = torch.from_numpy(out[big][0])
            for lo, n in cuts:
                parts[(big, lo, n)] = tuple(a.numpy() for a in net.inference(x[lo:lo + n])) + \
                    (net.inference_with_policy_logits(x[lo:lo + n])[0].numpy(),)
        out["parts"] = parts
        out["fallbacks"] = net.range_fallbacks()
        yield out
    finally:
        if old is None:
            del os.environ["TG_FWD_ALGO"]
        else:
            os.environ["TG_FWD_ALGO"] = old


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("b", gen.BATCHES)
def test_every_output_bit_is_the_parents(runs, b):
    fix = load_npz("w1d_bits_s9.npz")
    assert int(fix["seed"]) == gen.SEED and float(fix["gain"]) == gen.GAIN and int(fix["plane_seed"]) == gen.PLANE_SEED
    x, pol, lg, val, val2 = runs[b]
    assert gen.sha(x) == str(fix[f"b{b}_planes_sha256"]), "the planes are not the ones the fixture was generated from"
    # (the inputs test what they are meant to: low pieces non-zero, the border position zero inside)
    assert np.count_nonzero(x.astype(np.float16).astype(np.float32) != x) > np.count_nonzero(x) // 2
    assert not x[b - 1, :, 1:8, 1:8].any() and np.count_nonzero(x[b - 1]) == 6 * 32
    assert runs["kernel"][b] == gen.KERNEL[b]         # (the path the batch is here for: see the generator's docstring)
    for key, a in (("policy", pol), ("logits", lg), ("value", val)):
        if b in gen.HASHED:                           # (arrays too large to commit: their SHA-256)
            assert gen.sha(np.ascontiguousarray(a, dtype=np.float32)) == str(fix[f"b{b}_{key}_sha256"]), key
        else:
            assert np.array_equal(_bits(a), _bits(fix[f"b{b}_{key}"])), key
    assert np.array_equal(_bits(val2), _bits(val))


def test_same_inputs_against_the_oracle(runs):
    """The fixture cannot hide behind itself: the outputs it pins are the oracle's within the tolerance."""
    from oracle.net import OracleNet, make_state_dict
    ora = OracleNet(make_state_dict(9, gen.SEED, gen.GAIN))
    for b in gen.BATCHES:
        x, pol, lg, val, _ = runs[b]
        rp, rv = ora.inference(torch.from_numpy(x))
        rl, _ = ora.inference_with_policy_logits(torch.from_numpy(x))
        assert np.abs(pol - rp.numpy()).max() < TOL, b
        assert np.abs(val - rv.numpy()).max() < TOL, b
        assert np.abs(lg - rl.numpy()).max() < TOL * max(1.0, float(rl.abs().max())), b
    assert runs["fallbacks"] == 0                     # the split kernel itself computed them, not the exact fallback


def test_a_position_does_not_depend_on_its_launch(runs):
    """Position i of a launch of 260 (one group per workgroup) and of 1300 (second groups, a ragged group of one board) is
    the same bits as in a launch of 1 and of 3 (the one-board kernel)."""
    for (big, lo, n), (p, v, l) in runs["parts"].items():
        _, pol, lg, val, _ = runs[big]
        assert np.array_equal(_bits(p), _bits(pol[lo:lo + n])), (big, lo, n)
        assert np.array_equal(_bits(v), _bits(val[lo:lo + n])), (big, lo, n)
        assert np.array_equal(_bits(l), _bits(lg[lo:lo + n])), (big, lo, n)


def _butterfly(v):
    """the kernel's wave reduction: lane i adds lane i ^ o for o = 32, 16, 8, 4, 2, 1, in float32"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v


def test_logits_and_probabilities_are_one_computation(runs):
    """want_logits 0 / 1: the kernel derives both from the same l0, l1.  The value is the same bits either way (asserted with
    the pin); the probabilities are the kernel's softmax of the logits, replayed here operation by operation in float32:
    lane i holds logits i and i + 64 (-inf from 82 on), m = their maximum over the wave, e = expf(l - m) (0 from 82 on),
    sum = e0 + e1 reduced by the xor butterfly 32 .. 1, inv = 1 / sum, p = e * inv.  Everything but expf is a correctly rounded
    IEEE operation that numpy repeats bit for bit.  The device's expf is within 1 ulp of exp; the host's value here (exp in
    fp64, rounded) is the nearest float, so the two are at most one float apart.  Rounded +, 1 / x and * are monotone, so
    pushing every e one float down (up) through the same operations bounds p from below (above): the test asserts that
    interval (a few ulp wide)."""
    one = np.float32(1.0)
    for b in gen.BATCHES:
        _, pol, lg, _, _ = runs[b]
        n = lg.shape[0]
        l = np.full((n, 128), -np.inf, dtype=np.float32)
        l[:, :82] = lg
        m = l.max(axis=1, keepdims=True)
        d = l - m                                                    # float32, as the kernel's l - m
        e = np.exp(d.astype(np.float64)).astype(np.float32)
        e[:, 82:] = 0.0
        lo = np.maximum(np.nextafter(e, np.float32(-np.inf)), np.float32(0.0))
        hi = np.nextafter(e, np.float32(np.inf))
        lo[:, 82:] = hi[:, 82:] = 0.0
        s_lo, s_mid, s_hi = (_butterfly(v[:, :64] + v[:, 64:]) for v in (lo, e, hi))
        assert s_lo.dtype == np.float32
        p_lo = (lo * np.tile(one / s_hi, 2))[:, :82]
        p_hi = (hi * np.tile(one / s_lo, 2))[:, :82]
        p_mid = (e * np.tile(one / s_mid, 2))[:, :82]
        width = float(((p_hi - p_lo) / np.maximum(p_mid, np.float32(1e-30))).max())
        print(f"batch {b}: {np.count_nonzero(_bits(pol) == _bits(p_mid))} of {pol.size} probabilities are the host replay's bits, "
              f"largest relative interval {width:.3g}")
        assert (p_lo <= pol).all() and (pol <= p_hi).all(), b
        assert (pol[np.arange(n), lg.argmax(axis=1)] == pol.max(axis=1)).all(), b
