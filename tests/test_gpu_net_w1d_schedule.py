"""The rider placement of the three-board 9x9 tower (dualnet_fwd_w1d_kernel<3>) against the one-board kernel, whose
schedule is another one (needs a GPU).

A rider in the wrong slice can break a store-to-read pair ACROSS waves - a cell read in front of the store of its row, a V
slot rewritten under its last reader - without touching the arithmetic, and such a break need not show on every run.  So
the same positions go through launches of the three-board kernel and, in launches of at most one position per compute
unit, through the one-board kernel; policy, value and logits must be the same bits in both `want_logits` modes, and
sixteen repeats of a three-board launch must all be the first one's bits.  Planes are seeded uniform values that are not
f16-exact (both operand pieces carry information), weights and distribution those of tests/test_gpu_net_w1d_phases.py.

Launch sizes, C = the device's compute-unit count:
  3 (C + 1)  one more group than workgroups.  The host's ragged-tail rule (plan_forward: a remainder of at most C positions
             beyond whole rounds goes to a second launch of one-board workgroups) sends the last three positions to the
             one-board kernel: every workgroup of the three-board launch runs one full group.
  3 C + 1    likewise, the tail is one position.
  4 C + 4 (+ 0 .. 2, so that it is 1 mod 3)
             the remainder exceeds C: ONE three-board launch, workgroups take a second group from the ticket counter over
             the LDS their first group left, and the last group holds one board.
Which kernels a size runs is asserted through tg_net_kernel_name."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, GAIN, PLANE_SEED = 13, 1.4, 9421
REPEATS = 16


def _sizes(cus):
    ticketed = 4 * cus + 4
    ticketed += (1 - ticketed) % 3
    return {"one_more_group": 3 * (cus + 1), "last_group_one_board": 3 * cus + 1, "ticketed": ticketed}


@pytest.fixture(scope="module")
def runs():
    """The positions once through the one-board kernel (the reference: shared, never modified) and through each three-board
    launch, REPEATS times for two of them; everything is computed here once, the tests only compare."""
    import os
    from oracle.net import make_state_dict
    from tamago_amd import lib as tl
    from tamago_amd.nn.network.dual_net import DualNet
    old = os.environ.get("TG_FWD_ALGO")
    os.environ["TG_FWD_ALGO"] = "w1d"
    try:
        net = DualNet(torch.device("cuda:0"), 9)
        net.load_state_dict(make_state_dict(9, SEED, GAIN))
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        sizes = _sizes(cus)
        n = max(sizes.values())
        x = (np.random.RandomState(PLANE_SEED).uniform(-1.0, 1.0, size=(n, 6, 9, 9)) * 1.2345).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        lib = tl.load()
        name = lambda b: lib.tg_net_kernel_name(net.handle, b).decode()
        out = {"x": x, "cus": cus, "sizes": sizes, "names": {k: name(b) for k, b in sizes.items()}, "small_name": name(cus)}
        ref = {}
        for logits in (False, True):
            parts = [net.forward_device(xd[lo:lo + cus].contiguous(), want_logits=logits) for lo in range(0, n, cus)]
            ref[logits] = (torch.cat([p for p, _ in parts]).cpu().numpy(), torch.cat([v for _, v in parts]).cpu().numpy())
        out["ref"] = ref
        big = {}
        for key, b in sizes.items():
            xb = xd[:b].contiguous()
            for logits in (False, True):
                reps = REPEATS if key != "last_group_one_board" else 1
                res = [net.forward_device(xb, want_logits=logits) for _ in range(reps)]
                torch.cuda.synchronize()
                big[(key, logits)] = [(p.cpu().numpy(), v.cpu().numpy()) for p, v in res]
        out["big"] = big
        out["fallbacks"] = net.range_fallbacks()
        yield out
    finally:
        if old is None:
            del os.environ["TG_FWD_ALGO"]
        else:
            os.environ["TG_FWD_ALGO"] = old


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_launches_are_the_ones_meant(runs):
    x = runs["x"]
    assert np.count_nonzero(x.astype(np.float16).astype(np.float32) != x) > x.size // 2      # low pieces carry information
    assert runs["small_name"] == "dualnet_fwd_w1d_kernel<1>"
    for key in ("one_more_group", "last_group_one_board"):
        nm = runs["names"][key]
        assert "ragged tail" in nm and "<3>" in nm and "<1>" in nm, (key, nm)
    assert runs["names"]["ticketed"] == "dualnet_fwd_w1d_kernel<3>"
    b, cus = runs["sizes"]["ticketed"], runs["cus"]
    assert b % 3 == 1 and (b + 2) // 3 > cus and b % (3 * cus) > cus                        # second groups, one launch, a last group of one board
    assert runs["fallbacks"] == 0


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("key", ["one_more_group", "last_group_one_board", "ticketed"])
def test_three_board_launch_equals_one_board_launches(runs, key, logits):
    b = runs["sizes"][key]
    rp, rv = runs["ref"][logits]
    p, v = runs["big"][(key, logits)][0]
    assert p.shape == (b, 82) and v.shape == (b, 3)
    bad = np.flatnonzero((_bits(p) != _bits(rp[:b])).any(axis=1) | (_bits(v) != _bits(rv[:b])).any(axis=1))
    assert bad.size == 0, (key, logits, bad[:16].tolist(), bad.size)
    assert runs["fallbacks"] == 0


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("key", ["one_more_group", "ticketed"])
def test_repeats_of_a_launch_are_the_same_bits(runs, key, logits):
    res = runs["big"][(key, logits)]
    assert len(res) == REPEATS
    p0, v0 = res[0]
    for i, (p, v) in enumerate(res[1:], 1):
        assert np.array_equal(_bits(p), _bits(p0)) and np.array_equal(_bits(v), _bits(v0)), (key, logits, i)
