"""Oracle featurise + DualNet forward vs reference-generated fixtures."""
import numpy as np
import pytest
import torch

from oracle.board import GoBoard
from oracle.feature import generate_input_planes
from oracle.net import OracleNet, make_state_dict, forward_logits
from tests.helpers import load_npz, oracle_replay


@pytest.mark.parametrize("size", [9, 13, 19])
def test_feature_planes(size):
    fix = load_npz(f"feat_s{size}.npz")
    brd = load_npz(f"board_s{size}.npz")
    specials = fix["special_seqs"]
    for i in range(len(fix["game"])):
        g, ply, color = int(fix["game"][i]), int(fix["ply"][i]), int(fix["color"][i])
        if g >= 0:
            board = oracle_replay(size, brd[f"g{g}_move"], brd[f"g{g}_color"], ply)
        else:
            seq = [int(v) for v in specials[-g - 1] if v != -9]
            board = GoBoard(size)
            c = 1
            for mv in seq:
                board.put_stone(mv, c)
                c = 3 - c
        planes = generate_input_planes(board, color)
        assert planes.dtype == np.float32 and planes.shape == (6, size, size)
        assert np.array_equal(planes, fix["planes"][i].astype(np.float32)), i


@pytest.mark.parametrize("size", [9, 13, 19])
def test_dualnet_forward(size):
    fix = load_npz(f"net_s{size}.npz")
    for seed in (0, 7):
        sd = make_state_dict(size, seed, float(fix[f"w{seed}_gain"]))
        x = torch.from_numpy(fix[f"w{seed}_planes"].astype(np.float32))
        net = OracleNet(sd)
        logits, vlogits = forward_logits(sd, x)
        # same ops, same library, but possibly another CPU: allow a few ulp of fp32
        assert np.allclose(logits.numpy(), fix[f"w{seed}_logits"], atol=2e-5, rtol=1e-5)
        assert np.allclose(vlogits.numpy(), fix[f"w{seed}_vlogits"], atol=2e-5, rtol=1e-5)
        pol, val = net.inference(x)
        assert np.abs(pol.numpy() - fix[f"w{seed}_policy"]).max() < 1e-6
        assert np.abs(val.numpy() - fix[f"w{seed}_value"]).max() < 1e-6
        lg, val2 = net.inference_with_policy_logits(x)
        assert torch.equal(lg, logits) and torch.equal(val2, val)
        # fp32 forward vs the reference's own fp64 forward: error budget for the HIP path
        assert np.abs(logits.numpy() - fix[f"w{seed}_logits64"]).max() < 1e-4


@pytest.mark.parametrize("size", [9, 13, 19])
def test_rescale_mid_channels_keeps_every_bit(size):
    """rescale_mid_channels spreads the mid-block channel scales over 2^S and must leave the function alone: powers of two
    commute with every fp32 / fp64 rounding of the forward, so the logits of the rescaled network are the base network's bit
    for bit - which is what lets the GPU precision tests hold one fp64 reference and one fp32 error against every rung."""
    from oracle.net import rescale_mid_channels
    base = make_state_dict(size, 7, 1.5)
    rs = np.random.RandomState(4)
    x = torch.from_numpy(rs.randint(0, 2, size=(4, 6, size, size)).astype(np.float32))
    for dtype in (torch.float32, torch.float64):
        cast = lambda sd: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        want = forward_logits(cast(base), x.to(dtype))
        for S in (0, 8, 12, 16, 20, 24):
            sd = rescale_mid_channels(base, S, seed=1)
            assert sd is not base and torch.equal(base["blocks.0.conv2.weight"], make_state_dict(size, 7, 1.5)["blocks.0.conv2.weight"])
            if S > 0:                                              # the spread is there, and exactly 2^S
                ratio = sd["blocks.2.bn1.weight"].double() / base["blocks.2.bn1.weight"].double()
                assert float(ratio.max() / ratio.min()) == 2.0 ** S
                assert float(ratio[0]) == 2.0 ** -S and float(ratio[1]) == 1.0
                assert torch.equal(sd["blocks.2.conv2.weight"][:, 0], base["blocks.2.conv2.weight"][:, 0] * 2.0 ** S)
            else:
                assert all(torch.equal(sd[k], base[k]) for k in base)
            got = forward_logits(cast(sd), x.to(dtype))
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (dtype, S)
