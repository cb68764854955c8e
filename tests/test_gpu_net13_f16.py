"""13x13 forward on the f16 matrix pipe (TG_FWD_ALGO=split16): dualnet_fwd_split_kernel<13, 1, f16x2>, f16 x 2 operand
pieces with fp32 accumulation, one board per workgroup, and the exact-fp32 Winograd kernel behind it redoing the boards whose
pass left the f16 range.  Opt-in: with the variable unset 13x13 stays on dualnet_fwd_kernel<13, 1>.

The last test (no GPU) reads the built kernel's resource notes: no scratch, registers within one wave per SIMD."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import load_npz

TOL = 1e-4
SPLIT13 = "dualnet_fwd_split_kernel<13, 1, f16x2>"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(sd):
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), 13)
    net.load_state_dict(sd)
    return net


@pytest.mark.gpu
def test_selected_by_the_switch_and_named(monkeypatch):
    from oracle.net import make_state_dict
    from tamago_amd import lib as tl
    lib = tl.load()
    monkeypatch.delenv("TG_FWD_ALGO", raising=False)
    net = _net(make_state_dict(13, 0, 1.4))
    for b in (1, 5, 300):
        assert lib.tg_net_kernel_name(net.handle, b).decode() == "dualnet_fwd_kernel<13, 1>"
    direct = lib.tg_net_executed_flops_per_position(net.handle, 300, None, None)
    monkeypatch.setenv("TG_FWD_ALGO", "split16")
    for b in (1, 5, 300):
        name = lib.tg_net_kernel_name(net.handle, b).decode()
        assert name.startswith(SPLIT13) and "dualnet_fwd_wino8_kernel<13, 1>" in name, name
    # issued MFMA work of the tile plan: (2 stem + 12 x 18) k-chunks x 4 channel tiles x 12 row tiles x 3 products x 16 384 FLOP
    assert lib.tg_net_executed_flops_per_position(net.handle, 300, None, None) == (2 + 12 * 18) * 4 * 12 * 3 * 16384.0
    assert lib.tg_net_executed_flops_per_position(net.handle, 300, None, None) != direct
    for algo in ("wino", "direct", "w1d"):                     # any other value: the exact kernel as before
        monkeypatch.setenv("TG_FWD_ALGO", algo)
        assert lib.tg_net_kernel_name(net.handle, 300).decode() == "dualnet_fwd_kernel<13, 1>"


@pytest.mark.gpu
def test_forward_vs_reference_golden(monkeypatch):
    from oracle.net import make_state_dict
    monkeypatch.setenv("TG_FWD_ALGO", "split16")
    fix = load_npz("net_s13.npz")
    for seed in (0, 7):
        net = _net(make_state_dict(13, seed, float(fix[f"w{seed}_gain"])))
        x = torch.from_numpy(fix[f"w{seed}_planes"].astype(np.float32))
        pol, val = net.inference(x)
        assert np.abs(pol.numpy() - fix[f"w{seed}_policy"]).max() < TOL
        assert np.abs(val.numpy() - fix[f"w{seed}_value"]).max() < TOL
        lg, val2 = net.inference_with_policy_logits(x)
        assert torch.equal(val, val2)
        ref = fix[f"w{seed}_logits"]
        assert np.abs(lg.numpy() - ref).max() < TOL * max(1.0, np.abs(ref).max())
        err_hip = np.abs(lg.numpy() - fix[f"w{seed}_logits64"]).max()
        err_ref = np.abs(ref - fix[f"w{seed}_logits64"]).max()
        assert err_hip < 4 * err_ref + 1e-6, (seed, err_hip, err_ref)
        assert net.range_fallbacks() == 0


@pytest.mark.gpu
def test_forward_vs_oracle_random_planes(monkeypatch):
    from oracle.net import OracleNet, make_state_dict
    monkeypatch.setenv("TG_FWD_ALGO", "split16")
    sd = make_state_dict(13, 3, 1.4)
    net, ora = _net(sd), OracleNet(sd)
    rs = np.random.RandomState(5)
    for b in (1, 5, 300, 1301):                                # below and above the CU count, ragged
        x = torch.from_numpy(rs.randint(-1, 2, size=(b, 6, 13, 13)).astype(np.float32))
        pol, val = net.inference(x)
        rp, rv = ora.inference(x)
        assert np.abs(pol.numpy() - rp.numpy()).max() < TOL, b
        assert np.abs(val.numpy() - rv.numpy()).max() < TOL, b
        pd, vd = net.forward_device(x.cuda())
        torch.cuda.synchronize()
        assert torch.equal(pd.cpu(), pol) and torch.equal(vd.cpu(), val), b
    assert net.range_fallbacks() == 0


@pytest.mark.gpu
def test_results_do_not_depend_on_the_launch_size(monkeypatch):
    from oracle.net import make_state_dict
    monkeypatch.setenv("TG_FWD_ALGO", "split16")
    net = _net(make_state_dict(13, 5, 1.5))
    x = torch.from_numpy(np.random.RandomState(3).randint(-1, 2, size=(1000, 6, 13, 13)).astype(np.float32))
    big = net.inference_with_policy_logits(x)
    for lo, hi in ((0, 100), (7, 8), (500, 756), (997, 1000)):
        part = net.inference_with_policy_logits(x[lo:hi])
        assert torch.equal(part[0], big[0][lo:hi]) and torch.equal(part[1], big[1][lo:hi]), (lo, hi)


@pytest.mark.gpu
def test_one_hot_board_costs_one_boards_redo(monkeypatch):
    """The range guard at board granularity: the hot board alone is redone by the exact-fp32 kernel, every other board keeps the
    bits of an undisturbed launch, the counters say one launch and one position, and the next launch on the stream is clean."""
    from oracle.net import OracleNet, make_state_dict
    monkeypatch.setenv("TG_FWD_ALGO", "split16")
    n, hot = 300, 137
    sd = make_state_dict(13, 9, 1.4)
    x = torch.from_numpy(np.random.RandomState(21).randint(-1, 2, size=(n, 6, 13, 13)).astype(np.float32))
    net = _net(sd)
    clean = net.inference_with_policy_logits(x)
    assert net.range_fallbacks() == 0 and net.range_fallback_positions() == 0
    xh = x.clone()
    xh[hot] *= 3.0e4                                                  # stem output ~1e5: beyond the f16 guard
    got = net.inference_with_policy_logits(xh)
    assert net.range_fallbacks() == 1 and net.range_fallback_positions() == 1
    keep = torch.ones(n, dtype=torch.bool)
    keep[hot] = False
    assert torch.equal(got[0][keep], clean[0][keep]) and torch.equal(got[1][keep], clean[1][keep])
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    # the hot board: the exact kernel's result, alone or inside the launch, within the contract of the oracle's
    one = net.inference_with_policy_logits(xh[hot:hot + 1])
    assert net.range_fallbacks() == 2 and net.range_fallback_positions() == 2
    assert torch.equal(one[0], got[0][hot:hot + 1]) and torch.equal(one[1], got[1][hot:hot + 1])
    rl, rv = OracleNet(sd).inference_with_policy_logits(xh[hot:hot + 1])
    assert np.abs(one[0].numpy() - rl.numpy()).max() < TOL * max(1.0, float(np.abs(rl.numpy()).max()))
    assert np.abs(one[1].numpy() - rv.numpy()).max() < TOL
    again = net.inference_with_policy_logits(x)
    assert torch.equal(again[0], clean[0]) and torch.equal(again[1], clean[1])
    assert net.range_fallbacks() == 2 and net.range_fallback_positions() == 2


@pytest.mark.gpu
def test_puct_search_replays_into_the_oracle_tree(monkeypatch):
    """A 13x13 PUCT search on the f16 tower, every mini-batch replayed into the oracle tree with the network's outputs
    (tests/test_gpu_end_to_end.py::_run): same leaves, same visit counts, CPU parity within 1e-4."""
    from tests.test_gpu_end_to_end import _run
    monkeypatch.setenv("TG_FWD_ALGO", "split16")
    tree, root, _ = _run(13, 800, 64, 30, seed=6)
    assert root.node_visits == 800 and int(root.children_visits.sum()) == 800


@pytest.mark.gpu
def test_selfplay_shard_equals_games_played_alone(monkeypatch, tmp_path):
    """A 3-board 13x13 shard on the f16 tower writes the same games as each game played alone: a board's forward results do not
    depend on the boards it shares a launch with."""
    from tamago_amd.nn.network.dual_net import DualNet
    from tamago_amd.selfplay.worker import selfplay_shard
    monkeypatch.setenv("TG_FWD_ALGO", "split16")
    torch.manual_seed(22)
    net = DualNet(torch.device("cuda:0"), 13)
    idx = [1, 2, 3]
    flags = [i % 2 == 0 for i in idx]
    shard, solo = tmp_path / "shard", tmp_path / "solo"
    shard.mkdir(), solo.mkdir()
    a = selfplay_shard(str(shard), net, idx, 13, 24, boards=3, never_resign_flags=flags)
    assert a["games"] == 3
    for i, f in zip(idx, flags):
        selfplay_shard(str(solo), net, [i], 13, 24, boards=1, never_resign_flags=[f])
        text = open(shard / f"{i}.sgf").read()
        assert "SZ[13]" in text and text == open(solo / f"{i}.sgf").read(), i


def test_split13_kernel_resources():
    """The built 13x13 split kernel: no scratch (spills) and at most 512 registers per lane (one wave per SIMD).  (Its LDS plan
    is dynamic: SplitCfg's static_assert keeps it within the 160 KB of a CU at compile time.)"""
    import sys
    obj = os.path.join(REPO, "build", "obj", "net_forward_split.hip.o")
    if not os.path.exists(obj):
        pytest.skip("library not built")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from isa_check import LLVM
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not found")
    from kernel_resources import resources
    ks = [k for k in resources(obj) if "dualnet_fwd_split_kernelILi13ELi1E" in k.get("name", "")]
    assert len(ks) == 1
    k = ks[0]
    assert int(k["private_segment_fixed_size"]) == 0 and int(k.get("vgpr_spill_count", 0)) == 0
    assert int(k["vgpr_count"]) <= 512                         # (the unified count: VGPRs + AGPRs)
