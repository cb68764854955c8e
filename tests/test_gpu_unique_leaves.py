"""UNIQUE leaf layout (tg_search_select_gumbel / tg_search_backup with slots_per_tree -1, MCTSTree(unique_leaves=True),
selfplay_shard(unique_leaves=True)): each distinct leaf of a sequential-halving phase is evaluated once instead of once per
descent, and nothing else changes - the reference's trees (whole-tree digests), moves, improved policies, stream positions
and SGF bytes, in every kernel path and self-play scheme - while the network is given exactly the positions the host
predicts (mcts/sequential_halving.py unique_plane_caps).  Needs a GPU."""
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import load_json, load_npz, unhex
from tests.test_gpu_search import check_root, product_replay

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def gumbel_cases(size):
    return [r for r in load_json(f"trees_s{size}.json") if r["kind"] == "gumbel"]


def predicted_forward(n_root, visits, pipelined=None):
    """1 (root) + the plane ranges of the phases of one move of one board."""
    from tamago_amd.mcts.sequential_halving import get_candidates_and_visit_pairs, unique_plane_caps
    total = 1
    for w, c in get_candidates_and_visit_pairs(min(n_root, 16), visits).items():
        total += unique_plane_caps([w], [c], pipelined=pipelined)[0]
    return total


def run_tree_case(size, rec):
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.tree import MCTSTree
    from tamago_amd.mcts.time_manager import TimeManager, TimeControl
    brd = load_npz(f"board_s{size}.npz")
    board = product_replay(size, brd["g0_move"], brd["g0_color"], rec["ply"], rec["superko"])
    net = StubNet(salt=100 + rec["seed"])
    tree = MCTSTree(net, tree_size=160 if rec["visits"] <= 100 else 2048, unique_leaves=True)
    np.random.seed(rec["seed"])
    mv = tree.generate_move_with_sequential_halving(
        board, rec["color"], TimeManager(TimeControl.CONSTANT_PLAYOUT, rec["visits"]), True)
    check_root(tree, mv, rec)                                        # (incl. the sha256 over the whole tree)
    root = tree.get_root()
    assert np.array_equal(root.noise, unhex(rec["noise"]))
    assert np.array_equal(root.calculate_improved_policy(), unhex(rec["improved"]))
    assert float(np.random.random_sample()) == float.fromhex(rec["rng_after"])
    return tree, net


@pytest.mark.parametrize("size", [9, 13, 19])
def test_unique_trees_equal_the_reference_trees(size):
    for rec in gumbel_cases(size):
        tree, net = run_tree_case(size, rec)
        # the evaluator was called once per batch, with the predicted plane counts - fewer than the reference's leaves
        want = predicted_forward(rec["n"], rec["visits"])
        assert sum(net.calls) == tree._engine.forward_positions == want, rec
        assert len(net.calls) == len(rec["batches"]) and want <= sum(rec["batches"])
        if rec["visits"] >= 100 and rec["n"] >= 16:
            assert want < sum(rec["batches"])                      # (a 16-wide root: some phase makes more than 17 descents)


def test_unique_trees_one_by_one_through_the_job_ring(monkeypatch):
    monkeypatch.setenv("TG_GUMBEL_ONE_BY_ONE", "1")
    for rec in gumbel_cases(9):
        tree, net = run_tree_case(9, rec)
        assert sum(net.calls) == predicted_forward(rec["n"], rec["visits"])


@pytest.mark.parametrize("variant", ["serial", "one-by-one"])
def test_unique_trees_in_a_fresh_process_per_kernel_path(variant):
    """TG_SELECT_SERIAL=1 (read once per process): the one-wavefront kernel - plane ranges = the leaves, nothing saved, same
    trees; TG_GUMBEL_ONE_BY_ONE=1 from the start of a process: every entry through the job ring."""
    env = dict(os.environ, TG_DEBUG_KNOBS="1")
    for k in ("TG_SELECT_SERIAL", "TG_GUMBEL_WORKERS", "TG_GUMBEL_ONE_BY_ONE"):
        env.pop(k, None)
    env["TG_SELECT_SERIAL" if variant == "serial" else "TG_GUMBEL_ONE_BY_ONE"] = "1"
    res = subprocess.run([sys.executable, os.path.join(HERE, "_unique_trees.py")], env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().splitlines()
    cases = gumbel_cases(9)
    assert len(lines) == len(cases)
    for line, rec in zip(lines, cases):
        digest, mv, improved, rng_after, forwarded = line.split()
        assert digest == rec["digest"] and int(mv) == rec["move"] and rng_after == rec["rng_after"], rec
        assert improved == hashlib.sha256(unhex(rec["improved"]).tobytes()).hexdigest()[:16]
        want = rec["visits"] + 1 if variant == "serial" else predicted_forward(rec["n"], rec["visits"])
        assert int(forwarded) == want


# ---- games -----------------------------------------------------------------------------------------------------------------

def _flag(k):
    """never_resign as the reference worker draws it after random.seed(k) (worker.py:39,53)."""
    random.seed(k)
    random.choice([k])
    return random.randint(1, 10) == 1


def _read(d, i):
    return open(os.path.join(str(d), f"{i}.sgf"), encoding="utf-8").read()


@pytest.mark.parametrize("key", ["1,16", "2,16", "3,50"])
def test_unique_worker_reproduces_the_reference_games(key, tmp_path, monkeypatch):
    from oracle.stubnet import StubNet
    import tamago_amd.nn.utility as util
    from tamago_amd.selfplay.worker import selfplay_worker
    k, visits = (int(v) for v in key.split(","))
    monkeypatch.setattr(util, "load_network", lambda **kw: StubNet(salt=200 + k))
    random.seed(k)
    selfplay_worker(str(tmp_path), "/nonexistent/model.bin", [k], 9, visits, True, unique_leaves=True)
    assert _read(tmp_path, k) == load_json("selfplay_games.json")[key]


def test_unique_shard_reproduces_the_400_simulation_reference_games(tmp_path):
    from oracle.stubnet import StubNet
    from tamago_amd.selfplay.worker import selfplay_shard
    golden = load_json("selfplay_games_400.json")
    idx = [11, 12, 13, 14]
    stats = selfplay_shard(str(tmp_path), StubNet(salt=300), idx, 9, 400, boards=4,
                           never_resign_flags=[_flag(k) for k in idx], groups=1, unique_leaves=True)
    assert stats["games"] == 4 and stats["leaf_evals"] == stats["moves"] * 401
    for k in idx:
        assert _read(tmp_path, k) == golden[f"{k},400"], k
    assert stats["forward_positions"] <= schedule_bound(400) * stats["leaf_evals"]


def schedule_bound(visits):
    """(phases x E + 1) / (visits + 1): the most a move can forward of what it queues, from the schedule."""
    from tamago_amd.mcts.sequential_halving import UNIQUE_E, get_candidates_and_visit_pairs
    phases = max(len(get_candidates_and_visit_pairs(base, visits)) for base in range(1, 17))
    return (phases * UNIQUE_E + 1) / (visits + 1)


@pytest.fixture(scope="module")
def device_net():
    import torch
    from tamago_amd.nn.network.dual_net import DualNet
    torch.manual_seed(21)
    return DualNet(torch.device("cuda:0"), 9)


SCHEMES = ["chained", "round-trip", "lanes", "observer"]


def play(net, out, boards, visits, scheme, unique, monkeypatch):
    """One game per board.  Returns (stats, predicted): `predicted` = the forwarded positions the host expects from the
    schedules an observer saw (None without one)."""
    from tamago_amd.mcts.sequential_halving import unique_plane_caps
    from tamago_amd.selfplay.worker import selfplay_shard
    monkeypatch.delenv("TG_SP_CHAIN", raising=False)
    if scheme == "round-trip":
        monkeypatch.setenv("TG_SP_CHAIN", "0")
    idx = list(range(1, boards + 1))
    flags = [i % 3 == 0 for i in idx]
    seen = {"queued": 0, "planes": 0}

    def observer(engine, ev):
        if ev.kind == 0 and ev.phase >= 0:
            nc = [ev.num_considered[t] for t in range(ev.trees)]
            mc = [ev.max_count[t] for t in range(ev.trees)]
            caps = unique_plane_caps(nc, mc) if unique else [a * b for a, b in zip(nc, mc)]
            assert ev.positions == sum(caps)
            seen["queued"] += sum(a * b for a, b in zip(nc, mc))
            seen["planes"] += sum(caps)

    os.makedirs(out)
    stats = selfplay_shard(out, net, idx, 9, visits, boards=boards, never_resign_flags=flags, groups=1,
                           lanes=2 if scheme == "lanes" else 1, observer=observer if scheme == "observer" else None,
                           unique_leaves=unique)
    predicted = stats["leaf_evals"] - seen["queued"] + seen["planes"] if scheme == "observer" else None
    return stats, predicted


@pytest.mark.parametrize("boards,visits", [(16, 100), (16, 400), (64, 100), (64, 400)])
def test_device_games_are_the_same_files_with_fewer_positions_forwarded(boards, visits, device_net, tmp_path, monkeypatch):
    off, _ = play(device_net, str(tmp_path / "off"), boards, visits, "chained", False, monkeypatch)
    assert off["games"] == boards and off["range_fallbacks"] == 0
    assert off["forward_positions"] == off["leaf_evals"] == off["moves"] * (visits + 1)
    forwarded = set()
    for scheme in SCHEMES:
        out = str(tmp_path / scheme)
        on, predicted = play(device_net, out, boards, visits, scheme, True, monkeypatch)
        assert on["range_fallbacks"] == 0, scheme
        assert {k: on[k] for k in ("games", "moves", "leaf_evals")} == {k: off[k] for k in ("games", "moves", "leaf_evals")}, scheme
        for i in range(1, boards + 1):
            assert open(os.path.join(out, f"{i}.sgf"), "rb").read() == \
                open(os.path.join(str(tmp_path / "off"), f"{i}.sgf"), "rb").read(), (scheme, i)
        if predicted is not None:
            assert on["forward_positions"] == predicted
        forwarded.add(on["forward_positions"])
        if visits == 400:
            assert on["forward_positions"] <= schedule_bound(visits) * on["leaf_evals"], scheme
    assert len(forwarded) == 1                       # (the same games: every scheme forwards the observer run's prediction)
    assert forwarded.pop() < off["forward_positions"]


# ---- the buffers ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("one_by_one", [False, True])
def test_the_forward_pass_never_reads_uninitialised_planes(one_by_one, device_net, monkeypatch):
    """Ragged phases - an idle tree, a tree with ONE distinct leaf in a range of 17, ordinary ones - into a planes buffer full
    of NaN: every plane the forward pass covers has been written, its outputs are finite."""
    import torch
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import SearchEngine, DeviceEvaluator
    from tamago_amd.mcts.sequential_halving import unique_plane_caps
    if one_by_one:
        monkeypatch.setenv("TG_GUMBEL_ONE_BY_ONE", "1")
    else:
        monkeypatch.delenv("TG_GUMBEL_ONE_BY_ONE", raising=False)
    outputs = []

    class Keeping(DeviceEvaluator):
        def __call__(self, planes, want_logits):
            seen_planes.append(planes.clone())
            out = super().__call__(planes, want_logits)
            outputs.append(out)
            return out

    seen_planes = []
    eng = SearchEngine(9, 4, 160, 48, Keeping(device_net))
    boards = [GoBoard(9) for _ in range(4)]
    boards[1].put_stone(boards[1].onboard_pos[40], 1)
    boards[3].put_stone(boards[3].onboard_pos[10], 1)
    for t, b in enumerate(boards):
        eng.set_root(t, b, 1 if b.moves % 2 == 0 else 2, np.random.RandomState(10 + t).get_state())
    eng.root_eval(use_logit=True)
    eng.set_gumbel_noise()
    for nc, mc in (([8, 0, 1, 4], [3, 0, 40, 5]), ([4, 8, 0, 2], [5, 3, 0, 9])):
        eng.planes.fill_(float("nan"))
        eng.gumbel_phase(nc, mc, unique=True)
        caps = unique_plane_caps(nc, mc)
        assert list(eng.unique_caps) == caps
        planes = seen_planes[-1]
        assert planes.shape[0] == sum(caps)
        assert not torch.isnan(planes).any()
        assert torch.isnan(eng.planes[sum(caps):]).all()                      # ... and nothing was written past the ranges
        policy, value = outputs[-1]
        assert torch.isfinite(policy).all() and torch.isfinite(value).all()
        # tree 2 of the first phase has one root candidate: 40 descents, one leaf - the rest of its range repeats it
        if nc[2] == 1:
            lo = caps[0] + caps[1]
            assert all(torch.equal(planes[lo], planes[lo + i]) for i in range(1, caps[2]))
    stats = eng.read_root_stats()                                              # (surfaces sticky device errors)
    assert stats["children_visits"][0].sum() == 8 * 3 + 4 * 5 and stats["children_visits"][2].sum() == 40
    eng.close()


def test_unique_layout_equals_packed_on_ragged_phases():
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import SearchEngine, HostEvaluator

    def run(unique):
        eng = SearchEngine(9, 4, 160, 48, HostEvaluator(StubNet(3), torch.device("cuda:0")))
        boards = [GoBoard(9) for _ in range(4)]
        boards[1].put_stone(boards[1].onboard_pos[40], 1)
        boards[3].put_stone(boards[3].onboard_pos[10], 1)
        for t, b in enumerate(boards):
            eng.set_root(t, b, 1 if b.moves % 2 == 0 else 2, np.random.RandomState(10 + t).get_state())
        eng.root_eval(use_logit=True)
        eng.set_gumbel_noise()
        eng.gumbel_phase([8, 0, 1, 4], [3, 0, 40, 5], unique=unique)
        eng.gumbel_phase([4, 8, 0, 2], [5, 3, 0, 9], unique=unique)
        stats, nodes, batches = eng.read_root_stats(), eng.num_nodes(), list(eng.evaluator.batches)
        eng.close()
        return stats, nodes, batches

    a, na, ba = run(True)
    b, nb, bb = run(False)
    assert np.array_equal(na, nb)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert ba == [4, 17 + 0 + 17 + 17, 17 + 17 + 0 + 17] and bb == [4, 24 + 40 + 20, 20 + 24 + 18]


def test_misuse_is_refused():
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.lib import TamagoHipError
    from tamago_amd.mcts.engine import SearchEngine, HostEvaluator
    TG_ERR_ARG = -1
    eng = SearchEngine(9, 2, 160, 48, HostEvaluator(StubNet(3), torch.device("cuda:0")))
    for t in range(2):
        eng.set_root(t, GoBoard(9), 1, np.random.RandomState(5 + t).get_state())
    eng.root_eval(use_logit=True)
    eng.set_gumbel_noise()
    eng.gumbel_phase([8, 8], [2, 2])                                           # a PACKED selection + backup
    policy = torch.zeros((2 * 48, eng.A), dtype=torch.float32, device=eng.device)
    value = torch.zeros((2 * 48, 3), dtype=torch.float32, device=eng.device)
    # a unique backup needs a unique selection in front of it
    assert eng.lib.tg_search_backup(eng.handle, policy.data_ptr(), value.data_ptr(), -1, 1, eng._stream()) == TG_ERR_ARG
    assert b"unique" in eng.lib.tg_last_error()
    # a phase whose ranges do not fit the buffers (T * batch_size planes; 49 descents in 48 slots)
    nc, mc = np.array([7, 7], dtype=np.int32), np.array([7, 7], dtype=np.int32)
    assert eng.lib.tg_search_select_gumbel(eng.handle, nc.ctypes.data, mc.ctypes.data, -1, eng.planes.data_ptr(),
                                           eng._stream()) == TG_ERR_ARG
    with pytest.raises(TamagoHipError):
        eng.gumbel_phase([7, 7], [7, 7], unique=True)
    # ... and the tree is as the packed phase left it
    assert eng.read_root_stats()["children_visits"].sum() == 2 * 16
    eng.close()
