"""Reanalysis on the GPU (tamago_amd/mcts/reanalyse.py, tg_search_read_improved_policy): the read-out kernel against the
oracle's improved policy at every board size, the lock-step path against the single-tree path, the reanalysed training
chunks against the plain ones, and a generation of tools/rl_loop.py with reanalysis."""
import glob
import os
import random
import sys

import numpy as np
import pytest
import torch

from tests import _reanalyse_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(size, seed=11):
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), size)
    net.load_state_dict(make_state_dict(size, seed, 1.4))
    return net


@pytest.fixture(scope="module")
def net9():
    return _net(9)


def _searched(net, positions, visits, seeds, **kw):
    """One lock-step search over all positions: (rows [n][A] float32 on the host, the root views)."""
    from tamago_amd.mcts.reanalyse import searched_chunks
    out = []
    for engine, lo, hi in searched_chunks(net, positions, visits, seeds, **kw):
        rows = engine.read_improved_policy().cpu().numpy()
        stats = engine.read_root_stats()
        out += [(rows[k], engine.root_view(stats, k)) for k in range(hi - lo)]
    return out


@pytest.mark.parametrize("visits", [16, 50])
def test_read_out_9x9(net9, visits):
    """tg_search_read_improved_policy after searches of 16 and 50 simulations, each row against the oracle's
    calculate_improved_policy on the root read back with read_root_stats (rc.assert_row_within_bound)."""
    from tamago_amd.board.constant import PASS
    cases = rc.cases9()
    assert cases["after_pass"][0].prev_move(1) == PASS and cases["after_pass"][0].moves > 2
    got = dict(zip(cases, _searched(net9, list(cases.values()), visits, [40 + k for k in range(len(cases))])))
    for name, (row, root) in got.items():
        assert root.node_visits == visits, name
        rc.assert_row_within_bound(row, root, 9, f"9x9 {name} {visits}")
    assert got["empty"][1].num_children == 82                        # one full lane pass and a tail of 18
    assert 30 < got["midgame"][1].num_children < 82
    assert 1 < got["late"][1].num_children < 16                      # a short schedule
    assert got["pass_only"][1].num_children == 1 and got["pass_only"][1].action[0] == PASS
    assert got["pass_only"][0][81] == np.float32(1.0)
    # unvisited children are completed by the mixed value: their slots hold more than the filler
    empty_row, empty_root = got["empty"]
    unvisited = [i for i in range(82) if empty_root.children_visits[i] == 0]
    assert len(unvisited) >= 82 - visits
    assert np.all(empty_row[rc.slots_of(9, [empty_root.action[i] for i in unvisited])] > rc.FILL)


@pytest.mark.parametrize("size", [13, 19])
def test_read_out_on_larger_boards(size):
    """13x13: the empty board (170 children: three lane passes) and a midgame position; 19x19: the empty board (362)."""
    positions = rc.cases13() if size == 13 else {"empty": rc.played(19, [])}
    got = dict(zip(positions, _searched(_net(size, 3), list(positions.values()), 16, [7 + k for k in range(len(positions))])))
    for name, (row, root) in got.items():
        assert root.node_visits == 16, name
        rc.assert_row_within_bound(row, root, size, f"{size}x{size} {name} 16")
    assert got["empty"][1].num_children == size * size + 1


def test_an_unexpanded_root_is_refused():
    from oracle.stubnet import StubNet
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.lib import TamagoHipError
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    engine = SearchEngine(9, 2, 24, 8, HostEvaluator(StubNet(3), torch.device("cuda:0")))
    try:
        with pytest.raises(TamagoHipError, match=r"\(-1\).*tree 0: the root is not expanded"):      # a handle that never ran
            engine.read_improved_policy()
        for k in range(2):
            engine.set_root(k, GoBoard(9), 1, np.random.RandomState(k).get_state())
        with pytest.raises(TamagoHipError, match="tree 0: the root is not expanded"):               # staged, not expanded
            engine.read_improved_policy()
        engine.root_eval(use_logit=True)
        rows = engine.read_improved_policy().cpu().numpy()          # expanded and evaluated, not searched: the prior's softmax
        stats = engine.read_root_stats()
        for k in range(2):
            rc.assert_row_within_bound(rows[k], engine.root_view(stats, k), 9, f"root only, tree {k}")
        engine.set_root(1, GoBoard(9), 2, np.random.RandomState(5).get_state())
        with pytest.raises(TamagoHipError, match="tree 1: the root is not expanded"):
            engine.read_improved_policy()
    finally:
        engine.close()


@pytest.mark.parametrize("unique", [False, True])
@pytest.mark.parametrize("visits", [16, 50])
def test_lock_step_against_the_single_tree_path(net9, visits, unique):
    """Five positions, two trees per engine: chunks of 2 + 2 + 1, the last one padded with a copy.  Every root is the
    single-tree path's (the module's contract), every row is bit for bit the row the same kernel reads off that tree."""
    from tamago_amd.mcts.reanalyse import reanalyse_positions
    positions = list(rc.cases9().values())
    seeds = [300 + 7 * k for k in range(5)]
    searched = _searched(net9, positions, visits, seeds, max_trees=2, unique_leaves=unique)
    res = reanalyse_positions(net9, positions, visits, seeds=seeds, max_trees=2, unique_leaves=unique)
    assert res.range_fallbacks == 0 and res.rows.shape == (5, 82) and res.rows.is_cuda
    rows = res.rows.cpu().numpy()
    for k, ((board, color), seed) in enumerate(zip(positions, seeds)):
        tree, move, want = rc.single_tree(net9, board, color, seed, visits, unique)
        single_row = tree._engine.read_improved_policy().cpu().numpy()[0]
        row, root = searched[k]
        n = want.num_children
        assert (root.num_children, root.node_visits) == (n, want.node_visits) and want.node_visits == visits, k
        assert list(root.action[:n]) == list(want.action[:n]), k
        assert np.array_equal(root.children_visits[:n], want.children_visits[:n]), k
        assert np.array_equal(root.children_value_sum[:n].view(np.uint64), want.children_value_sum[:n].view(np.uint64)), k
        assert np.array_equal(row.view(np.uint32), single_row.view(np.uint32)), k
        assert np.array_equal(rows[k].view(np.uint32), single_row.view(np.uint32)), k
        assert (res.moves[k], res.visits[k]) == (move, visits), k
        assert res.raw_values[k] == float(want.raw_value), k
    if not unique:
        assert res.forward_positions == 3 * 2 * (1 + visits)       # three chunks of two trees: a root and `visits` leaves each


def _write_records(root):
    from tests._replay_records import random_record, sgf_text
    os.makedirs(root, exist_ok=True)
    moves = [random_record(9, n, 60 + k) for k, n in enumerate((12, 15, 10))]
    for k, m in enumerate(moves):
        with open(os.path.join(root, f"{k + 1}.sgf"), "w") as f:
            f.write(sgf_text(9, m, result=("B+1.5", "W+R", "B+R")[k], seed=k))
    return moves


def test_reanalysed_chunks(net9, tmp_path, monkeypatch):
    """iter_reanalysed_chunks against iter_reinforcement_learning_chunks from one saved global random state: planes and
    values byte for byte, the generators left in the same state, every policy row reanalyse_positions' row of that ply's
    board with that seed under that symmetry; a training step takes a chunk."""
    import tamago_amd.nn.data_generator as dg
    from tamago_amd.mcts.reanalyse import reanalyse_positions
    from tamago_amd.nn import learn
    from tamago_amd.nn.feature import symmetry_pos_table
    from oracle.net import make_state_dict
    monkeypatch.setattr(dg, "BATCH_SIZE", 8)
    monkeypatch.setattr(dg, "DATA_SET_SIZE", 16)
    kifu = str(tmp_path / "kifu")
    _write_records(kifu)
    np.random.seed(17)
    random.seed(17)
    np_state, py_state = np.random.get_state(), random.getstate()
    plain = list(dg.iter_reinforcement_learning_chunks([kifu], 9, 0))
    after = (np.random.get_state(), random.getstate())
    np.random.set_state(np_state)
    random.setstate(py_state)
    before = dict(dg.REANALYSE_STATS)
    fresh = list(dg.iter_reanalysed_chunks(net9, [kifu], 9, 8, device=0, seed=100, max_trees=5))
    got_after = (np.random.get_state(), random.getstate())
    assert got_after[1] == after[1] and got_after[0][2:] == after[0][2:] and np.array_equal(got_after[0][1], after[0][1])
    assert [int(c[0].shape[0]) for c in fresh] == [int(c[0].shape[0]) for c in plain] == [16, 8]
    for (planes, policy, value), (planes0, policy0, value0) in zip(fresh, plain):
        assert planes.dtype == planes0.dtype and torch.equal(planes, planes0)
        assert value.dtype == value0.dtype == torch.int64 and torch.equal(value, value0)
        assert policy.dtype == policy0.dtype == torch.float32 and policy.shape == policy0.shape and policy.is_cuda
        assert not torch.equal(policy, policy0)
    assert dg.REANALYSE_STATS["positions"] == before["positions"] + 24
    # the rows, from the records as the plain generator sampled them (the same random calls again)
    np.random.set_state(np_state)
    random.setstate(py_state)
    paths = glob.glob(os.path.join(kifu, "*.sgf"))
    random.shuffle(paths)
    records = [dg._rl_record(path, 9) for path in paths]
    boards = [rc.played(9, r.moves[:ply]) for r in records for ply in r.ply]
    sym = np.concatenate([r.sym for r in records])
    assert len(boards) == 24 and len(set(int(s) for s in sym)) > 1
    want = reanalyse_positions(net9, boards, 8, seeds=[100 + i for i in range(24)]).rows.cpu().numpy()
    got = torch.cat([c[1] for c in fresh]).cpu().numpy()
    table = symmetry_pos_table(9)
    for i in range(24):
        assert np.array_equal(got[i].view(np.uint32), want[i][rc.slots_of(9, table[sym[i]])].view(np.uint32)), i
    sums = got.astype(np.float64).sum(axis=1)
    assert np.all(np.abs(sums - 1.0) < 1e-5)
    # one training step on a reanalysed chunk
    hip = learn.HipTrainer(torch.device("cuda", 0), 9, 8, make_state_dict(9, 2, 1.0))
    planes, policy, value = fresh[1]
    hip.step(planes, policy, value, mode="rl")
    loss = hip.take_losses()
    assert np.isfinite(loss["loss"]) and loss["loss"] > 0 and np.isfinite(loss["policy"])


def test_two_generations_with_reanalysis(tmp_path, monkeypatch):
    """tools/rl_loop.py with reanalyse_visits: generation 1 trains on its own 8 games and on generation 0's, searched
    again by the network that plays generation 1."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rl_loop
    import tamago_amd.nn.data_generator as dg
    monkeypatch.setattr(dg, "BATCH_SIZE", 16)
    torch.manual_seed(13)
    np.random.seed(13)
    random.seed(13)
    prog = str(tmp_path)
    lines = []
    before = dict(dg.REANALYSE_STATS)
    s0, l0 = rl_loop.run_generation(prog, 0, 8, 4, 8, 16, log=lines.append, reanalyse_visits=8)
    assert len(lines) == 1 and dg.REANALYSE_STATS == before          # nothing to reanalyse in generation 0
    s1, l1 = rl_loop.run_generation(prog, 1, 8, 4, 8, 16, log=lines.append, reanalyse_visits=8)
    assert s0["games"] == s1["games"] == 8
    assert np.isfinite(l0["loss"]) and np.isfinite(l1["loss"]) and l1["loss"] > 0
    from tamago_amd.sgf.reader import SGFReader

    def samples(generation):                                          # 8 sampled plies per game (fewer in a shorter game)
        paths = glob.glob(os.path.join(prog, "archive", str(generation), "*.sgf"))
        assert len(paths) == 8
        return sum(min(8, SGFReader(path, 9).get_n_moves()) for path in paths)

    old_rows, new_rows = samples(0) // 16 * 16, samples(1) // 16 * 16
    assert old_rows > 0 and new_rows > 0
    assert len(lines) == 3 and f"reanalysed {old_rows} positions of generation 0 with 8 simulations" in lines[1]
    assert dg.REANALYSE_STATS["positions"] == before["positions"] + old_rows
    ck = torch.load(os.path.join(prog, "model", "rl-state.ckpt"), map_location="cpu")
    assert ck["num_trained_batches"] == (2 * old_rows + new_rows) // 16      # generation 0, generation 1, generation 0 again
