"""The device board rules - put_stone and gen_candidates of csrc/search.hip - on the dense positions of the rule corpus
(tests/_rule_corpus.py), against what the reference's own board found there (tests/golden/rule_corpus_s*.npz, written by
tools/gen_golden_rule_corpus.py) and against the oracle board below the roots.  Every comparison is exact: lists of
integers, bytes of cells, planes that hold only 0 and +-1.  Nothing here depends on the evaluator's numbers: the observable is
the action list of an expanded node, a pure function of the node's position."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _rule_corpus as rc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STREAM = np.random.RandomState(7).get_state()


def _engine(size, trees, superko):
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    return SearchEngine(size, trees, 8, 1, HostEvaluator(StubNet(0), torch.device("cuda:0")), check_superko=superko)


@functools.lru_cache(maxsize=None)
def _host_boards(size):
    """The host board of every entry (set_root reads its cells, scalars and hash history, not its superko flag)."""
    from tamago_amd.board.go_board import GoBoard
    boards = []
    for entry in rc.load_fixture(size).entries:
        board = GoBoard(size, 7.0, True)
        color = 1
        for pos in entry.moves:
            board.put_stone(pos, color)
            color = 3 - color
        boards.append(board)
    return boards


def _root_lists(eng):
    eng.root_eval(False)
    count, action, _ = eng.read_roots()
    return [[int(v) for v in action[t, :count[t]]] for t in range(eng.T)]


@pytest.mark.parametrize("superko", [False, True])
@pytest.mark.parametrize("size", rc.SIZES)
def test_root_candidates_of_staged_positions(size, superko):
    """set_root -> label_strings -> gen_candidates: the root action list of every corpus entry, the history-limit entries
    (GoBoard.moves = HMAX - 2 .. HMAX + 4) included, is the reference's candidate list."""
    fx = rc.load_fixture(size)
    eng = _engine(size, len(fx.entries), superko)
    for t, entry in enumerate(fx.entries):
        eng.set_root(t, _host_boards(size)[t], entry.to_move, STREAM)
    rc.check_roots(fx.entries, fx.cand[int(superko)], _root_lists(eng))
    eng.close()


@pytest.mark.parametrize("superko", [False, True])
@pytest.mark.parametrize("size", rc.SIZES)
def test_root_candidates_after_device_play(size, superko):
    """The same through tg_search_play from the empty board (put_stone on the device, ply by ply): cells at a few plies on the
    way, then cells, move counter, side to move and the root action list of every entry.  19x19 plays the records of up to
    600 plies; the history-limit entries run at 9x9 and 13x13."""
    from oracle.board import GoBoard as OracleBoard
    from tamago_amd.board.go_board import GoBoard
    fx = rc.load_fixture(size)
    keep = [i for i, e in enumerate(fx.entries) if size != 19 or len(e.moves) <= rc.PLAY_CAP_19]
    entries = [fx.entries[i] for i in keep]
    assert len(entries) >= len(fx.entries) - len(rc.HISTORY_OFFSETS)
    eng = _engine(size, len(entries), superko)
    for t in range(len(entries)):
        eng.set_root(t, GoBoard(size, 7.0, superko), 1, STREAM)
    plies = max(len(e.moves) for e in entries)
    watched = list(range(0, len(entries), 7))               # host copies of some boards for the cells on the way
    shadow = {t: OracleBoard(size, 7.0, False) for t in watched}
    check_at = {10, 45, 100, 171, 240, 333, 480, plies}
    w = size + 2
    for ply in range(plies):
        moves = np.array([e.moves[ply] if ply < len(e.moves) else -1 for e in entries], dtype=np.int32)
        eng.play(moves)
        for t in watched:
            if moves[t] >= 0:
                shadow[t].put_stone(int(moves[t]), 1 + ply % 2)
        if ply + 1 in check_at:
            cells, n_moves, to_move = eng.read_positions()
            for t in watched:
                assert bytes(cells[t]) == bytes(shadow[t].board), (entries[t].name, ply + 1)
                assert n_moves[t] == shadow[t].moves
    cells, n_moves, to_move = eng.read_positions()
    for t, i in enumerate(keep):
        onboard = cells[t].reshape(w, w)[1:-1, 1:-1].reshape(-1)
        assert np.array_equal(onboard, fx.cells[i]), entries[t].name
        assert n_moves[t] == fx.n_moves[i] and to_move[t] == entries[t].to_move, entries[t].name
    rc.check_roots(entries, [fx.cand[int(superko)][i] for i in keep], _root_lists(eng))
    eng.close()


VARIANTS = {"serial": {"TG_SELECT_SPLIT": "0", "TG_SELECT_SERIAL": "1"},
            "mpipe": {"TG_SELECT_SPLIT": "0"},
            "pipe": {"TG_SELECT_SPLIT": "0", "TG_SELECT_MPIPE_TREES": "0"},
            "split": {"TG_SELECT_SPLIT": "1"},
            "split1": {"TG_SELECT_SPLIT": "1", "TG_SPLIT_CFG": None}}


def _run_variant(mode, size, env_add, path):
    """One fresh process of tests/_rule_trees.py under the variant's environment (as test_pipelined_selection_equals_serial
    sets it); a process that fails or does not return fails the test at once, so nothing is started after it."""
    env = dict(os.environ)
    for key in ("TG_SELECT_SERIAL", "TG_SELECT_MPIPE_TREES", "TG_SPLIT_CFG", "TG_SELECT_SPLIT"):
        env.pop(key, None)
    for key, value in env_add.items():
        env[key] = value if value is not None else ("11016" if size == 9 else "11007")
    res = subprocess.run([sys.executable, os.path.join(HERE, "_rule_trees.py"), mode, str(size), path], env=env,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return dict(np.load(path))


def _nodes(data, key):
    off = data[f"o{key}"]
    return [([int(v) for v in data[f"a{key}"][off[i]:off[i + 1]]], [int(v) for v in data[f"c{key}"][off[i]:off[i + 1]]])
            for i in range(int(data[f"n{key}"]))]


def _same(a, b):
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("size", rc.SIZES)
def test_every_expanded_node_in_every_selection_kernel(size, tmp_path):
    """Short PUCT searches (root evaluation + mini-batches of 16, 16 and 9 descents) from dense corpus roots under the
    one-wave, mpipe, pipe and split selection kernels (split1: 9x9 and 19x19): every node's action list is
    search_candidates at the position its path leads to, every evaluated leaf's planes are the features of its node's
    position, every kernel wrote the same file, and the expanded nodes hold what the roots were chosen for (nodes with a
    ko-forbidden point, after a capture, with a slow self-atari point)."""
    fx = rc.load_fixture(size)
    roots = [fx.entries[i] for i in fx.tree_roots]
    names = [v for v in VARIANTS if not (v == "split1" and size == 13)]
    first = None
    for variant in names:
        data = _run_variant("puct", size, VARIANTS[variant], str(tmp_path / f"{variant}.npz"))
        if first is None:
            first = data
            reached = []
            for t, entry in enumerate(roots):
                nodes = _nodes(data, t)
                reached.append(rc.walk_tree(entry, nodes, True))
                assert len(data[f"q{t}"]) == len(data[f"p{t}"]) == 1 + 41
                rc.check_leaves(entry, reached[-1], zip(data[f"q{t}"], data[f"p{t}"]))
            got = rc.expanded_coverage(reached)
            print(f"expanded at {size}x{size}: {dict(got)}")
            for key, least in rc.EXPANDED_MINIMUMS[size].items():
                assert got[key] >= least, (key, got[key], least)
        else:
            assert _same(first, data), f"{variant} differs from {names[0]}"


@pytest.mark.parametrize("size", [9, 19])
def test_every_expanded_node_of_gumbel_searches(size, tmp_path):
    """generate_move_with_sequential_halving (16 and 50 simulations) from the first corpus roots under the default kernel and
    TG_SELECT_SERIAL=1, leaf by leaf and in the unique-leaf layout: the same node walk, and all four give the same trees."""
    fx = rc.load_fixture(size)
    first = None
    for variant, env_add in (("default", {}), ("serial", {"TG_SELECT_SERIAL": "1"})):
        data = _run_variant("gumbel", size, env_add, str(tmp_path / f"gumbel_{variant}.npz"))
        if first is None:
            first = data
            keys = sorted(k[1:] for k in data if k.startswith("n"))
            assert len(keys) == 4 * len([k for k in keys if k.endswith("_16_u0")]) >= 16
            total = 0
            for key in keys:
                root = int(key.split("_")[1])
                nodes = _nodes(data, key)
                total += len(nodes) - 1
                rc.walk_tree(fx.entries[fx.tree_roots[root]], nodes, True)
                if key.endswith("u1"):
                    other = key[:-1] + "0"
                    assert all(np.array_equal(data[p + key], data[p + other]) for p in "naco"), key
            print(f"gumbel nodes below the roots at {size}x{size}: {total}")
            assert total >= 16
        else:
            assert _same(first, data), f"{variant} differs from default"
