"""Tree reuse on the CPU: the compaction the GPU tests hold the device against (tests/_tree_reuse.py) on oracle trees, and
the GTP launcher's option checks (no GPU needed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._tree_reuse import compact_arrays, compact_oracle_tree, emulate_search, oracle_child, subtree_nodes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_tree(size, seed, visits, batch=4):
    from oracle.board import GoBoard
    from oracle.stubnet import StubNet
    from oracle.tree import MCTSTree, TimeManager, TimeControl
    rng = np.random.RandomState(seed)
    board = GoBoard(size, 7.0, False)
    color = 1
    for _ in range(rng.randint(0, 6)):
        legal = [p for p in board.onboard_pos if board.is_legal(p, color)]
        board.put_stone(int(rng.choice(legal)), color)
        color = 3 - color
    tree = MCTSTree(StubNet(salt=seed), size, tree_size=64, batch_size=batch)
    np.random.seed(seed)
    tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, visits))
    return tree, board, color


def _as_arrays(tree):
    n = tree.num_nodes
    parent, pedge = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for i in range(n):
        nd = tree.node[i]
        for e in range(nd.num_children):
            c = int(nd.children_index[e])
            if c >= 0:
                parent[c], pedge[c] = i, e
    nodes = tree.node[:n]
    return {"children_index": np.array([nd.children_index for nd in nodes]),
            "children_visits": np.array([nd.children_visits for nd in nodes]),
            "children_value_sum": np.array([nd.children_value_sum for nd in nodes]),
            "children_policy": np.array([nd.children_policy for nd in nodes]),
            "action": np.array([nd.action for nd in nodes]),
            "node_visits": np.array([nd.node_visits for nd in nodes]),
            "num_children": np.array([nd.num_children for nd in nodes]),
            "parent": parent, "pedge": pedge}


@pytest.mark.parametrize("seed", range(6))
def test_compaction_keeps_the_subtree_in_creation_order(seed):
    size = (9, 13, 19)[seed % 3]
    tree, _, _ = _oracle_tree(size, seed, 120)
    before = _as_arrays(tree)
    n = tree.num_nodes
    rng = np.random.RandomState(100 + seed)
    root = int(rng.choice([i for i in range(n) if before["num_children"][i] > 0]))
    keep = subtree_nodes(before["children_index"], before["num_children"], root)
    assert keep[0] == root and all(i >= root for i in keep)          # a child is created after its parent
    assert all(before["parent"][i] < i for i in range(1, n))
    want = compact_arrays(before, root)
    compact_oracle_tree(tree, root)
    got = _as_arrays(tree)
    assert tree.num_nodes == len(keep) == len(want["parent"])
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # links agree both ways; statistics travel with their node
    for new, old in enumerate(keep):
        for e in range(got["num_children"][new]):
            c = got["children_index"][new][e]
            if c >= 0:
                assert got["parent"][c] == new and got["pedge"][c] == e and c > new
        assert np.array_equal(got["children_visits"][new], before["children_visits"][old])
        assert got["node_visits"][new] == before["node_visits"][old]
    assert got["parent"][0] == -1 and got["pedge"][0] == -1


def test_emulated_reuse_tops_the_root_up_to_the_budget():
    """The emulation: no random draws for a reused root, threshold - root visits descents, k = 0 changes nothing when the
    budget is already spent."""
    from oracle.tree import TimeManager, TimeControl
    tree, board, color = _oracle_tree(9, 3, 60)
    assert tree.node[0].node_visits == 60
    state = np.random.get_state()
    emulate_search(tree, board, color, TimeManager(TimeControl.STRICT_PLAYOUT, 60), reuse_root=0)
    after = np.random.get_state()
    assert tree.node[0].node_visits == 60 and after[2] == state[2] and np.array_equal(after[1], state[1])
    mv = emulate_search(tree, board, color, TimeManager(TimeControl.STRICT_PLAYOUT, 100), reuse_root=0)
    assert tree.node[0].node_visits == 100
    child = oracle_child(tree, 0, mv)
    assert child > 0
    visits = int(tree.node[child].node_visits)
    board.put_stone(mv, color)
    emulate_search(tree, board, 3 - color, TimeManager(TimeControl.STRICT_PLAYOUT, visits + 20), reuse_root=child)
    assert tree.node[0].node_visits == visits + 20


def _launcher(*args):
    return subprocess.run([sys.executable, "-m", "tamago_amd.gtp", *args], input="quit\n", capture_output=True, text=True,
                          cwd=REPO, timeout=300)


@pytest.mark.parametrize("args,text", [(["--use-gpu", "false"], "--use-gpu"), (["--policy-move", "true"], "--policy-move"),
                                       (["--animation-pv-wait", "0.5"], "--animation"),
                                       (["--animation-move-wait", "1"], "--animation"), (["--size", "7"], "--size 7")])
def test_launcher_refuses_what_it_cannot_serve(args, text):
    proc = _launcher(*args)
    assert proc.returncode == 2 and text in proc.stderr and proc.stdout == ""


def test_launcher_options():
    from tamago_amd.gtp.__main__ import parser, check_options
    args = parser().parse_args([])
    assert (args.size, args.komi, args.visits, args.batch_size, args.tree_size, args.reuse_tree) == (9, 7.0, 1000, 1, 65536, False)
    assert check_options(args) == ""
    args = parser().parse_args(["--reuse-tree", "true", "--strict-visits", "50", "--cgos-mode", "True", "--size", "19"])
    assert args.reuse_tree and args.strict_visits == 50 and args.cgos_mode and check_options(args) == ""
    assert parser().parse_args(["--reuse-tree"]).reuse_tree
    with pytest.raises(SystemExit):
        parser().parse_args(["--visits", "0"])
