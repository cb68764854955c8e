"""Tree reuse across moves (MCTSTree(reuse_tree=True), tg_search_reroot, GtpClient(reuse_tree=True), the GTP launcher)
against its emulation on the oracle (tests/_tree_reuse.py).  StubNet evaluator on both sides: bit-exact everywhere."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._tree_reuse import compact_arrays, emulate_search, oracle_child
from tests.test_gpu_search import product_digest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _boards(size):
    from oracle.board import GoBoard as OBoard
    from tamago_amd.board.go_board import GoBoard
    return GoBoard(size, 7.0, False), OBoard(size, 7.0, False)


def _same_root(tree, otree):
    root, oroot = tree.get_root(), otree.node[0]
    n = root.num_children
    assert n == oroot.num_children
    assert [int(a) for a in root.action[:n]] == [int(a) for a in oroot.action[:n]]
    assert np.array_equal(root.children_visits[:n], oroot.children_visits[:n])
    assert np.array_equal(root.children_value_sum[:n], oroot.children_value_sum[:n])
    assert np.array_equal(root.children_policy[:n], oroot.children_policy[:n])
    assert int(root.node_visits) == int(oroot.node_visits)
    assert float(root.node_value_sum) == float(oroot.node_value_sum)
    assert float(root.raw_value) == float(oroot.raw_value)


def _play_both(board, oboard, move, color):
    board.put_stone(int(move), color)
    oboard.put_stone(int(move), color)


@pytest.mark.parametrize("size,visits,batch,strict", [(9, 400, 16, True), (9, 400, 16, False), (13, 200, 16, True),
                                                      (19, 200, 16, True)])
def test_reuse_equals_the_emulated_compaction(size, visits, batch, strict):
    """A game where every search continues the previous tree: one reply searched (k = 1), one reply played from the tree
    without a search (k = 2).  Move, root statistics, num_nodes, the whole-tree digest and numpy's stream afterwards
    equal the oracle's compacted tree continued by the reference's search loop."""
    from oracle.stubnet import StubNet
    from oracle.tree import MCTSTree as OTree, TimeManager as OTM, TimeControl as OTC
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    board, oboard = _boards(size)
    tree = MCTSTree(StubNet(salt=3), tree_size=4096, batch_size=batch, reuse_tree=True)
    otree = OTree(StubNet(salt=3), size, tree_size=4096, batch_size=batch)
    mode, omode = (TimeControl.STRICT_PLAYOUT, OTC.STRICT_PLAYOUT) if strict else \
        (TimeControl.CONSTANT_PLAYOUT, OTC.CONSTANT_PLAYOUT)
    np.random.seed(11)
    color, reuse_root, reused = 1, None, 0
    for step in range(5):
        state = np.random.get_state()
        mv = tree.search_best_move(board, color, TimeManager(mode, visits), {})
        after = np.random.get_state()
        np.random.set_state(state)
        omv = emulate_search(otree, oboard, color, OTM(omode, visits), reuse_root)
        assert int(mv) == int(omv), step
        assert (tree.reused_visits > 0) == (reuse_root is not None), step
        reused += tree.reused_visits
        _same_root(tree, otree)
        assert tree.num_nodes == otree.num_nodes
        assert product_digest(tree, tree.num_nodes) == product_digest(otree, otree.num_nodes), step
        oafter = np.random.get_state()
        assert after[2] == oafter[2] and np.array_equal(after[1], oafter[1]), step
        if mv <= 0:
            break
        node = oracle_child(otree, 0, mv)
        _play_both(board, oboard, mv, color)
        color = 3 - color
        if step == 2 and node >= 0:
            # the opponent's reply comes from the tree without a search of its own (k = 2 at the next search)
            reply = otree.node[node].action[otree.node[node].best_move_index()]
            child = oracle_child(otree, node, reply)
            _play_both(board, oboard, reply, color)
            color = 3 - color
            node = child
        reuse_root = node if node >= 0 else None
    assert reused > 0


def test_same_position_twice_continues_and_misses_rebuild():
    """k = 0: the tree continues (root visits = the budget, no root draws).  A reply that was never expanded and a changed
    komi each give exactly what a reuse-off tree gives from the same random state."""
    from oracle.stubnet import StubNet
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    tree = MCTSTree(StubNet(salt=5), tree_size=2048, batch_size=16, reuse_tree=True)
    board = GoBoard(9, 7.0, False)
    np.random.seed(2)
    tree.search_best_move(board, 1, TimeManager(TimeControl.STRICT_PLAYOUT, 100), {})
    state = np.random.get_state()
    tree.search_best_move(board, 1, TimeManager(TimeControl.STRICT_PLAYOUT, 300), {})
    assert tree.reused_visits == 100
    assert int(tree.get_root().node_visits) == 300
    # a second same-budget search: nothing to do, nothing drawn
    state = np.random.get_state()
    tree.search_best_move(board, 1, TimeManager(TimeControl.STRICT_PLAYOUT, 300), {})
    assert int(tree.get_root().node_visits) == 300
    after = np.random.get_state()
    assert after[2] == state[2] and np.array_equal(after[1], state[1])

    def fresh(b, color, seed_state):
        ref = MCTSTree(StubNet(salt=5), tree_size=2048, batch_size=16)
        np.random.set_state(seed_state)
        mv = ref.search_best_move(b, color, TimeManager(TimeControl.STRICT_PLAYOUT, 200), {})
        return mv, ref.get_root(), ref.num_nodes, product_digest(ref, ref.num_nodes), np.random.get_state()[1].copy()

    root = tree.get_root()
    unexpanded = [a for a, c in zip(root.action[:root.num_children], root.children_index[:root.num_children]) if c < 0]
    assert unexpanded
    board.put_stone(int(unexpanded[0]), 1)
    for change_komi in (False, True):
        if change_komi:
            mv = tree.search_best_move(board, 2, TimeManager(TimeControl.STRICT_PLAYOUT, 100), {})   # (remembered again)
            board.put_stone(int(mv), 2)
            board.set_komi(6.5)
        seed_state = np.random.get_state()
        mv = tree.search_best_move(board, board.get_to_move(), TimeManager(TimeControl.STRICT_PLAYOUT, 200), {})
        assert tree.reused_visits == 0
        got = (mv, tree.get_root(), tree.num_nodes, product_digest(tree, tree.num_nodes), np.random.get_state()[1].copy())
        want = fresh(board, board.get_to_move(), seed_state)
        assert got[0] == want[0] and got[2] == want[2] and got[3] == want[3] and np.array_equal(got[4], want[4])
        assert np.array_equal(got[1].children_visits, want[1].children_visits)


def _read_tree(engine, t, n):
    keys = ("children_index", "children_visits", "children_virtual_loss", "children_value_sum", "children_policy",
            "children_value")
    out = {k: [] for k in keys}
    out.update(num_children=[], node_visits=[], virtual_loss=[], node_value_sum=[], raw_value=[], action=[], parent=[],
               pedge=[])
    for i in range(n):
        nd = engine.read_node(t, i)
        for k in keys:
            out[k].append(getattr(nd, k).copy())
        out["num_children"].append(nd.num_children)
        out["node_visits"].append(nd.node_visits)
        out["virtual_loss"].append(nd.virtual_loss)
        out["node_value_sum"].append(np.float32(nd.node_value_sum))
        out["raw_value"].append(np.float32(nd.raw_value))
        out["action"].append(np.array(nd.action, dtype=np.int32))
        p, e = engine.read_node_links(t, i)
        out["parent"].append(p)
        out["pedge"].append(e)
    return {k: np.array(v) for k, v in out.items()}


class _FlatNet:
    """Uniform policy, even value: PUCT spreads its visits breadth first, so a tree of a million nodes stays shallow."""

    def __init__(self, size):
        self.a = size * size + 1

    def inference(self, planes):
        import torch
        b = planes.shape[0]
        return torch.full((b, self.a), 1.0 / self.a), torch.tensor([[0.25, 0.5, 0.25]]).repeat(b, 1)


def _grown_engine(size, trees, tree_size, batch, batches, seed=1, flat=False):
    from oracle.stubnet import StubNet
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import SearchEngine, HostEvaluator
    import torch
    if flat:
        evaluator = HostEvaluator(_FlatNet(size), torch.device("cuda", 0))
    else:
        evaluator = HostEvaluator(StubNet(salt=9), torch.device("cuda", 0))
    engine = SearchEngine(size, trees, tree_size, batch, evaluator)
    board = GoBoard(size, 7.0, False)
    for t in range(trees):
        np.random.seed(seed + t)
        engine.set_root(t, board, 1 + (t % 2), np.random.get_state())
    engine.root_eval()
    for _ in range(batches):
        engine.ensure_capacity(batch)
        engine.puct_batch(batch)
    return engine


def _stage_position(engine, t, node, root_color):
    """set_root(t, position of `node`): the moves along the parent links from the tree's root (an empty board)."""
    from tamago_amd.board.go_board import GoBoard
    moves = []
    while True:
        parent, edge = engine.read_node_links(t, node)
        if parent < 0:
            break
        moves.append(engine.read_node(t, parent).action[edge])
        node = parent
    board, color = GoBoard(engine.S, 7.0, False), root_color
    for mv in reversed(moves):
        board.put_stone(int(mv), color)
        color = 3 - color
    engine.set_root(t, board, color)


@pytest.mark.parametrize("size", [9, 13, 19])
def test_reroot_kernel_against_numpy_compaction(size):
    """T = 4, new roots per tree: -1, a root child, a deep node, the most recently created node.  Every node read back
    equals the numpy compaction of the pre-state, field by field (parents included); tree -1 is untouched."""
    engine = _grown_engine(size, 4, 1024, 8, 12)
    n = engine.num_nodes()
    before = [_read_tree(engine, t, int(n[t])) for t in range(4)]
    root1 = before[1]
    best = int(np.argmax(root1["children_visits"][0][:root1["num_children"][0]]))
    roots = [-1, int(root1["children_index"][0][best]), 0, int(n[3]) - 1]
    deep = [i for i in range(int(n[2])) if before[2]["parent"][i] > 0]
    assert deep and roots[1] > 0
    roots[2] = deep[len(deep) // 2]
    for t in (1, 2, 3):
        _stage_position(engine, t, roots[t], 1 + (t % 2))
    engine.reroot(roots)
    after_n = engine.num_nodes()
    assert int(after_n[0]) == int(n[0])
    got0 = _read_tree(engine, 0, int(n[0]))
    for k in before[0]:
        assert np.array_equal(got0[k], before[0][k]), k
    for t in (1, 2, 3):
        want = compact_arrays(before[t], roots[t])
        assert int(after_n[t]) == len(want["parent"])
        got = _read_tree(engine, t, int(after_n[t]))
        for k in want:
            assert np.array_equal(got[k], want[k]), (t, k)
    # the compacted trees keep searching: one more mini-batch leaves consistent parent links
    engine.puct_batch(8)
    n2 = engine.num_nodes()
    for t in (1, 2, 3):
        tr = _read_tree(engine, t, int(n2[t]))
        for i in range(1, int(n2[t])):
            assert tr["children_index"][tr["parent"][i]][tr["pedge"][i]] == i


def test_reroot_of_a_tree_of_400k_nodes():
    """One 9x9 tree grown past 400 000 nodes (over 5 000 windows of the in-place move): the compacted pool is checked node
    by node on a sample of the kept nodes, with its size and links.  (A single tree grown much further stops in the
    selection kernels with "path too deep" before reroot is reached: their move buffers hold kPathMax<9> = 256 levels, 512
    - kPipeMaxDepth - at 13x13 and 19x19 and in the mpipe kernel.  The 48 levels of kPathCap are no limit: a deeper leaf
    has no recorded path and is backed up along the parent pointers, tests/test_gpu_hard_trees.py.)"""
    engine = _grown_engine(9, 1, 1 << 17, 256, 4, flat=True)
    while int(engine.num_nodes()[0]) <= 400_000:
        engine.ensure_capacity(256)
        engine.puct_batch(256)
    n = int(engine.num_nodes()[0])
    root = engine.read_node(0, 0)
    # an early root child: its subtree (some N / 82 nodes) is spread over the whole pool, so the move walks every window
    # from the child's index to the end of the pool, and the subtree stays small enough to read back node by node
    cand = [i for i in range(root.num_children) if root.children_index[i] > 0 and root.children_visits[i] >= 1000]
    assert cand
    new_root = min(int(root.children_index[i]) for i in cand)
    # structure of the whole tree: children and num_children of every node (one bulk read each through the queue-free path)
    children, counts = {}, {}

    def fetch(i):
        if i not in children:
            nd = engine.read_node(0, i)
            children[i], counts[i] = nd.children_index.copy(), nd.num_children
        return children[i]

    # subtree by walking from the new root (reads only the subtree's nodes)
    keep, stack = [], [new_root]
    while stack:
        i = stack.pop()
        keep.append(i)
        stack.extend(int(c) for c in fetch(i)[:counts[i]] if c >= 0)
    keep.sort()
    sample = sorted(set(keep[:50] + keep[-50:] + keep[::max(1, len(keep) // 200)]))
    before = {i: engine.read_node(0, i) for i in sample}
    links = {i: engine.read_node_links(0, i) for i in sample}
    _stage_position(engine, 0, new_root, 1)
    engine.reroot([new_root])
    assert int(engine.num_nodes()[0]) == len(keep)
    remap = {old: new for new, old in enumerate(keep)}
    for old in sample:
        new = remap[old]
        got, want = engine.read_node(0, new), before[old]
        k = want.num_children
        assert got.num_children == k and got.node_visits == want.node_visits and got.virtual_loss == want.virtual_loss
        assert float(got.node_value_sum) == float(want.node_value_sum) and float(got.raw_value) == float(want.raw_value)
        assert list(got.action) == list(want.action)
        assert np.array_equal(got.children_visits, want.children_visits)
        assert np.array_equal(got.children_value_sum, want.children_value_sum)
        assert np.array_equal(got.children_policy, want.children_policy)
        assert np.array_equal(got.children_value, want.children_value)
        assert [int(c) for c in got.children_index] == [remap[int(c)] if c >= 0 else -1 for c in want.children_index]
        p, e = engine.read_node_links(0, new)
        if old == new_root:
            assert (p, e) == (-1, -1)
        else:
            assert (p, e) == (remap[links[old][0]], links[old][1])
    assert n > len(keep)


def _run_gtp(client, script):
    old = sys.stdout
    sys.stdout = io.StringIO()
    try:
        client.stdin = io.StringIO(script)
        client.run()
        return sys.stdout.getvalue()
    finally:
        sys.stdout = old


def test_gtp_reuse_continues_ponder_and_forgets_on_undo_and_clear_board(monkeypatch):
    from oracle.stubnet import StubNet
    from tamago_amd.gtp.client import GtpClient
    from tamago_amd.mcts.time_manager import TimeControl

    def client(reuse):
        return GtpClient(9, False, StubNet(4), visits=200, batch_size=16, tree_size=2048,
                         mode=TimeControl.STRICT_PLAYOUT, reuse_tree=reuse)

    # lz-analyze (no input arrives: the ponder runs until its node cap) then genmove on the same position
    import select
    monkeypatch.setattr(select, "select", lambda *a: ([], [], []))
    c = client(True)
    c.mcts.ponder_max_nodes = 4096
    np.random.seed(3)
    _run_gtp(c, "play b E5\nlz-analyze w 0\nquit\n")
    pondered = int(c.mcts.get_root().node_visits)
    assert pondered > 0
    _run_gtp(c, "genmove w\nquit\n")
    assert c.mcts.reused_visits == pondered

    # undo / clear_board: the same output as a reuse-off client from the same seed
    script = "play b E5\ngenmove w\nundo\ngenmove w\nclear_board\nplay b C3\ngenmove w\ngenmove b\nquit\n"
    outs = []
    for reuse in (False, True):
        np.random.seed(7)
        outs.append(_run_gtp(client(reuse), script))
    assert outs[0] == outs[1]


def test_gtp_launcher_runs_in_a_child_process(tmp_path):
    script = "boardsize 9\nclear_board\nplay b E5\ngenmove w\ngenmove b\nquit\n"
    outs = []
    for extra in ([], ["--reuse-tree", "true"]):
        cmd = [sys.executable, "-m", "tamago_amd.gtp", "--size", "9", "--model", str(tmp_path / "missing.bin"),
               "--strict-visits", "64", "--batch-size", "16", "--tree-size", "1024"] + extra
        proc = subprocess.run(cmd, input=script, capture_output=True, text=True, cwd=REPO, timeout=600)
        assert proc.returncode == 0, proc.stderr
        outs.append(proc.stdout)
    for out in outs:
        blocks = [b for b in out.split("\n\n") if b.strip()]
        assert blocks[0].endswith("= ") or "Failed to load" in blocks[0]
        assert sum(1 for b in blocks if b.lstrip("Failed to load").strip().startswith("=")) >= 5
