"""Whole-tree read-out on the GPU (csrc/search.hip: dump_scan_kernel, dump_walk_kernel; tg_search_dump_sizes /
tg_search_dump_trees / tg_search_tree_digests) against the node views of tg_search_read_node - the independent
path, one node per call -, against the dumps tools/gen_golden_tree_dump.py recorded from the reference, and against
tamago_amd/mcts/dump.py's numpy restatement of the digest.  The evaluator is oracle.stubnet.StubNet (one test adds a DualNet,
for the chained calls a host evaluator cannot take); every comparison is exact."""
import io
import json

import numpy as np
import pytest

from tamago_amd.mcts import dump
from tests import _tree_dump_cases as cases

pytestmark = pytest.mark.gpu

ERR_ARG = -1
ARRAY_KEYS = tuple(key for key, _, _ in dump.CHILD_ARRAYS)


def _stub(seed):
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.engine import HostEvaluator
    return HostEvaluator(StubNet(salt=seed), torch.device("cuda", 0))


def _bits(value):
    return np.array([value], dtype=np.float32).view(np.uint32)[0]


def assert_packed_equals_views(eng, t, packed):
    """Every node of tree t through tg_search_read_node against the packed tree: the scalars, and every child array below
    num_children."""
    n = int(eng.num_nodes()[t])
    assert packed["num_nodes"] == n and packed["current_root"] == 0
    total = 0
    for i in range(n):
        view = eng.read_node(t, i)
        nc, lo = int(view.num_children), int(packed["first_child"][i])
        assert lo == total, i
        assert (int(packed["num_children"][i]), int(packed["node_visits"][i]), int(packed["virtual_loss"][i])) == \
            (nc, int(view.node_visits), int(view.virtual_loss)), i
        assert _bits(packed["node_value_sum"][i]) == _bits(view.node_value_sum) and _bits(packed["raw_value"][i]) == _bits(view.raw_value), i
        for key, _, dtype in dump.CHILD_ARRAYS:
            want = np.asarray(getattr(view, key)[:nc], dtype=dtype)
            got = packed[key][lo:lo + nc]
            assert got.dtype == np.dtype(dtype)
            words = np.uint64 if got.dtype.itemsize == 8 else np.uint32
            assert np.array_equal(got.view(words), want.view(words)), (i, key)
        total += nc
    assert packed["total_children"] == total
    if n:
        parent, pedge = eng.read_node_links(t, n - 1)
        assert (int(packed["parent"][n - 1]), int(packed["pedge"][n - 1])) == (parent, pedge)


def assert_dict_equals_views(tree, tree_dict):
    """MCTSTree.to_dict() against tree.node[i]: the thirteen keys of every node, arrays of full length - below num_children
    the view's entries, beyond it the canonical tail (which is also what a view of a freshly expanded node holds)."""
    A = tree._engine.A
    assert tree_dict["num_nodes"] == len(tree_dict["node"]) == tree.num_nodes
    root_noise = tree.get_root().noise
    for i, state in enumerate(tree_dict["node"]):
        view = tree.node[i]
        nc = int(view.num_children)
        assert list(state) == ["node_visits", "virtual_loss", "node_value_sum", "raw_value", "action", "children_index",
                               "children_value", "children_visits", "children_policy", "children_virtual_loss",
                               "children_value_sum", "noise", "num_children"]
        assert (state["num_children"], state["node_visits"], state["virtual_loss"]) == (nc, int(view.node_visits), int(view.virtual_loss))
        assert state["node_value_sum"] == float(view.node_value_sum) and state["raw_value"] == float(view.raw_value)
        assert type(state["node_value_sum"]) is float and type(state["raw_value"]) is float
        for key in ARRAY_KEYS:
            want = [v for v in np.asarray(getattr(view, key)).tolist()]
            assert len(state[key]) == A
            assert state[key][:nc] == want[:nc], (i, key)
            assert all(v == (-1 if key == "children_index" else 0) for v in state[key][nc:]), (i, key)
        assert state["noise"] == (root_noise.tolist() if i == tree_dict["current_root"] else [0.0] * A)


# ---- dump against node views ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.SIZES)
def test_to_dict_equals_the_node_views(size):
    """A 64-visit PUCT search at batch 8 and a 32-simulation Gumbel search: every node and every field."""
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    board = cases.product_board(size, 20, True)
    tree = MCTSTree(StubNet(salt=size), tree_size=128, batch_size=8)
    assert tree.to_dict() == dump.empty_tree_dict(8, False)                       # before any search
    np.random.seed(size)
    tree.search_best_move(board, 1, TimeManager(TimeControl.STRICT_PLAYOUT, 64), {})
    puct = tree.to_dict()
    assert 32 < puct["num_nodes"] == tree.num_nodes and puct["to_move"] == "black" and puct["batch_size"] == 8
    assert_dict_equals_views(tree, puct)
    assert_packed_equals_views(tree._engine, 0, tree._engine.dump_trees()[0])
    assert np.array_equal(tree._engine.tree_digests()[0], dump.digest_of(puct))
    assert json.loads(tree.dump_to_json(board, True))["tree"] == puct
    tree.close()

    gumbel = MCTSTree(StubNet(salt=100 + size), tree_size=160)
    np.random.seed(size)
    gumbel.generate_move_with_sequential_halving(board, 1, TimeManager(TimeControl.CONSTANT_PLAYOUT, 32), True)
    state = gumbel.to_dict()
    assert state["num_nodes"] > 1 and any(state["node"][0]["noise"]) and state["to_move"] == "black"
    assert_dict_equals_views(gumbel, state)
    with pytest.raises(ValueError, match="max_nodes"):
        gumbel.to_dict(max_nodes=state["num_nodes"] - 1)
    gumbel.close()


# ---- dump against the reference's fixtures --------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.SIZES)
def test_to_dict_has_the_references_sha256(size):
    for case in cases.fixture(size)["cases"]:
        tree, _ = cases.product_tree(size, case)
        state = tree.to_dict()
        assert state["num_nodes"] == case["num_nodes"]
        assert cases.tool().canonical_sha256(state) == case["sha256"], case["index"]
        tree.close()


def test_the_small_dump_is_the_references_text():
    """json.loads of both texts is equal - the texts themselves are - and so is what enrich_mcts_dict adds."""
    small = cases.fixture(9)["small"]
    tree, board = cases.product_tree(9, cases.small_case())
    text = tree.dump_to_json(board, small["superko"])
    assert json.loads(text) == json.loads(small["json"])
    assert text == small["json"]
    state = json.loads(text)
    dump.enrich_mcts_dict(state)
    assert json.loads(json.dumps(cases.tool().enriched_fields(state))) == small["enriched"]
    tree.close()


# ---- the shapes where the kernels can go wrong ----------------------------------------------------------------------------
def test_shapes_in_one_engine_and_one_call():
    """One 19x19 lock-step engine, five trees, one call with the list in descending order: a tree with no root (advanced
    onto a child that was never expanded), a root-only tree - the empty board's root, 362 children: six lane passes -, a
    3-node tree, a tree of more than 2 048 nodes (the scan's carry crosses a chunk border twice) and a tree of some 67."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import SearchEngine
    size, batch = 19, 64
    eng = SearchEngine(size, 5, 2400, batch, _stub(19))
    try:
        boards = [cases.product_board(size, 30, False), GoBoard(size), cases.product_board(size, 60, False),
                  cases.product_board(size, 200, False), cases.product_board(size, 100, False)]
        for t, board in enumerate(boards):
            eng.set_root(t, board, 1, np.random.RandomState(t).get_state())
        eng.root_eval(False)
        eng.set_halt([0, 1, 0, 0, 0])                      # tree 1 stays root-only
        eng.puct_batch(2)
        eng.set_halt([0, 0, 1, 0, 0])                      # tree 2 stays at 3 nodes
        eng.puct_batch(batch)
        eng.set_halt([1, 0, 0, 0, 1])                      # trees 0 and 4: 66 visits
        for _ in range(33):                                # tree 3: 2 + 34 x 64 visits
            eng.puct_batch(batch)
        root = eng.read_node(0, 0)
        unexpanded = next(int(root.action[i]) for i in range(root.num_children) if root.children_index[i] == -1 and root.action[i] != 0)
        record = eng.advance([unexpanded, -1, -1, -1, -1])
        assert record["kept_visits"][0] == -1
        nodes, children = eng.dump_sizes()
        assert nodes.tolist() == eng.num_nodes().tolist()
        assert nodes[:3].tolist() == [0, 1, 3] and nodes[3] > 2 * 1024 + 64 and 3 < nodes[4] < 100
        assert children[0] == 0 and children[1] == 362
        order = [4, 3, 2, 1, 0]
        packed = eng.dump_trees(order)
        for t, tree in zip(order, packed):
            assert tree["to_move"] == (2 if t == 0 else 1) and tree["err"] == 0
            assert_packed_equals_views(eng, t, tree)
        empty = packed[4]
        assert empty["num_nodes"] == 0 and all(empty[key].size == 0 for key in ARRAY_KEYS)
        assert packed[3]["num_children"].tolist() == [362] and packed[2]["num_nodes"] == 3
        # the same trees by the all-trees call, and their digests: the device's are numpy's, listed or not, in any order
        for a, b in zip(eng.dump_trees(), reversed(packed)):
            assert all(np.array_equal(a[k], b[k]) for k in a)
        want = [dump.digest_of_packed(tree).tolist() for tree in packed]
        assert eng.tree_digests(order).tolist() == want and eng.tree_digests().tolist() == want[::-1]
        assert eng.tree_digests([3]).tolist() == [want[1]]
        assert want[4] == dump.digest_of(dump.empty_tree_dict(1, False)).tolist()
        assert len({tuple(w) for w in want}) == 5
    finally:
        eng.close()


def test_after_two_reroots_and_after_a_grown_pool():
    """MCTSTree(reuse_tree=True) whose tree was compacted in place twice, and a tree whose pool tg_search_grow doubled during
    the search: the dump is still the node views."""
    from oracle.stubnet import StubNet
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    tree = MCTSTree(StubNet(salt=3), tree_size=512, batch_size=8, reuse_tree=True)
    board = GoBoard(9)
    np.random.seed(3)
    color, reused = 1, []
    for _ in range(3):
        move = tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, 120), {})
        assert move > 0
        reused.append(tree.reused_visits)
        state = tree.to_dict()
        assert state["to_move"] == ("black" if color == 1 else "white")
        assert_dict_equals_views(tree, state)
        assert np.array_equal(tree._engine.tree_digests()[0], dump.digest_of(state))
        board.put_stone(move, color)
        color = 3 - color
    assert reused[0] == 0 and reused[1] > 0 and reused[2] > 0
    tree.close()

    grown = MCTSTree(StubNet(salt=2), tree_size=16, batch_size=8)
    np.random.seed(4)
    grown.search_best_move(GoBoard(9), 1, TimeManager(TimeControl.STRICT_PLAYOUT, 100), {})
    assert grown.tree_size >= 128
    state = grown.to_dict()
    assert 64 < state["num_nodes"] == grown.num_nodes
    assert_dict_equals_views(grown, state)
    grown.close()


# ---- digests --------------------------------------------------------------------------------------------------------------
def _engine_16(seeds, halt_after=True):
    """Sixteen 9x9 trees on different positions; tree t is halted after t + 1 mini-batches of 4: sixteen depths."""
    from tamago_amd.mcts.engine import SearchEngine
    eng = SearchEngine(9, 16, 80, 4, _stub(16))
    for t in range(16):
        eng.set_root(t, cases.product_board(9, 5 * t, t % 2 == 0), 1 + t % 2, np.random.RandomState(seeds[t]).get_state())
    eng.root_eval(False)
    for b in range(16):
        eng.puct_batch(4)
        eng.set_halt(np.arange(16) == b)
    return eng


def test_device_digests_equal_digest_of():
    eng = _engine_16(list(range(16)))
    other = _engine_16([0, 1, 2, 3, 4, 77, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])
    try:
        nodes = eng.num_nodes().tolist()
        assert nodes[0] == 5 and max(nodes) > 50 and len(set(nodes)) >= 10        # different depths
        got = eng.tree_digests()
        assert got.shape == (16, 2) and got.dtype == np.uint64
        for t, packed in enumerate(eng.dump_trees()):
            state = dump.tree_to_dict(packed, eng.A, 4, False)
            assert np.array_equal(got[t], dump.digest_of(state)) and np.array_equal(got[t], dump.digest_of_packed(packed)), t
        assert len({tuple(row) for row in got.tolist()}) == 16
        assert np.array_equal(eng.tree_digests(), got)                            # reading changes nothing
        # two engines that differ in one seed differ in that tree's digest, in both words, and in no other
        theirs = other.tree_digests()
        differ = [t for t in range(16) if not np.array_equal(got[t], theirs[t])]
        assert differ == [5] and got[5, 0] != theirs[5, 0] and got[5, 1] != theirs[5, 1]
    finally:
        eng.close()
        other.close()


def test_lockstep_trees_have_the_digests_of_single_searches():
    """Eight PUCT trees searched in lock-step, 48 visits at batch 8, against the same eight searches one tree at a time."""
    from tamago_amd.mcts.engine import SearchEngine
    plies = (0, 7, 14, 21, 28, 35, 42, 49)

    def search(eng, members):
        for t, k in enumerate(members):
            eng.set_root(t, cases.product_board(9, plies[k], True), 1 + k % 2, np.random.RandomState(50 + k).get_state())
        eng.root_eval(False)
        for _ in range(6):
            eng.puct_batch(8)
        return eng.tree_digests()

    together = SearchEngine(9, 8, 64, 8, _stub(8), check_superko=True)
    alone = SearchEngine(9, 1, 64, 8, _stub(8), check_superko=True)
    try:
        want = search(together, range(8))
        for k in range(8):
            assert np.array_equal(search(alone, [k])[0], want[k]), k
        assert len({tuple(row) for row in want.tolist()}) == 8
    finally:
        together.close()
        alone.close()


@pytest.mark.parametrize("evaluator", ["stub", "dualnet"])
def test_compact_chain_and_plain_chain_give_equal_digests(evaluator):
    """puct_chain(compact=True) against the same mini-batches without compaction, a halted tree among the five: equal digests
    on every tree - the whole trees, not samples of them.  Under the host StubNet a chain is the per-mini-batch loop
    (engine.can_chain) on either side; under a DualNet the calls are tg_search_puct_chain_compact and tg_search_puct_chain."""
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    batches = [8] * 5 + [3]

    def run(compact):
        if evaluator == "stub":
            ev = _stub(4)
        else:
            from tests.test_gpu_early_stop import _dualnet
            ev = DeviceEvaluator(_dualnet(9))
        eng = SearchEngine(9, 5, 64, 8, ev)
        try:
            for t, ply in enumerate((0, 10, 20, 30, 40)):
                eng.set_root(t, cases.product_board(9, ply, False), 1, np.random.RandomState(9).get_state())
            eng.root_eval(False)
            eng.puct_batch(8)
            eng.set_halt([0, 0, 1, 0, 0])
            if compact or evaluator == "dualnet":
                assert eng.puct_chain(batches, compact=compact) == len(batches)
            else:
                for k in batches:
                    eng.puct_batch(k)
            return eng.num_nodes().tolist(), eng.tree_digests(), eng.forward_positions
        finally:
            eng.close()

    nodes, want, plain_positions = run(False)
    nodes_c, got, compact_positions = run(True)
    assert nodes == nodes_c and nodes[2] == 9 and min(nodes[:2] + nodes[3:]) > 40
    assert np.array_equal(got, want) and len({tuple(row) for row in got.tolist()}) == 5
    if evaluator == "stub":                                                       # (the halted tree left the forward passes)
        assert compact_positions < plain_positions


# ---- refusals and the front end -------------------------------------------------------------------------------------------
def test_refusals_and_a_capacity_one_byte_short():
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.lib import TamagoHipError
    from tamago_amd.mcts.engine import SearchEngine
    eng = SearchEngine(9, 3, 16, 4, _stub(1))
    try:
        for t in range(3):
            eng.set_root(t, GoBoard(9), 1, np.random.RandomState(t).get_state())
        eng.root_eval(False)
        eng.puct_batch(4)
        lib, h, st = eng.lib, eng.handle, eng._stream()
        i64 = np.zeros(8, dtype=np.int64)
        u64 = np.zeros((4, 2), dtype=np.uint64)
        buf = np.zeros(1 << 16, dtype=np.uint8)

        def trees(*items):
            return np.array(items, dtype=np.int32)

        def message():
            return lib.tg_last_error().decode()
        ok = trees(2, 0)
        # null pointers
        assert lib.tg_search_dump_sizes(None, ok.ctypes.data, 2, i64.ctypes.data, i64.ctypes.data, st) == ERR_ARG
        assert lib.tg_search_dump_sizes(h, ok.ctypes.data, 2, None, i64.ctypes.data, st) == ERR_ARG and "null" in message()
        assert lib.tg_search_dump_sizes(h, ok.ctypes.data, 2, i64.ctypes.data, None, st) == ERR_ARG
        assert lib.tg_search_dump_trees(h, ok.ctypes.data, 2, None, buf.size, i64.ctypes.data, st) == ERR_ARG
        assert lib.tg_search_dump_trees(h, ok.ctypes.data, 2, buf.ctypes.data, buf.size, None, st) == ERR_ARG
        assert lib.tg_search_tree_digests(h, ok.ctypes.data, 2, None, st) == ERR_ARG and "null" in message()
        assert lib.tg_search_tree_digests(None, None, 0, u64.ctypes.data, st) == ERR_ARG
        # a tree out of range, a duplicate, an empty list - in each of the three
        for bad, word in ((trees(0, 3), "out of range"), (trees(-1), "out of range"), (trees(1, 2, 1), "twice"), (trees(0), "holds 0")):
            n = 0 if word == "holds 0" else bad.size
            assert lib.tg_search_dump_sizes(h, bad.ctypes.data, n, i64.ctypes.data, i64.ctypes.data, st) == ERR_ARG and word in message()
            assert lib.tg_search_dump_trees(h, bad.ctypes.data, n, buf.ctypes.data, buf.size, i64.ctypes.data, st) == ERR_ARG and word in message()
            assert lib.tg_search_tree_digests(h, bad.ctypes.data, n, u64.ctypes.data, st) == ERR_ARG and word in message()
        assert not buf.any() and not u64.any() and not i64.any()                  # a refused call wrote nothing
        with pytest.raises(TamagoHipError, match="twice"):
            eng.dump_trees([1, 1])
        with pytest.raises(TamagoHipError, match="out of range"):
            eng.tree_digests([3])
        # capacity: one byte short writes nothing and names the size; the exact size is taken
        nodes, children = eng.dump_sizes(ok)
        need = sum(dump.record_bytes(int(a), int(b)) for a, b in zip(nodes, children))
        buf[:] = 0xAB
        offsets = np.full(3, -7, dtype=np.int64)
        assert lib.tg_search_dump_trees(h, ok.ctypes.data, 2, buf.ctypes.data, need - 1, offsets.ctypes.data, st) == ERR_ARG
        assert f"take {need} bytes" in message() and (buf == 0xAB).all() and (offsets == -7).all()
        assert lib.tg_search_dump_trees(h, ok.ctypes.data, 2, buf.ctypes.data, need, offsets.ctypes.data, st) == 0
        assert offsets.tolist() == [0, dump.record_bytes(int(nodes[0]), int(children[0])), need] and (buf[need:] == 0xAB).all()
        assert_packed_equals_views(eng, 2, dump.parse_record(buf[:offsets[1]]))
        assert_packed_equals_views(eng, 0, dump.parse_record(buf[offsets[1]:need]))
    finally:
        eng.close()


def test_a_tree_in_error_is_dumped_and_the_host_layer_raises():
    """A pool too small for the mini-batch: the tree's sticky error word travels in the record's head; SearchEngine.dump_trees
    raises with the text of csrc/readout.h, check=False hands the packed tree out."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.lib import TamagoHipError
    from tamago_amd.mcts.engine import SearchEngine
    eng = SearchEngine(9, 1, 8, 16, _stub(0))
    try:
        eng.set_root(0, GoBoard(9), 1, np.random.RandomState(0).get_state())
        eng.root_eval(False)
        eng.puct_batch(16)
        with pytest.raises(TamagoHipError, match="node pool full"):
            eng.dump_trees()
        packed = eng.dump_trees(check=False)[0]
        assert packed["err"] & 1 and 1 <= packed["num_nodes"] <= 8 and packed["num_children"][0] == 82
        assert np.array_equal(eng.tree_digests()[0], dump.digest_of_packed(packed))
    finally:
        eng.close()


def test_gtp_dump_tree():
    """tamago-dump_tree: "= ", a newline, the JSON on one line, a blank line; before any search the empty tree; after a
    genmove the tree of mcts.to_dict(); the command is listed."""
    from oracle.stubnet import StubNet
    from tamago_amd.gtp.client import GtpClient
    from tamago_amd.mcts.time_manager import TimeControl
    out = io.StringIO()
    client = GtpClient(9, True, StubNet(8), visits=40, batch_size=8, tree_size=128, mode=TimeControl.STRICT_PLAYOUT, stdout=out)
    np.random.seed(5)
    client.stdin = io.StringIO("list_commands\ntamago-dump_tree\nplay b E5\ngenmove w\n3 tamago-dump_tree\nquit\n")
    client.run()
    blocks = out.getvalue().split("\n\n")
    assert "tamago-dump_tree" in blocks[0].split("\n")
    head, text = blocks[1].split("\n")
    assert head == "= "
    before = json.loads(text)
    assert before["tree"] == dump.empty_tree_dict(8, False) and before["move_history"] == [] and before["board_size"] == 9
    assert blocks[3].startswith("= ")
    head, text = blocks[4].split("\n")
    assert head == "=3 "
    after = json.loads(text)
    assert after["tree"] == client.mcts.to_dict() and after["tree"]["to_move"] == "white"
    assert 20 < after["tree"]["num_nodes"] == client.mcts.num_nodes
    # (the dump is taken after the generated move was played: the history holds it)
    assert [c for c, _ in after["move_history"]] == ["black", "white"] and after["superko"] is True
    assert out.getvalue().endswith(text + "\n\n= \n\n")
    dump.enrich_mcts_dict(after)
    assert sorted(after["tree"]["sorted_indices_list"]) == list(range(after["tree"]["num_nodes"]))
