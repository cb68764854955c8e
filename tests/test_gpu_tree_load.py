"""Whole-tree write-in on the GPU (csrc/search.hip: load_walk_kernel; tg_search_load_trees): trees dumped from one
engine and loaded into other slots of another, searches taken up again from snapshots, a tree built by the CPU oracle staged
directly, the reference's own dump continued, and the refusals.  The evaluator is oracle.stubnet.StubNet through HostEvaluator;
every comparison is exact.  Every tree that is loaded belongs to the position it is loaded under."""
import ctypes
import io
import json

import numpy as np
import pytest

from tamago_amd.mcts import dump
from tests import _tree_dump_cases as cases

pytestmark = pytest.mark.gpu

ERR_ARG = -1


def _stub(seed):
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.engine import HostEvaluator
    return HostEvaluator(StubNet(salt=seed), torch.device("cuda", 0))


def _engine(size, trees, tree_size, batch, salt, superko=False):
    from tamago_amd.mcts.engine import SearchEngine
    return SearchEngine(size, trees, tree_size, batch, _stub(salt), check_superko=superko)


def _occupy(eng, plies, superko=False, visits=0, size=9):
    """Every tree of the engine gets a root of its own and `visits` descents at the engine's batch: pool rows in use."""
    for t in range(eng.T):
        eng.set_root(t, cases.product_board(size, plies[t % len(plies)], superko), 1 + plies[t % len(plies)] % 2,
                     np.random.RandomState(900 + t).get_state())
    eng.root_eval(False)
    for _ in range(visits // eng.K):
        eng.puct_batch(eng.K)


def _queued(eng, t):
    idx = np.zeros(eng.K, dtype=np.int32)
    n = ctypes.c_int32(-1)
    assert eng.lib.tg_search_read_queue(eng.handle, t, idx.ctypes.data, eng.K, ctypes.byref(n)) == 0
    return n.value


def assert_canonical_tails(eng, t):
    for i in range(int(eng.num_nodes()[t])):
        view = eng.read_node(t, i)
        nc = int(view.num_children)
        assert np.all(np.asarray(view.children_index)[nc:] == -1), (t, i)
        for key in ("children_visits", "children_virtual_loss", "action"):
            assert not np.any(np.asarray(getattr(view, key))[nc:]), (t, i, key)
        for key in ("children_value_sum", "children_policy", "children_value"):
            assert not np.any(np.asarray(getattr(view, key), dtype=np.float64)[nc:].view(np.uint64)), (t, i, key)     # (+0.0 bits)


def same_record(a, b):
    return np.array_equal(dump.make_record(a), dump.make_record(b))


# ---- load equals source ---------------------------------------------------------------------------------------------------
SOURCE_PLIES = (0, 11, 20, 31)


def _source(size=9, tree_size=256, batch=8):
    """Four trees of different shapes: tree t halted after t + 1 mini-batches."""
    eng = _engine(size, 4, tree_size, batch, 3)
    for t, ply in enumerate(SOURCE_PLIES):
        eng.set_root(t, cases.product_board(size, ply, False), 1 + ply % 2, np.random.RandomState(t).get_state())
    eng.root_eval(False)
    for b in range(4):
        eng.puct_batch(batch)
        eng.set_halt(np.arange(4) == b)
    return eng


def test_loaded_trees_equal_their_sources():
    x = _source()
    y = _engine(9, 6, 128, 4, 3)
    try:
        records = x.dump_trees()
        want = x.tree_digests()
        assert [int(r["num_nodes"]) for r in records] == x.num_nodes().tolist() and len(set(x.num_nodes().tolist())) == 4
        # y: larger, different trees in every slot, a halt word on one of the slots to be loaded
        _occupy(y, (5, 16, 25, 36, 45, 2), visits=60)
        before_nodes, before = y.num_nodes().copy(), y.tree_digests()
        assert before_nodes.min() > max(int(r["num_nodes"]) for r in records)
        y.set_halt(np.arange(6) == 5)
        order, slots = [2, 0, 3, 1], [5, 2, 0, 3]                      # record order[j] goes to slot slots[j]
        for j, t in zip(order, slots):
            y.set_root(t, cases.product_board(9, SOURCE_PLIES[j], False), 1 + SOURCE_PLIES[j] % 2)
        flags = y.load_trees([records[j] for j in order], slots)
        assert flags.tolist() == [0, 0, 0, 0]
        got = y.tree_digests(slots)
        assert np.array_equal(got, want[order])
        assert all(np.array_equal(got[k], dump.digest_of_packed(records[j])) for k, j in enumerate(order))
        back = y.dump_trees(slots)
        assert all(same_record(back[k], records[j]) for k, j in enumerate(order))
        assert [int(b["err"]) for b in back] == [0] * 4
        assert y.num_nodes()[slots].tolist() == [int(records[j]["num_nodes"]) for j in order]
        for t in slots:
            assert_canonical_tails(y, t)
            assert _queued(y, t) == 0
        halted, _ = y.read_halt()
        assert not halted.any()                                        # slot 5's word went with the load
        # the untouched neighbours
        assert np.array_equal(y.tree_digests([1, 4]), before[[1, 4]]) and y.num_nodes()[[1, 4]].tolist() == before_nodes[[1, 4]].tolist()
        # root positions: the load did not touch them
        cells_x, cells_y = x.read_positions()[0], y.read_positions()[0]
        assert all(np.array_equal(cells_y[t], cells_x[j]) for j, t in zip(order, slots))
        assert y.node_bound >= max(int(r["num_nodes"]) for r in records)
    finally:
        x.close()
        y.close()


@pytest.mark.parametrize("size", [13, 19])
def test_one_tree_on_the_larger_boards(size):
    """A 19x19 root has 362 children: six lane passes; 13x13: 170, three, the last one partly tail."""
    from tamago_amd.board.go_board import GoBoard
    x = _engine(size, 1, 64, 4, size)
    y = _engine(size, 2, 96, 4, size)
    try:
        x.set_root(0, GoBoard(size), 1, np.random.RandomState(size).get_state())
        x.root_eval(False)
        for _ in range(3):
            x.puct_batch(4)
        record = x.dump_trees()[0]
        assert record["num_children"][0] == size * size + 1 and 8 <= record["num_nodes"] <= 13
        _occupy(y, (30, 60), visits=24, size=size)
        y.set_root(1, GoBoard(size), 1)
        y.load_trees([record], [1])
        assert np.array_equal(y.tree_digests([1])[0], x.tree_digests()[0])
        assert same_record(y.dump_trees([1])[0], record)
        assert_canonical_tails(y, 1)
    finally:
        x.close()
        y.close()


# ---- continuation ---------------------------------------------------------------------------------------------------------
def _best(eng, t):
    rec = eng.best_moves(0.0, False)[t]
    return tuple(rec[name].item() for name in rec.dtype.names)


def _stream_words(eng, t):
    state = eng.streams[t].final_state()
    return np.asarray(state[1]).tolist(), int(state[2])


@pytest.mark.parametrize("variant", ["batches", "chain", "superko", "reroot", "checkpoint"])
def test_a_search_continues_from_a_snapshot(variant, tmp_path):
    """Engine x: root + two mini-batches, a snapshot, two more mini-batches.  Engine y - other slot, other pool size, other
    trees beside it - restores the snapshot and runs the same two mini-batches: the same tree, move, stream and root."""
    superko = variant == "superko"
    if variant == "chain":                                           # (tg_search_puct_chain takes a device network: one DualNet for both)
        from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
        from tests.test_gpu_early_stop import _dualnet
        net = _dualnet(9)
        x, y = SearchEngine(9, 2, 256, 8, DeviceEvaluator(net)), SearchEngine(9, 3, 512, 8, DeviceEvaluator(net))
    else:
        x = _engine(9, 2, 256, 8, 6, superko)
        y = _engine(9, 3, 512, 8, 6, superko)
    try:
        board, color = cases.product_board(9, 14, superko), 1
        x.set_root(0, board, color, np.random.RandomState(21).get_state())
        x.set_root(1, cases.product_board(9, 3, superko), 2, np.random.RandomState(22).get_state())
        x.root_eval(False)
        for _ in range(2 if variant != "reroot" else 4):
            x.puct_batch(8)
        if variant == "reroot":                                      # a compacted tree: the most visited child becomes the root
            root = x.read_node(0, 0)
            k = int(np.argmax(np.asarray(root.children_visits)[:root.num_children]))
            child, move = int(root.children_index[k]), int(root.action[k])
            assert child > 0 and move > 0
            board.put_stone(move, color)
            color = 3 - color
            x.set_root(0, board, color)
            x.reroot([child, -1])
            assert 1 < int(x.num_nodes()[0])
        snaps = x.snapshot([0])
        if variant == "checkpoint":
            from tamago_amd.mcts import checkpoint
            checkpoint.save(tmp_path / "search.npz", snaps)
            snaps = checkpoint.load(tmp_path / "search.npz")
        assert snaps[0]["tree"]["num_nodes"] == int(x.num_nodes()[0]) and snaps[0]["halt"] == 0
        middle = x.tree_digests([0])[0].copy()

        def go_on(eng):
            if variant == "chain":
                eng.puct_chain([8, 8])
            else:
                eng.puct_batch(8)
                eng.puct_batch(8)
        go_on(x)
        _occupy(y, (7, 22, 9), superko, visits=40)
        y.restore(snaps, [2])
        assert np.array_equal(y.tree_digests([2])[0], middle)
        assert _stream_words(y, 2) == (np.asarray(snaps[0]["stream_key"]).tolist(), snaps[0]["stream_pos"])
        go_on(y)
        assert not np.array_equal(x.tree_digests([0])[0], middle)
        assert np.array_equal(y.tree_digests([2])[0], x.tree_digests([0])[0])
        assert same_record(y.dump_trees([2])[0], x.dump_trees([0])[0])
        assert _best(y, 2) == _best(x, 0)
        assert _stream_words(y, 2) == _stream_words(x, 0)
        rx, ry = x.read_root_state(0), y.read_root_state(2)
        assert np.array_equal(rx.pop("history"), ry.pop("history")) and rx == ry
        assert np.array_equal(x.read_positions()[0][0], y.read_positions()[0][2])
    finally:
        x.close()
        y.close()


def test_a_gumbel_root_continues_from_a_snapshot():
    """Snapshot after the first sequential-halving phase, with its noise; the next phase on both: equal trees and equal
    improved-policy rows."""
    from tamago_amd.mcts.constant import MAX_CONSIDERED_NODES
    from tamago_amd.mcts.sequential_halving import get_candidates_and_visit_pairs
    visits = 32
    x = _engine(9, 1, 160, visits, 12)
    y = _engine(9, 2, 256, visits, 12)
    try:
        board = cases.product_board(9, 10, False)
        x.set_root(0, board, 1, np.random.RandomState(31).get_state())
        x.root_eval(use_logit=True)
        x.set_gumbel_noise()
        base = min(int(x.root_children[0]), MAX_CONSIDERED_NODES)
        phases = list(get_candidates_and_visit_pairs(base, visits).items())
        assert len(phases) >= 2
        x.gumbel_phase([phases[0][0]], [phases[0][1]])
        snaps = x.snapshot()
        assert np.any(snaps[0]["noise"] != 0.0)
        x.gumbel_phase([phases[1][0]], [phases[1][1]])
        for t in range(2):
            y.set_root(t, board, 1, np.random.RandomState(40 + t).get_state())
        y.root_eval(use_logit=True)
        y.set_gumbel_noise()
        y.gumbel_phase([phases[0][0]] * 2, [phases[0][1]] * 2)
        y.restore(snaps, [1])
        assert np.array_equal(y.noise[1], snaps[0]["noise"])
        y.gumbel_phase([phases[1][0]] * 2, [phases[1][1]] * 2)
        assert np.array_equal(y.tree_digests([1])[0], x.tree_digests()[0])
        assert not np.array_equal(y.tree_digests([0])[0], x.tree_digests()[0])
        rows_x, rows_y = x.read_improved_policy().cpu().numpy(), y.read_improved_policy().cpu().numpy()
        assert np.array_equal(rows_x[0].view(np.uint32), rows_y[1].view(np.uint32))
    finally:
        x.close()
        y.close()


# ---- trees that never were on a device ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_small():
    """The CPU oracle's 10-visit tree of the small case, numpy's state behind that search, and its fresh 16-visit tree."""
    case = cases.small_case()
    ten = cases.oracle_tree_dict(9, case)
    state = np.random.get_state()
    sixteen = cases.oracle_tree_dict(9, dict(case, visits=16))
    final = np.random.get_state()
    return case, ten, state, sixteen, final


def test_an_oracle_built_tree_is_staged_and_searched_on(oracle_small):
    """A STRICT search of 16 visits at batch 2 passes through the 10-visit tree after five mini-batches - the same draws, the
    same mini-batches, the same stream positions - so the oracle's 10-visit tree, loaded, then three more mini-batches, is
    the oracle's fresh 16-visit tree."""
    case, ten, state, sixteen, _ = oracle_small
    eng = _engine(9, 1, case["tree_size"], case["batch"], case["seed"], case["superko"])
    try:
        packed = dump.packed_of_dict(ten)
        packed["to_move"] = case["color"]
        eng.set_root(0, cases.product_board(9, case["ply"], case["superko"]), case["color"], state)
        assert eng.load_trees([packed]).tolist() == [0]
        assert np.array_equal(eng.tree_digests()[0], dump.digest_of(ten))
        assert dump.tree_to_dict(eng.dump_trees()[0], 82, case["batch"], False) == ten
        for _ in range(3):
            eng.puct_batch(case["batch"])
        assert np.array_equal(eng.tree_digests()[0], dump.digest_of(sixteen))
        assert dump.tree_to_dict(eng.dump_trees()[0], 82, case["batch"], False) == sixteen
    finally:
        eng.close()


def test_the_references_file_is_continued(oracle_small):
    """MCTSTree(reuse_tree=True).load_json of the reference's own text, then 16 strict visits: the uninterrupted 16-visit
    search's tree.  Without reuse_tree the next search rebuilds and equals a plain search."""
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    case, ten, state, sixteen, final = oracle_small
    text = cases.fixture(9)["small"]["json"]
    tree = MCTSTree(StubNet(salt=case["seed"]), tree_size=case["tree_size"], batch_size=case["batch"], reuse_tree=True)
    board, color = tree.load_json(text)
    assert color.value == case["color"] and tree.num_nodes == case["num_nodes"] and tree.to_dict() == json.loads(text)["tree"]
    assert tree.dump_to_json(board, True) == text
    np.random.set_state(state)
    move = tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, 16), {})
    assert tree.reused_visits == 10 and tree.to_dict() == sixteen
    assert np.array_equal(np.random.get_state()[1], final[1]) and np.random.get_state()[2] == final[2]
    tree.close()

    plain, plain_board = cases.product_tree(9, dict(case, visits=16))
    assert plain.to_dict() == sixteen
    want_move = plain._engine.read_node(0, 0)
    want_move = want_move.action[want_move.get_best_move_index()]
    assert move == want_move
    plain.close()
    rebuilt = MCTSTree(StubNet(salt=case["seed"]), tree_size=case["tree_size"], batch_size=case["batch"])
    board, color = rebuilt.load_json(text)
    np.random.seed(case["seed"])
    rebuilt.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, 16), {})
    assert rebuilt.reused_visits == 0 and rebuilt.to_dict() == sixteen
    rebuilt.close()


def test_an_interrupted_mctstree_is_finished():
    """512 of 1 000 strict visits at batch 256, dump_to_json, close; a new MCTSTree(reuse_tree=True) loads the text and
    finishes to 1 000: the digest, the move and numpy's final state of the uninterrupted search."""
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    board = cases.product_board(9, 18, True)

    def tree():
        return MCTSTree(StubNet(salt=9), tree_size=2048, batch_size=256, reuse_tree=True)
    whole = tree()
    np.random.seed(77)
    want_move = whole.search_best_move(board, 1, TimeManager(TimeControl.STRICT_PLAYOUT, 1000), {})
    want, want_state = whole._engine.tree_digests()[0].copy(), np.random.get_state()
    whole.close()

    first = tree()
    np.random.seed(77)
    first.search_best_move(board, 1, TimeManager(TimeControl.STRICT_PLAYOUT, 512), {})
    text = first.dump_to_json(board, True)
    first.close()
    second = tree()
    loaded_board, color = second.load_json(text)
    move = second.search_best_move(loaded_board, color, TimeManager(TimeControl.STRICT_PLAYOUT, 1000), {})
    assert second.reused_visits == 512
    assert np.array_equal(second._engine.tree_digests()[0], want) and move == want_move
    state = np.random.get_state()
    assert np.array_equal(state[1], want_state[1]) and state[2] == want_state[2]
    second.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from tamago_amd.lib import TamagoHipError
    x = _source()
    y = _engine(9, 4, 30, 8, 3)
    try:
        records = x.dump_trees()
        _occupy(y, SOURCE_PLIES, visits=24)                              # (the records' positions: tree t's is record t's)
        before = y.tree_digests().copy()
        lib, h, st = y.lib, y.handle, y._stream()

        def call(packed_list, trees):
            recs = [dump.make_record(p) for p in packed_list]
            offsets = np.zeros(len(recs) + 1, dtype=np.int64)
            offsets[1:] = np.cumsum([r.size for r in recs])
            blob = np.concatenate(recs)
            flags = np.full(max(len(recs), 1), -7, dtype=np.int32)
            arr = None if trees is None else np.array(trees, dtype=np.int32)
            rc = lib.tg_search_load_trees(h, None if arr is None else arr.ctypes.data, 0 if arr is None else int(arr.size),
                                          blob.ctypes.data, offsets.ctypes.data, flags.ctypes.data, st)
            return rc, lib.tg_last_error().decode(), flags

        def untouched(flags):
            return (flags == -7).all() and np.array_equal(y.tree_digests(), before)
        small = [r for r in records if r["num_nodes"] <= 30]
        assert len(small) >= 3
        # an inadmissible record in a list of three refuses all three
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in small[1].items()}
        bad["children_index"][int(np.flatnonzero(bad["children_index"] > 0)[0])] = 0
        rc, msg, flags = call([small[0], bad, small[2]], [0, 1, 2])
        assert rc == ERR_ARG and "list entry 1" in msg and "child index" in msg and untouched(flags)
        # a duplicate tree, a tree out of range, an empty list
        for trees, word in (([0, 1, 0], "twice"), ([0, 1, 4], "out of range"), ([0, -1, 2], "out of range")):
            rc, msg, flags = call(small[:3], trees)
            assert rc == ERR_ARG and word in msg and untouched(flags)
        rc, msg, flags = call(small[:1], [])
        assert rc == ERR_ARG and "holds 0" in msg and untouched(flags)
        # num_nodes > tree_size
        big = next(r for r in records if r["num_nodes"] > 30)
        rc, msg, flags = call([big], [3])
        assert rc == ERR_ARG and "tree_size" in msg and untouched(flags)
        with pytest.raises(TamagoHipError, match="tree_size"):
            y.load_trees([big], [3])
        assert np.array_equal(y.tree_digests(), before)
        # null pointers
        i64, i32, u8 = np.zeros(2, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(64, dtype=np.uint8)
        assert lib.tg_search_load_trees(None, None, 0, u8.ctypes.data, i64.ctypes.data, i32.ctypes.data, st) == ERR_ARG
        assert lib.tg_search_load_trees(h, None, 0, None, i64.ctypes.data, i32.ctypes.data, st) == ERR_ARG
        assert lib.tg_search_load_trees(h, None, 0, u8.ctypes.data, i64.ctypes.data, None, st) == ERR_ARG
        assert np.array_equal(y.tree_digests(), before)
        # a wrong side to move: flag 1 and an untouched tree, while its neighbour in the same call loads
        j0, j1 = [j for j, r in enumerate(records) if r["num_nodes"] <= 30][:2]
        wrong = dict(records[j0], to_move=3 - records[j0]["to_move"])
        y.set_halt(np.arange(4) == j0)
        flags = y.load_trees([wrong, records[j1]], [j0, j1], check=False)
        assert flags.tolist() == [1, 0]
        after = y.tree_digests()
        assert np.array_equal(after[j0], before[j0]) and np.array_equal(after[j1], x.tree_digests([j1])[0])
        assert y.read_halt()[0].tolist() == [t == j0 for t in range(4)]         # the refused tree kept its halt word
        with pytest.raises(TamagoHipError, match="side to move"):
            y.load_trees([wrong], [j0])
    finally:
        x.close()
        y.close()


def test_mctstree_refuses_virtual_losses_and_illegal_actions(oracle_small):
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.tree import MCTSTree
    case, ten, _, _, _ = oracle_small
    tree = MCTSTree(StubNet(salt=case["seed"]), tree_size=case["tree_size"], batch_size=case["batch"], reuse_tree=True)
    board, color = tree.load_json(cases.fixture(9)["small"]["json"])
    before = tree._engine.tree_digests()[0].copy()
    pending = json.loads(json.dumps(ten))
    pending["node"][0]["children_virtual_loss"][2] = 1
    pending["node"][0]["virtual_loss"] = 1
    with pytest.raises(ValueError, match="virtual loss"):
        tree.load_dict(pending, board, color)
    illegal = json.loads(json.dumps(ten))
    illegal["node"][0]["action"][1] = int(json.loads(cases.fixture(9)["small"]["json"])["move_history"][0][1])
    with pytest.raises(ValueError, match="not legal"):
        tree.load_dict(illegal, board, color)
    assert np.array_equal(tree._engine.tree_digests()[0], before)
    tree.close()


# ---- GTP ------------------------------------------------------------------------------------------------------------------
def test_gtp_load_tree(tmp_path):
    """tamago-load_tree of a file tamago-dump_tree wrote in another client: the same board, the node count as the answer, and
    the next tamago-dump_tree gives the same text.  A missing file and a truncated file are failures that leave the board."""
    from oracle.stubnet import StubNet
    from tamago_amd.gtp.client import GtpClient
    from tamago_amd.mcts.time_manager import TimeControl

    def client(script, superko):
        out = io.StringIO()
        c = GtpClient(9, superko, StubNet(8), visits=40, batch_size=8, tree_size=128, mode=TimeControl.STRICT_PLAYOUT, stdout=out,
                      stdin=io.StringIO(script))
        c.run()
        return c, out.getvalue().split("\n\n")
    np.random.seed(5)
    # (undo: the dumped tree's root is the board's position again - a dump straight after genmove holds the move as well)
    first, blocks = client("komi 5.5\nplay b E5\ngenmove w\nundo\ntamago-dump_tree\nquit\n", True)
    head, text = blocks[4].split("\n")
    assert head == "= " and json.loads(text)["tree"]["num_nodes"] > 20 and json.loads(text)["tree"]["to_move"] == "white"
    good, cut, missing = tmp_path / "tree.json", tmp_path / "cut.json", tmp_path / "none.json"
    good.write_text(blocks[4] + "\n\n")                                 # (the answer as it came, "= " line included)
    cut.write_text(text[:len(text) // 2])
    second, blocks = client(f"list_commands\nplay b C3\ntamago-load_tree {missing}\ntamago-load_tree {cut}\nshowboard\n"
                            f"7 tamago-load_tree {good}\ntamago-dump_tree\ntamago-load_tree\nquit\n", False)
    assert "tamago-load_tree" in blocks[0].split("\n")
    assert blocks[2].startswith("? cannot load") and blocks[3].startswith("? cannot load")
    assert blocks[5] == f"=7 {json.loads(text)['tree']['num_nodes']}"
    assert blocks[6] == "= \n" + text
    assert blocks[7].startswith("? ")
    assert second.board.get_board_string() == first.board.get_board_string()
    assert second.board.get_komi() == 5.5 and second.superko is True and second.board.check_superko
    assert second.history == first.history
    first.mcts.close()
    second.mcts.close()

    # a dump taken straight after genmove: the board holds the generated move, the tree's root is the position before it
    np.random.seed(6)
    fourth, blocks = client("play b E5\ngenmove w\ntamago-dump_tree\nquit\n", True)
    text = blocks[2].split("\n")[1]
    after = tmp_path / "after.json"
    after.write_text(text)
    fifth, blocks = client(f"tamago-load_tree {after}\ntamago-dump_tree\nquit\n", True)
    assert blocks[0] == f"= {json.loads(text)['tree']['num_nodes']}" and blocks[1] == "= \n" + text
    assert fifth.board.get_board_string() == fourth.board.get_board_string() and fifth.history == fourth.history
    fourth.mcts.close()
    fifth.mcts.close()

    # a failed load leaves the session as it was
    third, blocks = client(f"play b C3\ntamago-load_tree {cut}\ntamago-dump_tree\nquit\n", False)
    state = json.loads(blocks[2].split("\n")[1])
    assert blocks[1].startswith("? ") and len(state["move_history"]) == 1 and state["tree"]["num_nodes"] == 0
    assert third.superko is False and third.board.get_komi() == 7.0
