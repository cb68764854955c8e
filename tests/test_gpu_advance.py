"""Roots advanced by a move on the device (tg_search_advance) and the root expansion of the fresh trees only
(tg_search_root_planes_fresh), DESIGN 4.15: four trees searched to 60 visits at batch 8, then advanced by the best move (an
expanded child), a legal move whose child is unexpanded, PASS and -1 - node arrays against the numpy compaction of the pool
read before the call, root positions against a host GoBoard, halt words, stream cursors and the records."""
import numpy as np
import pytest

from tests._tree_reuse import compact_arrays

pytestmark = pytest.mark.gpu

OPENING = [(40, 1), (41, 2), (52, 1), (30, 2), (63, 1)]
VISITS, BATCH, SALT = 60, 8, 9


def _board(plies):
    from tamago_amd.board.go_board import GoBoard
    board = GoBoard(9, 7.0, True)
    for move, color in OPENING[:plies]:
        board.put_stone(move, color)
    return board, 1 + plies % 2


def _stream(eng, t):
    state = eng.streams[t].final_state()
    return int(state[2]), np.asarray(state[1], dtype=np.uint32).tobytes()


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_advance_and_fresh_root_expansion():
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.engine import ADVANCE_LEFT_ALONE, HostEvaluator, SearchEngine
    from tests.test_gpu_tree_reuse import _read_tree
    device = torch.device("cuda", 0)
    eng = SearchEngine(9, 4, 128, BATCH, HostEvaluator(StubNet(salt=SALT), device), check_superko=True)
    boards, colors = zip(*(_board(t + 1) for t in range(4)))
    for t in range(4):
        eng.set_root(t, boards[t], colors[t], np.random.RandomState(100 + t).get_state())
    eng.root_eval()
    for leaves in [BATCH] * (VISITS // BATCH) + [VISITS % BATCH]:
        eng.puct_batch(leaves)
    n = eng.num_nodes()
    before = [_read_tree(eng, t, int(n[t])) for t in range(4)]
    streams = [_stream(eng, t) for t in range(4)]
    roots = [{k: v[0] for k, v in tr.items()} for tr in before]
    assert all(int(r["node_visits"]) == VISITS for r in roots)
    nc = [int(r["num_children"]) for r in roots]
    best = int(np.argmax(roots[0]["children_visits"][:nc[0]]))
    unexpanded = [i for i in range(nc[1]) if roots[1]["children_index"][i] < 0 and roots[1]["action"][i] != 0]
    pass_edge = [i for i in range(nc[2]) if roots[2]["action"][i] == 0]
    assert roots[0]["children_index"][best] > 0 and unexpanded and len(pass_edge) == 1
    moves = [int(roots[0]["action"][best]), int(roots[1]["action"][unexpanded[len(unexpanded) // 2]]), 0, -1]
    child = [int(roots[0]["children_index"][best]), -1, int(roots[2]["children_index"][pass_edge[0]]), -1]

    eng.set_halt([1, 1, 1, 1])
    records = eng.advance(moves)
    halted, _ = eng.read_halt()
    assert halted.tolist() == [False, False, False, True]            # cleared for the advanced trees only
    after_n = eng.num_nodes()
    for t in range(3):
        boards[t].put_stone(moves[t], colors[t])
        state = eng.read_root_state(t)
        board = boards[t]
        assert state["hash"] == int(board.hash) and state["moves"] == board.moves
        assert (state["ko_pos"], state["ko_move"]) == (board.ko_pos, board.ko_move)
        assert (state["prev"], state["prevprev"]) == (board.prev_move(1), board.prev_move(2))
        assert state["to_move"] == 3 - colors[t] and state["hist_len"] == board.moves
        assert np.array_equal(state["history"], np.asarray(board.rec_hash[:board.moves], dtype=np.uint64))
    cells, _, to_move = eng.read_positions()
    for t in range(3):
        assert np.array_equal(cells[t], np.asarray(boards[t].cells, dtype=np.uint8)) and int(to_move[t]) == 3 - colors[t]
    kept = {}
    for t in range(4):
        rec = records[t]
        if t == 3:
            assert int(rec["status"]) == ADVANCE_LEFT_ALONE and int(rec["kept_visits"]) == -1
            assert int(after_n[3]) == int(n[3]) and _stream(eng, 3) == streams[3]
            _same(_read_tree(eng, 3, int(n[3])), before[3])
            assert eng.read_root_state(3)["moves"] == boards[3].moves
            continue
        assert int(rec["status"]) == 0
        if child[t] < 0:
            assert (int(rec["kept_visits"]), int(rec["kept_nodes"]), int(rec["num_children"])) == (-1, 0, 0)
            assert int(after_n[t]) == 0
            continue
        want = compact_arrays(before[t], child[t])
        assert int(after_n[t]) == len(want["parent"]) == int(rec["kept_nodes"])
        assert int(rec["kept_visits"]) == int(before[t]["node_visits"][child[t]])
        assert int(rec["num_children"]) == int(before[t]["num_children"][child[t]]) == int(eng.root_children[t])
        kept[t] = _read_tree(eng, t, int(after_n[t]))
        _same(kept[t], want)
    assert 0 in kept and int(after_n[1]) == 0                          # an expanded child was kept, an unexpanded one was not
    assert eng.node_bound >= max(int(v) for v in after_n)
    assert all(_stream(eng, t) == streams[t] for t in range(4))      # an advance draws nothing

    # ---- the root expansion of the fresh trees only ----
    eng.root_eval_fresh()
    halted, _ = eng.read_halt()
    assert halted.tolist() == [False, False, False, True]
    now_n = eng.num_nodes()
    fresh = [t for t in range(3) if t not in kept]
    for t, tree in kept.items():
        assert int(now_n[t]) == int(after_n[t]) and _stream(eng, t) == streams[t]
        _same(_read_tree(eng, t, int(now_n[t])), tree)
    _same(_read_tree(eng, 3, int(n[3])), before[3])
    assert _stream(eng, 3) == streams[3]
    for t in fresh:
        ref = SearchEngine(9, 1, 16, BATCH, HostEvaluator(StubNet(salt=SALT), device), check_superko=True)
        key = np.frombuffer(streams[t][1], dtype=np.uint32)
        ref.set_root(0, boards[t], 3 - colors[t], ("MT19937", key, streams[t][0], 0, 0.0))
        ref.root_eval()
        assert int(now_n[t]) == 1
        _same(_read_tree(eng, t, 1), _read_tree(ref, 0, 1))
        assert _stream(eng, t) == _stream(ref, 0) and _stream(eng, t) != streams[t]
        assert int(eng.root_children[t]) == int(ref.root_children[0]) == int(_read_tree(ref, 0, 1)["num_children"][0])
        ref.close()
    # every tree but the halted one searches on: consistent parent links, the kept visits topped up
    eng.puct_batch(BATCH)
    n2 = eng.num_nodes()
    for t in range(3):
        tr = _read_tree(eng, t, int(n2[t]))
        for i in range(1, int(n2[t])):
            assert tr["children_index"][tr["parent"][i]][tr["pedge"][i]] == i
        base = int(records[t]["kept_visits"]) if t in kept else 0
        assert int(tr["node_visits"][0]) == base + BATCH
    assert int(n2[3]) == int(n[3])
    eng.close()


def test_advance_refuses_bad_moves():
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd import lib as tl
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    eng = SearchEngine(9, 2, 32, 4, HostEvaluator(StubNet(salt=SALT), torch.device("cuda", 0)))
    board, color = _board(2)
    for t in range(2):
        eng.set_root(t, board, color, np.random.RandomState(t).get_state())
    eng.root_eval()
    for bad in (121, -2):
        with pytest.raises(tl.TamagoHipError, match="tg_search_advance"):
            eng.advance([bad, -1])
    with pytest.raises(tl.TamagoHipError, match="not empty"):           # a stone is there: not played, the sticky error set
        eng.advance([-1, OPENING[0][0]])
    assert eng.read_root_state(1)["moves"] == board.moves
    eng.close()
