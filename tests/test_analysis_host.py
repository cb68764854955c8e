"""CPU checks of the batch analyser's host side (tamago_amd/mcts/analysis.py, python -m tamago_amd.analyze)."""
import json
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(text):
    from tamago_amd.sgf.reader import SGFReader
    return SGFReader(text, 9, literal=True)


def test_positions_of_a_record_include_passes_and_the_final_position():
    from tamago_amd.board.constant import PASS
    from tamago_amd.board.stone import Stone
    from tamago_amd.mcts.analysis import game_positions
    sgf = _record("(;GM[1]SZ[9]KM[6.5];B[ee];W[cc];B[];W[gg])")
    pos = game_positions(sgf, False, "g")
    assert [p.move_number for p in pos] == [1, 2, 3, 4, 5]
    assert [p.color for p in pos] == [Stone.BLACK, Stone.WHITE, Stone.BLACK, Stone.WHITE, Stone.BLACK]
    assert pos[2].played == PASS and pos[4].played is None
    assert [p.board.moves for p in pos] == [1, 2, 3, 4, 5]
    assert pos[0].board.get_komi() == 6.5
    assert int(pos[4].board.cells[pos[0].board.coordinate.convert_from_gtp_format("E5")]) == 1
    assert int(pos[0].board.cells[pos[0].board.coordinate.convert_from_gtp_format("E5")]) == 0
    sizes = {}
    for size in (13, 19):
        sizes[size] = game_positions(_record(f"(;SZ[{size}];B[aa])"))[1].board.board_size
    assert sizes == {13: 13, 19: 19}
    with pytest.raises(ValueError, match="board size 11"):
        game_positions(_record("(;SZ[11];B[aa])"))


def test_game_seeds_depend_on_the_position_only():
    from tamago_amd.mcts.analysis import game_seeds
    assert game_seeds(7, 4) == [7, 8, 9, 10]
    assert game_seeds(0, 0) == []


def test_chunk_planning():
    from tamago_amd.mcts.analysis import plan_chunks, default_max_trees, pool_bytes_per_node
    assert plan_chunks(0, 8) == (0, [])
    assert plan_chunks(5, 8) == (5, [(0, 5)])
    assert plan_chunks(100, 64) == (50, [(0, 50), (50, 100)])
    assert plan_chunks(7, 1) == (1, [(i, i + 1) for i in range(7)])
    trees, chunks = plan_chunks(53, 7)
    assert trees <= 7 and chunks[0][0] == 0 and chunks[-1][1] == 53
    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    with pytest.raises(ValueError):
        plan_chunks(3, 0)
    assert pool_bytes_per_node(9) == 3148 and pool_bytes_per_node(19) == 13788
    assert default_max_trees(9, 1000) == 2048
    assert default_max_trees(19, 1600) == (8 << 30) // (1616 * 13788)
    assert default_max_trees(19, 10 ** 7) == 1


def _hand_built():
    from tamago_amd.mcts.analysis import PositionAnalysis
    status = [{"move": "D5", "visits": 30, "winrate": 0.625, "prior": 0.5, "lcb": 0.625, "order": 0, "pv": "D5 C4"},
              {"move": "C4", "visits": 20, "winrate": 0.5, "prior": 0.25, "lcb": 0.5, "order": 1, "pv": "C4"},
              {"move": "E3", "visits": 9, "winrate": 0.25, "prior": 0.125, "lcb": 0.25, "order": 2, "pv": "E3 D5"},
              {"move": "F6", "visits": 1, "winrate": 0.0, "prior": 0.125, "lcb": 0.0, "order": 3, "pv": "F6"}]
    return PositionAnalysis(best_move=59, visits=61, value_sum=30.5, status=status, board_size=9)


def test_position_analysis_strings():
    a = _hand_built()
    assert a.best_move_gtp() == "D5"
    assert a.winrate == 0.5
    assert a.lz().startswith("info move D5 visits 30 winrate 6250 prior 5000 lcb 6250 order 0 pv D5 C4 info move C4 ")
    assert a.lz().endswith("\n")
    cg = json.loads(a.cgos())
    assert cg == {"winrate": 0.5, "visits": 61, "moves": a.status}
    assert a.move_stats("C4") == (20, 0.5, 1) and a.move_stats("A1") == (0, None, None)


def test_jsonl_record_and_sgf_comment():
    from tamago_amd.mcts.analysis import GameAnalysis, game_positions
    pos = game_positions(_record("(;SZ[9];B[dd];W[ee])"), False, "g.sgf")
    g = GameAnalysis(pos[1], _hand_built())                      # white to move, played E5
    rec = g.record()
    assert rec == {"game": "g.sgf", "move_number": 2, "color": "W", "best": "D5", "visits": 61, "winrate": 0.5,
                   "played": "E5", "played_visits": 0, "played_winrate": None, "played_rank": None,
                   "moves": _hand_built().status}
    assert json.loads(json.dumps(rec)) == rec
    assert g.comment() == ("W to move, winrate 50.0%, best D5 (30 visits), played E5 (0 visits, winrate -), "
                           "top: D5 30 62.5%, C4 20 50.0%, E3 9 25.0%")
    last = GameAnalysis(pos[2], _hand_built()).record()
    assert last["played"] is None and last["played_rank"] is None and last["color"] == "B"
    g0 = GameAnalysis(pos[0], _hand_built())
    g0.position.played = g0.position.board.coordinate.convert_from_gtp_format("C4")
    assert "played C4 (20 visits, winrate 50.0%)" in g0.comment()


def test_annotated_sgf_reads_back():
    from tamago_amd.mcts.analysis import GameAnalysis, annotated_sgf, game_positions
    text = "(;SZ[9]KM[6.5]PB[x]PW[y];B[dd];W[];B[ee])"
    sgf = _record(text)
    pos = game_positions(sgf)
    out = annotated_sgf([GameAnalysis(p, _hand_built()) for p in pos], sgf)
    back = _record(out)
    assert back.get_n_moves() == 3 and back.komi == 6.5
    assert [back.get_move_data(i) for i in range(3)] == [sgf.get_move_data(i) for i in range(3)]
    assert [back.get_color(i) for i in range(3)] == [sgf.get_color(i) for i in range(3)]
    assert back.get_comment(0).startswith("B to move, winrate 50.0%")
    assert back.get_comment(1).startswith("W to move")


def test_cli_options_and_refusals(tmp_path, capsys):
    from tamago_amd import analyze
    args = analyze.parser().parse_args(["a.sgf", "b.sgf", "--visits", "200", "--batch-size", "8", "--trees", "64",
                                        "--superko", "yes", "--cgos-mode", "0", "--seed", "3", "--pv-depth", "4",
                                        "--format", "lz", "--sgf-out", "out"])
    assert args.games == ["a.sgf", "b.sgf"] and args.visits == 200 and args.batch_size == 8 and args.trees == 64
    assert args.superko is True and args.cgos_mode is False and args.seed == 3 and args.pv_depth == 4
    assert args.format == "lz" and args.sgf_out == "out"
    d = analyze.parser().parse_args(["a.sgf"])
    assert (d.visits, d.batch_size, d.trees, d.format, d.pv_depth, d.seed) == (1000, 16, None, "jsonl", 32, 0)
    for bad in (["a.sgf", "--format", "xml"], ["a.sgf", "--superko", "maybe"], ["a.sgf", "--visits", "0"], []):
        with pytest.raises(SystemExit):
            analyze.parser().parse_args(bad)
    odd = tmp_path / "odd.sgf"
    odd.write_text("(;SZ[11];B[aa])")
    with pytest.raises(SystemExit) as exc:
        analyze.main([str(odd)])
    assert exc.value.code == 2 and "board size 11" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        analyze.main([str(tmp_path / "missing.sgf")])


class _FakeNode:
    def __init__(self, visits, action, children_visits, children_index):
        from tamago_amd.mcts.node import MCTSNode
        n = MCTSNode(len(action))
        n.node_visits = visits
        n.num_children = len(action)
        n.action = list(action)
        n.children_visits = np.array(children_visits, np.int32)
        n.children_index = np.array(children_index, np.int32)
        self.node = n


def test_host_pv_continuation():
    from tamago_amd.mcts.engine import continue_pv
    tree = {5: _FakeNode(9, [10, 11, 12], [1, 4, 4], [6, 7, 8]).node,      # tie: first index wins -> 11, node 7
            7: _FakeNode(4, [20, 21], [0, 0], [9, -1]).node,               # all zero: child 0 -> 20, node 9
            9: _FakeNode(2, [30, 31], [0, 1], [-1, -1]).node}              # -> 31, index -1: stop
    reads = []

    def read_node(i):
        reads.append(i)
        return tree[i]

    assert continue_pv([1, 2], 5, read_node) == [1, 2, 11, 20, 31]
    assert reads == [5, 7, 9]
    tree[7] = _FakeNode(0, [20], [3], [9]).node                             # no visits: stop without appending
    assert continue_pv([1], 5, read_node) == [1, 11]
