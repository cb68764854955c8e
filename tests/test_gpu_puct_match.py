"""PUCT matches in lock-step on the device (tamago_amd/selfplay/puct_match.py, tg_search_best_moves) against the CPU oracle's
PUCT match game (tests/_puct_match_cases.py): byte-identical records, results and final streams on 1, 2 and 3 boards, the
one-child roots inside natural games, resignation of each colour and its switch, the swapped leg, a game against the product's
own one-tree MCTSTree, DualNets across launch shapes, 13x13, the read-out kernel alone on the hard trees, and the RL loop's gate."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import _puct_match_cases as pc
from tests._match_cases import make_net
from tests._puct_match_cases import S301, S302

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3, 6)


def _read(d, index):
    return open(os.path.join(d, f"{index}.sgf"), encoding="utf-8").read()


def _setups(black=S301, white=S302, black_search=pc.BLACK_SEARCH, white_search=pc.WHITE_SEARCH):
    from tamago_amd.selfplay.puct_match import EngineSetup
    return EngineSetup(make_net(black), *black_search), EngineSetup(make_net(white), *white_search)


def _check_games(out, games, d, a_is_black=None):
    """Records, per-game results and final streams of a match against oracle games (text, (moves, ending), numpy state)."""
    a_is_black = a_is_black or [True] * len(games)
    want = [pc.oracle_result(text, *end, a_is_black=side) for (text, end, _), side in zip(games, a_is_black)]
    got = [{k: r[k] for k in ("winner", "is_resign", "moves", "a_is_black")} for r in out["results"]]
    assert got == want
    for i, (text, _, state) in enumerate(games):
        assert _read(d, i) == text, i
        assert pc.same_stream(out["results"][i]["stream"], state), i
    return want


def _check_tally(out, want):
    from tamago_amd.selfplay.match import rating, tally
    counts = tally(want)
    for key in ("games", "wins_a", "wins_b", "draws", "unfinished", "as_black", "as_white", "resignations", "mean_length"):
        assert out[key] == counts[key], key
    for key, value in rating(counts["wins_a"], counts["wins_b"], counts["draws"]).items():
        assert out[key] == value, key


def test_the_oracle_games_are_the_cases_the_tests_need():
    """Two passes, the move limit, a short game; one-child roots followed by searched moves of the same game (seeds 1, 3) and
    at a game's end only (seed 2)."""
    games = {seed: pc.oracle_puct_game(seed, S301, S302) for seed in SEEDS}
    assert [games[s][1] for s in SEEDS] == [(96, "passes"), (128, "passes"), (162, "limit"), (32, "passes")]
    assert "RE[B+12.0]" in games[1][0] and "RE[B+55.0]" in games[2][0] and "RE[0]" in games[3][0] and "RE[B+3.0]" in games[6][0]
    assert pc.one_child_plies(1) == [91, 95] and pc.one_child_plies(3) == [116, 148] and pc.one_child_plies(2) == [127]
    assert "C[" not in games[1][0] and "PB[A]PW[B]" in games[1][0]


@pytest.mark.parametrize("boards", [1, 2, 3])
def test_lockstep_games_equal_the_oracle_games(boards, tmp_path):
    """Seeds 1, 2, 3, 6 on 1, 2 and 3 boards: slots refill and wait for a black call, every game is the oracle's - SGF bytes,
    result and the stream at its end (a one-child root that searched and kept its draws would move it)."""
    from tamago_amd.selfplay.puct_match import puct_match
    games = [pc.oracle_puct_game(seed, S301, S302) for seed in SEEDS]
    out = puct_match(*_setups(), 4, boards=boards, seeds=list(SEEDS), save_dir=str(tmp_path))
    want = _check_games(out, games, tmp_path)
    _check_tally(out, want)
    assert out["games"] == 4 and [r["index"] for r in out["results"]] == [0, 1, 2, 3] and [r["seed"] for r in out["results"]] == list(SEEDS)
    assert out["unfinished"] == 1 and out["wins_a"] == 3
    assert out["slot_calls"] == out["calls"] * boards and out["moves"] == 96 + 128 + 162 + 32
    assert out["one_child_roots"] == 5
    assert out["leaf_evals"] > 0 and "unique_leaves" not in out


@pytest.mark.parametrize("black,white,loser,ply", [(("despair", 301, 60), S302, "B", 138), (S301, ("despair", 302, 65), "W", 111)])
def test_resignation_of_each_colour_and_its_switch(black, white, loser, ply, tmp_path):
    """A crafted evaluator (Despair) makes its user resign: the resigning move is neither played nor recorded.  With
    resign_threshold 0.0 the same pair plays on."""
    from tamago_amd.selfplay.puct_match import puct_match
    resigned = pc.oracle_puct_game(1, black, white)
    played_on = pc.oracle_puct_game(1, black, white, resign_threshold=0.0)
    assert resigned[1] == (ply, "resign") and ply % 2 == (0 if loser == "B" else 1)
    assert ("RE[W+R]" if loser == "B" else "RE[B+R]") in resigned[0]
    assert played_on[1][1] == "passes" and played_on[1][0] > ply
    d1, d2 = tmp_path / "resign", tmp_path / "on"
    out = puct_match(*_setups(black, white), 1, boards=1, seeds=[1], save_dir=str(d1))
    _check_tally(out, _check_games(out, [resigned], d1))
    assert out["resignations"] == 1 and out["results"][0]["moves"] == ply
    out = puct_match(*_setups(black, white), 1, boards=1, seeds=[1], save_dir=str(d2), resign_threshold=0.0)
    _check_tally(out, _check_games(out, [played_on], d2))
    assert out["resignations"] == 0


def test_the_swapped_leg_equals_its_oracle_game(tmp_path):
    """Seed 6 from both sides: the second leg is the oracle game with the setups - network, visits and batch - exchanged."""
    from tamago_amd.selfplay.puct_match import puct_match
    first = pc.oracle_puct_game(6, S301, S302)
    second = pc.oracle_puct_game(6, S302, S301, black_search=pc.WHITE_SEARCH, white_search=pc.BLACK_SEARCH, names=("B", "A"))
    assert "PB[B]PW[A]" in second[0] and second[0] != first[0].replace("PB[A]PW[B]", "PB[B]PW[A]")
    out = puct_match(*_setups(), 1, boards=1, seeds=[6], swap=True, save_dir=str(tmp_path))
    want = _check_games(out, [first, second], tmp_path, a_is_black=[True, False])
    _check_tally(out, want)
    assert out["games"] == 2 and [r["index"] for r in out["results"]] == [0, 1] and [r["seed"] for r in out["results"]] == [6, 6]
    assert out["as_black"]["wins_a"] + out["as_black"]["wins_b"] + out["as_black"]["draws"] + out["as_black"]["unfinished"] == 1
    assert out["decided"] == out["wins_a"] + out["wins_b"] + out["draws"]


def test_a_game_equals_the_one_tree_search_move_by_move(tmp_path):
    """Independent of the oracle: equal setups (StubNet 301, 26 visits, batch 8) against a loop of the product's own one-tree
    MCTSTree.search_best_move under STRICT_PLAYOUT on a host GoBoard after one np.random.seed - moves, ending and numpy's
    state afterwards."""
    from tamago_amd.board.constant import PASS, RESIGN
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.board.stone import Stone
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    seed, visits, batch = 1, 26, 8
    saved = np.random.get_state()
    try:
        np.random.seed(seed)
        board = GoBoard(board_size=9, komi=7.0, check_superko=False)
        tree = MCTSTree(make_net(S301), tree_size=64, batch_size=batch)
        color, passes, moves, ending = Stone.BLACK, 0, [], "limit"
        for _ in range(2 * 81):
            pos = tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, visits))
            if pos == RESIGN:
                ending = "resign"
                break
            board.put_stone(pos, color)
            moves.append((1 if color == Stone.BLACK else 2, int(pos)))
            passes = passes + 1 if pos == PASS else 0
            color = Stone.get_opponent_color(color)
            if passes == 2:
                ending = "passes"
                break
        state = np.random.get_state()
        score = board.count_score() - board.get_komi()
    finally:
        np.random.set_state(saved)
    import re
    from tamago_amd.board.coordinate import Coordinate
    net = make_net(S301)
    out = puct_match(EngineSetup(net, visits, batch), EngineSetup(net, visits, batch), 1, boards=1, seeds=[seed],
                     save_dir=str(tmp_path))
    played = re.findall(r";([BW])\[([a-z]{2})\]", _read(tmp_path, 0))
    coord = Coordinate(9)
    assert played == [("B" if c == 1 else "W", coord.convert_to_sgf_format(p)) for c, p in moves]
    assert len(moves) >= 20
    result = out["results"][0]
    assert result["moves"] == len(moves) and result["is_resign"] == (ending == "resign")
    assert (result["winner"] is None) == (ending == "limit")
    if ending == "passes":
        assert result["score"] == score
    assert pc.same_stream(result["stream"], state)


def test_dualnets_play_the_same_games_on_four_boards_and_on_one(tmp_path):
    """Two random-init DualNets, 48 visits in mini-batches of 16 against 8, chained launches on the device: the records do
    not depend on the boards that share the launches.  Counts only while no f16 range fallback was taken - asserted, not
    skipped."""
    from tests import _match_games as mg
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    net_a, net_b = mg.two_nets()
    setups = (EngineSetup(net_a, 48, 16), EngineSetup(net_b, 48, 8))
    wide, solo = tmp_path / "four", tmp_path / "one"
    out4 = puct_match(*setups, 4, boards=4, seeds=[1, 2, 3, 4], save_dir=str(wide))
    out1 = puct_match(*setups, 4, boards=1, seeds=[1, 2, 3, 4], save_dir=str(solo))
    assert out4["range_fallbacks"] == 0 and out1["range_fallbacks"] == 0, "an f16 range fallback was taken: the comparison does not count"
    for i in range(4):
        assert _read(wide, i) == _read(solo, i), i
        a, b = out4["results"][i], out1["results"][i]
        assert {k: a[k] for k in ("winner", "is_resign", "moves", "score")} == {k: b[k] for k in ("winner", "is_resign", "moves", "score")}
        assert pc.same_stream(a["stream"], ("MT19937", b["stream"][0], b["stream"][1], 0, 0.0)), i
        assert a["moves"] >= 10


def test_a_13x13_game_equals_the_oracle_game(tmp_path):
    """Nothing is hard-wired to 9: one 13x13 game at 16 visits (batches 8 and 6)."""
    from tamago_amd.selfplay.puct_match import puct_match
    game = pc.oracle_puct_game(1, S301, S302, black_search=(16, 8), white_search=(16, 6), size=13)
    assert game[1][1] in ("passes", "resign") and game[1][0] >= 10 and "SZ[13]" in game[0]
    out = puct_match(*_setups(black_search=(16, 8), white_search=(16, 6)), 1, size=13, boards=1, seeds=[1], save_dir=str(tmp_path))
    _check_tally(out, _check_games(out, [game], tmp_path))


# ---- tg_search_best_moves alone ----------------------------------------------------------------------------------------------
def _host_rule(stats, tree, threshold):
    """The record tg_search_best_moves must write, off tg_search_read_root_stats: the end of search_best_move."""
    n = int(stats["num_children"][tree])
    visits, value_sum = stats["children_visits"][tree], stats["children_value_sum"][tree]
    best = 0 if n == 1 else int(np.argmax(visits[:n]))
    value = 0.5 if visits[best] == 0 else value_sum[best] / np.float64(visits[best])
    move = 0 if n == 1 else (-1 if value < threshold else int(stats["action"][tree][best]))
    return {"num_children": n, "move": move, "best": best, "visits": int(visits[best]), "value_sum": float(value_sum[best]),
            "node_visits": int(stats["node_visits"][tree]), "status": 0}, float(value)


def _record(row):
    return {name: (float(row[name]) if name == "value_sum" else int(row[name])) for name in row.dtype.names}


def _hard_names():
    from tests import _hard_trees as ht
    return [n for n in ht.LINE + ht.TIES if ht.records()[n]["kind"] == "puct"]


@pytest.mark.parametrize("name", _hard_names())
def test_best_moves_on_the_hard_trees_equal_the_host_rule(name):
    """Exact visit ties, zero-visit children, values of exactly 0 / 0.5 / 1: every record field equals the host rule applied
    to tg_search_read_root_stats, at the reference's threshold, with resignation off, at a threshold EQUAL to the best
    child's exact quotient (<, not <=: no resignation) and one ulp above it (resignation); nothing is played with play = 0.
    With play = 1 the position equals tg_search_play of the same move."""
    from tests import _hard_trees as ht
    from tests.helpers import load_npz
    from tamago_amd.board.go_board import GoBoard
    rec = ht.records()[name]
    tree, _, _ = ht.product_search(rec, with_leaves=False)
    engine = tree._engine
    stats = engine.read_root_stats()
    before = engine.read_positions()
    _, value = _host_rule(stats, 0, 0.05)
    thresholds = [0.05, 0.0, 1.0, value, float(np.nextafter(value, 2.0))]
    for threshold in thresholds:
        want, _ = _host_rule(stats, 0, threshold)
        got = engine.best_moves(threshold, False)
        assert _record(got[0]) == want, threshold
    assert _host_rule(stats, 0, value)[0]["move"] != -1 or stats["num_children"][0] == 1
    if stats["num_children"][0] > 1:
        assert _host_rule(stats, 0, float(np.nextafter(value, 2.0)))[0]["move"] == -1
    after = engine.read_positions()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    state0 = engine.read_root_state(0)
    # RESIGN plays nothing (a threshold above every value)
    got = engine.best_moves(2.0, True)
    if stats["num_children"][0] > 1:
        assert int(got[0]["move"]) == -1
        assert all(np.array_equal(a, b) for a, b in zip(before, engine.read_positions()))
    # play = 1 against tg_search_play on the same root
    got = engine.best_moves(0.0, True)
    move = int(got[0]["move"])
    assert move == _host_rule(stats, 0, 0.0)[0]["move"] and move >= 0
    played = (engine.read_positions(), engine.read_root_state(0))
    size = rec["size"]
    brd = load_npz(f"board_s{size}.npz")
    board = GoBoard(size, 7.0, rec["superko"])
    for mv, c in zip(brd["g0_move"][:rec["ply"]], brd["g0_color"][:rec["ply"]]):
        board.put_stone(int(mv), int(c))
    engine.set_root(0, board, rec["color"])
    engine.play([move])
    again = (engine.read_positions(), engine.read_root_state(0))
    assert all(np.array_equal(a, b) for a, b in zip(played[0], again[0]))
    for key in ("hash", "moves", "ko_pos", "ko_move", "prev", "prevprev", "to_move", "hist_len"):
        assert played[1][key] == again[1][key], key
    assert np.array_equal(played[1]["history"], again[1]["history"])
    assert played[1]["moves"] == state0["moves"] + 1 and played[1]["to_move"] == 3 - state0["to_move"]


@pytest.fixture(scope="module")
def three_trees():
    """Three searched trees of one engine (StubNet, 20 visits in batches of 6 and 2) on different positions."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.board.stone import Stone
    from tamago_amd.mcts.engine import SearchEngine, evaluator_for
    engine = SearchEngine(9, 3, 64, 6, evaluator_for(make_net(S301)))
    boards = []
    for k in range(3):
        board = GoBoard(board_size=9, komi=7.0, check_superko=False)
        color = Stone.BLACK
        for pos in [(3 + k) + 4 * 11, 5 + (6 - k) * 11][:k + 1]:
            board.put_stone(pos, color)
            color = Stone.get_opponent_color(color)
        boards.append((board, color))
        engine.set_root(k, board, color, np.random.RandomState(40 + k).get_state())
    engine.root_eval(use_logit=False)
    for leaves in (6, 6, 6, 2):
        engine.puct_batch(leaves)
    yield engine, boards
    engine.close()


def test_a_tree_that_sits_out_is_left_alone(three_trees):
    """sit_out: the tree's record is zero but for its status and its position is untouched by play = 1; the others are
    decided and played, each by its own root."""
    from tamago_amd.mcts.engine import BEST_SAT_OUT
    engine, _ = three_trees
    stats = engine.read_root_stats()
    cells0, moves0, to_move0 = engine.read_positions()
    got = engine.best_moves(0.0, True, sit_out=[0, 1, 0])                      # (resignation off: every decided tree plays)
    assert _record(got[1]) == {"num_children": 0, "move": 0, "best": 0, "visits": 0, "value_sum": 0.0, "node_visits": 0,
                               "status": BEST_SAT_OUT}
    for tree in (0, 2):
        want, _ = _host_rule(stats, tree, 0.0)
        assert _record(got[tree]) == want and want["node_visits"] >= 20 and want["move"] >= 0
    cells1, moves1, to_move1 = engine.read_positions()
    assert np.array_equal(cells1[1], cells0[1]) and moves1[1] == moves0[1] and to_move1[1] == to_move0[1]
    for tree in (0, 2):
        move = int(got[tree]["move"])
        assert moves1[tree] == moves0[tree] + 1 and to_move1[tree] == 3 - to_move0[tree]
        assert move == 0 or (cells1[tree][move] == to_move0[tree] and cells0[tree][move] == 0)


def test_argument_errors_through_the_abi(three_trees):
    from tamago_amd import lib as tl
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.board.stone import Stone
    from tamago_amd.mcts.engine import BEST_MOVE, SearchEngine, evaluator_for
    engine, _ = three_trees
    lib, out = engine.lib, np.zeros(3, dtype=BEST_MOVE)
    before = engine.read_positions()
    assert lib.tg_search_best_moves(None, 0.05, 0, None, out.ctypes.data, None) == -1
    assert lib.tg_search_best_moves(engine.handle, 0.05, 0, None, None, None) == -1 and b"null" in lib.tg_last_error()
    assert lib.tg_search_best_moves(engine.handle, 0.05, 2, None, out.ctypes.data, None) == -1 and b"play 2" in lib.tg_last_error()
    assert lib.tg_search_best_moves(engine.handle, float("nan"), 1, None, out.ctypes.data, None) == -1
    assert b"not a number" in lib.tg_last_error()
    assert all(np.array_equal(a, b) for a, b in zip(before, engine.read_positions()))
    fresh = SearchEngine(9, 1, 32, 4, evaluator_for(make_net(S301)))
    try:
        fresh.set_root(0, GoBoard(board_size=9, komi=7.0, check_superko=False), Stone.BLACK, np.random.RandomState(1).get_state())
        one = np.zeros(1, dtype=BEST_MOVE)
        assert lib.tg_search_best_moves(fresh.handle, 0.05, 1, None, one.ctypes.data, fresh._stream()) == -3   # TG_ERR_STATE
        assert b"no expanded root" in lib.tg_last_error()
        with pytest.raises(tl.TamagoHipError):
            fresh.best_moves(0.05, False)
    finally:
        fresh.close()
    scores = np.zeros(1, dtype=np.int32)
    assert lib.tg_search_count_scores(None, 9, 1, scores.ctypes.data) == -1
    cells = np.ascontiguousarray(before[0][:1])
    assert lib.tg_search_count_scores(cells.ctypes.data, 0, 1, scores.ctypes.data) == -1


def test_count_scores_equal_the_board_s_count_score(three_trees):
    engine, boards = three_trees
    want = [board.count_score() for board, _ in boards]
    got = engine.count_scores(np.stack([np.asarray(board.cells, dtype=np.uint8) for board, _ in boards]))
    assert [int(v) for v in got] == want


def test_rl_loop_gates_a_generation_with_a_puct_match(tmp_path, monkeypatch):
    """tools/rl_loop.py with gate_search puct and gate_visits > 0: the trained network against the one before under PUCT
    search; gate_search gumbel keeps the Gumbel gate."""
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import rl_loop
    import tamago_amd.nn.data_generator as dg
    monkeypatch.setattr(dg, "BATCH_SIZE", 32)
    torch.manual_seed(11)
    np.random.seed(11)
    lines = []
    rl_loop.run_generation(str(tmp_path), 0, 16, 16, 16, 32, log=lines.append, gate_games=4, gate_visits=16, gate_search="puct",
                           gate_batch=8)
    gate = [line for line in lines if "new against previous" in line]
    assert len(gate) == 1 and "over 8 PUCT games at 16 visits in mini-batches of 8" in gate[0] and "Elo" in gate[0], lines
    with pytest.raises(ValueError, match="gate_search"):
        rl_loop.run_generation(str(tmp_path), 1, 16, 16, 16, 32, log=lines.append, gate_games=4, gate_visits=16, gate_search="mcts")
