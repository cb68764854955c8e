"""Host side of the search match (tamago_amd/selfplay/match.py): the slot-restart rule, the tally / score / Elo arithmetic, the
command line, the refusal of groups and lanes, the record's player names, and the oracle helper the GPU tests are held to."""
import math

import pytest

from tests.helpers import load_json


def test_slot_restart_rule_for_both_schemes_and_both_ending_parities():
    from tamago_amd.board.stone import Stone
    from tamago_amd.selfplay.match import first_mover, slot_may_start
    B, W = Stone.BLACK, Stone.WHITE
    # chained: a started slot sits out the coming call, which must be white's (its chain evaluates with black's network)
    assert first_mover(True) is W and slot_may_start(True, first_mover(True))
    assert slot_may_start(True, W) and not slot_may_start(True, B)
    # round trip / phase by phase: a started slot is searched in the coming call, which must be black's
    assert first_mover(False) is B and slot_may_start(False, first_mover(False))
    assert slot_may_start(False, B) and not slot_may_start(False, W)

    def calls_parked(chained, ended_on):
        """Calls a slot whose game ended on `ended_on`'s call spends before it may start its next game."""
        mover, parked = Stone.get_opponent_color(ended_on), 0
        while not slot_may_start(chained, mover):
            mover, parked = Stone.get_opponent_color(mover), parked + 1
        return parked

    assert calls_parked(True, B) == 0        # chained, ended on black's call: restarted at once, sits out white's call
    assert calls_parked(True, W) == 1        # chained, ended on white's call: one extra call
    assert calls_parked(False, W) == 0       # round trip, ended on white's call: the next call is black's
    assert calls_parked(False, B) == 1


@pytest.mark.parametrize("knobs,text,chained", [(None, "0", True), ("1", "0", False), ("1", "1abc", True), ("1", None, True)])
def test_the_scheme_is_the_librarys_answer_not_the_environments(knobs, text, chained):
    """TG_SP_CHAIN is a debug knob: the library ignores it unless TG_DEBUG_KNOBS=1 and reads it as a C integer.  The driver
    asks the library (tg_selfplay_chained) and never reads the variable itself - with TG_SP_CHAIN=0 and no TG_DEBUG_KNOBS the
    handles run chained, and a driver that believed the environment would play the colours the wrong way round.  (The library
    reads TG_DEBUG_KNOBS once per process: a child process per case.)"""
    import inspect
    import os
    import subprocess
    import sys
    import tamago_amd.selfplay.match as match
    assert "environ" not in inspect.getsource(match)
    env = dict(os.environ)
    for key, value in (("TG_DEBUG_KNOBS", knobs), ("TG_SP_CHAIN", text)):
        env.pop(key, None)
        if value is not None:
            env[key] = value
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from tamago_amd import lib; from tamago_amd.selfplay.match import "
            "handle_is_chained; print('chained' if handle_is_chained(lib.load()) else 'round trip')")
    res = subprocess.run([sys.executable, "-c", code, root], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.strip().splitlines()[-1] == ("chained" if chained else "round trip")


def test_turns_alternate_and_ask_the_one_rule():
    from tamago_amd.board.stone import Stone
    from tamago_amd.selfplay.match import _Turns
    for chained, first in ((True, Stone.WHITE), (False, Stone.BLACK)):
        turns = _Turns(chained)
        assert turns.mover is first and turns.may_start()
        turns.flip()
        assert turns.mover is Stone.get_opponent_color(first) and turns.other is first and not turns.may_start()
        turns.flip()
        assert turns.mover is first and turns.may_start()


def _game(winner, a_is_black, moves=50, is_resign=False):
    return {"winner": winner, "is_resign": is_resign, "moves": moves, "a_is_black": a_is_black}


def test_tally_splits_by_colour_and_counts_draws_and_unfinished_games():
    from tamago_amd.selfplay.match import tally
    results = [_game("black", True, 40, True), _game("white", True, 60), _game("draw", True, 80), _game(None, True, 162),
               _game("black", False, 30), _game("white", False, 50, True), _game("white", False, 70), _game("draw", False, 90)]
    out = tally(results)
    assert out["games"] == 8
    assert (out["wins_a"], out["wins_b"], out["draws"], out["unfinished"]) == (3, 2, 2, 1)
    assert out["as_black"] == {"wins_a": 1, "wins_b": 1, "draws": 1, "unfinished": 1}
    assert out["as_white"] == {"wins_a": 2, "wins_b": 1, "draws": 1, "unfinished": 0}
    assert out["resignations"] == 2
    assert out["mean_length"] == (40 + 60 + 80 + 162 + 30 + 50 + 70 + 90) / 8
    assert tally([])["games"] == 0 and tally([])["mean_length"] == 0.0


def test_score_elo_and_interval():
    from tamago_amd.selfplay.match import rating
    r = rating(3, 1, 0)
    assert r["decided"] == 4 and r["score_a"] == 0.75
    assert r["elo"] == pytest.approx(400 * math.log10(3), abs=1e-9)          # 190.8
    half = 1.96 * math.sqrt(0.75 * 0.25 / 4)                                  # win / loss only: a binomial proportion
    assert r["elo_interval"][0] == pytest.approx(400 * math.log10((0.75 - half) / (0.25 + half)), abs=1e-9)
    assert r["elo_interval"][1] is None                                       # 0.75 + 0.42 leaves (0, 1)
    # draws count half and carry less variance than a win and a loss
    r = rating(40, 40, 20)
    assert r["score_a"] == 0.5 and r["elo"] == 0.0
    half = 1.96 * math.sqrt((80 * 0.25 / 100) / 100)
    assert r["elo_interval"][1] == pytest.approx(400 * math.log10((0.5 + half) / (0.5 - half)), abs=1e-9)
    assert r["elo_interval"][0] == pytest.approx(-r["elo_interval"][1], abs=1e-9)
    r = rating(60, 30, 10)
    assert r["score_a"] == pytest.approx(0.65) and r["elo"] == pytest.approx(400 * math.log10(0.65 / 0.35))
    assert r["elo_interval"][0] < r["elo"] < r["elo_interval"][1]
    # all wins / all losses: no finite Elo; only draws: level, an interval of width 0; nothing decided: nothing to say
    assert rating(5, 0, 0) == {"decided": 5, "score_a": 1.0, "elo": None, "elo_interval": [None, None]}
    assert rating(0, 5, 0)["score_a"] == 0.0 and rating(0, 5, 0)["elo"] is None
    assert rating(0, 0, 4) == {"decided": 4, "score_a": 0.5, "elo": 0.0, "elo_interval": [0.0, 0.0]}
    assert rating(0, 0, 0) == {"decided": 0, "score_a": None, "elo": None, "elo_interval": [None, None]}


def test_command_line_arguments():
    from tamago_amd.selfplay.match import parse_args
    from tamago_amd.selfplay.worker import SELF_PLAY_VISITS
    args = parse_args(["--black", "a.bin", "--white", "b.bin", "--games", "8"])
    assert (args.black, args.white, args.games, args.size, args.visits, args.boards, args.komi, args.swap, args.save_dir,
            args.unique_leaves) == ("a.bin", "b.bin", 8, 9, SELF_PLAY_VISITS, None, 7.0, False, None, False)
    args = parse_args(["--black", "a.bin", "--white", "b.bin", "--games", "8", "--size", "13", "--visits", "400", "--boards",
                       "4", "--komi", "6.5", "--swap", "true", "--save-dir", "out", "--unique-leaves", "yes"])
    assert (args.size, args.visits, args.boards, args.komi, args.swap, args.save_dir, args.unique_leaves) == \
        (13, 400, 4, 6.5, True, "out", True)
    with pytest.raises(SystemExit):
        parse_args(["--black", "a.bin", "--games", "8"])
    import tamago_amd.match as entry                                          # python -m tamago_amd.match
    assert entry.main is not None and entry.search_match is not None


def test_groups_and_lanes_are_refused():
    from tamago_amd.selfplay.match import search_match
    with pytest.raises(ValueError, match="one lock-step group"):
        search_match(object(), object(), 2, groups=2)
    with pytest.raises(ValueError, match="one lock-step group"):
        search_match(object(), object(), 2, lanes=2)
    with pytest.raises(ValueError, match="one entry per game"):
        search_match(object(), object(), 2, seeds=[1])


def test_record_spells_the_players_names_and_keeps_the_defaults():
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.board.stone import Stone
    from tamago_amd.sgf.selfplay_record import SelfPlayRecord
    named = SelfPlayRecord("", Coordinate(9), players=("gen-7", "gen-6")).to_sgf(Stone.BLACK, 7.0, True, 0.0)
    assert named == "(;FF[4]GM[1]SZ[9]\nAP[TamaGo]PB[gen-7]PW[gen-6]RE[B+R]KM[7.0]\n)"
    plain = SelfPlayRecord("", Coordinate(9)).to_sgf(Stone.WHITE, 7.0, False, -3.0)
    assert plain == "(;FF[4]GM[1]SZ[9]\nAP[TamaGo]PB[TamaGo-Black]PW[TamaGo-White]RE[W+3.0]KM[7.0]\n)"
    assert load_json("selfplay_games.json")["1,16"].startswith("(;FF[4]GM[1]SZ[9]\nAP[TamaGo]PB[TamaGo-Black]PW[TamaGo-White]RE[")


def test_oracle_match_game_with_one_evaluator_is_the_reference_selfplay_game():
    """The helper the GPU tests are held to, pinned to a game the reference's worker wrote: seed 1, salt 201, 16 simulations
    and the reference's never-resign draw (tests/test_gpu_selfplay.py)."""
    from oracle.stubnet import StubNet
    from tests._match_cases import oracle_match_game, reference_never_resign
    net = StubNet(201)
    text, (moves, ending) = oracle_match_game(1, net, net, 16, 9, reference_never_resign(1))
    assert text == load_json("selfplay_games.json")["1,16"]
    assert ending == "passes" and text.count(";B[") + text.count(";W[") == moves


def test_despair_makes_its_user_resign_on_the_oracle():
    from tests import _match_cases as mc
    text, (moves, ending) = mc.oracle_game(1, mc.S301, ("despair", 302, 51))
    assert ending == "resign" and moves == 33 and "RE[B+R]" in text
    assert mc.oracle_result(text, moves, ending) == {"winner": "black", "is_resign": True, "moves": 33, "a_is_black": True}
