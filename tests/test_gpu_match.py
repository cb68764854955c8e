"""Matches between two evaluators under Gumbel search (tamago_amd/selfplay/match.py, tg_selfplay_play_move2) against the CPU
oracle's match game (tests/_match_cases.py: the reference worker's loop with the mover's network per move): byte-identical
records, the tally, lock-step independence with the slot-restart rule, the one-call path against the phase-by-phase path in
every scheme, and the library's refusals."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _match_cases as mc
from tests._match_cases import S301, S302

pytestmark = pytest.mark.gpu


def _read(d, index):
    return open(os.path.join(d, f"{index}.sgf"), encoding="utf-8").read()


def _check_tally(out, expected):
    """search_match's counts against the tally of the oracle's results."""
    from tamago_amd.selfplay.match import tally, rating
    want = tally(expected)
    for key in ("games", "wins_a", "wins_b", "draws", "unfinished", "as_black", "as_white", "resignations", "mean_length"):
        assert out[key] == want[key], key
    for key, value in rating(want["wins_a"], want["wins_b"], want["draws"]).items():
        assert out[key] == value, key
    got = [{k: r[k] for k in ("winner", "is_resign", "moves", "a_is_black")} for r in out["results"]]
    assert got == expected


def test_one_board_games_equal_the_oracle_games(tmp_path):
    """StubNet(301) black against StubNet(302) white, seeds 1 and 2: one ends on white's call, one on black's."""
    from tamago_amd.selfplay.match import search_match
    games = [mc.oracle_game(seed, S301, S302) for seed in (1, 2)]
    assert [g[1] for g in games] == [(102, "passes"), (97, "passes")]         # both ending parities, two passes each
    out = search_match(mc.make_net(S301), mc.make_net(S302), 2, visits=mc.VISITS, boards=1, seeds=[1, 2], save_dir=str(tmp_path))
    for i, (text, _) in enumerate(games):
        assert _read(tmp_path, i) == text, i
    _check_tally(out, [mc.oracle_result(text, *end) for text, end in games])
    assert out["wins_a"] == 1 and out["wins_b"] == 1 and out["unfinished"] == 0


def test_swapped_leg_and_a_drawn_game_equal_the_oracle_games(tmp_path):
    """Seed 12 from both sides (swap): the leg with 302 as black is a draw by count_score - RE[0] with a winner of "draw"."""
    from tamago_amd.selfplay.match import search_match
    first = mc.oracle_game(12, S301, S302)
    second = mc.oracle_game(12, S302, S301, names=("B", "A"))
    assert second[1] == (98, "passes") and "RE[0]" in second[0]
    out = search_match(mc.make_net(S301), mc.make_net(S302), 1, visits=mc.VISITS, boards=1, seeds=[12], swap=True,
                       save_dir=str(tmp_path))
    assert _read(tmp_path, 0) == first[0]
    assert _read(tmp_path, 1) == second[0]
    assert "PB[B]PW[A]" in second[0]
    _check_tally(out, [mc.oracle_result(first[0], *first[1]), mc.oracle_result(second[0], *second[1], a_is_black=False)])
    assert out["draws"] == 1 and out["as_white"]["draws"] == 1


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("black,white,loser", [(S301, ("despair", 302, 51), "W"), (("despair", 301, 50), S302, "B")])
def test_resignation_of_each_colour_equals_the_oracle_game(black, white, loser, seed, tmp_path):
    """A crafted evaluator (Despair) makes its user resign; with never_resign the same pair plays on to two passes."""
    from tamago_amd.selfplay.match import search_match
    resigned = mc.oracle_game(seed, black, white)
    played_on = mc.oracle_game(seed, black, white, True)
    moves, ending = resigned[1]
    assert ending == "resign" and moves >= 10 and moves % 2 == (1 if loser == "W" else 0)
    assert ("RE[B+R]" if loser == "W" else "RE[W+R]") in resigned[0]
    assert played_on[1][1] == "passes" and played_on[1][0] > moves
    out = search_match(mc.make_net(black), mc.make_net(white), 2, visits=mc.VISITS, boards=2, seeds=[seed, seed],
                       never_resign_flags=[False, True], save_dir=str(tmp_path))
    assert _read(tmp_path, 0) == resigned[0]
    assert _read(tmp_path, 1) == played_on[0]
    _check_tally(out, [mc.oracle_result(resigned[0], *resigned[1]), mc.oracle_result(played_on[0], *played_on[1])])
    assert out["resignations"] == 1


@pytest.mark.parametrize("boards", [1, 2, 3])
def test_lockstep_boards_play_the_single_board_games(boards, tmp_path):
    """Games 1-5 share a launch with 1, 2 and 3 boards: the same files (the oracle's, which the one-board run equals), every
    game played - no slot stays parked for ever, whichever call its game ended on."""
    from tamago_amd.selfplay.match import search_match
    seeds = [1, 2, 3, 4, 5]
    games = [mc.oracle_game(seed, S301, S302) for seed in seeds]
    assert {g[1][0] % 2 for g in games} == {0, 1}                             # games that end on white's and on black's call
    assert all(g[1][1] == "passes" for g in games)
    out = search_match(mc.make_net(S301), mc.make_net(S302), 5, visits=mc.VISITS, boards=boards, seeds=seeds,
                       save_dir=str(tmp_path))
    assert out["games"] == 5 and sorted(r["index"] for r in out["results"]) == [0, 1, 2, 3, 4]
    for i, (text, _) in enumerate(games):
        assert _read(tmp_path, i) == text, (boards, i)
    _check_tally(out, [mc.oracle_result(text, *end) for text, end in games])
    assert out["slot_calls"] == out["calls"] * boards and 0 <= out["parked_slot_calls"] <= 5


def test_one_evaluator_on_both_sides_plays_the_selfplay_games(tmp_path):
    """Two StubNets with the same salt: selfplay_shard's games with the same seeds and flags, apart from PB / PW."""
    from oracle.stubnet import StubNet
    from tamago_amd.selfplay.match import search_match
    from tamago_amd.selfplay.worker import selfplay_shard
    idx = [1, 5, 6]
    flags = [mc.reference_never_resign(1), True, False]
    shard, match = tmp_path / "shard", tmp_path / "match"
    shard.mkdir()
    selfplay_shard(str(shard), StubNet(salt=201), idx, 9, 16, boards=2, never_resign_flags=flags)
    search_match(StubNet(salt=201), StubNet(salt=201), 3, visits=16, boards=2, seeds=idx, never_resign_flags=flags,
                 save_dir=str(match))
    for g, i in enumerate(idx):
        text = _read(match, g)
        assert "PB[A]PW[B]" in text
        assert text.replace("PB[A]PW[B]", "PB[TamaGo-Black]PW[TamaGo-White]") == _read(shard, i), i


@pytest.fixture(scope="module")
def dualnet_match():
    """Two differently seeded DualNets and their swapped match of games 1-6, 48 simulations, on 4 boards through
    tg_selfplay_play_move2: (nets, digest, tally)."""
    from tests import _match_games as mg
    nets = mg.two_nets()
    digest, tally, out = mg.play(*nets, 4, 6, 48)
    assert tally["games"] == 12 and out["range_fallbacks"] == 0
    return nets, digest, tally


class HostOnly:
    def __init__(self, net):
        self.net = net

    def inference(self, planes):
        return self.net.inference(planes)

    def inference_with_policy_logits(self, planes):
        return self.net.inference_with_policy_logits(planes)


@pytest.mark.parametrize("wrap", ["both", "black only"])
def test_one_call_path_equals_the_phase_by_phase_path(dualnet_match, wrap):
    """Wrapped so that they are not recognised as DualNets, the same networks go through the phase-by-phase path (a mixed pair
    does too): same forward kernel, same bits, so identical files and an identical tally."""
    from tests import _match_games as mg
    (net_a, net_b), digest, tally = dualnet_match
    slow = mg.play(HostOnly(net_a), HostOnly(net_b) if wrap == "both" else net_b, 4, 6, 48)
    assert (slow[0], slow[1]) == (digest, tally)


def test_one_board_at_a_time_plays_the_same_match(dualnet_match):
    """ONE board: every game's end leaves the group with nothing live - calls that launch no phase at all, and after a game
    that ended on white's call one with no game in any slot."""
    from tests import _match_games as mg
    (net_a, net_b), digest, tally = dualnet_match
    solo = mg.play(net_a, net_b, 1, 6, 48)
    assert (solo[0], solo[1]) == (digest, tally)
    assert solo[2]["parked_slot_calls"] > 0


@pytest.mark.parametrize("variant", ["round trip", "unique leaves", "knob ignored"])
def test_schemes_play_the_same_match(dualnet_match, variant):
    """TG_SP_CHAIN=0 (the round-trip scheme: a slot starts only when the next call is black's) and the UNIQUE leaf layout,
    each in a process of its own; and TG_SP_CHAIN=0 without TG_DEBUG_KNOBS, which the library ignores - the handles run chained,
    and the driver, which asks the handle, must not start the colours as if they ran the round trip."""
    _, digest, tally = dualnet_match
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_match_games.py")
    env = dict(os.environ)
    env.pop("TG_SP_CHAIN", None)
    if variant in ("round trip", "knob ignored"):
        env["TG_SP_CHAIN"] = "0"
    if variant == "knob ignored":
        env.pop("TG_DEBUG_KNOBS", None)
    else:
        env["TG_DEBUG_KNOBS"] = "1"
    res = subprocess.run([sys.executable, script, "4", "6", "48", "1" if variant == "unique leaves" else "0"], env=env,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["range_fallbacks"] == 0 and got["chained"] == (variant != "round trip")
    assert (got["digest"], got["tally"]) == (digest, json.loads(json.dumps(tally)))


def test_the_library_refuses_calls_that_would_move_both_colours(dualnet_match):
    """Through the ABI on a 2-board handle: a game started for a call in which black moves, and boards with both sides to move."""
    from tamago_amd import lib as tl
    from tamago_amd.board.stone import Stone
    from tamago_amd.mcts.engine import DeviceEvaluator
    from tamago_amd.selfplay.worker import _LockStep
    (net_a, net_b), _, _ = dualnet_match
    queue = [(0, True), (1, True)]
    group = _LockStep(None, DeviceEvaluator(net_a), 9, 16, 2, {0: 1, 1: 2}, 0, lambda: queue.pop(0), False)
    lib, handle, engine = group.lib, group.handle, group.engine
    try:
        policy, value = group.outputs()

        def call(to_move, nxt):
            return lib.tg_selfplay_play_move2(handle, to_move.handle, nxt.handle, engine.planes.data_ptr(), policy.data_ptr(),
                                              value.data_ptr(), engine._stream(), group.finished.ctypes.data,
                                              group.counts.ctypes.data)

        assert group.start(0)
        engine.set_root(1, group.start_board, Stone.BLACK, np.random.RandomState(0).get_state())
        tl.check(lib.tg_selfplay_start_game(handle, 1, -1, 0), "tg_selfplay_start_game")
        tl.check(call(net_b, net_a), "first call")                # roots only: black's network evaluates slot 0's
        assert call(net_b, net_a) == -3                           # the networks the wrong way round: net_a's turn to search
        assert "take turns" in lib.tg_last_error().decode()
        assert group.start(1)                                     # ... before a call in which black moves
        assert call(net_a, net_b) == -3                           # TG_ERR_STATE, nothing launched
        message = lib.tg_last_error().decode()
        assert "slot 1" in message and "black moves" in message
        tl.check(call(net_a, net_a), "one network")               # one network: no rule; slot 0 moves, slot 1's root is evaluated
        assert call(net_b, net_a) == -3                           # slot 0 has white to move, slot 1 black
        message = lib.tg_last_error().decode()
        assert "slot 1 has black to move but slot 0 has white" in message
        result = np.zeros(4, dtype=np.int32)
        score = ctypes.c_double()
        assert lib.tg_selfplay_game_result(handle, 0, result.ctypes.data, ctypes.byref(score)) == -3    # no game has ended
    finally:
        group.close()


def test_rl_loop_gates_a_generation_with_a_search_match(tmp_path, monkeypatch):
    """tools/rl_loop.py with gate_visits > 0: the trained network against the one before under search, logged with its Elo
    estimate; gate_visits = 0 keeps the policy gate."""
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import rl_loop
    import tamago_amd.nn.data_generator as dg
    monkeypatch.setattr(dg, "BATCH_SIZE", 32)
    torch.manual_seed(11)
    np.random.seed(11)
    lines = []
    rl_loop.run_generation(str(tmp_path), 0, 16, 16, 16, 32, log=lines.append, gate_games=4, gate_visits=16)
    gate = [line for line in lines if "new against previous" in line]
    assert len(gate) == 1 and "over 8 search games at 16 simulations" in gate[0] and "Elo" in gate[0], lines
    rl_loop.run_generation(str(tmp_path), 1, 16, 16, 16, 32, log=lines.append, gate_games=4)
    assert "over 8 policy games" in [line for line in lines if "new against previous" in line][1]


def test_a_13x13_game_equals_the_oracle_game(tmp_path):
    """Nothing is hard-wired to 9: one 13x13 game, 16 simulations."""
    from tamago_amd.selfplay.match import search_match
    text, (moves, ending) = mc.oracle_game(1, S301, S302, size=13)
    assert ending in ("passes", "resign") and moves >= 10 and "SZ[13]" in text
    out = search_match(mc.make_net(S301), mc.make_net(S302), 1, size=13, visits=mc.VISITS, boards=1, seeds=[1],
                       save_dir=str(tmp_path))
    assert _read(tmp_path, 0) == text
    _check_tally(out, [mc.oracle_result(text, moves, ending)])
