"""PUCT matches with tree reuse in lock-step on the device (puct_match(reuse_tree=True): tg_search_advance,
tg_search_root_planes_fresh, visit budgets) against the reuse game on the CPU oracle
(tests/_puct_reuse_cases.py): byte-identical records, results, tallies and both final streams on 3 boards, on 1 board and with
compact_idle; a game against two of the product's own MCTSTree(reuse_tree=True); the refusals."""
import os
import re

import numpy as np
import pytest

from tests import _puct_match_cases as pc
from tests import _puct_reuse_cases as rc
from tests._match_cases import make_net
from tests._puct_match_cases import S301, S302

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3


def _read(d, index):
    return open(os.path.join(d, f"{index}.sgf"), encoding="utf-8").read()


def _setups(black=S301, white=S302, black_search=pc.BLACK_SEARCH, white_search=pc.WHITE_SEARCH):
    from tamago_amd.selfplay.puct_match import EngineSetup
    return EngineSetup(make_net(black), *black_search), EngineSetup(make_net(white), *white_search)


@pytest.mark.parametrize("boards,compact_idle", [(3, False), (1, False), (3, True)], ids=["3boards", "1board", "3boards_compact"])
def test_reuse_games_equal_the_oracle_games(boards, compact_idle, tmp_path):
    from tamago_amd.selfplay.match import rating, tally
    from tamago_amd.selfplay.puct_match import puct_match
    games = [rc.oracle_reuse_game(seed) for seed in rc.GPU_SEEDS]
    out = puct_match(*_setups(), 4, boards=boards, seeds=list(rc.GPU_SEEDS), save_dir=str(tmp_path), reuse_tree=True,
                     compact_idle=compact_idle, poll_every=1)
    want = [pc.oracle_result(text, *end) for text, end, _, _ in games]
    got = [{k: r[k] for k in ("winner", "is_resign", "moves", "a_is_black")} for r in out["results"]]
    assert got == want
    for i, (text, _, (black_state, white_state), _) in enumerate(games):
        assert _read(tmp_path, i) == text, i
        assert pc.same_stream(out["results"][i]["stream"], black_state), i
        assert pc.same_stream(out["results"][i]["stream_white"], white_state), i
    counts = tally(want)
    for key in ("games", "wins_a", "wins_b", "draws", "unfinished", "as_black", "as_white", "resignations", "mean_length"):
        assert out[key] == counts[key], key
    for key, value in rating(counts["wins_a"], counts["wins_b"], counts["draws"]).items():
        assert out[key] == value, key
    searches = [s for _, _, _, ss in games for s in ss]
    one_child = out["one_child_roots"]
    reused = sum(1 for _, kept in searches if kept is not None)
    assert out["reused_searches"] + out["fresh_searches"] == len(searches) - one_child
    assert 0 < out["reused_searches"] <= reused and out["fresh_searches"] > 0 and 0.0 < out["kept_share"] < 1.0
    if compact_idle:
        plain = sum((26 if color == 1 else 20) for color, _ in searches)
        assert out["forward_positions"] < plain * boards                  # idle trees and spent budgets are not evaluated


def test_a_game_equals_two_reusing_trees_move_by_move(tmp_path):
    """Independent of the oracle: one game between two of the product's own MCTSTree(reuse_tree=True), one per colour, each
    with its colour's stream (numpy's state swapped per mover), under STRICT_PLAYOUT on a host GoBoard."""
    from tamago_amd.board.constant import PASS, RESIGN
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.board.stone import Stone
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    from tamago_amd.selfplay.puct_match import puct_match, white_seed
    seed = rc.GPU_SEEDS[1]
    search = {Stone.BLACK: pc.BLACK_SEARCH, Stone.WHITE: pc.WHITE_SEARCH}
    nets = {Stone.BLACK: make_net(S301), Stone.WHITE: make_net(S302)}
    saved = np.random.get_state()
    try:
        states = {Stone.BLACK: np.random.RandomState(seed).get_state(), Stone.WHITE: np.random.RandomState(white_seed(seed)).get_state()}
        trees = {c: MCTSTree(nets[c], tree_size=search[c][0] + 16, batch_size=search[c][1], reuse_tree=True) for c in nets}
        board = GoBoard(board_size=9, komi=7.0, check_superko=False)
        color, passes, moves, reused = Stone.BLACK, 0, [], 0
        for _ in range(2 * 81):
            np.random.set_state(states[color])
            pos = trees[color].search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, search[color][0]))
            states[color] = np.random.get_state()
            reused += trees[color].reused_visits > 0
            if pos == RESIGN:
                break
            board.put_stone(pos, color)
            moves.append((1 if color == Stone.BLACK else 2, int(pos)))
            passes = passes + 1 if pos == PASS else 0
            color = Stone.get_opponent_color(color)
            if passes == 2:
                break
    finally:
        np.random.set_state(saved)
    out = puct_match(*_setups(), 1, boards=1, seeds=[seed], save_dir=str(tmp_path), reuse_tree=True)
    played = re.findall(r";([BW])\[([a-z]{2})\]", _read(tmp_path, 0))
    coord = Coordinate(9)
    assert played == [("B" if c == 1 else "W", coord.convert_to_sgf_format(p)) for c, p in moves]
    assert len(moves) >= 20 and reused > 0
    assert _read(tmp_path, 0) == rc.oracle_reuse_game(seed)[0]
    assert pc.same_stream(out["results"][0]["stream"], states[Stone.BLACK])
    assert pc.same_stream(out["results"][0]["stream_white"], states[Stone.WHITE])


def test_reuse_needs_strict_setups_and_off_is_todays_match(tmp_path):
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    black, white = _setups()
    with pytest.raises(ValueError, match="strict"):
        puct_match(black, EngineSetup(white.network, white.visits, white.batch_size, strict=False), 1, reuse_tree=True)
    seeds = list(rc.GPU_SEEDS[:2])
    out = puct_match(black, white, 2, boards=2, seeds=seeds, save_dir=str(tmp_path), reuse_tree=False)
    for i, seed in enumerate(seeds):
        text, end, state = pc.oracle_puct_game(seed, S301, S302)
        assert _read(tmp_path, i) == text
        assert {k: out["results"][i][k] for k in ("winner", "is_resign", "moves", "a_is_black")} == pc.oracle_result(text, *end)
        assert pc.same_stream(out["results"][i]["stream"], state) and "stream_white" not in out["results"][i]
    assert "reused_searches" not in out


def test_the_chain_is_refused_before_the_fresh_root_launch():
    """After an advance the budget chain is refused (TG_ERR_STATE) until root_planes_fresh has run."""
    import ctypes
    import torch
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    from tests.test_gpu_early_stop import _dualnet
    eng = SearchEngine(9, 2, 64, 8, DeviceEvaluator(_dualnet(9)))
    try:
        for t in range(2):
            eng.set_root(t, GoBoard(9), 1, np.random.RandomState(t).get_state())
        eng.root_eval(False)
        eng.puct_batch(8)
        arr = np.array([8, 8], dtype=np.int32)
        policy = torch.empty((16, 82), dtype=torch.float32, device=eng.device)
        value = torch.empty((16, 3), dtype=torch.float32, device=eng.device)
        ran, pos = ctypes.c_int32(0), ctypes.c_int64(0)

        def chain():
            return eng.lib.tg_search_puct_chain_budget(eng.handle, eng.evaluator.network.handle, arr.ctypes.data, 2, 1, 0, 1,
                                                       eng.planes.data_ptr(), policy.data_ptr(), value.data_ptr(), eng._stream(),
                                                       ctypes.byref(ran), ctypes.byref(pos))
        eng.set_budget(24)
        best = eng.best_moves(0.0, False)
        records = eng.advance(best["move"])
        assert (records["status"] == 0).all()
        visits = eng.read_root_stats()["node_visits"].tolist()
        assert chain() == ERR_STATE
        assert eng.read_root_stats()["node_visits"].tolist() == visits   # nothing was launched by the refused call
        eng.root_eval_fresh()
        assert chain() == 0 and ran.value == 2
        eng._collect_rng()
        assert eng.read_root_stats()["node_visits"].tolist() == [max(int(k), 0) + 16 for k in records["kept_visits"]]
    finally:
        eng.close()
