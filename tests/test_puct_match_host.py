"""CPU checks of the PUCT match (tamago_amd/selfplay/puct_match.py, tests/_puct_match_cases.py): the oracle game against a
plain loop of oracle searches, the liveness of the one-child-root case, and the driver - slots, the swapped leg, the stream
put back around a launch, argument errors, the command line - on a fake engine that runs the oracle tree per slot the way a
lock-step launch runs the device trees: EVERY slot searches, whether its game wants to or not."""
import numpy as np
import pytest

from tests import _puct_match_cases as pc
from tests._match_cases import make_net
from tests._puct_match_cases import S301, S302


def test_equal_setups_with_one_mini_batch_play_a_plain_loop_of_oracle_searches():
    """batch_size >= visits, one network: the game's moves are those of search_best_move called in a loop on one tree."""
    import re
    from oracle.board import GoBoard, BLACK, PASS, RESIGN
    from oracle.tree import MCTSTree, TimeControl, TimeManager
    from tamago_amd.board.coordinate import Coordinate
    text, (moves, ending), state = pc.oracle_puct_game(6, S301, S301, black_search=(20, 32), white_search=(20, 32))
    saved = np.random.get_state()
    try:
        np.random.seed(6)
        tree = MCTSTree(make_net(S301), 9, tree_size=64, batch_size=32)
        board, color, passes, played = GoBoard(9, 7.0, False), BLACK, 0, []
        for _ in range(162):
            pos = tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, 20))
            if pos == RESIGN:
                break
            board.put_stone(pos, color)
            played.append(("B" if color == BLACK else "W", Coordinate(9).convert_to_sgf_format(pos)))
            passes = passes + 1 if pos == PASS else 0
            color = 3 - color
            if passes == 2:
                break
        after = np.random.get_state()
    finally:
        np.random.set_state(saved)
    assert re.findall(r";([BW])\[([a-z]{2})\]", text) == played and len(played) == moves >= 10
    assert pc.same_stream((after[1], after[2]), state)


def test_an_oracle_that_searches_one_child_roots_plays_another_game():
    """The case is live: seed 1 has one-child roots at plies 91 and 95, and an oracle that searches them - as a lock-step
    launch does - leaves the game's stream elsewhere; in seed 3 (plies 116 and 148) the record itself changes.  (Seed 1's
    moves survive the shifted draws: the tentative priors they change are overwritten by the network's policy before they
    decide a move there.  Its stream at the end, which the match tests compare, does not.)"""
    assert pc.one_child_plies(1) == [91, 95] and pc.one_child_plies(3) == [116, 148]
    right, wrong = pc.oracle_puct_game(1, S301, S302), pc.oracle_puct_game(1, S301, S302, search_one_child=True)
    assert not pc.same_stream((wrong[2][1], wrong[2][2]), right[2])
    right, wrong = pc.oracle_puct_game(3, S301, S302), pc.oracle_puct_game(3, S301, S302, search_one_child=True)
    assert right[0] != wrong[0] and right[1] == (162, "limit") and wrong[1] != right[1]


# ---- the driver on a fake engine ---------------------------------------------------------------------------------------------
class _Stream:
    def __init__(self, engine, tree):
        self.engine, self.tree = engine, tree

    def final_state(self):
        return self.engine.states[self.tree]


class FakeEngine:
    """What puct_match asks of a SearchEngine, on oracle trees: one per slot, each with a numpy state of its own."""

    def __init__(self, leg, log=None):
        from oracle.tree import MCTSTree
        self.leg, self.T = leg, leg.boards
        self.size = leg.size
        self.trees = [MCTSTree(None, leg.size, tree_size=64) for _ in range(self.T)]
        self.boards, self.colors, self.states = [None] * self.T, [1] * self.T, [None] * self.T
        self.streams = [None] * self.T
        self.root_children = np.zeros(self.T, dtype=np.int64)
        self.evaluator = None
        self.log = log if log is not None else []
        self.closed = False

    def _with_stream(self, tree, fn):
        saved = np.random.get_state()
        try:
            np.random.set_state(self.states[tree])
            fn()
            self.states[tree] = np.random.get_state()
        finally:
            np.random.set_state(saved)

    def set_root(self, tree, board, color, rng_state=None):
        from oracle.board import GoBoard
        assert board.moves == 1                              # a match only ever sets the empty board
        self.boards[tree] = GoBoard(self.size, board.get_komi(), bool(board.check_superko))
        self.colors[tree] = 1
        self.log.append(("start", tree))
        if rng_state is not None:
            self.set_stream(tree, rng_state)

    def set_stream(self, tree, state):
        self.states[tree] = state
        self.streams[tree] = _Stream(self, tree)

    def root_eval(self, use_logit=False):
        self.log.append(("call", self.evaluator))
        for t in range(self.T):
            self.trees[t].network = self.evaluator
            self._with_stream(t, lambda: self.trees[t]._initialize_search(self.boards[t], self.colors[t]))
            self.root_children[t] = self.trees[t].node[0].num_children

    def can_chain(self, total):
        return False

    def ensure_capacity(self, leaves):
        return False

    def puct_batch(self, leaves):
        self.log.append(("batch", leaves))

        def descend(t):
            tree, scratch = self.trees[t], self.boards[t].clone()
            tree.batch_size = leaves
            for _ in range(leaves):
                scratch.copy_from(self.boards[t])
                tree.search_mcts(scratch, self.colors[t], 0, [])
            assert len(tree.batch_queue.node_index) == 0

        for t in range(self.T):                              # EVERY tree searches
            self._with_stream(t, lambda: descend(t))

    def best_moves(self, threshold, play, sit_out=None):
        from tamago_amd.mcts.engine import BEST_MOVE, BEST_SAT_OUT
        out = np.zeros(self.T, dtype=BEST_MOVE)
        for t in range(self.T):
            if sit_out is not None and sit_out[t]:
                out[t]["status"] = BEST_SAT_OUT
                continue
            root = self.trees[t].node[0]
            n = root.num_children
            best = 0 if n == 1 else root.best_move_index()
            move = 0 if n == 1 else (-1 if root.value_evaluation(best) < threshold else root.action[best])
            out[t] = (n, move, best, root.children_visits[best], root.children_value_sum[best], root.node_visits, 0)
            if play and move >= 0:
                self.boards[t].put_stone(move, self.colors[t])
                self.colors[t] = 3 - self.colors[t]
        return out

    def read_positions(self):
        cells = np.empty(self.T, dtype=object)
        for t in range(self.T):
            cells[t] = self.boards[t]
        return cells, None, None

    def count_scores(self, boards):
        return np.array([b.count_score() for b in boards], dtype=np.int32)

    def close(self):
        self.closed = True


def _fake_match(*args, **kwargs):
    from tamago_amd.selfplay.puct_match import puct_match
    engines = []

    def make(leg):
        engines.append(FakeEngine(leg))
        return engines[-1]

    return puct_match(*args, _make_engine=make, **kwargs), engines


def _setups():
    from tamago_amd.selfplay.puct_match import EngineSetup
    return EngineSetup(make_net(S301), *pc.BLACK_SEARCH), EngineSetup(make_net(S302), *pc.WHITE_SEARCH)


def test_the_driver_plays_the_oracle_games_on_shared_launches(tmp_path):
    """Seeds 6, 1, 6 on two slots: every call searches every slot, so seed 1's one-child roots (plies 91, 95) search too -
    its record, result and final stream are the oracle's only if the driver puts the stream back; the third game starts in
    the slot the first one frees, before a black call only; records, indices, seeds and the lock-step counts."""
    from tamago_amd.board.stone import Stone
    from tamago_amd.selfplay.match import slot_may_start
    games = [pc.oracle_puct_game(seed, S301, S302) for seed in (6, 1, 6)]
    out, (engine,) = _fake_match(*_setups(), 3, boards=2, seeds=[6, 1, 6], save_dir=str(tmp_path))
    for i, (text, end, state) in enumerate(games):
        assert open(tmp_path / f"{i}.sgf", encoding="utf-8").read() == text, i
        got = {k: out["results"][i][k] for k in ("winner", "is_resign", "moves", "a_is_black")}
        assert got == pc.oracle_result(text, *end), i
        assert pc.same_stream(out["results"][i]["stream"], state), i
    assert [r["index"] for r in out["results"]] == [0, 1, 2] and [r["seed"] for r in out["results"]] == [6, 1, 6]
    assert out["results"][0]["score"] == 3.0 and out["results"][1]["score"] == 12.0
    assert out["games"] == 3 and out["wins_a"] == 3 and out["one_child_roots"] == 2 and out["moves"] == 32 + 96 + 32
    assert out["calls"] == 96 and out["slot_calls"] == 192 and out["parked_slot_calls"] == 0      # game 6 ends on white's call
    assert engine.closed
    # the launches: the mover's network, the mover's mini-batches, black first; a slot starts right before a black call
    calls = [i for i, e in enumerate(engine.log) if e[0] == "call"]
    black, white = engine.log[calls[0]][1], engine.log[calls[1]][1]
    assert black is not white and all(engine.log[i][1] is (black, white)[k % 2] for k, i in enumerate(calls))
    assert engine.log[calls[0] + 1:calls[1]] == [("batch", 8), ("batch", 8), ("batch", 8), ("batch", 2)]
    assert engine.log[calls[1] + 1:calls[2]] == [("batch", 6), ("batch", 6), ("batch", 6), ("batch", 2)]
    starts = [i for i, e in enumerate(engine.log) if e[0] == "start"]
    assert [engine.log[i] for i in starts] == [("start", 0), ("start", 1), ("start", 0)]
    assert engine.log[starts[2] + 1][0] == "call" and engine.log[starts[2] + 1][1] is black
    assert slot_may_start(False, Stone.BLACK) and not slot_may_start(False, Stone.WHITE)


def test_a_slot_freed_on_blacks_call_waits_for_the_next_black_call():
    """One slot, two games that black resigns at ply 138: a game ended on black's call leaves a white call next, for which
    the slot is parked (no game is live: nothing is launched), and the second game starts before the call after.  The
    resigning move is neither played nor recorded.  (A game that ends on white's call restarts at once: the test above.)"""
    from tamago_amd.selfplay.puct_match import EngineSetup
    first = pc.oracle_puct_game(1, ("despair", 301, 60), S302)
    assert first[1] == (138, "resign") and "RE[W+R]" in first[0]
    out, (engine,) = _fake_match(EngineSetup(make_net(("despair", 301, 60)), *pc.BLACK_SEARCH),
                                 EngineSetup(make_net(S302), *pc.WHITE_SEARCH), 2, boards=1, seeds=[1, 1])
    # black resigns in its 70th call, the game's 139th; then one parked white call; then 139 more
    assert [r["moves"] for r in out["results"]] == [138, 138] and out["wins_b"] == 2 and out["as_black"]["wins_b"] == 2
    assert out["resignations"] == 2 and all(r["is_resign"] and r["winner"] == "white" for r in out["results"])
    assert out["calls"] == 139 + 1 + 139 and out["parked_slot_calls"] == 1 and out["slot_calls"] == out["calls"]
    assert len([e for e in engine.log if e[0] == "call"]) == 278               # the parked call launched nothing


def test_the_swapped_leg_replays_the_seeds_with_the_setups_exchanged(tmp_path):
    first = pc.oracle_puct_game(6, S301, S302)
    second = pc.oracle_puct_game(6, S302, S301, black_search=pc.WHITE_SEARCH, white_search=pc.BLACK_SEARCH, names=("B", "A"))
    out, engines = _fake_match(*_setups(), 1, seeds=[6], swap=True, save_dir=str(tmp_path))
    assert len(engines) == 2 and all(e.closed for e in engines)
    assert open(tmp_path / "0.sgf", encoding="utf-8").read() == first[0]
    assert open(tmp_path / "1.sgf", encoding="utf-8").read() == second[0]
    assert [(r["index"], r["seed"], r["a_is_black"]) for r in out["results"]] == [(0, 6, True), (1, 6, False)]
    want = [pc.oracle_result(first[0], *first[1]), pc.oracle_result(second[0], *second[1], a_is_black=False)]
    assert [{k: r[k] for k in want[0]} for r in out["results"]] == want
    from tamago_amd.selfplay.match import rating, tally
    counts = tally(want)
    assert all(out[k] == counts[k] for k in counts)
    assert all(out[k] == v for k, v in rating(counts["wins_a"], counts["wins_b"], counts["draws"]).items())
    for key in ("leaf_evals", "forward_positions", "range_fallbacks", "seconds", "games_per_second", "between_calls_seconds"):
        assert key in out
    assert out["range_fallbacks"] == 0


def test_argument_errors():
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    a, b = EngineSetup(object(), 8, 4), EngineSetup(object(), 8, 4)
    assert EngineSetup(None) == (None, 100, 1)                                 # PLAYOUTS, NN_BATCH_SIZE
    with pytest.raises(ValueError, match="games must be"):
        puct_match(a, b, 0)
    with pytest.raises(ValueError, match="one entry per game"):
        puct_match(a, b, 2, seeds=[1])
    with pytest.raises(ValueError, match="EngineSetup"):
        puct_match(object(), b, 1)
    with pytest.raises(ValueError, match="at least 1"):
        puct_match(EngineSetup(object(), 0, 4), b, 1)
    with pytest.raises(ValueError, match="at least 1"):
        puct_match(a, EngineSetup(object(), 8, 0), 1)
    with pytest.raises(ValueError, match="resign_threshold"):
        puct_match(a, b, 1, resign_threshold=float("nan"))
    with pytest.raises(ValueError, match="resign_threshold"):
        puct_match(a, b, 1, resign_threshold=1.5)
    with pytest.raises(ValueError, match="board size"):
        puct_match(a, b, 1, size=11)
    with pytest.raises(ValueError, match="boards"):
        puct_match(a, b, 1, boards=0)

    class Sized:
        board_size = 13

    with pytest.raises(ValueError, match="13x13"):
        puct_match(EngineSetup(Sized(), 8, 4), b, 1, size=9)


def test_the_command_line_takes_the_puct_flags_and_keeps_its_defaults():
    from tamago_amd.selfplay.match import parse_args, puct_setups
    from tamago_amd.selfplay.worker import SELF_PLAY_VISITS
    args = parse_args(["--black", "a.bin", "--white", "b.bin", "--games", "8"])
    assert (args.black, args.white, args.games, args.size, args.visits, args.boards, args.komi, args.swap, args.save_dir,
            args.unique_leaves) == ("a.bin", "b.bin", 8, 9, SELF_PLAY_VISITS, None, 7.0, False, None, False)
    assert (args.search, args.batch_size, args.white_visits, args.white_batch_size, args.cgos_mode, args.superko) == \
        ("gumbel", None, None, None, False, False)
    args = parse_args(["--black", "a.bin", "--white", "b.bin", "--games", "8", "--search", "puct", "--visits", "1000",
                       "--batch-size", "256", "--white-visits", "400", "--white-batch-size", "16", "--cgos-mode", "--superko"])
    assert (args.search, args.visits, args.batch_size, args.white_visits, args.white_batch_size, args.cgos_mode, args.superko) == \
        ("puct", 1000, 256, 400, 16, True, True)
    assert puct_setups(args, "A", "B") == (("A", 1000, 256), ("B", 400, 16))
    args = parse_args(["--black", "a.bin", "--white", "b.bin", "--games", "8", "--search", "puct", "--visits", "50"])
    assert puct_setups(args, "A", "B") == (("A", 50, 16), ("B", 50, 16))
    for bad in (["--batch-size", "8"], ["--white-visits", "8"], ["--superko"], ["--search", "puct", "--unique-leaves", "true"],
                ["--search", "mcts"]):
        with pytest.raises(SystemExit):
            parse_args(["--black", "a.bin", "--white", "b.bin", "--games", "8"] + bad)
