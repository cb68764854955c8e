"""Shared cases of the early-stop tests (test_stop_rule_host.py, test_gpu_early_stop.py): CONSTANT_PLAYOUT searches on the CPU
oracle (oracle.tree.MCTSTree with oracle.tree.TimeManager.is_move_decided, mcts/time_manager.py:146-163) under the bit-exact
evaluators of the other search tests - StubNet, and oracle/hardnets.py's FlatNet and SpikyNet - and the same searches under
three WRONG stop rules, which the corpus has to tell from the right one.

A case is (name, evaluator, seed, ply, colour, visits, batch): the position before move `ply` of game 0 of
tests/golden/board_s9.npz, the evaluator salted and numpy seeded with `seed`.  The cases were chosen by scanning seeds on the
CPU (nothing here was taken from a device run) until, between them,
- the rule fires at its first test, at the last full mini-batch, and never;
- a test meets remaining == cutoff (only a strict < goes on searching there);
- a test meets two leaders with equal visits (the cutoff is 0 there: a second largest taken as the second DISTINCT value stops);
- a search is decided by its last, partial mini-batch (no test follows it: the tree is not halted).
"""
import functools

import numpy as np

SIZE = 9

# (name, evaluator, seed, ply, colour, visits, batch)
CASES = (
    ("first_test", "stub", 3, 30, 1, 30, 16),              # [16, 14]: decided by the first mini-batch
    ("last_full", "flat", 1, 30, 1, 30, 4),                # 7 of 8 mini-batches: decided at the last test
    ("mid_batch4", "stub", 3, 30, 1, 30, 4),               # 4 of 8
    ("mid_batch1", "stub", 1, 4, 1, 20, 1),                # 11 of 20: a test after every descent
    ("never", "flat", 1, 0, 1, 30, 4),
    ("never_120", "stub", 1, 0, 1, 120, 16),               # not halted, though its partial last mini-batch decides it
    ("equality", "stub", 1, 30, 1, 50, 16),                # a test with remaining == cutoff: goes on
    ("equality_white", "spiky", 3, 1, 2, 20, 16),
    ("tied_leaders", "stub", 2, 20, 1, 50, 16),            # a test with two equal leaders: goes on
)

# five positions for one lock-step engine: (evaluator, seed, visits, batch) shared, one tree per ply - plies 0, 10 and 20 never
# halt, ply 4 halts at its last test, ply 30 after 4 of 8 mini-batches
LOCKSTEP = ("stub", 3, 30, 4, (0, 4, 10, 20, 30))


def lockstep_cases():
    kind, seed, visits, batch, plies = LOCKSTEP
    return tuple((f"lockstep_p{ply}", kind, seed, ply, 1, visits, batch) for ply in plies)

RULES = ("right", "le", "distinct", "partial")


def make_evaluator(kind: str, seed: int):
    from oracle.hardnets import make_net
    from oracle.stubnet import StubNet
    return StubNet(salt=seed) if kind == "stub" else make_net(kind, seed)


def rule_decides(rule: str, children_visits, node_visits: int, total: int) -> bool:
    """is_move_decided of CONSTANT_PLAYOUT ("right", "partial": oracle.tree.TimeManager's own text is used for these by
    oracle_search) and its wrong variants: "le" tests <=, "distinct" takes the second DISTINCT value as the second largest
    (0 if there is none)."""
    ordered = sorted(int(v) for v in children_visits)
    remaining = total - int(node_visits)
    if rule == "distinct":
        values = sorted(set(ordered))
        return remaining < values[-1] - (values[-2] if len(values) > 1 else 0)
    cutoff = ordered[-1] - ordered[-2]
    return remaining <= cutoff if rule == "le" else remaining < cutoff


def _time_manager(rule: str, visits: int):
    from oracle.tree import TimeControl, TimeManager

    class Wrong(TimeManager):
        def is_move_decided(self, root, threshold):
            return rule_decides(rule, root.children_visits, root.node_visits, threshold)

    return (TimeManager if rule in ("right", "partial") else Wrong)(TimeControl.CONSTANT_PLAYOUT, visits)


def oracle_board(ply: int, size: int = SIZE, superko: bool = False):
    from tests.helpers import load_npz, oracle_replay
    brd = load_npz(f"board_s{size}.npz")
    return oracle_replay(size, brd["g0_move"], brd["g0_color"], ply, superko)


def product_board(ply: int, size: int = SIZE, superko: bool = False):
    from tamago_amd.board.go_board import GoBoard
    from tests.helpers import load_npz
    brd = load_npz(f"board_s{size}.npz")
    board = GoBoard(size, 7.0, superko)
    for mv, c in zip(brd["g0_move"][:ply], brd["g0_color"][:ply]):
        board.put_stone(int(mv), int(c))
    return board


def search_oracle(case, rule: str = "right") -> dict:
    """What the oracle's search_best_move leaves behind for a case under `rule`: move, num_nodes, the whole-tree digest
    (tests/_hard_trees.py tree_digest), the root's visits, numpy's next draw, the mini-batches the search ran, and what the
    device's halt word and stopped_at must read: halted iff the search was cut short ("partial": or the rule holds after
    the last mini-batch, where the right search tests nothing), stopped_at the root's visits then."""
    from oracle.tree import MCTSTree
    from tests._hard_trees import tree_digest
    name, kind, seed, ply, color, visits, batch = case
    board = oracle_board(ply)
    tree = MCTSTree(make_evaluator(kind, seed), SIZE, tree_size=visits + 16, batch_size=batch)
    saved = np.random.get_state()
    np.random.seed(seed)
    try:
        move = tree.search_best_move(board, color, _time_manager(rule, visits))
        rng_after = float(np.random.random_sample())
    finally:
        np.random.set_state(saved)
    root = tree.node[tree.current_root]
    ran = tree.batch_log[1:]                                       # (the first entry is the root's evaluation)
    halted = sum(ran) < visits
    if rule == "partial" and not halted and root.num_children > 1:
        halted = rule_decides("right", root.children_visits, root.node_visits, visits)
    return {"move": int(move), "num_nodes": int(tree.num_nodes), "digest": tree_digest(tree, tree.num_nodes),
            "node_visits": int(root.node_visits), "child_visits": [int(v) for v in root.children_visits[:root.num_children]],
            "rng_after": rng_after, "batches": [int(b) for b in ran], "halted": bool(halted),
            "stopped_at": int(root.node_visits) if halted else 0}


@functools.lru_cache(maxsize=None)
def oracle_result(name: str, rule: str = "right") -> dict:
    """search_oracle by case name, computed once per process and shared by the tests."""
    return search_oracle(next(c for c in CASES + lockstep_cases() if c[0] == name), rule)


def rule_tests(case):
    """(remaining, first, second, second distinct) at every test of the right search of a case, in order: after each full
    mini-batch that has descents to follow."""
    from oracle.tree import MCTSTree, TimeControl, TimeManager
    name, kind, seed, ply, color, visits, batch = case
    seen = []

    class Spy(TimeManager):
        def is_move_decided(self, root, threshold):
            ordered = sorted(int(v) for v in root.children_visits)
            values = sorted(set(ordered))
            row = (threshold - int(root.node_visits), ordered[-1], ordered[-2], values[-2] if len(values) > 1 else 0)
            if int(root.node_visits) and (not seen or seen[-1] != row):       # (asked after every descent: the inputs move per mini-batch)
                seen.append(row)
            return super().is_move_decided(root, threshold)

    tree = MCTSTree(make_evaluator(kind, seed), SIZE, tree_size=visits + 16, batch_size=batch)
    saved = np.random.get_state()
    np.random.seed(seed)
    try:
        tree.search_best_move(oracle_board(ply), color, Spy(TimeControl.CONSTANT_PLAYOUT, visits))
    finally:
        np.random.set_state(saved)
    return seen


# ---- PUCT match games with setups that are not strict ---------------------------------------------------------------------
def oracle_early_match_game(seed, black, white, black_search, white_search, strict, **kwargs):
    """tests/_puct_match_cases.py oracle_puct_match_game - the loop tamago_amd/selfplay/puct_match.py states - with
    TimeManager(STRICT_PLAYOUT if strict[colour] else CONSTANT_PLAYOUT, visits) per colour; strict = (black's, white's);
    black / white: evaluator specs of tests/_match_cases.py make_net."""
    from oracle.board import PASS, RESIGN
    from oracle.tree import TimeControl, TimeManager
    from tests import _puct_match_cases as P
    from tests._match_cases import make_net

    def best_move(tree, board, color, visits, resign_threshold=P.RESIGN_THRESHOLD, search_one_child=False):
        tm = TimeManager(TimeControl.STRICT_PLAYOUT if strict[color - 1] else TimeControl.CONSTANT_PLAYOUT, visits)
        tree._initialize_search(board, color)
        tm.start_timer()
        root = tree.node[tree.current_root]
        if root.num_children == 1:
            return PASS
        tree.search(board, color, tm)
        if len(tree.batch_queue.node_index) > 0:
            tree.process_mini_batch(board)
        best = root.best_move_index()
        return RESIGN if root.value_evaluation(best) < resign_threshold else root.action[best]

    saved = P.oracle_best_move
    P.oracle_best_move = best_move
    try:
        return P.oracle_puct_match_game(seed, make_net(black), make_net(white), black_search, white_search, **kwargs)
    finally:
        P.oracle_best_move = saved


@functools.lru_cache(maxsize=None)
def oracle_early_game(seed, black, white, black_search, white_search, strict):
    return oracle_early_match_game(seed, black, white, black_search, white_search, strict)


def one_child_plies_of(text: str, size: int = SIZE, komi: float = 7.0):
    """The plies (0-based) of a game record that a one-child root answered (tests/_puct_match_cases.py one_child_plies, for a
    record's text): the game replayed on the oracle board."""
    import re
    from oracle.board import GoBoard, BLACK
    board, color, out = GoBoard(size, komi, False), BLACK, []
    for ply, (_, sgf) in enumerate(re.findall(r";([BW])\[([a-z]{2})\]", text)):
        if len(board.search_candidates(color)) == 1:
            out.append(ply)
        pos = 0 if sgf == "tt" else (ord(sgf[0]) - ord("a") + 1) + (ord(sgf[1]) - ord("a") + 1) * (size + 2)
        board.put_stone(pos, color)
        color = 3 - color
    return out
