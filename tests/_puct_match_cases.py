"""Shared cases of the PUCT match tests (test_puct_match_host.py, test_gpu_puct_match.py): the PUCT match game on the CPU
oracle - the loop tamago_amd/selfplay/puct_match.py states, on oracle.tree.MCTSTree - with the evaluators of _match_cases."""
import functools
import re

import numpy as np

from tests._match_cases import make_net

SIZE = 9
BLACK_SEARCH, WHITE_SEARCH = (26, 8), (20, 6)               # (visits, batch_size) of the two colours unless a test says otherwise
S301, S302 = ("stub", 301), ("stub", 302)
RESIGN_THRESHOLD = 0.05                                      # mcts/constant.py:38


def oracle_best_move(tree, board, color, visits, resign_threshold=RESIGN_THRESHOLD, search_one_child=False):
    """oracle.tree.MCTSTree.search_best_move (mcts/tree.py:57-105) under STRICT_PLAYOUT with the resign threshold as an
    argument.  search_one_child: the WRONG rule - a one-child root is searched like any other, as a lock-step launch does to
    it; its answer is still PASS, but the stream has moved on."""
    from oracle.board import PASS, RESIGN
    from oracle.tree import TimeControl, TimeManager
    tm = TimeManager(TimeControl.STRICT_PLAYOUT, visits)
    tree._initialize_search(board, color)
    tm.start_timer()
    root = tree.node[tree.current_root]
    one_child = root.num_children == 1
    if one_child and not search_one_child:
        return PASS
    tree.search(board, color, tm)
    if len(tree.batch_queue.node_index) > 0:
        tree.process_mini_batch(board)
    if one_child:
        return PASS
    best = root.best_move_index()
    if root.value_evaluation(best) < resign_threshold:
        return RESIGN
    return root.action[best]


def oracle_puct_match_game(seed, net_black, net_white, black_search=BLACK_SEARCH, white_search=WHITE_SEARCH, size=SIZE,
                           komi=7.0, cgos_mode=False, check_superko=False, resign_threshold=RESIGN_THRESHOLD,
                           names=("A", "B"), search_one_child=False):
    """The PUCT match game after np.random.seed(seed).  Returns (SGF text without comments, (moves played, ending), numpy's
    state at the end); ending is "resign", "passes" or "limit".  The caller's numpy state is restored."""
    from oracle.board import GoBoard, BLACK, PASS, RESIGN
    from oracle.tree import MCTSTree
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.board.stone import Stone
    from tamago_amd.sgf.selfplay_record import SelfPlayRecord
    nets = {1: net_black, 2: net_white}
    search = {1: black_search, 2: white_search}
    tree = MCTSTree(net_black, size, tree_size=max(black_search[0], white_search[0]) + 16, cgos_mode=cgos_mode)
    record = SelfPlayRecord("", Coordinate(size), players=names)
    saved = np.random.get_state()
    np.random.seed(seed)
    try:
        board = GoBoard(size, komi, check_superko)
        color, passes, moves = BLACK, 0, 0
        winner, is_resign, score, ending = Stone.EMPTY, False, 0.0, "limit"
        for _ in range(size * size * 2):
            tree.network = nets[color]
            tree.batch_size = search[color][1]
            pos = oracle_best_move(tree, board, color, search[color][0], resign_threshold, search_one_child)
            if pos == RESIGN:
                winner, is_resign, ending = (Stone.WHITE if color == BLACK else Stone.BLACK), True, "resign"
                break
            board.put_stone(pos, color)
            passes = passes + 1 if pos == PASS else 0
            record.colors.append(color)
            record.moves.append(record.coord.convert_to_sgf_format(pos))
            record.comments.append("")
            color = 3 - color
            moves += 1
            if passes == 2:
                score = board.count_score() - board.get_komi()
                winner = Stone.BLACK if score > 0.1 else (Stone.WHITE if score < -0.1 else Stone.OUT_OF_BOARD)
                ending = "passes"
                break
        text = record.to_sgf(winner, board.get_komi(), is_resign, score).replace("C[]", "")
        return text, (moves, ending), np.random.get_state()
    finally:
        np.random.set_state(saved)


@functools.lru_cache(maxsize=None)
def oracle_puct_game(seed, black, white, black_search=BLACK_SEARCH, white_search=WHITE_SEARCH, size=SIZE, komi=7.0,
                     cgos_mode=False, check_superko=False, resign_threshold=RESIGN_THRESHOLD, names=("A", "B"),
                     search_one_child=False):
    """oracle_puct_match_game for evaluator specs (_match_cases.make_net), computed once per process and shared by the tests."""
    return oracle_puct_match_game(seed, make_net(black), make_net(white), black_search, white_search, size, komi, cgos_mode,
                                  check_superko, resign_threshold, names, search_one_child)


def oracle_result(text: str, moves: int, ending: str, a_is_black: bool = True) -> dict:
    """The per-game result puct_match reports (winner, is_resign, moves, a_is_black), read off an oracle game."""
    result = re.search(r"RE\[([^\]]*)\]", text).group(1)
    winner = {"B": "black", "W": "white"}.get(result[0]) if result != "0" else ("draw" if ending == "passes" else None)
    return {"winner": winner, "is_resign": ending == "resign", "moves": moves, "a_is_black": a_is_black}


def same_stream(got, want) -> bool:
    """Is the MT19937 state (key, position) a result carries the numpy state `want`?  Compared by what the two generators draw
    next: position 624 of one key block and position 0 of the next are the same state."""
    a, b = np.random.RandomState(), np.random.RandomState()
    a.set_state(("MT19937", np.asarray(got[0], dtype=np.uint32), int(got[1]), 0, 0.0))
    b.set_state(want)
    return a.random_sample(700).tobytes() == b.random_sample(700).tobytes()


def one_child_plies(seed, black=S301, white=S302, **kwargs):
    """The plies (0-based) of an oracle game that were answered by a one-child root: where the record passes and the wrong
    oracle's stream parts from the right one's is not observable ply by ply, so the game is replayed on the oracle board."""
    from oracle.board import GoBoard, BLACK
    text, (moves, _), _ = oracle_puct_game(seed, black, white, **kwargs)
    played = re.findall(r";([BW])\[([a-z]{2})\]", text)
    assert len(played) == moves
    size = kwargs.get("size", SIZE)
    board = GoBoard(size, kwargs.get("komi", 7.0), kwargs.get("check_superko", False))
    out = []
    color = BLACK
    for ply, (_, sgf) in enumerate(played):
        if len(board.search_candidates(color)) == 1:
            out.append(ply)
        pos = 0 if sgf == "tt" else (ord(sgf[0]) - ord("a") + 1) + (ord(sgf[1]) - ord("a") + 1) * (size + 2)
        board.put_stone(pos, color)
        color = 3 - color
    return out
