"""Shared cases of the tree-reuse match tests (test_puct_reuse_host.py, test_gpu_puct_reuse.py): the PUCT match game with tree
reuse (puct_match(reuse_tree=True)) on the CPU oracle.  There is no reference counterpart - the reference
rebuilds its tree every move - so the contract is the product's own single-tree path: each colour's moves are those of an
MCTSTree(reuse_tree=True)-equivalent tree that sees every move of the game.

The game keeps TWO oracle trees, one per colour, each searched with its own network, visits and mini-batch, and one legacy
stream per game and colour: black RandomState(seed), white RandomState((seed + 2**31) % 2**32); numpy's global state is
swapped per mover.  Before a colour's search its tree's reuse root is the node reached from its last root by the moves
played since (its own move and the reply); None - a fresh root: expansion, draws, evaluation - before the colour's first
search and when a step is unexpanded.  A reused root draws nothing and owes visits - kept root visits descents.  A root
with one child answers PASS without a search, reused or not.  Resign rule, two passes, move limit, count_score, record text
and tally: those of _puct_match_cases."""
import functools

import numpy as np

from tests._match_cases import make_net
from tests._puct_match_cases import BLACK_SEARCH, RESIGN_THRESHOLD, S301, S302, SIZE, WHITE_SEARCH, oracle_result  # noqa: F401
from tests._tree_reuse import compact_oracle_tree, oracle_child

RULES = ("right", "expand_again", "from_zero")
GPU_SEEDS = (0, 1, 2, 3)                                    # the games test_gpu_puct_reuse.py plays


def white_seed(seed: int) -> int:
    return (int(seed) + 2 ** 31) % 2 ** 32


def reuse_root_of(tree, pending):
    """The node reached from the tree's root by `pending` (the moves played since its last search; None: it never searched),
    None when there is no such expanded node."""
    if pending is None:
        return None
    node = 0
    for move in pending:
        node = oracle_child(tree, node, move)
        if node < 0:
            return None
    return node


def reuse_best_move(tree, board, color, visits, reuse_root, resign_threshold=RESIGN_THRESHOLD, rule="right"):
    """_tree_reuse.emulate_search under STRICT_PLAYOUT with the resign threshold as an argument (the same steps; with the
    oracle's own threshold test_puct_reuse_host.py holds the two to each other).  Returns (move, kept root visits or None).
    rule "expand_again": WRONG - a reused root takes the draws of an expansion again; "from_zero": WRONG - a reused tree
    owes `visits` descents, not visits less the kept ones."""
    from oracle.board import PASS, RESIGN
    from oracle.tree import tentative_policy
    kept = None
    if reuse_root is None:
        tree._initialize_search(board, color)
    else:
        compact_oracle_tree(tree, reuse_root)
        kept = int(tree.node[0].node_visits)
        if rule == "expand_again":
            tentative_policy(tree.node[0].num_children)
    root = tree.node[0]
    if root.num_children == 1:
        return PASS, kept
    owed = visits if (rule == "from_zero" or kept is None) else max(0, visits - kept)
    search_board = board.clone()
    for _ in range(owed):
        search_board.copy_from(board)
        tree.search_mcts(search_board, color, 0, [])
    if len(tree.batch_queue.node_index) > 0:
        tree.process_mini_batch(board)
    best = root.best_move_index()
    if root.value_evaluation(best) < resign_threshold:
        return RESIGN, kept
    return root.action[best], kept


def oracle_reuse_match_game(seed, net_black, net_white, black_search=BLACK_SEARCH, white_search=WHITE_SEARCH, size=SIZE,
                            komi=7.0, cgos_mode=False, check_superko=False, resign_threshold=RESIGN_THRESHOLD,
                            names=("A", "B"), rule="right"):
    """The reuse game of `seed`.  Returns (SGF text without comments, (moves played, ending), (black's numpy state at the end,
    white's), searches): searches = one (colour, kept root visits or None for a fresh root) per search, in move order.
    The caller's numpy state is restored."""
    from oracle.board import GoBoard, BLACK, PASS, RESIGN
    from oracle.tree import MCTSTree
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.board.stone import Stone
    from tamago_amd.sgf.selfplay_record import SelfPlayRecord
    nets = {1: net_black, 2: net_white}
    search = {1: black_search, 2: white_search}
    trees = {c: MCTSTree(nets[c], size, tree_size=search[c][0] + 16, batch_size=search[c][1], cgos_mode=cgos_mode) for c in (1, 2)}
    streams = {1: np.random.RandomState(seed).get_state(), 2: np.random.RandomState(white_seed(seed)).get_state()}
    pending = {1: None, 2: None}
    record = SelfPlayRecord("", Coordinate(size), players=names)
    searches = []
    saved = np.random.get_state()
    try:
        board = GoBoard(size, komi, check_superko)
        color, passes, moves = BLACK, 0, 0
        winner, is_resign, score, ending = Stone.EMPTY, False, 0.0, "limit"
        for _ in range(size * size * 2):
            np.random.set_state(streams[color])
            pos, kept = reuse_best_move(trees[color], board, color, search[color][0], reuse_root_of(trees[color], pending[color]),
                                        resign_threshold, rule)
            streams[color] = np.random.get_state()
            searches.append((color, kept))
            if pos == RESIGN:
                winner, is_resign, ending = (Stone.WHITE if color == BLACK else Stone.BLACK), True, "resign"
                break
            board.put_stone(pos, color)
            pending[color] = [pos]
            if pending[3 - color] is not None:
                pending[3 - color].append(pos)
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
        return text, (moves, ending), (streams[1], streams[2]), searches
    finally:
        np.random.set_state(saved)


@functools.lru_cache(maxsize=None)
def oracle_reuse_game(seed, black=S301, white=S302, black_search=BLACK_SEARCH, white_search=WHITE_SEARCH, size=SIZE, komi=7.0,
                      cgos_mode=False, check_superko=False, resign_threshold=RESIGN_THRESHOLD, names=("A", "B"), rule="right"):
    """oracle_reuse_match_game for evaluator specs (_match_cases.make_net), computed once per process and shared by the tests."""
    return oracle_reuse_match_game(seed, make_net(black), make_net(white), black_search, white_search, size, komi, cgos_mode,
                                   check_superko, resign_threshold, names, rule)
