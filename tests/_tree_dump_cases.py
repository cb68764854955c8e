"""Shared cases of the whole-tree dump tests (test_dump_host.py, test_gpu_tree_dump.py): the fixtures
tests/golden/tree_dump_s{9,13,19}.json that tools/gen_golden_tree_dump.py recorded from the reference, the canonical
serialisation that tool defines (imported from it, not restated), and the same searches on the CPU oracle and on the product."""
import functools
import importlib.util
import os

import numpy as np

from tests.helpers import load_json, load_npz, oracle_replay

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (9, 13, 19)


@functools.lru_cache(maxsize=None)
def tool():
    spec = importlib.util.spec_from_file_location("gen_golden_tree_dump", os.path.join(REPO, "tools", "gen_golden_tree_dump.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@functools.lru_cache(maxsize=None)
def fixture(size: int):
    return load_json(f"tree_dump_s{size}.json")


def small_case():
    """The small 9x9 search as a case: STRICT_PLAYOUT PUCT, 10 visits at batch 2."""
    small = fixture(9)["small"]
    return dict(kind="puct", mode="STRICT", cgos=False, **{k: small[k] for k in ("seed", "visits", "batch", "ply", "superko", "color",
                                                                                  "num_nodes", "sha256", "tree_size")})


def product_board(size: int, ply: int, superko: bool):
    from tamago_amd.board.go_board import GoBoard
    brd = load_npz(f"board_s{size}.npz")
    board = GoBoard(size, 7.0, superko)
    for mv, c in zip(brd["g0_move"][:ply], brd["g0_color"][:ply]):
        board.put_stone(int(mv), int(c))
    return board


def oracle_tree_dict(size: int, case):
    """The case's search on oracle.tree.MCTSTree, put through the host half of the read-out (dump.pack_nodes) and
    dump.tree_to_dict."""
    from oracle.stubnet import StubNet
    from oracle.tree import MCTSTree, TimeControl, TimeManager
    from tamago_amd.mcts import dump
    brd = load_npz(f"board_s{size}.npz")
    board = oracle_replay(size, brd["g0_move"], brd["g0_color"], case["ply"], case["superko"])
    np.random.seed(case["seed"])
    if case["kind"] == "puct":
        tree = MCTSTree(StubNet(salt=case["seed"]), size, tree_size=case.get("tree_size", 2048), batch_size=case["batch"],
                        cgos_mode=case["cgos"])
        mode = TimeControl.STRICT_PLAYOUT if case["mode"] == "STRICT" else TimeControl.CONSTANT_PLAYOUT
        tree.search_best_move(board, case["color"], TimeManager(mode, case["visits"]))
        noise = None
    else:
        tree = MCTSTree(StubNet(salt=100 + case["seed"]), size, tree_size=160 if case["visits"] <= 100 else 2048)
        tree.generate_move_with_sequential_halving(board, case["color"], TimeManager(TimeControl.CONSTANT_PLAYOUT, case["visits"]), True)
        noise = tree.node[tree.current_root].noise
    # (the reference's to_move is the colour of the last search(), mcts/tree.py:139: a sequential-halving search leaves it black)
    packed = dump.pack_nodes(tree.node, tree.num_nodes, tree.current_root, case["color"] if case["kind"] == "puct" else 1)
    return dump.tree_to_dict(packed, size * size + 1, tree.batch_size, tree.cgos_mode, noise=noise)


def product_tree(size: int, case):
    """The case's search on the product's MCTSTree (GPU): (tree, board)."""
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    board = product_board(size, case["ply"], case["superko"])
    np.random.seed(case["seed"])
    if case["kind"] == "puct":
        tree = MCTSTree(StubNet(salt=case["seed"]), tree_size=case.get("tree_size", 2048), batch_size=case["batch"],
                        cgos_mode=case["cgos"])
        mode = TimeControl.STRICT_PLAYOUT if case["mode"] == "STRICT" else TimeControl.CONSTANT_PLAYOUT
        tree.search_best_move(board, case["color"], TimeManager(mode, case["visits"]), {})
    else:
        tree = MCTSTree(StubNet(salt=100 + case["seed"]), tree_size=160 if case["visits"] <= 100 else 2048)
        tree.generate_move_with_sequential_halving(board, case["color"], TimeManager(TimeControl.CONSTANT_PLAYOUT, case["visits"]), True)
    return tree, board
