#!/usr/bin/env python3
"""Golden batch analysis (tests/test_gpu_analysis.py): the REFERENCE's own single-tree search and analysis strings for
the positions of the self-play record tests/golden/selfplay_games.json["1,16"], with the deterministic stub network of
the tree fixtures.  Needs a checkout of the reference project, imported from its own directory (never copied):

    PYTHONPATH=<reference checkout>:<this repository> python tools/gen_golden_analysis.py

For position k (the board before move k + 1, the final position last) of every other position (k even) and with seed
5 + k: np.random.seed(5 + k); MCTSTree(StubNet(8), tree_size=76, batch_size=16).search_best_move(board, colour,
TimeManager(STRICT_PLAYOUT, 60), {}) and root.get_analysis(board, "lz" / "cgos", tree.get_pv_lists); superko on.
-> tests/golden/analysis_s9.json {game, seed0, visits, batch_size, tree_size, superko, positions: [{k, color, best, lz,
cgos}]} (the cgos string for every fourth position only, to keep the file small)."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAME, SEED0, VISITS, BATCH, STEP, CGOS_STEP = "1,16", 5, 60, 16, 2, 4


def main():
    from board.go_board import GoBoard
    from board.stone import Stone
    from mcts.time_manager import TimeControl, TimeManager
    from mcts.tree import MCTSTree
    from sgf.reader import SGFReader
    from oracle.stubnet import StubNet
    text = json.load(open(os.path.join(REPO, "tests", "golden", "selfplay_games.json")))[GAME]
    sgf = SGFReader(text, 9, literal=True)
    board = GoBoard(9, sgf.komi, True)
    n = sgf.get_n_moves()
    out = []
    devnull = open(os.devnull, "w")
    for k in range(n + 1):
        color = sgf.get_color(k) if k < n else board.get_to_move()
        if k % STEP == 0:
            np.random.seed(SEED0 + k)
            tree = MCTSTree(StubNet(8), tree_size=VISITS + 16, batch_size=BATCH)
            old_err, sys.stderr = sys.stderr, devnull
            try:
                best = tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, VISITS), {})
                root = tree.get_root()
                rec = {"k": k, "color": "B" if color == Stone.BLACK else "W", "best": int(best),
                       "lz": root.get_analysis(board, "lz", tree.get_pv_lists)}
                if k % CGOS_STEP == 0 and root.node_visits > 0:
                    rec["cgos"] = root.get_analysis(board, "cgos", tree.get_pv_lists)
            finally:
                sys.stderr = old_err
            out.append(rec)
        if k < n:
            board.put_stone(sgf.get_move_data(k), color)
    path = os.path.join(REPO, "tests", "golden", "analysis_s9.json")
    with open(path, "w") as f:
        json.dump({"game": GAME, "seed0": SEED0, "visits": VISITS, "batch_size": BATCH, "tree_size": VISITS + 16,
                   "superko": True, "positions": out}, f, indent=0)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "positions")


if __name__ == "__main__":
    main()
