"""Tree reuse (MCTSTree(reuse_tree=True)) against the rebuilt tree: one tree plays both sides of a game, move after move,
with reuse off and on.

    python tools/bench_reuse.py [--moves 30] [--sizes 9,19] [--only on|off|both]

9x9: 1 000 STRICT_PLAYOUT visits, batch 256; 19x19: 1 600 STRICT_PLAYOUT visits, batch 64 (a randomly initialised
DualNet on the device forward).  Prints one JSON line per (size, mode): ms per move (after one warm-up move), descents run
per move, the share of the visit budget the reused trees started with.  The compaction kernels' own time comes from a
separate run under `rocprofv3 --kernel-trace --stats -- python tools/bench_reuse.py --only on` (kernels reroot_*)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIG = {9: (1000, 256), 13: (1000, 128), 19: (1600, 64)}


def play(size, moves, reuse, seed=0):
    import numpy as np
    import torch
    from tamago_amd.board.constant import PASS, RESIGN
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    from tamago_amd.nn.network.dual_net import DualNet
    visits, batch = CONFIG[size]
    torch.manual_seed(seed)
    net = DualNet(torch.device("cuda:0"), size)
    tree = MCTSTree(net, tree_size=1 << 16, batch_size=batch, reuse_tree=reuse)
    board = GoBoard(size, 7.0, False)
    np.random.seed(seed)
    color, times, descents, reused = 1, [], [], []
    for k in range(moves + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mv = tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, visits), {})
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        root_visits = int(tree.get_root().node_visits)
        if k > 0:                                       # (move 0: warm-up)
            times.append(dt)
            descents.append(root_visits - tree.reused_visits)
            reused.append(tree.reused_visits)
        if mv == RESIGN:
            mv = PASS
        board.put_stone(mv, color)
        color = 3 - color
    return {"size": size, "visits": visits, "batch": batch, "reuse_tree": reuse, "moves": moves,
            "ms_per_move": round(1e3 * sum(times) / len(times), 2),
            "descents_per_move": round(sum(descents) / len(descents), 1),
            "reused_share": round(sum(reused) / (visits * len(reused)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--moves", type=int, default=30)
    ap.add_argument("--sizes", default="9,19")
    ap.add_argument("--only", choices=("on", "off", "both"), default="both")
    args = ap.parse_args()
    modes = {"on": [True], "off": [False], "both": [False, True]}[args.only]
    for size in (int(s) for s in args.sizes.split(",")):
        for reuse in modes:
            print(json.dumps(play(size, args.moves, reuse)), flush=True)


if __name__ == "__main__":
    main()
