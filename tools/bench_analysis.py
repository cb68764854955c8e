"""Batch analysis (tamago_amd.mcts.analysis.analyze_positions) against the per-position MCTSTree loop, on one GPU.

    python tools/bench_analysis.py [--quick] [--out profiles/analysis_bench.json]

Positions: plies of seeded random play-outs; network: a randomly initialised DualNet on the device forward; STRICT
PUCT visits.  Rows:
- 9x9, 1 000 visits: analyze_positions with max_trees T = 1, 64, 512, 2 048 and batch 16 / 256 (T positions per run; T = 1:
  8 positions), positions/s after one warm-up run;
- the same settings through a per-position MCTSTree loop (search_best_move + get_analysis("cgos") with the host PV walk)
  over 16 positions, positions/s;
- tg_search_read_analysis on one 2 048-tree batch against the host walk (MCTSTree.get_pv_lists's read_node chain), the
  host walk timed on 32 of the trees and scaled to 2 048;
- every position of 80 game records (9x9, 100 visits batch 16 and 1 000 visits batch 256, T = 2 048) end to end, set up by
  the host replay with its deep copy per position and, "device_roots": true, written on the device from the records - the
  same positions in the same process, the host row being the yardstick;
- 19x19, 1 600 visits, T = 256, batch 64.
Writes one JSON document (with build.source_digest()) and prints it."""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def positions(size, count, seed=0):
    import numpy as np
    from tamago_amd.board.go_board import GoBoard
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        board, color = GoBoard(size), 1
        for _ in range(rs.randint(0, size * 3)):
            legal = board.get_all_legal_pos(color)
            board.put_stone(int(legal[rs.randint(len(legal))]), color)
            color = 3 - color
        out.append((copy.deepcopy(board), color))
    return out


def network(size):
    import torch
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), size)
    net.load_state_dict(make_state_dict(size, 11, 1.4))
    return net


def batched(net, pos, visits, batch, trees):
    import torch
    from tamago_amd.mcts.analysis import analyze_positions
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = analyze_positions(net, pos, visits, batch_size=batch, max_trees=trees)
    for a in res:
        a.cgos()
    torch.cuda.synchronize()
    return len(pos) / (time.perf_counter() - t0)


def single_loop(net, pos, visits, batch):
    import numpy as np
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    tree = MCTSTree(net, tree_size=visits + 16, batch_size=batch)
    t0 = time.perf_counter()
    for k, (board, color) in enumerate(pos):
        np.random.seed(k)
        tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, visits), {})
        root = tree.get_root()
        if root.node_visits:
            root.get_analysis(board, "cgos", tree.get_pv_lists)
    return len(pos) / (time.perf_counter() - t0)


def readout(net, pos, visits, batch):
    """(kernel read-out ms, host walk ms scaled to all trees, trees) on one searched batch."""
    import numpy as np
    import torch
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.mcts.engine import SearchEngine, continue_pv, evaluator_for
    engine = SearchEngine(9, len(pos), visits + 16, batch, evaluator_for(net))
    for k, (board, color) in enumerate(pos):
        engine.set_root(k, board, color, np.random.RandomState(k).get_state())
    engine.root_eval()
    engine.puct_chain([batch] * (visits // batch) + ([visits % batch] if visits % batch else []))
    coord = Coordinate(9)
    engine.read_analysis(32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ana = engine.read_analysis(32)
    lists = [f(root, coord) for root, f in ana]
    kernel_ms = 1e3 * (time.perf_counter() - t0)
    sample = 32
    t0 = time.perf_counter()
    for t in range(sample):
        root = engine.read_node(t, 0)
        for i in range(root.num_children):
            if root.children_visits[i] > 0:
                start = int(root.children_index[i])
                continue_pv([root.action[i]], start if start != -1 else engine.N - 1, lambda n: engine.read_node(t, n))
    host_ms = 1e3 * (time.perf_counter() - t0) * len(pos) / sample
    engine.close()
    return kernel_ms, host_ms, sum(len(x) for x in lists)


def game_records(size, games, seed=2):
    """Move lists of seeded random play-outs (legal moves, colours alternating from black)."""
    import numpy as np
    from tamago_amd.board.go_board import GoBoard
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(games):
        board, color, moves = GoBoard(size), 1, []
        for _ in range(rs.randint(size * 2, size * 4)):
            legal = board.get_all_legal_pos(color)
            moves.append(int(legal[rs.randint(len(legal))]))
            board.put_stone(moves[-1], color)
            color = 3 - color
        out.append(moves)
    return out


def game_leg(net, recs, size, visits, batch, trees, device_roots):
    """Every position of the records (the final ones included) end to end: the host replay with a deep copy per position
    that game_positions makes, or the roots written on the device from the records.  (positions/s, seconds of the replay,
    positions)."""
    import torch
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.analysis import analyze_positions
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if device_roots:
        members = [(g, k) for g, moves in enumerate(recs) for k in range(len(moves) + 1)]
        t1 = time.perf_counter()
        res = analyze_positions(net, members, visits, batch_size=batch, max_trees=trees, records=recs, board_size=size)
    else:
        members = []
        for moves in recs:
            board, color = GoBoard(size), 1
            for pos in moves + [None]:
                members.append((copy.deepcopy(board), color))
                if pos is not None:
                    board.put_stone(pos, color)
                    color = 3 - color
        t1 = time.perf_counter()
        res = analyze_positions(net, members, visits, batch_size=batch, max_trees=trees)
    for a in res:
        if a.visits:
            a.cgos()
    torch.cuda.synchronize()
    return len(members) / (time.perf_counter() - t0), t1 - t0, len(members)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="T <= 64 and no 19x19 row (a smoke run of the tool)")
    ap.add_argument("--out", default=os.path.join("profiles", "analysis_bench.json"))
    args = ap.parse_args()
    from tamago_amd import build
    net9 = network(9)
    pool = positions(9, 2048)
    rows = []
    trees_list = (1, 64) if args.quick else (1, 64, 512, 2048)
    for batch in (16, 256):
        batched(net9, pool[:8], 1000, batch, 8)                       # warm-up
        for trees in trees_list:
            count = max(trees, 8)
            rate = batched(net9, pool[:count], 1000, batch, trees)
            rows.append({"size": 9, "visits": 1000, "batch": batch, "trees": trees, "positions": count,
                         "batched_positions_per_s": round(rate, 2)})
            print(json.dumps(rows[-1]), flush=True)
        single_loop(net9, pool[:2], 1000, batch)                       # warm-up
        rate = single_loop(net9, pool[:16], 1000, batch)
        rows.append({"size": 9, "visits": 1000, "batch": batch, "loop_positions": 16,
                     "single_tree_loop_positions_per_s": round(rate, 2)})
        print(json.dumps(rows[-1]), flush=True)
    n = 64 if args.quick else 2048
    kernel_ms, host_ms, pvs = readout(net9, pool[:n], 1000, 256)
    rows.append({"readout_trees": n, "pv_lists": pvs, "kernel_readout_ms": round(kernel_ms, 2),
                 "host_walk_ms_scaled": round(host_ms, 1)})
    print(json.dumps(rows[-1]), flush=True)
    # game records, every position of them: the host replay against the roots written on the device, in this process
    recs = game_records(9, 4 if args.quick else 80)
    for visits, batch in ((100, 16), (1000, 256)):
        game_leg(net9, recs[:1], 9, visits, batch, 64, False)          # warm-up
        game_leg(net9, recs[:1], 9, visits, batch, 64, True)
        for device_roots in (False, True):
            rate, replay, count = game_leg(net9, recs, 9, visits, batch, 64 if args.quick else 2048, device_roots)
            rows.append({"size": 9, "visits": visits, "batch": batch, "trees": 64 if args.quick else 2048, "games": len(recs),
                         "positions": count, "device_roots": device_roots, "game_positions_per_s": round(rate, 2),
                         "host_replay_seconds": round(replay, 3)})
            print(json.dumps(rows[-1]), flush=True)
    if not args.quick:
        net19 = network(19)
        pool19 = positions(19, 256, 1)
        batched(net19, pool19[:4], 1600, 64, 4)
        rate = batched(net19, pool19, 1600, 64, 256)
        rows.append({"size": 19, "visits": 1600, "batch": 64, "trees": 256, "positions": 256,
                     "batched_positions_per_s": round(rate, 2)})
        print(json.dumps(rows[-1]), flush=True)
    doc = {"source_digest": build.source_digest(), "rows": rows}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
