"""Policy-only games on the device (tamago_amd.nn.policy_player.policy_games) on one GPU.

    python tools/bench_policy_games.py [--quick] [--out profiles/policy_games_bench.json]
    python tools/bench_policy_games.py --trace SIZE,BOARDS       # a short run for `rocprofv3 --kernel-trace --stats -- ...`
    python tools/bench_policy_games.py --kernel-table DB --out profiles/policy_games_bench.json   # add that run's per-kernel table

Two randomly initialised DualNets play each other.  Per (board size, boards) row, `runs` runs of 8 x boards games (19x19:
4 x boards) after a warm-up run, median and range of
- games/s and plies/s (= positions forwarded per second: every ply forwards one position per board) over the whole call -
  streams seeded, handles created, results turned into Python objects - and plies/s over the ply loop alone,
- the share of forwarded positions that belonged to parked slots (a slot waits for an even ply, and for the last games of a
  run),
- the forward-only rate at the same batch (the loop of tools/bench_net.py), the ceiling of plies/s.
Baseline: what the library allowed before this path - the host path of generate_move_from_policy, one DualNet.inference
per move followed by Python - over the first games of the same run (same seeds, same rule), games/s, median of 3 runs.
Writes one JSON document (with build.source_digest()) and prints it."""
import argparse
import json
import os
import random
import sqlite3
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def networks(size):
    import torch
    from tamago_amd.nn.network.dual_net import DualNet
    torch.manual_seed(41)
    black = DualNet(torch.device("cuda:0"), size)
    torch.manual_seed(42)
    return black, DualNet(torch.device("cuda:0"), size)


def device_run(nets, size, boards, games, max_moves):
    """(seconds, result) of one policy_games run, the clock stopped behind a device synchronise."""
    import torch
    from tamago_amd.nn.policy_player import policy_games
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = policy_games(nets[0], nets[1], games, size=size, boards=boards, max_moves=max_moves)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


class HostOnly:
    """A DualNet seen through its host API alone: generate_move_from_policy then takes the path every network object that is
    no DualNet takes - inference, then Python."""

    def __init__(self, net):
        self.net = net

    def inference(self, planes):
        return self.net.inference(planes)


def host_games(nets, size, games, max_moves):
    """The same games on the host path: seconds for `games` games (seeds 0.., the pass rule of gtp/client.py:209-211)."""
    from tamago_amd.board.constant import PASS
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.nn.policy_player import generate_move_from_policy
    players = HostOnly(nets[0]), HostOnly(nets[1])
    t0 = time.perf_counter()
    moves = 0
    for g in range(games):
        random.seed(g)
        board, color, passes = GoBoard(size, 7.0, True), 1, 0
        for _ in range(max_moves):
            pos = generate_move_from_policy(players[color - 1], board, color)
            if board.moves > 1 and board.prev_move(1) == PASS:
                pos = PASS
            board.put_stone(pos, color)
            moves += 1
            passes = passes + 1 if pos == PASS else 0
            color = 3 - color
            if passes == 2:
                break
    return time.perf_counter() - t0, moves


def forward_only(net, size, batch, iters=20):
    import torch
    x = torch.randint(-1, 2, (batch, 6, size, size), device="cuda").float()
    out = (torch.empty((batch, size * size + 1), device="cuda"), torch.empty((batch, 3), device="cuda"))
    for _ in range(3):
        net.forward_device(x, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        net.forward_device(x, out=out)
    e1.record()
    torch.cuda.synchronize()
    return batch * iters / (e0.elapsed_time(e1) * 1e-3)


def spread(values):
    return {"median": round(statistics.median(values), 2), "min": round(min(values), 2), "max": round(max(values), 2)}


def row(nets, size, boards, games, max_moves, runs):
    device_run(nets, size, min(boards, 64), min(boards, 64), max_moves)        # warm-up: code objects, the small launches
    device_run(nets, size, boards, boards, 8)                                  # ... and this batch's forward kernel
    gps, pps, loop_pps, parked, lengths, parts = [], [], [], [], [], []
    for _ in range(runs):
        seconds, res = device_run(nets, size, boards, games, max_moves)
        played = sum(g["length"] for g in res["games"])
        gps.append(games / seconds)
        pps.append(res["positions"] / seconds)
        loop_pps.append(res["positions"] / (res["seconds"][1] + res["seconds"][2]))     # first ply enqueued .. device drained
        parked.append(1.0 - played / res["positions"])
        lengths.append(played / games)
        parts.append(res["seconds"])
    ceiling = forward_only(nets[0], size, boards)
    out = {"size": size, "boards": boards, "games": games, "max_moves": max_moves, "runs": runs,
           "games_per_s": spread(gps), "plies_per_s": spread(pps), "plies_per_s_ply_loop_only": spread(loop_pps),
           "seconds_setup_enqueue_drain_objects": [round(statistics.median(p[k] for p in parts), 4) for k in range(4)],
           "plies": res["plies"], "parked_share": round(statistics.median(parked), 4),
           "mean_length": round(statistics.median(lengths), 1), "unfinished": sum(g["winner"] is None for g in res["games"]),
           "forward_only_positions_per_s": round(ceiling, 0),
           "plies_over_forward_only": round(statistics.median(pps) / ceiling, 3),
           "ply_loop_over_forward_only": round(statistics.median(loop_pps) / ceiling, 3)}
    print(json.dumps(out), flush=True)
    return out


def baseline(nets, size, games, max_moves):
    host_games(nets, size, 1, 10)
    rates, moves = [], 0
    for _ in range(3):
        seconds, moves = host_games(nets, size, games, max_moves)
        rates.append(games / seconds)
    out = {"size": size, "host_path_games": games, "host_path_moves": moves, "max_moves": max_moves,
           "host_path_games_per_s": spread(rates)}
    print(json.dumps(out), flush=True)
    return out


def kernel_table(db_path):
    """Per-kernel totals of a `rocprofv3 --kernel-trace --stats` run (its rocpd sqlite database)."""
    cur = sqlite3.connect(db_path).cursor()
    rows = list(cur.execute("select name, count(*), sum(duration), avg(duration), min(duration), max(duration), max(grid_x), "
                            "max(workgroup_x), max(lds_size), max(vgpr_count) from kernels group by name "
                            "order by sum(duration) desc"))
    total = sum(r[2] for r in rows) or 1
    return [{"kernel": r[0], "calls": r[1], "total_us": round(r[2] / 1e3, 1), "avg_us": round(r[3] / 1e3, 2),
             "min_us": round(r[4] / 1e3, 2), "max_us": round(r[5] / 1e3, 2), "share": round(r[2] / total, 4), "grid_x": r[6],
             "workgroup_x": r[7], "lds_bytes": r[8], "vgprs": r[9]} for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="64 and 1 024 boards at 9x9, 256 at 19x19 (a smoke run of the tool)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--trace", default=None, help="SIZE,BOARDS: one run of BOARDS games for a kernel trace, nothing written")
    ap.add_argument("--kernel-table", default=None, help="rocpd database of a traced run: its per-kernel table goes into --out")
    ap.add_argument("--trace-title", default="")
    ap.add_argument("--out", default=os.path.join("profiles", "policy_games_bench.json"))
    args = ap.parse_args()
    if args.kernel_table:
        with open(args.out) as f:
            doc = json.load(f)
        doc.setdefault("kernel_tables", []).append({"run": args.trace_title, "kernels": kernel_table(args.kernel_table)})
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
        print(json.dumps(doc["kernel_tables"][-1]))
        return
    if args.trace:
        size, boards = (int(v) for v in args.trace.split(","))
        nets = networks(size)
        seconds, res = device_run(nets, size, boards, boards, None)
        print(json.dumps({"size": size, "boards": boards, "plies": res["plies"], "seconds": round(seconds, 3)}))
        return
    from tamago_amd import build
    rows, baselines = [], []
    nets9 = networks(9)
    for boards in ((64, 1024) if args.quick else (64, 1024, 4096, 16384)):
        rows.append(row(nets9, 9, boards, 8 * boards, None, args.runs))
    baselines.append(baseline(nets9, 9, 4, 162))
    nets19 = networks(19)
    for boards in ((256,) if args.quick else (256, 4096)):
        rows.append(row(nets19, 19, boards, 4 * boards, None, args.runs))
    baselines.append(baseline(nets19, 19, 1, 722))
    doc = {"source_digest": build.source_digest(), "rows": rows, "baseline": baselines}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
