"""Evaluation of a network on game records on one GPU: evaluate_records (records replayed, scored and reduced on the device)
against a host pipeline on the same records in the same process.

    python tools/bench_evaluate.py [--quick] [--runs 3] [--out profiles/evaluate_bench.json]

  9x9     self-play records (selfplay_shard as tools/selfplay_main.py drives it: a random network, 16 visits)
  19x19   records written from the moves of policy-against-policy games (two random networks, at most 300 moves): self-play at
          19x19 takes minutes per record set, and what is timed here does not depend on who played

Every step that uses the GPU - making the records, the timed leg of each board size - is a process of its own under a time
limit of its own; the first step that fails ends the run.  A timed leg evaluates two records once (library and code objects
loaded, first allocations made) and then

  device    evaluate_records on all records, `runs` times: positions/s by wall time (median, min, max), and the split of the
            median run between replay + masks, forward and scoring from timed events around the three stages
  host      GoBoard replay, generate_input_planes and the host candidate filter per position, tg_net_forward_host per chunk,
            numpy scoring - on the first `host_games` records (the Python board is the slow part): positions/s
  ceiling   the forward pass alone on resident planes at the chunk size, as tools/bench_net.py times it

Writes one JSON document."""
import argparse
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STEP_LIMITS = {"records": 300, "time": 500}           # seconds per process
CHUNK_ROWS = 65536


def make_records(work, size, games):
    import torch
    from tamago_amd.nn.network.dual_net import DualNet
    out = os.path.join(work, f"kifu{size}")
    os.makedirs(out, exist_ok=True)
    t0 = time.perf_counter()
    if size == 9:
        from tamago_amd.selfplay.worker import selfplay_shard
        torch.manual_seed(7)
        net = DualNet(torch.device("cuda:0"), 9)
        stats = selfplay_shard(out, net, list(range(1, games + 1)), 9, 16, boards=games)
        return {"games": stats["games"], "seconds": round(time.perf_counter() - t0, 2)}
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.nn.policy_player import policy_games
    torch.manual_seed(41)
    black = DualNet(torch.device("cuda:0"), size)
    torch.manual_seed(42)
    white = DualNet(torch.device("cuda:0"), size)
    res = policy_games(black, white, games, size=size, boards=games, max_moves=300)
    coordinate = Coordinate(size)
    for g, game in enumerate(res["games"]):
        result = {"black": "B+R", "white": "W+R"}.get(game["winner"], "0")
        body = "".join(f";{'BW'[i % 2]}[{'' if pos == 0 else coordinate.convert_to_sgf_format(int(pos))}]"
                       for i, pos in enumerate(game["moves"]))
        with open(os.path.join(out, f"{g + 1:05d}.sgf"), "w", encoding="utf-8") as f:
            f.write(f"(;FF[4]GM[1]SZ[{size}]PB[a]PW[b]RE[{result}]KM[7.0]{body})\n")
    return {"games": games, "seconds": round(time.perf_counter() - t0, 2)}


def host_evaluate(network, records, size, chunk_rows):
    """The host pipeline; returns (positions, top-1 count) - the count is there so that nothing is optimised away and so that
    the two paths can be seen to look at the same rows."""
    import numpy as np
    import torch
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.board.stone import Stone
    from tamago_amd.nn import evaluate as ev
    from tamago_amd.nn.feature import generate_input_planes
    positions = top1 = 0
    for g0, count in ev.chunk_games(records, 1, 0, chunk_rows):
        planes, masks, move = [], [], []
        for rec in records[g0:g0 + count]:
            board, color = GoBoard(size), Stone.BLACK
            actions = ev.move_actions(rec.moves, size)
            for i, pos in enumerate(rec.moves):
                planes.append(generate_input_planes(board, color, 0))
                masks.append(ev.candidate_words(board, color, size))
                move.append(int(actions[i]))
                board.put_stone(int(pos), color)
                color = Stone.get_opponent_color(color)
        policy, value = network.inference(torch.from_numpy(np.stack(planes).reshape(-1, 6, size, size)))
        policy, move = policy.numpy(), np.array(move)
        valid = move >= 0
        p_move = policy[np.arange(len(move)), np.where(valid, move, 0)]
        rank = (policy > p_move[:, None]).sum(axis=1) + ((policy == p_move[:, None]) & (np.arange(policy.shape[1])[None, :] < move[:, None])).sum(axis=1)
        bits = np.unpackbits(np.stack(masks).view(np.uint8), axis=1, bitorder="little")[:, :policy.shape[1]].astype(bool)
        mass = np.where(bits, policy.astype(np.float64), 0.0).sum(axis=1)
        assert mass.shape == rank.shape and value.shape[1] == 3
        positions += len(move)
        top1 += int(((rank == 0) & valid).sum())
    return positions, top1


def timed_leg(work, size, runs, host_games):
    import torch
    from tamago_amd.nn import evaluate as ev
    from tamago_amd.nn.network.dual_net import DualNet
    torch.manual_seed(3)
    net = DualNet(torch.device("cuda:0"), size)
    paths = sorted(glob.glob(os.path.join(work, f"kifu{size}", "*.sgf")))
    records = ev.as_records(paths, size)
    ev.evaluate_records(net, records[:2], size)
    host_evaluate(net, records[:2], size, CHUNK_ROWS)
    seconds, splits, report = [], [], None
    for _ in range(runs):
        timing = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        report = ev.evaluate_records(net, records, size, chunk_rows=CHUNK_ROWS, timing=timing)
        torch.cuda.synchronize()
        seconds.append(time.perf_counter() - t0)
        splits.append(timing)
    positions = report["positions"]
    median = sorted(range(runs), key=lambda i: seconds[i])[runs // 2]
    t0 = time.perf_counter()
    host_positions, host_top1 = host_evaluate(net, records[:host_games], size, CHUNK_ROWS)
    host_seconds = time.perf_counter() - t0
    # the forward pass alone at the size of the (largest) chunk
    b = min(positions, CHUNK_ROWS)
    x = torch.randint(-1, 2, (b, 6, size, size), device="cuda").float()
    out = (torch.empty((b, size * size + 1), device="cuda"), torch.empty((b, 3), device="cuda"))
    for _ in range(3):
        net.forward_device(x, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        net.forward_device(x, out=out)
    e1.record()
    torch.cuda.synchronize()
    forward_ms = e0.elapsed_time(e1) / 10
    device_rate = positions / statistics.median(seconds)
    return {"board_size": size, "games": len(records), "positions": positions, "runs": runs, "chunk_rows": CHUNK_ROWS,
            "device": {"seconds": {"median": round(statistics.median(seconds), 4), "min": round(min(seconds), 4), "max": round(max(seconds), 4)},
                       "positions_per_s": {"median": round(device_rate), "min": round(positions / max(seconds)),
                                           "max": round(positions / min(seconds))},
                       "event_ms_median_run": {k: round(v, 3) for k, v in sorted(splits[median].items())},
                       "games_redone_on_host": len(report["host_games"]), "range_fallbacks": report["range_fallbacks"],
                       "totals": report["totals"]},
            "host": {"games": min(host_games, len(records)), "positions": host_positions, "seconds": round(host_seconds, 3),
                     "positions_per_s": round(host_positions / host_seconds, 1), "top1_rows": host_top1},
            "forward_only": {"batch": b, "ms": round(forward_ms, 4), "positions_per_s": round(b / forward_ms * 1e3)},
            "device_over_host": round(device_rate / (host_positions / host_seconds), 1),
            "device_over_forward_only": round(device_rate / (b / forward_ms * 1e3), 4)}


def step(args, limit):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    print("[bench_evaluate]", " ".join(args), flush=True)
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit, cwd=REPO)
    if res.returncode != 0:
        raise SystemExit(f"step {args} ended with status {res.returncode}: nothing further is started")
    line = [text for text in res.stdout.splitlines() if text.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="32 9x9 records and 4 19x19 records (a smoke run of the tool)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "evaluate_bench.json"))
    ap.add_argument("--step", default=None)
    ap.add_argument("--work", default=None)
    ap.add_argument("--size", type=int, default=9)
    ap.add_argument("--games", type=int, default=0)
    ap.add_argument("--host-games", type=int, default=2)
    args = ap.parse_args()
    if args.step == "records":
        print(json.dumps(make_records(args.work, args.size, args.games)))
        return
    if args.step == "time":
        print(json.dumps(timed_leg(args.work, args.size, args.runs, args.host_games)))
        return
    from tamago_amd import build
    work = tempfile.mkdtemp(prefix="bench_evaluate_")
    try:
        doc = {"source_digest": build.source_digest(), "records": {}, "legs": {}}
        plan = {9: (32, 4), 19: (4, 1)} if args.quick else {9: (256, 16), 19: (32, 2)}          # size -> (games, host games)
        for size, (games, host_games) in plan.items():
            doc["records"][str(size)] = step(["--step", "records", "--work", work, "--size", str(size), "--games", str(games)],
                                             STEP_LIMITS["records"])
            doc["legs"][str(size)] = step(["--step", "time", "--work", work, "--size", str(size), "--runs", str(args.runs),
                                           "--host-games", str(host_games)], STEP_LIMITS["time"])
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
