"""Training-data generation from game records on one GPU: the host path (device_replay=False: Python board, one featurise
launch per chunk) against the device path (device_replay=True: tg_replay_run) of the same checkout, on the same records.

    python tools/bench_datagen.py [--quick] [--runs 3] [--out profiles/datagen_replay_bench.json]

  RL leg   9x9 records of a small selfplay_shard run (random network, 16 visits), generate_reinforcement_learning_data
  SL leg   19x19 records written from the moves tg_policy_games_results returns (two random networks, at most 300 moves),
           generate_supervised_learning_data

Every step that uses the GPU - making the records, each timed path of each leg - is a process of its own under a time limit
of its own; the first step that fails ends the run.  A timed step runs its generator once on two records (library and code
objects loaded, the handle's first allocations made) and then `runs` times on all of them.  Per run the wall time of the
call, split by wrapping the functions of tamago_amd.nn.data_generator (exclusive times, so nothing is counted twice):

  parse          host: SGFReader;                       device: _sl_record / _rl_record (SGFReader + choice of samples)
  replay_planes  host: put_stone, _Samples.add (descriptors), _Samples.planes (upload, featurise kernel, planes to host)
                 device: _ReplayPending._replay (upload, replay_samples_kernel, flags back) + planes to host
  targets        host: generate_target_data / generate_rl_target_data;   device: _ReplayPending._targets
  write          np.savez_compressed and the array conversions around it
  other          the rest of the call (loops, chunk bookkeeping)

The last run's files of the two paths are compared array by array.  Writes one JSON document: games/s per path (median,
min, max over the runs), milliseconds per game and stage (median run), the ratio device / host of games/s."""
import argparse
import glob
import hashlib
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

STEP_LIMITS = {"records-rl": 300, "records-sl": 300, "time": 600}     # seconds per process


# ---- steps (each runs in a process of its own) ---------------------------------------------------------------------------
def make_rl_records(work, games):
    import torch
    from tamago_amd.nn.network.dual_net import DualNet
    from tamago_amd.selfplay.worker import selfplay_shard
    torch.manual_seed(7)
    net = DualNet(torch.device("cuda:0"), 9)
    out = os.path.join(work, "rl_kifu")
    os.makedirs(out, exist_ok=True)
    t0 = time.perf_counter()
    stats = selfplay_shard(out, net, list(range(1, games + 1)), 9, 16, boards=games)
    return {"games": stats["games"], "seconds": round(time.perf_counter() - t0, 2)}


def make_sl_records(work, games):
    import torch
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.nn.network.dual_net import DualNet
    from tamago_amd.nn.policy_player import policy_games
    torch.manual_seed(41)
    black = DualNet(torch.device("cuda:0"), 19)
    torch.manual_seed(42)
    white = DualNet(torch.device("cuda:0"), 19)
    res = policy_games(black, white, games, size=19, boards=games, max_moves=300)
    coordinate = Coordinate(19)
    out = os.path.join(work, "sl_kifu")
    os.makedirs(out, exist_ok=True)
    total = 0
    for g, game in enumerate(res["games"]):
        result = {"black": "B+R", "white": "W+R"}.get(game["winner"], "0")
        body = "".join(f";{'BW'[i % 2]}[{'' if pos == 0 else coordinate.convert_to_sgf_format(int(pos))}]"
                       for i, pos in enumerate(game["moves"]))
        with open(os.path.join(out, f"{g + 1:05d}.sgf"), "w", encoding="utf-8") as f:
            f.write(f"(;FF[4]GM[1]SZ[19]PB[a]PW[b]RE[{result}]KM[7.0]{body})\n")
        total += game["length"]
    return {"games": games, "mean_moves": round(total / games, 1)}


class Stages:
    """Exclusive wall time per stage: a wrapped call's time goes to its stage, less what wrapped calls inside it took."""

    def __init__(self):
        self.seconds = {}
        self.stack = []

    def wrap(self, owner, name, stage):
        inner = getattr(owner, name)

        def timed(*args, **kwargs):
            self.stack.append(0.0)
            t0 = time.perf_counter()
            try:
                return inner(*args, **kwargs)
            finally:
                spent = time.perf_counter() - t0
                below = self.stack.pop()
                self.seconds[stage] = self.seconds.get(stage, 0.0) + spent - below
                if self.stack:
                    self.stack[-1] += spent
        setattr(owner, name, timed)

    def take(self):
        out, self.seconds = self.seconds, {}
        return out


def timed_path(work, leg, device_replay, runs):
    import torch
    import tamago_amd.nn.data_generator as dg
    from tamago_amd.board.go_board import GoBoard
    size = 9 if leg == "rl" else 19
    kifu = os.path.join(work, f"{leg}_kifu")
    stages = Stages()
    if device_replay:
        stages.wrap(dg, "_sl_record", "parse")
        stages.wrap(dg, "_rl_record", "parse")
        stages.wrap(dg._ReplayPending, "_replay", "replay_planes")
        stages.wrap(dg, "_planes_to_host", "replay_planes")
        stages.wrap(dg._ReplayPending, "_targets", "targets")
        stages.wrap(dg, "_save_arrays", "write")
    else:
        stages.wrap(dg, "SGFReader", "parse")
        stages.wrap(GoBoard, "put_stone", "replay_planes")
        stages.wrap(dg._Samples, "add", "replay_planes")
        stages.wrap(dg._Samples, "planes", "replay_planes")
        stages.wrap(dg, "generate_target_data", "targets")
        stages.wrap(dg, "generate_rl_target_data", "targets")
        stages.wrap(dg, "_save_data", "write")

    def generate(prog, source):
        shutil.rmtree(prog, ignore_errors=True)
        os.makedirs(os.path.join(prog, "data"))
        import random
        import numpy as np
        random.seed(5)
        np.random.seed(5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if leg == "rl":
            dg.generate_reinforcement_learning_data(prog, [source], size, device_replay=device_replay)
        else:
            dg.generate_supervised_learning_data(prog, source, size, device_replay=device_replay)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    warm = os.path.join(work, f"{leg}_warm")
    shutil.rmtree(warm, ignore_errors=True)
    os.makedirs(warm)
    for path in sorted(glob.glob(os.path.join(kifu, "*.sgf")))[:2]:
        shutil.copy(path, warm)
    batch = dg.BATCH_SIZE
    dg.BATCH_SIZE = 8                                   # (two records are less than one mini-batch of 256)
    generate(os.path.join(work, "warm_prog"), warm)
    dg.BATCH_SIZE = batch
    stages.take()
    games = len(glob.glob(os.path.join(kifu, "*.sgf")))
    prog = os.path.join(work, f"{leg}_{'device' if device_replay else 'host'}")
    seconds, split = [], []
    for _ in range(runs):
        seconds.append(generate(prog, kifu))
        part = stages.take()
        part["other"] = seconds[-1] - sum(part.values())
        split.append(part)
    digest, samples = {}, 0
    import numpy as np
    for path in sorted(glob.glob(os.path.join(prog, "data", "*.npz"))):
        z = np.load(path)
        samples += len(z["value"])
        for key in ("input", "policy", "value", "kifu_count"):
            a = np.ascontiguousarray(z[key])
            digest[f"{os.path.basename(path)}:{key}"] = f"{a.dtype}{list(a.shape)}{hashlib.sha256(a.tobytes()).hexdigest()}"
    median = sorted(range(runs), key=lambda i: seconds[i])[runs // 2]
    out = {"games": games, "samples_written": samples, "runs": runs,
           "seconds": {"median": round(statistics.median(seconds), 4), "min": round(min(seconds), 4), "max": round(max(seconds), 4)},
           "games_per_s": {"median": round(games / statistics.median(seconds), 2), "min": round(games / max(seconds), 2),
                           "max": round(games / min(seconds), 2)},
           "ms_per_game": {k: round(1e3 * v / games, 4) for k, v in sorted(split[median].items())},
           "digest": digest}
    if device_replay:
        out["replay_stats"] = dict(dg.REPLAY_STATS)
    return out


# ---- the run ---------------------------------------------------------------------------------------------------------------
def step(args, limit):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    print("[bench_datagen]", " ".join(args), flush=True)
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit, cwd=REPO)
    if res.returncode != 0:
        raise SystemExit(f"step {args} ended with status {res.returncode}: nothing further is started")
    line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
    print(line if len(line) < 2000 else line[:2000] + " ...", flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="64 self-play records and 4 policy-game records (a smoke run of the tool)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "datagen_replay_bench.json"))
    ap.add_argument("--step", default=None)
    ap.add_argument("--work", default=None)
    ap.add_argument("--games", type=int, default=0)
    ap.add_argument("--leg", default="rl")
    ap.add_argument("--device-replay", type=int, default=0)
    args = ap.parse_args()
    if args.step == "records-rl":
        print(json.dumps(make_rl_records(args.work, args.games)))
        return
    if args.step == "records-sl":
        print(json.dumps(make_sl_records(args.work, args.games)))
        return
    if args.step == "time":
        print(json.dumps(timed_path(args.work, args.leg, bool(args.device_replay), args.runs)))
        return
    from tamago_amd import build
    work = tempfile.mkdtemp(prefix="bench_datagen_")
    try:
        doc = {"source_digest": build.source_digest(), "legs": {}}
        rl_games, sl_games = (64, 4) if args.quick else (256, 16)
        doc["records"] = {"rl": step(["--step", "records-rl", "--work", work, "--games", str(rl_games)], STEP_LIMITS["records-rl"]),
                          "sl": step(["--step", "records-sl", "--work", work, "--games", str(sl_games)], STEP_LIMITS["records-sl"])}
        for leg in ("rl", "sl"):
            rows = {}
            for name, flag in (("host", 0), ("device", 1)):
                rows[name] = step(["--step", "time", "--work", work, "--leg", leg, "--device-replay", str(flag),
                                   "--runs", str(args.runs)], STEP_LIMITS["time"])
            identical = rows["host"].pop("digest") == rows["device"].pop("digest")
            doc["legs"][leg] = {"board_size": 9 if leg == "rl" else 19, "host": rows["host"], "device": rows["device"],
                                "files_identical": identical,
                                "device_over_host_games_per_s": round(rows["device"]["games_per_s"]["median"] /
                                                                      rows["host"]["games_per_s"]["median"], 2)}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
