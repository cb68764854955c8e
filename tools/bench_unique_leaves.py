#!/usr/bin/env python3
"""The UNIQUE leaf layout against the default one (tools/bench_selfplay.py's shard, `--unique-leaves` off / on), one session:

    python tools/bench_unique_leaves.py OUT.json [rounds]

Rows: 9x9 x 400 simulations with 16, 64 and 1 024 boards, 9x9 x 100 with 64 boards, 19x19 x 100 with 16 boards; per row the
two layouts alternate in ONE process (`rounds` times each, default 3, after a warm-up of both; every run plays max(boards,
256) games to their end at 9x9, one per board at 19x19) and the median run of each is reported with their ratio - the yardstick is the off run of the same session.  One more on-row per 9x9 x 400 configuration runs
with TG_SP_SUBGROUPS=1 (the sub-group count and the forward caps were tuned for full-size launches), for information.  Every
row is a process of its own (the network, the handles and the knobs start fresh)."""
import json, os, statistics, subprocess, sys

ROWS = [(9, 400, 16), (9, 400, 64), (9, 400, 1024), (9, 100, 64), (19, 100, 16)]


def run_row(size, visits, boards, rounds, one_group):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    if one_group:
        os.environ["TG_DEBUG_KNOBS"] = "1"
        os.environ["TG_SP_SUBGROUPS"] = "1"
    import torch
    import bench_selfplay as bs
    from tamago_amd.nn.network.dual_net import DualNet
    torch.manual_seed(0)
    net = DualNet(torch.device("cuda:0"), size)
    for unique in (False, True):
        bs.warm_up(net, boards, size, unique)
    layouts = (True,) if one_group else (False, True)
    games = max(boards, 256) if size == 9 else boards        # (a timed run of about a second or more: at least 256 9x9 games)
    runs = {u: [] for u in layouts}
    for _ in range(rounds):
        for unique in layouts:
            runs[unique].append(bs.measure(net, boards, visits, games, 0, size, unique))
    out = {"size": size, "visits": visits, "boards": boards, "rounds": rounds, "one_sub_group": bool(one_group)}
    for unique, rs in runs.items():
        rs.sort(key=lambda r: r["seconds"])
        med = rs[len(rs) // 2]
        key = "on" if unique else "off"
        out[key] = {k: med[k] for k in ("games", "moves", "leaf_evals", "forward_positions", "range_fallbacks", "seconds",
                                        "games_per_s", "leaf_evals_per_s", "forward_positions_per_s", "forwarded_share")}
        out[key]["seconds_all"] = [r["seconds"] for r in rs]
    if "off" in out:
        out["on_over_off_games_per_s"] = out["on"]["games_per_s"] / out["off"]["games_per_s"]
        out["same_games"] = all(out["on"][k] == out["off"][k] for k in ("games", "moves", "leaf_evals"))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "--row":
        run_row(*(int(v) for v in sys.argv[2:7]))
        sys.exit(0)
    path, rounds = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rows = []
    jobs = [(s, v, b, 0) for s, v, b in ROWS] + [(s, v, b, 1) for s, v, b in ROWS if (s, v) == (9, 400)]
    for size, visits, boards, one_group in jobs:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", str(size), str(visits), str(boards),
                              str(rounds), str(one_group)], capture_output=True, text=True, timeout=1500)
        if res.returncode != 0:
            sys.exit(f"row {size}x{size} {visits} {boards}: exit {res.returncode}\n{res.stderr[-2000:]}")
        rows.append(json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]))
        print(json.dumps(rows[-1]), flush=True)
        with open(path, "w") as f:                       # (kept up to date row by row)
            json.dump({"tool": "tools/bench_unique_leaves.py", "rounds": rounds, "rows": rows}, f, indent=1)
            f.write("\n")
