#!/usr/bin/env python3
"""Throughput of the lock-step Gumbel self-play shard (BASELINE.json configs 3 / 4): argv = boards, visits, games, groups (0: default), board size (9).
Switches (anywhere on the command line): --unique-leaves = evaluate each distinct leaf of a halving phase once
(selfplay_shard(unique_leaves=True)); --json = one JSON line with the figures as well."""
import json, os, sys, time, tempfile, shutil
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")          # before torch loads the HIP runtime (tamago_amd/__init__.py)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from tamago_amd.nn.network.dual_net import DualNet
from tamago_amd.selfplay.worker import selfplay_shard


def measure(net, boards, visits, games, groups, size, unique):
    """One timed shard: `games` games on `boards` boards, every game played to its end."""
    out = tempfile.mkdtemp(prefix="sp_")
    try:
        t0 = time.time()
        stats = selfplay_shard(out, net, list(range(1, games + 1)), size, visits, boards=boards,
                               never_resign_flags=[True] * games, groups=groups, unique_leaves=unique)
        torch.cuda.synchronize()
        dt = time.time() - t0
    finally:
        shutil.rmtree(out, ignore_errors=True)
    return {"size": size, "boards": boards, "visits": visits, "groups": groups, "unique_leaves": bool(unique),
            "games": stats["games"], "moves": stats["moves"], "leaf_evals": stats["leaf_evals"],
            "forward_positions": stats["forward_positions"], "range_fallbacks": stats["range_fallbacks"], "seconds": dt,
            "games_per_s": stats["games"] / dt, "leaf_evals_per_s": stats["leaf_evals"] / dt,
            "forward_positions_per_s": stats["forward_positions"] / dt,
            "forwarded_share": stats["forward_positions"] / max(stats["leaf_evals"], 1)}


def warm_up(net, boards, size, unique=False):
    n = min(boards, 4)
    out = tempfile.mkdtemp(prefix="sp_")
    try:
        selfplay_shard(out, net, list(range(1000, 1000 + n)), size, 16, boards=n, never_resign_flags=[False] * n,
                       unique_leaves=unique)
    finally:
        shutil.rmtree(out, ignore_errors=True)


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    unknown = [f for f in flags if f not in ("--unique-leaves", "--json")]
    if unknown:
        sys.exit(f"unknown switch {unknown[0]} (--unique-leaves, --json)")
    unique = "--unique-leaves" in flags
    boards = int(argv[0]) if len(argv) > 0 else 16
    visits = int(argv[1]) if len(argv) > 1 else 400
    games = int(argv[2]) if len(argv) > 2 else boards
    groups = int(argv[3]) if len(argv) > 3 else 0
    size = int(argv[4]) if len(argv) > 4 else 9
    torch.manual_seed(0)
    net = DualNet(torch.device("cuda:0"), size)
    # warm-up: one short batch of games
    warm_up(net, boards, size, unique)
    r = measure(net, boards, visits, games, groups, size, unique)
    print(f"selfplay {size}x{size} boards={boards} groups={groups or 'auto'} visits={visits}"
          f"{' unique-leaves' if unique else ''}: {r['games']} games, {r['moves']} moves, "
          f"{r['leaf_evals']} leaf-evals ({r['forward_positions']} positions forwarded) in {r['seconds']:.1f} s -> "
          f"{r['leaf_evals_per_s']:.0f} leaf-evals/s, {r['games_per_s'] * 3600:.0f} games/hour")
    if "--json" in flags:
        print(json.dumps(r))
