"""What playing a round robin in ONE lock-step engine gains or loses against the same games played as duels, in one
process on one device:

    python tools/bench_tournament.py [--entrants 2 4 8] [--boards 256 2048] [--visits 1000] [--batch 256] [--rounds-per-board 1]
                                     [--repeats 2] [--time-kernels] [--out profiles/tournament_bench.json]

Workload: 9x9, visits x batch, G random-init scaled DualNets, one game per ordered pair and slot - games_per_pair = boards x
rounds-per-board, so G (G - 1) x that many games.  Leg "tournament": puct_tournament on `boards` slots.  Leg "duels": the SAME
games - same black network, white network and seed - as G (G - 1) consecutive puct_match(..., compact_idle=True) calls of
`boards` slots each, the best way to get them without the tournament.  The legs alternate (the host is shared), `repeats`
passes per leg after a warm-up of the first setting.  That the games are the same is checked by a digest of the records of
both legs (an assertion, not a figure).

Per setting: games/s of every pass, best, median and spread (max - min) / median per leg; the positions the launches
evaluated and the positions that belonged to live searching games (leaf_evals); the forward launches per mini-batch of the
tournament and their mean size (positions / launches), against one launch per mini-batch of a duel; gain = median games/s of
the tournament over the duels.  --time-kernels: the time of group_rank_kernel (with its read-back) and of one gather and one
scatter launch alone at T = boards, from timed events around repeated launches.

The expectation to confirm or refute: one tail instead of G (G - 1) tails and no parity parking outweigh G smaller forward
launches per mini-batch.  Nothing is asserted about the rates.  19x19 runs on the same code and is not benchmarked here."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def summary(values):
    med = statistics.median(values)
    return {"passes": values, "best": max(values), "median": med, "spread": (max(values) - min(values)) / med}


def make_nets(count):
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    nets = []
    for seed in range(21, 21 + count):
        net = DualNet(torch.device("cuda", 0), 9)
        net.load_state_dict(make_state_dict(9, seed, 1.3))
        nets.append(net)
    return nets


def records_digest(by_seed):
    h = hashlib.sha256()
    for seed in sorted(by_seed):
        h.update(f"{seed}\n".encode())
        h.update(by_seed[seed].encode())
    return h.hexdigest()


def tournament_leg(nets, names, boards, per_pair, visits, batch):
    from tamago_amd.selfplay.tournament import puct_tournament
    with tempfile.TemporaryDirectory() as d:
        out = puct_tournament(list(zip(names, nets)), visits, batch, games_per_pair=per_pair, boards=boards, save_dir=d)
        texts = {r["seed"]: open(os.path.join(d, f"{r['index']}.sgf"), encoding="utf-8").read() for r in out["results"]}
    mini_batches = -(-visits // batch)
    return {"games_per_second": out["games_per_second"], "seconds": out["seconds"], "games": out["games"], "moves": out["moves"],
            "forward_positions": out["forward_positions"], "leaf_evals": out["leaf_evals"], "calls": out["calls"],
            "range_fallbacks": out["range_fallbacks"], "digest": records_digest(texts),
            "forward_launches_per_mini_batch_at_most": len(nets),
            "mean_positions_per_call": out["forward_positions"] / max(out["calls"], 1),
            "mini_batches_per_call": mini_batches}


def duels_leg(nets, names, boards, per_pair, visits, batch):
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    from tamago_amd.selfplay.tournament import schedule
    pairs = schedule(len(nets), 1)
    total = {"seconds": 0.0, "games": 0, "moves": 0, "forward_positions": 0, "leaf_evals": 0, "calls": 0, "range_fallbacks": 0}
    texts = {}
    for p, (b, w) in enumerate(pairs):
        seeds = [r * len(pairs) + p for r in range(per_pair)]
        with tempfile.TemporaryDirectory() as d:
            out = puct_match(EngineSetup(nets[b], visits, batch), EngineSetup(nets[w], visits, batch), per_pair, boards=boards, seeds=seeds,
                             save_dir=d, names=(names[b], names[w]), compact_idle=True)
            for r in out["results"]:
                texts[r["seed"]] = open(os.path.join(d, f"{r['index']}.sgf"), encoding="utf-8").read()
        for key in total:
            total[key] += out[key]
    return dict(total, games_per_second=total["games"] / max(total["seconds"], 1e-9), digest=records_digest(texts),
                forward_launches_per_mini_batch_at_most=1, mean_positions_per_call=total["forward_positions"] / max(total["calls"], 1))


def time_kernels(boards, groups, repeats=50):
    """ms per group_live call (launch + read-back of the counts) and per gather / scatter launch of the planes' rows at T = boards."""
    import numpy as np
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    eng = SearchEngine(9, boards, 4, 1, DeviceEvaluator(make_nets(1)[0]))
    try:
        board = GoBoard(9)
        for t in range(boards):
            eng.set_root(t, board, 1)
        eng.seed_trees(range(boards))
        eng.root_eval(False)
        group = np.arange(boards) % groups
        rows = torch.zeros((boards, 6, 9, 9), dtype=torch.float32, device=eng.device)
        out = {}
        for name, call in (("group_live_ms", lambda: eng.group_live((group, groups))),
                           ("gather_planes_ms", lambda: eng.gather_rows_by_rank(eng.planes, rows)),
                           ("scatter_planes_ms", lambda: eng.scatter_rows_by_rank(rows, eng.planes[:boards]))):
            call()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(repeats):
                call()
            end.record()
            end.synchronize()
            out[name] = start.elapsed_time(end) / repeats
        return out
    finally:
        eng.close()


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--entrants", type=int, nargs="+", default=[2, 4, 8])
    parser.add_argument("--boards", type=int, nargs="+", default=[256, 2048])
    parser.add_argument("--visits", type=int, default=1000)
    parser.add_argument("--batch", type=int, default=256)
    parser.add_argument("--rounds-per-board", type=int, default=1)
    parser.add_argument("--repeats", type=int, default=2)
    parser.add_argument("--time-kernels", action="store_true")
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "tournament_bench.json"))
    args = parser.parse_args(argv)
    from tamago_amd import build
    result = {"tool": "tools/bench_tournament.py", "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(),
              "visits": args.visits, "batch": args.batch, "settings": []}
    nets = make_nets(max(args.entrants))
    warm = False
    for count in args.entrants:
        names = [f"n{k}" for k in range(count)]
        for boards in args.boards:
            per_pair = boards * args.rounds_per_board
            legs = {"tournament": [], "duels": []}
            for rep in range(args.repeats + (0 if warm else 1)):           # (the very first pass warms up)
                for name, leg in (("tournament", tournament_leg), ("duels", duels_leg)):
                    out = leg(nets[:count], names, boards, per_pair, args.visits, args.batch)
                    if warm or rep:
                        legs[name].append(out)
            warm = True
            first = {name: legs[name][0] for name in legs}
            assert first["tournament"]["digest"] == first["duels"]["digest"], "the two legs played different games"
            row = {"entrants": count, "boards": boards, "games": first["tournament"]["games"], "moves": first["tournament"]["moves"],
                   "records_digest": first["tournament"]["digest"]}
            for name in legs:
                row[name] = dict(summary([o["games_per_second"] for o in legs[name]]), unit="games/s",
                                 **{k: first[name][k] for k in ("forward_positions", "leaf_evals", "calls", "range_fallbacks",
                                                                "forward_launches_per_mini_batch_at_most", "mean_positions_per_call")})
                row[name]["live_share"] = first[name]["leaf_evals"] / max(first[name]["forward_positions"], 1)
            row["gain"] = row["tournament"]["median"] / row["duels"]["median"]
            if args.time_kernels:
                row["kernels"] = time_kernels(boards, count)
            result["settings"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")


if __name__ == "__main__":
    main()
