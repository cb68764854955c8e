"""What tree reuse in lock-step PUCT matches saves and costs, in one process on one device:

    python tools/bench_puct_reuse.py [--boards 256 2048] [--visits 1000] [--batch 256] [--games-per-board 2] [--repeats 2]
                                     [--compact 0 1] [--resources FILE] [--bench-parent FILE] [--bench-commit FILE]
                                     [--out profiles/puct_reuse_bench.json]

The PUCT match of tools/bench_puct_match.py - two DualNets, 9x9, visits x batch on both sides, strict, games-per-board x boards
games - with reuse_tree off and on, the legs in alternation (off, on, off, on, ...: the host is shared), `repeats` passes per
leg after a warm-up match, without and with compact_idle.  The two legs play DIFFERENT games (a reused tree searches
differently, and each colour has its own stream), so the rate is reported per game and per move.  Per leg: games/s and moves/s
of every pass with best, median and spread (max - min) / median, the positions evaluated per move, and for the reuse leg the
mean share of the visit budget that was found kept, the share of searches that started on a fresh root and the host's wall
time in advance (both engines) and in the fresh root launch with its read-out, per call.

Without compact_idle the number of mini-batches of a call is set by the tree that kept least, so reuse can only save
selection work there; with it the forward passes shrink as budgets are spent, at the granularity of the host's looks.
--resources takes the register table of the four PUCT selectors at the parent and at this commit (made from the compiler's
resource remarks), --bench-parent / --bench-commit files of bench.py result lines measured in one session on the two builds:
both are copied into the profile; without them it says "not measured".  The profile is rewritten after every row.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def summary(values):
    med = statistics.median(values)
    return {"passes": values, "best": max(values), "median": med, "spread": (max(values) - min(values)) / med}


def match_legs(net_a, net_b, boards, visits, batch, games_per_board, repeats, compact):
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    games = boards * games_per_board
    legs = {False: [], True: []}
    for _ in range(repeats):
        for reuse in (False, True):                            # (alternating: the host is shared)
            out = puct_match(EngineSetup(net_a, visits, batch), EngineSetup(net_b, visits, batch), games, boards=boards,
                             compact_idle=compact, reuse_tree=reuse, poll_every=1 if reuse else None)
            out.pop("results")
            legs[reuse].append(out)
    row = {"boards": boards, "games": games, "visits": visits, "batch": batch, "compact_idle": compact,
           "mini_batches_per_move": -(-visits // batch)}
    for reuse, name in ((False, "off"), (True, "on")):
        first = legs[reuse][0]
        row[name] = {"games_per_second": summary([o["games_per_second"] for o in legs[reuse]]),
                     "moves_per_second": summary([o["moves"] / o["seconds"] for o in legs[reuse]]),
                     "moves": first["moves"], "mean_length": first["mean_length"], "leaf_evals": first["leaf_evals"],
                     "forward_positions": first["forward_positions"],
                     "positions_per_move": first["forward_positions"] / max(first["moves"], 1),
                     "range_fallbacks": sum(o["range_fallbacks"] for o in legs[reuse])}
        if reuse:
            searches = first["reused_searches"] + first["fresh_searches"]
            row[name].update(kept_share=first["kept_share"], fresh_share=first["fresh_searches"] / max(searches, 1),
                             advance_ms_per_call=1e3 * statistics.median(o["advance_seconds"] / o["calls"] for o in legs[reuse]),
                             root_fresh_ms_per_call=1e3 * statistics.median(o["root_fresh_seconds"] / o["calls"] for o in legs[reuse]))
    row["gain_games_per_second"] = row["on"]["games_per_second"]["median"] / row["off"]["games_per_second"]["median"]
    row["gain_moves_per_second"] = row["on"]["moves_per_second"]["median"] / row["off"]["moves_per_second"]["median"]
    row["positions_per_move_ratio"] = row["on"]["positions_per_move"] / row["off"]["positions_per_move"]
    print(json.dumps(row), flush=True)
    return row


def read_lines(path):
    if not path or not os.path.exists(path):
        return "not measured"
    out = []
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            rec = json.loads(line)
            out.append({k: rec[k] for k in ("value", "unit", "ms_per_step") if k in rec})
    return out or "not measured"


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--boards", type=int, nargs="*", default=[256, 2048])
    parser.add_argument("--visits", type=int, default=1000)
    parser.add_argument("--batch", type=int, default=256)
    parser.add_argument("--games-per-board", type=int, default=2)
    parser.add_argument("--repeats", type=int, default=2)
    parser.add_argument("--compact", type=int, nargs="+", choices=(0, 1), default=[0, 1])
    parser.add_argument("--resources", default=None)
    parser.add_argument("--bench-parent", default=None)
    parser.add_argument("--bench-commit", default=None)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "puct_reuse_bench.json"))
    args = parser.parse_args(argv)
    from oracle.net import make_state_dict
    from tamago_amd import build
    from tamago_amd.nn.network.dual_net import DualNet
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    device = torch.device("cuda", 0)
    nets = []
    for seed in (21, 22):                                      # (the scaled networks of tools/bench_compact_idle.py)
        net = DualNet(device, 9)
        net.load_state_dict(make_state_dict(9, seed, 1.3))
        nets.append(net)
    result = {"tool": "tools/bench_puct_reuse.py", "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(),
              "match": []}
    result["selector_resources"] = json.load(open(args.resources)) if args.resources and os.path.exists(args.resources) else "not measured"
    result["bench_headline"] = {"parent": read_lines(args.bench_parent), "commit": read_lines(args.bench_commit),
                                "note": "bench.py --gpus 1 runs the PUCT selectors with a null budget pointer; the two builds "
                                        "measured in alternation in one session"}

    def write():
        result["settings_that_lose"] = [f"{r['boards']} boards, compact_idle {r['compact_idle']}" for r in result["match"]
                                        if r["gain_moves_per_second"] < 1.0]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    write()
    for reuse in (False, True):                                # warm-up
        puct_match(EngineSetup(nets[0], 32, 16), EngineSetup(nets[1], 32, 16), 8, boards=8, compact_idle=True, reuse_tree=reuse)
    for boards in args.boards:
        for compact in args.compact:
            result["match"].append(match_legs(nets[0], nets[1], boards, args.visits, args.batch, args.games_per_board, args.repeats,
                                              bool(compact)))
            write()


if __name__ == "__main__":
    main()
