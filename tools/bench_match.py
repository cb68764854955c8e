"""Search matches (tamago_amd.selfplay.match.search_match) next to self-play at the same boards and simulations, one GPU.

    python tools/bench_match.py [--quick] [--runs N] [--out profiles/match_bench.json]

Two randomly initialised 9x9 DualNets play each other under Gumbel search.  Per (simulations, boards) row - 16 and 400
simulations, 256 and 2 048 boards - after a warm-up run, `runs` runs of 2 x boards games each of
- the match (A black, one leg; records written, resignation allowed), games/s and leaf-evals/s over the whole call,
- selfplay_shard with network A alone in the same process: the same seeds, boards, simulations and resignation flags, as ONE
  lock-step group and lane (what the match runs as), records written,
and the match's share of slot-calls spent parked for parity: slots whose game had ended and that waited for a call they may
start on (selfplay/match.py: slot_may_start), over boards x lock-step calls.  `match_over_selfplay` is the ratio of the median
leaf-evals/s - null where the runs of either side spread by more than 10 % of their median, which allows no ratio
(`ratio_withheld_for_spread`).  Writes one JSON document (with build.source_digest()) and prints it."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def networks(size):
    import torch
    from tamago_amd.nn.network.dual_net import DualNet
    torch.manual_seed(41)
    net_a = DualNet(torch.device("cuda:0"), size)
    torch.manual_seed(42)
    return net_a, DualNet(torch.device("cuda:0"), size)


def match_run(nets, visits, boards, games):
    import torch
    from tamago_amd.selfplay.match import search_match
    with tempfile.TemporaryDirectory() as d:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = search_match(nets[0], nets[1], games, size=9, visits=visits, boards=boards, seeds=list(range(1, games + 1)),
                           save_dir=d)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out


def selfplay_run(net, visits, boards, games):
    import torch
    from tamago_amd.selfplay.worker import selfplay_shard
    with tempfile.TemporaryDirectory() as d:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = selfplay_shard(d, net, list(range(1, games + 1)), 9, visits, boards=boards,
                               never_resign_flags=[False] * games, groups=1, lanes=1)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, stats


def spread(values, digits=1):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


MAX_SPREAD = 0.10          # (max - min) / median of a side's runs beyond which no ratio is given


def ratio(match_rates, selfplay_rates):
    """Median over median, or None where either side's runs spread too widely for it to mean anything."""
    for rates in (match_rates, selfplay_rates):
        if (max(rates) - min(rates)) / statistics.median(rates) > MAX_SPREAD:
            return None
    return round(statistics.median(match_rates) / statistics.median(selfplay_rates), 3)


def row(nets, visits, boards, runs):
    games = 2 * boards
    match_run(nets, visits, min(boards, 64), min(boards, 64))                  # warm-up: code objects, both networks' images
    selfplay_run(nets[0], visits, min(boards, 64), min(boards, 64))
    m_gps, m_lps, s_gps, s_lps, parked, lengths, s_lengths = [], [], [], [], [], [], []
    for _ in range(runs):
        seconds, out = match_run(nets, visits, boards, games)
        m_gps.append(games / seconds)
        m_lps.append(out["leaf_evals"] / seconds)
        parked.append(out["parked_slot_calls"] / out["slot_calls"])
        lengths.append(out["mean_length"])
        seconds, stats = selfplay_run(nets[0], visits, boards, games)
        s_gps.append(games / seconds)
        s_lps.append(stats["leaf_evals"] / seconds)
        s_lengths.append(stats["moves"] / games)
    res = {"size": 9, "visits": visits, "boards": boards, "games": games, "runs": runs,
           "match_games_per_s": spread(m_gps, 2), "match_leaf_evals_per_s": spread(m_lps, 0),
           "selfplay_games_per_s": spread(s_gps, 2), "selfplay_leaf_evals_per_s": spread(s_lps, 0),
           "match_over_selfplay": ratio(m_lps, s_lps), "ratio_withheld_for_spread": ratio(m_lps, s_lps) is None,
           "parked_share_of_slot_calls": round(statistics.median(parked), 5),
           "match_calls": out["calls"], "match_mean_length": round(statistics.median(lengths), 1),
           "selfplay_mean_moves": round(statistics.median(s_lengths), 1), "match_resignations": out["resignations"],
           "match_range_fallbacks": out["range_fallbacks"], "selfplay_groups": 1, "selfplay_lanes": 1}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="16 simulations on 256 boards only (a smoke run of the tool)")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "match_bench.json"))
    args = ap.parse_args()
    from tamago_amd import build
    nets = networks(9)
    cases = ((16, 256),) if args.quick else ((16, 256), (16, 2048), (400, 256), (400, 2048))
    rows = [row(nets, visits, boards, args.runs) for visits, boards in cases]
    doc = {"source_digest": build.source_digest(), "rows": rows}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
