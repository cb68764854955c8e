"""What the evaluation cache saves and costs, in one process on one device:

    python tools/bench_eval_cache.py [--boards 256 2048] [--visits 1000] [--batch 256] [--games-per-board 2] [--repeats 2]
                                     [--entries 4194304] [--analysis-records 4] [--analysis-visits 200] [--analysis-batch 16]
                                     [--bench-parent FILE] [--bench-commit FILE] [--out profiles/eval_cache_bench.json]

1. The strict PUCT match of tools/bench_puct_match.py - 9x9, visits x batch on both sides, games-per-board x boards games - on two
   legs: (a) ONE DualNet on both sides (one cache), (b) the two scaled DualNets of the other match benches (a cache each).  Three
   ways in alternation (the host is shared): "off" - today's default, the chained calls; "passthrough" - the parent's own
   mini-batch by mini-batch path, taken by wrapping the evaluator in a wrapper that only forwards; "on" - eval_cache=entries.
   passthrough against off is what leaving the chain costs, on against passthrough what the cache itself saves or costs.  Per way:
   games/s of every pass, best, median, spread; positions handed over and positions evaluated, hit rate, table occupancy
   (inserts less evictions over entries) and evictions.  The games of the three ways are compared game by game - winner, resignation,
   length, score and the final state of the game's random stream, as one digest - and must be equal whenever no f16 range fallback
   was taken.
2. The cache's calls alone on one launch of boards x batch rows, with nothing resident and with everything resident: host time of
   the probe call (three launches and the one stream wait) and of the commit call, and - through the library's timing-only path
   (tg_evalcache_set_timing: timed events around each launch) - the probe, rank, gather and commit KERNEL times.
3. analyze_positions over all plies of a few records, off / passthrough / on.

--bench-parent / --bench-commit: files of bench.py result lines measured in one session on the two builds, copied into the profile.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def summary(values):
    med = statistics.median(values)
    return {"passes": values, "best": max(values), "median": med, "spread": (max(values) - min(values)) / med}


class PassThrough:
    """An evaluator that only forwards: not exactly DeviceEvaluator, so the engine leaves the chained calls - the parent's
    mini-batch by mini-batch path, with nothing else changed."""

    def __init__(self, inner):
        self.inner, self.network, self.batches = inner, inner.network, inner.batches

    def __call__(self, planes, want_logits):
        return self.inner(planes, want_logits)


def run_match(net_a, net_b, boards, games, visits, batch, way, entries):
    import tamago_amd.mcts.engine as engine
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    real = engine.evaluator_for
    if way == "passthrough":
        engine.evaluator_for = lambda network, device_index=0, eval_cache=None: PassThrough(real(network, device_index))
    try:
        out = puct_match(EngineSetup(net_a, visits, batch, True), EngineSetup(net_b, visits, batch, True), games, boards=boards,
                         **(dict(eval_cache=entries) if way == "on" else {}))
    finally:
        engine.evaluator_for = real
    # the games themselves: every game's moves, result and final stream state, as one digest
    import hashlib
    h = hashlib.sha256()
    for r in out.pop("results"):
        h.update(repr((r["index"], r["winner"], r["is_resign"], r["moves"], float(r["score"]), int(r["stream"][1]))).encode())
        h.update(bytes(memoryview(r["stream"][0])))
    out["games_digest"] = h.hexdigest()[:16]
    return out


def match_legs(nets, boards, visits, batch, games_per_board, repeats, entries):
    rows = []
    games = boards * games_per_board
    for leg, (net_a, net_b) in nets.items():
        runs = {"off": [], "passthrough": [], "on": []}
        for _ in range(repeats):
            for way in runs:                                    # (alternating)
                runs[way].append(run_match(net_a, net_b, boards, games, visits, batch, way, entries))
        fallbacks = sum(o["range_fallbacks"] for way in runs for o in runs[way])
        digests = {o["games_digest"] for way in runs for o in runs[way]}       # (every pass of every way)
        same = len(digests) == 1
        assert same or fallbacks, "the games depend on the cache although no range fallback was taken"
        row = {"leg": leg, "boards": boards, "games": games, "visits": visits, "batch": batch, "entries": entries,
               "moves": runs["off"][0]["moves"], "same_games": same, "range_fallbacks": fallbacks}
        for way in runs:
            first = runs[way][0]
            row[way] = dict(summary([o["games_per_second"] for o in runs[way]]), unit="games/s",
                            forward_positions=first["forward_positions"],
                            between_calls_seconds=first["between_calls_seconds"])
        on = runs["on"][0]
        stats = on["eval_cache_stats"]
        row["on"].update(evaluated_positions=on["evaluated_positions"], hit_rate=stats["hits"] / max(stats["lookups"], 1),
                         occupancy=(stats["inserts"] - stats["evictions"]) / stats["entries"], stats=stats)
        row["cost_of_leaving_the_chain"] = row["passthrough"]["median"] / row["off"]["median"]
        row["cache_against_passthrough"] = row["on"]["median"] / row["passthrough"]["median"]
        row["cache_against_default"] = row["on"]["median"] / row["off"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def call_times(net, rows_count, entries, repeats=5):
    """The cache's own calls on one launch of rows_count distinct real rows (ms, median of `repeats`)."""
    import numpy as np
    from tamago_amd.nn.eval_cache import EvalCache
    from tamago_amd.nn.feature import featurize_batch
    rnd = np.random.RandomState(0)
    planes = featurize_batch(9, rnd.choice([0, 1, 2], size=(rows_count, 81)).astype(np.uint8), rnd.choice([1, 2], size=rows_count),
                             np.zeros(rows_count, dtype=np.int32), np.zeros(rows_count, dtype=np.int32))
    policy = torch.empty((rows_count, 82), device=planes.device)
    value = torch.empty((rows_count, 3), device=planes.device)
    out = {"rows": rows_count, "probe_all_miss_ms": [], "commit_ms": [], "probe_all_hit_ms": [], "host_wait_ms_empty_stream": []}
    out.update(kernels_all_miss=[], kernels_all_hit=[])
    cache = EvalCache(9, entries)
    try:
        cache.set_timing(True)
        for _ in range(repeats + 1):
            cache.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_miss, miss = cache.probe(planes, False, policy, value)
            t1 = time.perf_counter()
            cache.commit(policy[:n_miss], value[:n_miss], policy, value)
            torch.cuda.synchronize()
            t2_commit = time.perf_counter()
            out["kernels_all_miss"].append(cache.read_timing())
            t2 = time.perf_counter()
            n_hit_miss, _ = cache.probe(planes, False, policy, value)
            t3 = time.perf_counter()
            cache.commit(None, None, policy, value) if n_hit_miss == 0 else cache.commit(policy[:n_hit_miss], value[:n_hit_miss], policy, value)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            torch.cuda.current_stream().synchronize()
            t5 = time.perf_counter()
            out["kernels_all_hit"].append(cache.read_timing())
            out["probe_all_miss_ms"].append((t1 - t0) * 1e3)
            out["commit_ms"].append((t2_commit - t1) * 1e3)
            out["probe_all_hit_ms"].append((t3 - t2) * 1e3)
            out["host_wait_ms_empty_stream"].append((t5 - t4) * 1e3)
            out["missed_when_resident"] = n_hit_miss
        for key in ("probe_all_miss_ms", "commit_ms", "probe_all_hit_ms", "host_wait_ms_empty_stream"):
            out[key] = statistics.median(out[key][1:])
        for key in ("kernels_all_miss", "kernels_all_hit"):
            out[key] = {name: statistics.median(t[name] for t in out[key][1:]) for name in out[key][0]}
    finally:
        cache.close()
    return out


def analysis_legs(net, records, visits, batch, repeats, entries):
    import tamago_amd.mcts.analysis as analysis
    import tamago_amd.mcts.engine as engine
    from tools.bench_early_stop import game_positions
    games = [game_positions(net, 200 + 7 * g, batch, 40) for g in range(records)]
    positions = [p for game in games for p in game]
    runs = {"off": [], "passthrough": [], "on": []}
    outputs = {}
    report = {}
    for rep in range(repeats + 1):                             # (the first pass warms up)
        for way in runs:
            real = analysis.evaluator_for
            if way == "passthrough":
                analysis.evaluator_for = lambda network, device_index=0, eval_cache=None: PassThrough(engine.evaluator_for(network, device_index))
            try:
                torch.cuda.synchronize()
                start = time.perf_counter()
                res = analysis.analyze_positions(net, positions, visits, batch_size=batch,
                                                 **(dict(eval_cache=entries) if way == "on" else {}))
                if way == "on":
                    report = res.cache_report
                torch.cuda.synchronize()
                seconds = time.perf_counter() - start
            finally:
                analysis.evaluator_for = real
            outputs[way] = [(r.best_move, r.visits, r.value_sum) for r in res]
            if rep:
                runs[way].append(len(positions) / seconds)
    fallbacks = net.range_fallbacks()
    same = outputs["off"] == outputs["on"] == outputs["passthrough"]
    assert same or fallbacks, "the analysis depends on the cache although no range fallback was taken"
    row = {"records": records, "positions": len(positions), "visits": visits, "batch": batch, "same_output": same,
           "range_fallbacks_of_the_network_so_far": fallbacks}
    for way in runs:
        row[way] = dict(summary(runs[way]), unit="positions/s")
    stats = report["eval_cache_stats"]
    row["on"].update(forward_positions=report["forward_positions"], evaluated_positions=report["evaluated_positions"],
                     hit_rate=stats["hits"] / max(stats["lookups"], 1), stats=stats)
    row["cache_against_passthrough"] = row["on"]["median"] / row["passthrough"]["median"]
    row["cache_against_default"] = row["on"]["median"] / row["off"]["median"]
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
    parser.add_argument("--entries", type=int, default=1 << 22)
    parser.add_argument("--analysis-records", type=int, default=4)
    parser.add_argument("--analysis-visits", type=int, default=200)
    parser.add_argument("--analysis-batch", type=int, default=16)
    parser.add_argument("--bench-parent", default=None)
    parser.add_argument("--bench-commit", default=None)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_cache_bench.json"))
    args = parser.parse_args(argv)
    from oracle.net import make_state_dict
    from tamago_amd import build
    from tamago_amd.nn.network.dual_net import DualNet
    device = torch.device("cuda", 0)
    scaled = []
    for seed in (21, 22):
        net = DualNet(device, 9)
        net.load_state_dict(make_state_dict(9, seed, 1.3))
        scaled.append(net)
    nets = {"one_network_both_sides": (scaled[0], scaled[0]), "two_scaled_networks": (scaled[0], scaled[1])}
    result = {"tool": "tools/bench_eval_cache.py", "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(),
              "forward_source_digest": build.source_digest(build.FORWARD_SOURCES), "match": [], "calls": [], "analysis": []}
    run_match(scaled[0], scaled[1], 8, 8, 32, 16, "on", 1 << 12)                       # warm-up
    for boards in args.boards:
        result["match"] += match_legs(nets, boards, args.visits, args.batch, args.games_per_board, args.repeats, args.entries)
        result["calls"].append(call_times(scaled[0], boards * args.batch, args.entries))
        print(json.dumps(result["calls"][-1]), flush=True)
    if args.analysis_records:
        result["analysis"].append(analysis_legs(scaled[0], args.analysis_records, args.analysis_visits, args.analysis_batch, args.repeats,
                                                args.entries))
    result["settings_that_lose_against_the_default"] = [f"{r['leg']} on {r['boards']} boards" for r in result["match"]
                                                        if r["cache_against_default"] < 1.0]
    result["bench_headline"] = {"parent": read_lines(args.bench_parent), "commit": read_lines(args.bench_commit),
                                "note": "bench.py --gpus 1 runs none of the cache's code; the two builds measured in alternation in one session"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
