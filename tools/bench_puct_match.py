"""What a PUCT match costs next to the bare PUCT move loop bench.py times, in one process on one device:

    python tools/bench_puct_match.py [--boards 256 2048] [--visits 1000] [--batch 256] [--games-per-board 2]
                                     [--loop-moves 40] [--out profiles/puct_match_bench.json]

Per board count: puct_match between two random-init DualNets, both sides at (visits, batch), games-per-board x boards games -
games/s, leaf evaluations/s of the live games, positions/s the launches evaluated (parked slots, finished games at a leg's
tail and pass-only roots search too), the calls spent parked and the share of wall time between a call's last read-out and
the next call's root launch - and the loop of bench.py's run_step (root evaluation, mini-batches, tg_search_play(-2)) on one
engine of the same trees, visits and batch for loop-moves moves.  ratio = the match's launched positions/s over the loop's:
the match should cost what the loop costs plus the two read-outs and the host's bookkeeping."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def move_loop(net, boards, visits, batch, moves, size=9):
    """bench.py run_step on one engine: leaf evaluations/s over `moves` moves after 2 warm-up moves."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    engine = SearchEngine(size, boards, visits + 16, batch, DeviceEvaluator(net))
    try:
        fresh = GoBoard(size, 7.0, False)
        for t in range(boards):
            engine.set_root(t, fresh, 1)
        engine.seed_trees(list(range(boards)))
        first = min(batch, visits)
        plies = 0

        def step():
            nonlocal plies
            engine.root_eval(False, first_batch=first)
            done = 0
            while done < visits:
                k = min(batch, visits - done)
                engine.puct_batch(k)
                done += k
            engine.prefetch_rng(first)
            plies += 1
            if plies > 2 * engine.P - 8:
                for t in range(boards):
                    engine.set_root(t, fresh, 1)
                plies = 0
            else:
                engine.play(np.full(boards, -2, dtype=np.int32))

        for _ in range(2):
            step()
        torch.cuda.synchronize(engine.device)
        start = time.perf_counter()
        for _ in range(moves):
            step()
        torch.cuda.synchronize(engine.device)
        seconds = time.perf_counter() - start
        return {"moves": moves, "seconds": seconds, "leaf_evals_per_second": boards * (1 + visits) * moves / seconds}
    finally:
        engine.close()


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--boards", type=int, nargs="+", default=[256, 2048])
    parser.add_argument("--visits", type=int, default=1000)
    parser.add_argument("--batch", type=int, default=256)
    parser.add_argument("--games-per-board", type=int, default=2)
    parser.add_argument("--loop-moves", type=int, default=40)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "puct_match_bench.json"))
    args = parser.parse_args(argv)
    from tamago_amd import build
    from tamago_amd.nn.network.dual_net import DualNet
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    device = torch.device("cuda", 0)
    torch.manual_seed(21)
    net_a = DualNet(device, 9)
    torch.manual_seed(22)
    net_b = DualNet(device, 9)
    puct_match(EngineSetup(net_a, 32, 16), EngineSetup(net_b, 32, 16), 8, boards=8)          # warm-up: kernels loaded
    rows = []
    for boards in args.boards:
        games = boards * args.games_per_board
        out = puct_match(EngineSetup(net_a, args.visits, args.batch), EngineSetup(net_b, args.visits, args.batch), games,
                         boards=boards)
        out.pop("results")
        loop = move_loop(net_a, boards, args.visits, args.batch, args.loop_moves)
        launched = out["forward_positions"] / out["seconds"]
        row = {"boards": boards, "games": games, "visits": args.visits, "batch": args.batch, "match": out, "loop": loop,
               "match_games_per_second": out["games_per_second"],
               "match_leaf_evals_per_second": out["leaf_evals"] / out["seconds"],
               "match_launched_positions_per_second": launched,
               "match_over_loop": launched / loop["leaf_evals_per_second"],
               "live_share_of_launched": out["leaf_evals"] / out["forward_positions"],
               "parked_share_of_slot_calls": out["parked_slot_calls"] / out["slot_calls"],
               "between_calls_share_of_seconds": out["between_calls_seconds"] / out["seconds"]}
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k not in ("match", "loop")}), flush=True)
    result = {"tool": "tools/bench_puct_match.py", "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(),
              "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
