"""What the device early stop costs and saves, in one process on one device:

    python tools/bench_early_stop.py [--visits 1000] [--batches 256 16] [--moves 40] [--rounds 5] [--repeats 4]
                                     [--nets random scaled] [--boards 256 2048] [--games-per-board 2]
                                     [--out profiles/early_stop_bench.json]

Two kinds of network, because what an early stop saves depends on how often a search is decided early: `random` - torch's
default initialisation, as tools/bench_puct_match.py uses (flat priors: at 1 000 visits no search of the runs below stops
early, so these rows price the mechanism alone) - and `scaled` - oracle.net.make_state_dict(9, seed, 1.3), the networks of the
tests (peaked priors: most searches stop early).

1. One 9x9 tree, MCTSTree.search_best_move under TimeManager(CONSTANT_PLAYOUT, visits) over the first `moves` positions of a
   game the strict search plays (the same positions for every variant), per mini-batch size: ms per move with
   device_early_stop off - the host loop with a read_node round trip per mini-batch - and on with poll_every 1, 2, 4 and 0
   (never: everything is queued); a timed pass searches the positions `rounds` times over (200 searches: 0.3 s at batch 256,
   2.4 s at batch 16), `repeats` passes per variant in alternation after a warm-up pass, best and median pass, and the spread
   (max - min) / median of a variant's passes; and the visits the searches spent (equal for every variant: asserted) and the
   mini-batches each variant launched.
2. puct_match between two DualNets of that kind, 9x9, visits x batch 256 on both sides, games-per-board x boards games: strict
   setups (the row of profiles/puct_match_bench.json) against setups that are not, those once polled after every mini-batch
   (poll_every 1) and once at puct_match's default (SearchEngine.DEFAULT_POLL_EVERY; every row records the poll_every it ran
   with and the mini-batches per move) - games/s, positions the launches evaluated,
   leaf evaluations of live searching trees, and idle_share = 1 - leaf_evals / forward_positions: the share of evaluated slots
   that belonged to trees that were not searching (halted, finished, parked, one-child) - what compacting the slots away
   would save at most.

The rule kernel's own time per launch comes from a kernel trace in a run of its own (--trace-workload runs just a chained
single-tree search for the profiler to wrap):

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_early_stop.py --trace-workload
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

VARIANTS = (("off", None), ("poll_1", 1), ("poll_2", 2), ("poll_4", 4), ("poll_never", 0))


def game_positions(net, visits, batch, moves):
    """The first `moves` positions of the game a strict search plays against itself from the empty board."""
    from tamago_amd.board.constant import PASS, RESIGN
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.board.stone import Stone
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    import copy
    tree = MCTSTree(net, tree_size=visits + 16, batch_size=batch)
    board, color, out = GoBoard(9, 7.0, False), Stone.BLACK, []
    np.random.seed(5)
    for _ in range(moves):
        out.append((copy.deepcopy(board), color))
        mv = tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, visits), {})
        board.put_stone(PASS if mv == RESIGN else mv, color)
        color = Stone.get_opponent_color(color)
    return out


def single_tree(net, visits, batch, moves, repeats, rounds):
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    positions = game_positions(net, visits, batch, moves)
    trees = {name: MCTSTree(net, tree_size=visits + 16, batch_size=batch, device_early_stop=poll is not None, poll_every=poll)
             for name, poll in VARIANTS}
    spent, launched, seconds = {}, {}, {name: [] for name, _ in VARIANTS}

    def one_pass(name):
        tree = trees[name]
        visits_spent, batches = [], 0
        torch.cuda.synchronize()
        start = time.perf_counter()
        for _ in range(rounds):
            visits_spent = []
            for k, (board, color) in enumerate(positions):
                np.random.seed(100 + k)
                tree.search_best_move(board, color, TimeManager(TimeControl.CONSTANT_PLAYOUT, visits), {})
                visits_spent.append(int(tree.get_root().node_visits))
        torch.cuda.synchronize()
        took = (time.perf_counter() - start) / rounds
        batches = len(tree._engine.evaluator.batches) / rounds
        tree._engine.evaluator.batches.clear()
        return took, visits_spent, batches

    for name, _ in VARIANTS:                                   # warm-up: every variant's launches once
        _, spent[name], launched[name] = one_pass(name)
    for _ in range(repeats):
        for name, _ in VARIANTS:                                # (alternating: the host is shared)
            took, again, _ = one_pass(name)
            assert again == spent[name]
            seconds[name].append(took)
    assert all(spent[name] == spent["off"] for name in spent), "the variants searched different trees"
    rows = {name: {"ms_per_move_best": 1e3 * min(s) / moves, "ms_per_move_median": 1e3 * statistics.median(s) / moves,
                   "spread": (max(s) - min(s)) / statistics.median(s), "launches_per_move": launched[name] / moves}
            for name, s in seconds.items()}
    return {"net": None, "visits": visits, "batch": batch, "moves": moves, "repeats": repeats, "rounds": rounds, "mean_visits_spent": sum(spent["off"]) / moves,
            "moves_stopped_early": sum(v < visits for v in spent["off"]), "variants": rows}


def matches(net_a, net_b, boards, visits, batch, games_per_board):
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    rows = []
    from tamago_amd.mcts.engine import SearchEngine
    for strict, poll_every in ((True, None), (False, 1), (False, SearchEngine.DEFAULT_POLL_EVERY)):
        games = boards * games_per_board
        out = puct_match(EngineSetup(net_a, visits, batch, strict), EngineSetup(net_b, visits, batch, strict), games, boards=boards,
                         poll_every=poll_every)
        out.pop("results")
        rows.append({"net": None, "strict": strict, "poll_every": poll_every, "mini_batches_per_move": -(-visits // batch), "boards": boards, "games": games, "visits": visits, "batch": batch,
                     "games_per_second": out["games_per_second"], "seconds": out["seconds"], "moves": out["moves"],
                     "forward_positions": out["forward_positions"], "leaf_evals": out["leaf_evals"],
                     "idle_share": 1.0 - out["leaf_evals"] / out["forward_positions"], "range_fallbacks": out["range_fallbacks"],
                     "mean_length": out["mean_length"], "score_a": out["score_a"]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--visits", type=int, default=1000)
    parser.add_argument("--batches", type=int, nargs="+", default=[256, 16])
    parser.add_argument("--moves", type=int, default=40)
    parser.add_argument("--repeats", type=int, default=4)
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--boards", type=int, nargs="*", default=[256, 2048])
    parser.add_argument("--games-per-board", type=int, default=2)
    parser.add_argument("--match-batch", type=int, default=256)
    parser.add_argument("--trace-workload", action="store_true")
    parser.add_argument("--nets", nargs="+", choices=("random", "scaled"), default=["random", "scaled"])
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "early_stop_bench.json"))
    args = parser.parse_args(argv)
    from tamago_amd import build
    from tamago_amd.nn.network.dual_net import DualNet
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    device = torch.device("cuda", 0)

    def make_nets(kind):
        nets = []
        for seed in (21, 22):
            torch.manual_seed(seed)
            net = DualNet(device, 9)
            if kind == "scaled":
                from oracle.net import make_state_dict
                net.load_state_dict(make_state_dict(9, seed, 1.3))
            nets.append(net)
        return nets

    net_a, net_b = make_nets(args.nets[0])
    if args.trace_workload:
        from tamago_amd.mcts.time_manager import TimeControl, TimeManager
        from tamago_amd.mcts.tree import MCTSTree
        from tamago_amd.board.go_board import GoBoard
        tree = MCTSTree(net_a, tree_size=args.visits + 16, batch_size=16, device_early_stop=True, poll_every=0)
        for k in range(20):
            np.random.seed(k)
            tree.search_best_move(GoBoard(9, 7.0, False), 1, TimeManager(TimeControl.CONSTANT_PLAYOUT, args.visits), {})
        torch.cuda.synchronize()
        return
    result = {"tool": "tools/bench_early_stop.py", "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(),
              "single_tree": [], "match": []}
    for kind in args.nets:
        net_a, net_b = make_nets(kind)
        for batch in args.batches:
            row = dict(single_tree(net_a, args.visits, batch, args.moves, args.repeats, args.rounds), net=kind)
            result["single_tree"].append(row)
            print(json.dumps(row), flush=True)
        if args.boards:
            puct_match(EngineSetup(net_a, 32, 16, False), EngineSetup(net_b, 32, 16, False), 8, boards=8)  # warm-up: kernels loaded
        for boards in args.boards:
            result["match"] += [dict(r, net=kind) for r in matches(net_a, net_b, boards, args.visits, args.match_batch, args.games_per_board)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
