"""Whole-tree read-out against the loop over tg_search_read_node - the only way to look inside a tree without
it -, on one GPU.

    python tools/bench_tree_dump.py [--quick] [--out profiles/tree_dump_bench.json]

Network: a randomly initialised DualNet on the device forward; STRICT PUCT visits.  Rows, milliseconds each, after one
warm-up call, the baseline measured by this script on the same trees:
- MCTSTree.to_dict() of one 9x9 tree after 1 000 visits (batch 16), against [tree.node[i] for i in range(num_nodes)];
- the same for one 19x19 tree after 1 600 visits (batch 64);
- SearchEngine.tree_digests() over all trees of a 2 048-tree 9x9 engine after one 1 000-visit move (batch 256), against the
  read_node loop over every node of 16 of the trees, scaled to the nodes of all trees; and, for scale, dump_trees() of 64 of them.
The launches and copies of the read-out do not depend on the number of nodes: the rows record nodes and bytes beside the times.
Writes one JSON document (with build.source_digest()) and prints it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def network(size):
    import torch
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), size)
    net.load_state_dict(make_state_dict(size, 11, 1.4))
    return net


def timed(fn, repeat=3):
    """Best of `repeat` calls in milliseconds (after one warm-up call), and the last result."""
    import torch
    out = fn()
    best = None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ms = 1e3 * (time.perf_counter() - t0)
        best = ms if best is None else min(best, ms)
    return best, out


def single_tree(size, visits, batch):
    import numpy as np
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    tree = MCTSTree(network(size), tree_size=visits + 64, batch_size=batch)
    np.random.seed(size)
    tree.search_best_move(GoBoard(size), 1, TimeManager(TimeControl.STRICT_PLAYOUT, visits), {})
    dump_ms, state = timed(tree.to_dict)
    loop_ms, views = timed(lambda: [tree.node[i] for i in range(tree.num_nodes)], repeat=1)
    digest_ms, _ = timed(lambda: tree._engine.tree_digests())
    row = {"size": size, "visits": visits, "batch": batch, "nodes": state["num_nodes"],
           "children": int(sum(n["num_children"] for n in state["node"])), "to_dict_ms": round(dump_ms, 3),
           "read_node_loop_ms": round(loop_ms, 3), "tree_digests_ms": round(digest_ms, 3)}
    assert len(views) == state["num_nodes"]
    tree.close()
    return row


def many_trees(trees, visits, batch, sample=16):
    import numpy as np
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import SearchEngine, evaluator_for
    eng = SearchEngine(9, trees, visits + 16, batch, evaluator_for(network(9)))
    board = GoBoard(9)
    for t in range(trees):
        eng.set_root(t, board, 1)
    eng.seed_trees(range(trees))
    eng.root_eval()
    eng.puct_chain([batch] * (visits // batch) + ([visits % batch] if visits % batch else []))
    nodes = eng.num_nodes()
    digest_ms, digests = timed(eng.tree_digests)
    listed = list(range(min(64, trees)))                # (a dump of 2 048 such trees is gigabytes of rows: 64 of them)
    dump_ms, packed = timed(lambda: eng.dump_trees(listed), repeat=1)
    sample = min(sample, trees)
    t0 = time.perf_counter()
    for t in range(sample):
        for i in range(int(nodes[t])):
            eng.read_node(t, i)
    loop_ms = 1e3 * (time.perf_counter() - t0) * float(nodes.sum()) / float(nodes[:sample].sum())
    row = {"size": 9, "trees": trees, "visits": visits, "batch": batch, "nodes": int(nodes.sum()),
           "tree_digests_ms": round(digest_ms, 3), "dump_trees_listed": len(listed),
           "dump_trees_children": int(sum(p["total_children"] for p in packed)), "dump_trees_ms": round(dump_ms, 3),
           "read_node_loop_ms_scaled": round(loop_ms, 1), "loop_sample_trees": sample,
           "distinct_digests": len({tuple(d) for d in digests.tolist()})}
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="64 trees and 200 visits (a smoke run of the tool)")
    ap.add_argument("--out", default=os.path.join("profiles", "tree_dump_bench.json"))
    args = ap.parse_args()
    from tamago_amd import build
    rows = []
    for row in (single_tree(9, 200 if args.quick else 1000, 16), single_tree(19, 200 if args.quick else 1600, 64),
                many_trees(64 if args.quick else 2048, 200 if args.quick else 1000, 256 if not args.quick else 40)):
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc = {"source_digest": build.source_digest(), "quick": args.quick, "rows": rows}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
