"""Whole-tree write-in beside the read-out of the same trees and beside searching them again, on one GPU.

    python tools/bench_tree_load.py [--quick] [--out profiles/tree_load_bench.json]

Network: a randomly initialised DualNet on the device forward; STRICT PUCT visits (tools/bench_tree_dump.py's shapes).  Rows,
milliseconds each, best of three calls after one warm-up:
- 64 trees of a 2 048-tree 9x9 engine after one 1 000-visit move (batch 256; the records of all 2 048 are gigabytes of rows,
  as in the read-out's bench): tg_search_dump_trees and tg_search_load_trees on the same records, C calls alone, with bytes
  per second; SearchEngine.load_trees (make_record included); the time the engine took to search all its trees, and that
  time's share of 64 trees;
- one 19x19 tree after 1 600 visits (batch 64): the same, the search time being that tree's;
- MCTSTree.load_dict's verify (dump.verify_tree, host only) of one 9x9 tree after 1 000 visits and of the 19x19 tree.
A load goes back into the slots the records came from (the trees belong to those positions).  Writes one JSON document (with
build.source_digest()) and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_tree_dump import network, timed  # noqa: E402


def raw_calls(eng, listed):
    """(dump ms, load ms, bytes) of the two C calls on the listed trees' records."""
    from tamago_amd import lib as _lib
    from tamago_amd.mcts import dump
    arr = np.ascontiguousarray(listed, dtype=np.int32)
    nodes, children = eng.dump_sizes(arr)
    size = sum(dump.record_bytes(int(a), int(b)) for a, b in zip(nodes, children))
    records = np.zeros(size, dtype=np.uint8)
    offsets = np.zeros(arr.size + 1, dtype=np.int64)
    flags = np.zeros(arr.size, dtype=np.int32)

    def do_dump():
        _lib.check(eng.lib.tg_search_dump_trees(eng.handle, arr.ctypes.data, arr.size, records.ctypes.data, size, offsets.ctypes.data,
                                                eng._stream()), "tg_search_dump_trees")

    def do_load():
        _lib.check(eng.lib.tg_search_load_trees(eng.handle, arr.ctypes.data, arr.size, records.ctypes.data, offsets.ctypes.data,
                                                flags.ctypes.data, eng._stream()), "tg_search_load_trees")
    dump_ms, _ = timed(do_dump)
    want = eng.tree_digests(arr).copy()
    load_ms, _ = timed(do_load)
    assert not flags.any() and np.array_equal(eng.tree_digests(arr), want)
    return dump_ms, load_ms, size


def rates(row, dump_ms, load_ms, size):
    row.update({"record_bytes": int(size), "dump_trees_c_ms": round(dump_ms, 3), "load_trees_c_ms": round(load_ms, 3),
                "dump_gb_per_s": round(size / dump_ms / 1e6, 3), "load_gb_per_s": round(size / load_ms / 1e6, 3)})


def many_trees(trees, visits, batch):
    import torch
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import SearchEngine, evaluator_for
    eng = SearchEngine(9, trees, visits + 16, batch, evaluator_for(network(9)))
    board = GoBoard(9)
    for t in range(trees):
        eng.set_root(t, board, 1)
    eng.seed_trees(range(trees))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.root_eval()
    eng.puct_chain([batch] * (visits // batch) + ([visits % batch] if visits % batch else []))
    nodes = eng.num_nodes()                                    # (waits for the stream)
    search_ms = 1e3 * (time.perf_counter() - t0)
    listed = list(range(min(64, trees)))
    row = {"size": 9, "trees": trees, "listed": len(listed), "visits": visits, "batch": batch, "nodes_listed": int(nodes[listed].sum()),
           "search_all_trees_ms": round(search_ms, 1), "search_share_of_listed_ms": round(search_ms * len(listed) / trees, 1)}
    rates(row, *raw_calls(eng, listed))
    packed = eng.dump_trees(listed)
    py_ms, _ = timed(lambda: eng.load_trees(packed, listed), repeat=1)
    row["load_trees_python_ms"] = round(py_ms, 3)
    eng.close()
    return row


def single_tree(size, visits, batch, raw=True):
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts import dump
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    tree = MCTSTree(network(size), tree_size=visits + 64, batch_size=batch)
    board = GoBoard(size)
    np.random.seed(size)
    t0 = time.perf_counter()
    tree.search_best_move(board, 1, TimeManager(TimeControl.STRICT_PLAYOUT, visits), {})
    search_ms = 1e3 * (time.perf_counter() - t0)
    packed = tree._engine.dump_trees([0])[0]
    row = {"size": size, "visits": visits, "batch": batch, "nodes": int(packed["num_nodes"]), "children": int(packed["total_children"]),
           "search_ms": round(search_ms, 1)}
    if raw:
        rates(row, *raw_calls(tree._engine, [0]))
    t0 = time.perf_counter()
    dump.verify_tree(packed, board, 1)
    row["verify_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    tree.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="64 trees and 200 visits (a smoke run of the tool)")
    ap.add_argument("--out", default=os.path.join("profiles", "tree_load_bench.json"))
    args = ap.parse_args()
    from tamago_amd import build
    q = args.quick
    rows = []
    for make in (lambda: many_trees(64 if q else 2048, 200 if q else 1000, 40 if q else 256),
                 lambda: single_tree(19, 200 if q else 1600, 64),
                 lambda: single_tree(9, 200 if q else 1000, 16, raw=False)):
        rows.append(make())
        print(json.dumps(rows[-1]), flush=True)
    doc = {"source_digest": build.source_digest(), "quick": q, "rows": rows}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
