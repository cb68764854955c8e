#!/usr/bin/env python3
"""Whole-tree dump fixtures from the REFERENCE itself: tests/golden/tree_dump_s{9,13,19}.json.

    python tools/gen_golden_tree_dump.py --reference <checkout of the reference>
    python tools/gen_golden_tree_dump.py --size 9      # worker mode (PYTHONPATH must point at a reference tree)

The reference is imported in a worker process and never copied into the repository (tools/gen_golden.py's pattern): for
13x13 and 19x19 a scratch copy with the board-size constant changed (board/constant.py:4) is made in a temporary directory
at run time and deleted afterwards.  The evaluator is oracle.stubnet.StubNet.  The fixtures are data only.

Per size: CASES picks two PUCT cases and one Gumbel case of tests/golden/trees_s<size>.json by index; a case of the fixture
repeats their parameters (kind, seed, visits, batch, mode, cgos, ply, superko, color), and adds num_nodes and the sha256 of
canonical_bytes(MCTSTree.to_dict()) of the reference's tree after that search.

9x9 also records one SMALL search (10 visits at batch 2): the complete dump_to_json text, and per node the fields that
enrich_mcts_dict (mcts/dump.py:35-111) adds to it.  With StubNet every scalar of the reference's to_dict() is a plain Python
int or float (node.py:245-252 turns arrays into lists and tensors into numbers), so json.dumps takes it as it is: the text is
the reference's own, unconverted.

canonical_bytes is defined here and imported by the tests: keys in a fixed order, integers and integer arrays as little-endian
int32, floats and float arrays as little-endian float64 (raw_value and node_value_sum: float64 of what the tree holds).
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

# indices into trees_s<size>.json: two PUCT cases, one Gumbel case
CASES = {9: (2, 8, 13), 13: (0, 2, 4), 19: (0, 1, 5)}
# (seed, batch, visits, ply, superko): STRICT_PLAYOUT PUCT on game 0 of board_s9.npz, the side to move searching
SMALL = {"seed": 4, "batch": 2, "visits": 10, "ply": 12, "superko": True, "tree_size": 64}

TREE_INT_KEYS = ("num_nodes", "root", "current_root", "batch_size")
NODE_INT_KEYS = ("node_visits", "virtual_loss", "num_children")
NODE_FLOAT_KEYS = ("node_value_sum", "raw_value")
NODE_INT_ARRAYS = ("action", "children_index", "children_visits", "children_virtual_loss")
NODE_FLOAT_ARRAYS = ("children_value", "children_policy", "children_value_sum", "noise")
ENRICHED_KEYS = ("index", "parent_index", "index_in_brother", "expanded_children_index", "order", "level", "orders_along_path",
                 "gtp_moves_along_path", "to_move", "board_string", "policy", "visits", "value", "value_sum", "gtp_move",
                 "mean_value", "raw_black_winrate", "mean_black_winrate")


def canonical_bytes(tree_dict) -> bytes:
    """The canonical byte serialisation of a to_dict() (the reference's or ours)."""
    parts = [np.array([int(tree_dict[k]) for k in TREE_INT_KEYS] + [int(bool(tree_dict["cgos_mode"]))], dtype="<i4").tobytes(),
             tree_dict["to_move"].encode("ascii")]
    for node in tree_dict["node"]:
        parts.append(np.array([int(node[k]) for k in NODE_INT_KEYS], dtype="<i4").tobytes())
        parts.append(np.array([float(node[k]) for k in NODE_FLOAT_KEYS], dtype="<f8").tobytes())
        for k in NODE_INT_ARRAYS:
            parts.append(np.asarray(node[k], dtype="<i4").tobytes())
        for k in NODE_FLOAT_ARRAYS:
            parts.append(np.asarray(node[k], dtype="<f8").tobytes())
    return b"".join(parts)


def canonical_sha256(tree_dict) -> str:
    return hashlib.sha256(canonical_bytes(tree_dict)).hexdigest()


def enriched_fields(state):
    """Per node, what enrich_mcts_dict added (the keys a node has), and the tree's sorted_indices_list."""
    return {"nodes": [{k: node[k] for k in ENRICHED_KEYS if k in node} for node in state["tree"]["node"]],
            "sorted_indices_list": state["tree"]["sorted_indices_list"]}


def orchestrate(reference: str):
    if not reference or not os.path.isdir(reference):
        print("no reference checkout (--reference): nothing to do")
        return 1
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for size in (9, 13, 19):
        scratch = tempfile.mkdtemp(prefix=f"ref{size}_")
        try:
            tree = reference
            if size != 9:
                tree = os.path.join(scratch, "ref")
                shutil.copytree(reference, tree, ignore=shutil.ignore_patterns(".git", "__pycache__"))
                path = os.path.join(tree, "board", "constant.py")
                text = open(path, encoding="utf-8").read().replace("BOARD_SIZE = 9", f"BOARD_SIZE = {size}")
                open(path, "w", encoding="utf-8").write(text)
            env["PYTHONPATH"] = tree + os.pathsep + REPO
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--size", str(size)], env=env, cwd=scratch)
        finally:
            shutil.rmtree(scratch, ignore_errors=True)
    return 0


# ======================================================================================
# worker: runs with the reference on sys.path
# ======================================================================================
def worker(size: int):
    import torch

    from board.constant import BOARD_SIZE
    assert BOARD_SIZE == size, (BOARD_SIZE, size)
    from board.go_board import GoBoard
    from board.stone import Stone
    from mcts.dump import enrich_mcts_dict
    from mcts.time_manager import TimeControl, TimeManager
    from mcts.tree import MCTSTree

    from oracle.stubnet import StubNet

    torch.set_grad_enabled(False)
    brd = np.load(os.path.join(GOLD, f"board_s{size}.npz"))
    recs = json.load(open(os.path.join(GOLD, f"trees_s{size}.json")))

    def col(c):
        return Stone.BLACK if c == 1 else Stone.WHITE

    def replay(upto, superko):
        board = GoBoard(board_size=size, komi=7.0, check_superko=superko)
        for mv, c in zip(brd["g0_move"][:upto], brd["g0_color"][:upto]):
            board.put_stone(int(mv), col(int(c)))
        return board

    def quiet(fn):
        stderr, sys.stderr = sys.stderr, open(os.devnull, "w")
        try:
            return fn()
        finally:
            sys.stderr = stderr

    out = {"cases": []}
    for index in CASES[size]:
        rec = recs[index]
        board = replay(rec["ply"], rec["superko"])
        np.random.seed(rec["seed"])
        if rec["kind"] == "puct":
            tree = MCTSTree(StubNet(salt=rec["seed"]), tree_size=2048, batch_size=rec["batch"], cgos_mode=rec["cgos"])
            mode = TimeControl.STRICT_PLAYOUT if rec["mode"] == "STRICT" else TimeControl.CONSTANT_PLAYOUT
            quiet(lambda: tree.search_best_move(board, col(rec["color"]), TimeManager(mode, constant_visits=rec["visits"]), {}))
        else:
            tree = MCTSTree(StubNet(salt=100 + rec["seed"]), tree_size=160 if rec["visits"] <= 100 else 2048)
            tree.generate_move_with_sequential_halving(board, col(rec["color"]),
                                                       TimeManager(TimeControl.CONSTANT_PLAYOUT, constant_visits=rec["visits"]), True)
        assert tree.num_nodes == rec["num_nodes"], (index, tree.num_nodes, rec["num_nodes"])
        case = {k: rec.get(k) for k in ("kind", "seed", "visits", "batch", "mode", "cgos", "ply", "superko", "color")}
        case.update(index=index, num_nodes=int(tree.num_nodes), sha256=canonical_sha256(tree.to_dict()))
        out["cases"].append(case)

    if size == 9:
        small = dict(SMALL)
        board = replay(small["ply"], small["superko"])
        color = 3 - int(brd["g0_color"][small["ply"] - 1])
        np.random.seed(small["seed"])
        tree = MCTSTree(StubNet(salt=small["seed"]), tree_size=small["tree_size"], batch_size=small["batch"])
        quiet(lambda: tree.search_best_move(board, col(color), TimeManager(TimeControl.STRICT_PLAYOUT, constant_visits=small["visits"]), {}))
        text = tree.dump_to_json(board, small["superko"])
        state = json.loads(text)
        enrich_mcts_dict(state)
        small.update(color=color, num_nodes=int(tree.num_nodes), sha256=canonical_sha256(tree.to_dict()), json=text,
                     enriched=enriched_fields(state))
        out["small"] = small

    path = os.path.join(GOLD, f"tree_dump_s{size}.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=0)
    ap.add_argument("--reference", default=os.environ.get("TAMAGO_REFERENCE", ""))
    args = ap.parse_args()
    if args.size:
        worker(args.size)
    else:
        sys.exit(orchestrate(args.reference))
