#!/usr/bin/env python3
"""Reference-written expectations for the board-rule corpus (tests/_rule_corpus.py): every entry is replayed on the
REFERENCE's own GoBoard (board/go_board.py), with check_superko off and on, and what the search would see there is recorded.
The reference is imported at run time from the checkout named by TAMAGO_REFERENCE (never copied into this repository; one
process per board size on a scratch copy with the board-size constant changed, deleted afterwards, as
tools/gen_golden_policy.py does):

    TAMAGO_REFERENCE=<reference checkout> python tools/gen_golden_rule_corpus.py

-> tests/golden/rule_corpus_s{9,13,19}.npz, per size:
   moves / moves_off   the entries' records back to back (padded coordinates, 0 = PASS) and where each one starts
   to_move, names      colour to move and the entry's name
   cand0 / cand0_off   candidate lists of mcts/tree.py:260-264 (legal, check_self_atari_stone < 7, no complete eye, PASS last)
   cand1 / cand1_off   ... with check_superko on
   cells               the on-board cells, row-major
   ko_pos, ko_move, n_moves   the board's ko scalars and move counter
   hash                the positional hash under this repository's Zobrist table (written into the reference's key array
                       before the first board is made)
   tree_roots          the corpus entries the short searches of tests/test_gpu_board_rules.py start from
The files hold data only; the same corpus gives the same bytes."""
import argparse
import io
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")


def orchestrate():
    ref = os.environ.get("TAMAGO_REFERENCE")
    if not ref or not os.path.isdir(ref):
        print("set TAMAGO_REFERENCE to a checkout of the reference - nothing to do")
        return 1
    os.makedirs(GOLD, exist_ok=True)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for size in (9, 13, 19):
        scratch = tempfile.mkdtemp(prefix=f"ref{size}_")
        try:
            tree = os.path.join(scratch, "ref")
            shutil.copytree(ref, tree, ignore=shutil.ignore_patterns(".git", "__pycache__"))
            path = os.path.join(tree, "board", "constant.py")
            text = open(path, encoding="utf-8").read().replace("BOARD_SIZE = 9", f"BOARD_SIZE = {size}")
            open(path, "w", encoding="utf-8").write(text)
            env["PYTHONPATH"] = tree + os.pathsep + REPO + os.pathsep + os.path.join(REPO, "tests")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--size", str(size)], env=env, cwd=scratch)
        finally:
            shutil.rmtree(scratch, ignore_errors=True)
    return 0


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as archive:
        for name, array in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(array), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            archive.writestr(info, buf.getvalue())


def ragged(lists, dtype=np.int16):
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(v) for v in lists])
    flat = np.concatenate([np.asarray(v, dtype=dtype) for v in lists]) if lists else np.zeros(0, dtype)
    return flat, off


def worker(size: int):
    from board.constant import BOARD_SIZE, PASS
    assert BOARD_SIZE == size, (BOARD_SIZE, size)
    import board.zobrist_hash as ref_hash
    from board.go_board import GoBoard
    from board.stone import Stone

    import _rule_corpus as rc
    from tamago_amd.board.go_board import zobrist_keys

    assert ref_hash.hash_bit_mask.shape == zobrist_keys(size).shape
    ref_hash.hash_bit_mask[:] = zobrist_keys(size)                      # the repository's table, in place

    entries = rc.corpus(size)
    out = {"cand0": [], "cand1": [], "cells": [], "ko_pos": [], "ko_move": [], "n_moves": [], "hash": []}
    stderr = sys.stderr
    for entry in entries:
        for flag in (0, 1):
            board = GoBoard(board_size=size, check_superko=bool(flag))
            color = Stone.BLACK
            sys.stderr = io.StringIO()                                # "Cannot save move record." beyond MAX_RECORDS
            try:
                for pos in entry.moves:
                    board.put_stone(pos, color)
                    color = Stone.get_opponent_color(color)
            finally:
                sys.stderr = stderr
            assert color.value == entry.to_move
            cands = board.get_all_legal_pos(color)
            cands = [c for c in cands if board.check_self_atari_stone(c, color) < 7 and not board.is_complete_eye(c, color)]
            cands.append(PASS)
            out[f"cand{flag}"].append([int(c) for c in cands])
        out["cells"].append(board.get_board_data(0))
        out["ko_pos"].append(int(board.ko_pos))
        out["ko_move"].append(int(board.ko_move))
        out["n_moves"].append(int(board.moves))
        out["hash"].append(int(board.positional_hash[0]))
    arrays = {}
    arrays["moves"], arrays["moves_off"] = ragged([e.moves for e in entries])
    arrays["to_move"] = np.array([e.to_move for e in entries], dtype=np.uint8)
    arrays["names"] = np.array([e.name for e in entries])
    for flag in (0, 1):
        arrays[f"cand{flag}"], arrays[f"cand{flag}_off"] = ragged(out[f"cand{flag}"])
    arrays["cells"] = np.array(out["cells"], dtype=np.uint8)
    for key in ("ko_pos", "ko_move", "n_moves"):
        arrays[key] = np.array(out[key], dtype=np.int32)
    arrays["hash"] = np.array(out["hash"], dtype=np.uint64)
    arrays["tree_roots"] = np.array(rc.tree_roots(size), dtype=np.int32)
    path = os.path.join(GOLD, f"rule_corpus_s{size}.npz")
    save_npz(path, arrays)
    differ = sum(a != b for a, b in zip(out["cand0"], out["cand1"]))
    print(size, len(entries), "entries,", differ, "whose candidates depend on superko,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--size", type=int, default=0)
    args = parser.parse_args()
    sys.exit(worker(args.size) or 0 if args.size else orchestrate())
