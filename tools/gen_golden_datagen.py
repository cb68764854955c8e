#!/usr/bin/env python3
"""Golden fixtures for the "next" row 8(f).3 (SGF reader + RL / SL data generator), produced by
running the REFERENCE's sgf/reader.py and nn/data_generator.py on the reference-recorded
self-play games of tests/golden/selfplay_games.json.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/root/reference python tools/gen_golden_datagen.py

The reference's chunk sizes (learning_param.py: BATCH_SIZE 256, DATA_SET_SIZE 1 024 000) are
patched down IN THE IMPORTED MODULE so that three games exercise the chunking and the
remainder path; the patched values are recorded in the fixture.  RL games sit in one directory
each (kifu_dir_list order is then the list order - a plain glob order is file-system
dependent and feeds random.shuffle).

    TAMAGO_REFERENCE=<checkout of the reference> python tools/gen_golden_datagen.py --large

writes tests/golden/datagen_s13.{json,npz} and datagen_s19.{json,npz}: the reference's SL generator on two seeded random
legal records per size (40 moves each, generated here with this repo's board and kept in the JSON as SGF text).  The
reference's board size is a module constant (board/constant.py:4), so each size runs in a process of its own on a
scratch copy of the reference with that constant changed - the recipe of tools/gen_golden_policy.py."""
import glob
import hashlib
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


def main():
    import nn.data_generator as dg                      # the reference
    from sgf.reader import SGFReader
    games = json.load(open(os.path.join(GOLD, "selfplay_games.json")))
    keys = sorted(games)
    work = tempfile.mkdtemp(prefix="dg_")
    dirs = []
    for k in keys:
        d = os.path.join(work, "g" + k.replace(",", "_"))
        os.makedirs(d)
        with open(os.path.join(d, k.split(",")[0] + ".sgf"), "w", encoding="utf-8") as f:
            f.write(games[k])
        dirs.append(d)
    alld = os.path.join(work, "all")
    os.makedirs(alld)
    for k in keys:
        with open(os.path.join(alld, k.split(",")[0] + ".sgf"), "w", encoding="utf-8") as f:
            f.write(games[k])

    # --- reader ---
    reader = {}
    for k in keys:
        r = SGFReader(games[k], 9, literal=True)
        reader[k] = {
            "size": r.size, "komi": r.komi, "value_label": r.get_value_label(), "n_moves": r.get_n_moves(),
            "moves": [int(r.get_move_data(i)) for i in range(r.get_n_moves())],
            "colors": [int(r.get_color(i).value) for i in range(r.get_n_moves())],
            "comment_sha": [hashlib.sha256(r.get_comment(i).encode()).hexdigest()[:16] for i in range(r.get_n_moves())],
            "comment0": r.get_comment(0),
            "application": r.application, "black": r.black_player_name, "white": r.white_player_name,
        }
    # reader edge cases: passes written as "B[]" and "B[tt]", ignored tags, handicap-less header
    text = "(;GM[1]FF[4]SZ[9]KM[6.5]RE[W+R]PB[a]PW[b]DT[2024-01-01];B[ee]C[first];W[];B[tt]C[x y:1];W[aa])"
    r = SGFReader(text, 9, literal=True)
    reader["edge"] = {"text": text, "komi": r.komi, "value_label": r.get_value_label(),
                      "moves": [int(r.get_move_data(i)) for i in range(r.get_n_moves())],
                      "comments": [r.get_comment(i) for i in range(r.get_n_moves())]}

    # --- RL data ---
    dg.BATCH_SIZE, dg.DATA_SET_SIZE = 8, 16
    prog = os.path.join(work, "prog")
    os.makedirs(os.path.join(prog, "data"))
    random.seed(11)
    np.random.seed(11)
    dg.generate_reinforcement_learning_data(prog, dirs, 9)
    out = {}
    meta = {"rl_batch_size": 8, "rl_data_set_size": 16, "rl_seed": 11, "keys": keys, "reader": reader}
    files = sorted(glob.glob(os.path.join(prog, "data", "rl_data_*.npz")))
    meta["rl_files"] = [os.path.basename(f) for f in files]
    for f in files:
        z = np.load(f)
        name = os.path.basename(f)[:-4]
        for key in ("input", "policy", "value", "kifu_count"):
            out[f"{name}_{key}"] = z[key]
    # --- SL data (digests: 8 symmetries of every position) ---
    dg.BATCH_SIZE, dg.DATA_SET_SIZE = 64, 1024
    prog2 = os.path.join(work, "prog2")
    os.makedirs(os.path.join(prog2, "data"))
    dg.generate_supervised_learning_data(prog2, alld, 9)
    files = sorted(glob.glob(os.path.join(prog2, "data", "sl_data_*.npz")))
    meta["sl_batch_size"], meta["sl_data_set_size"] = 64, 1024
    meta["sl_files"] = {}
    for f in files:
        z = np.load(f)
        meta["sl_files"][os.path.basename(f)] = {
            key: {"shape": list(z[key].shape), "dtype": str(z[key].dtype), "sha256": digest(z[key])}
            for key in ("input", "policy", "value", "kifu_count")}
        name = os.path.basename(f)[:-4]
        out[f"{name}_input_head"] = z["input"][:16]
        out[f"{name}_policy_head"] = z["policy"][:16]
        out[f"{name}_value_head"] = z["value"][:16]
    np.savez_compressed(os.path.join(GOLD, "datagen_s9.npz"), **out)
    json.dump(meta, open(os.path.join(GOLD, "datagen_s9.json"), "w"), indent=1)
    print("wrote datagen_s9.npz / .json:", meta["rl_files"], list(meta["sl_files"]))


LARGE = {13: (131, 132), 19: (191, 192)}          # board size -> seeds of its two records
LARGE_MOVES = 40
LARGE_BATCH_SIZE, LARGE_DATA_SET_SIZE = 64, 512    # 2 x 40 x 8 = 640 samples: one full chunk that splits the second game, and a tail


def large_orchestrate():
    ref = os.environ.get("TAMAGO_REFERENCE")
    if not ref or not os.path.isdir(ref):
        print("set TAMAGO_REFERENCE to a checkout of the reference - nothing to do")
        return 1
    sys.path.insert(0, REPO)
    from tests._replay_records import random_record, sgf_text
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for size, seeds in LARGE.items():
        scratch = tempfile.mkdtemp(prefix=f"ref{size}_")
        try:
            tree = os.path.join(scratch, "ref")
            shutil.copytree(ref, tree, ignore=shutil.ignore_patterns(".git", "__pycache__"))
            path = os.path.join(tree, "board", "constant.py")
            text = open(path, encoding="utf-8").read().replace("BOARD_SIZE = 9", f"BOARD_SIZE = {size}")
            open(path, "w", encoding="utf-8").write(text)
            games = {f"{i + 1:02d}": sgf_text(size, random_record(size, LARGE_MOVES, seed), ("B+2.5", "W+R")[i])
                     for i, seed in enumerate(seeds)}
            json.dump({"size": size, "seeds": list(seeds), "games": games}, open(os.path.join(scratch, "in.json"), "w"))
            env["PYTHONPATH"] = tree
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--large-worker", os.path.join(scratch, "in.json")],
                                  env=env, cwd=scratch)
        finally:
            shutil.rmtree(scratch, ignore_errors=True)
    return 0


def large_worker(spec_path):
    import nn.data_generator as dg                      # the reference, at the size its constant was set to
    from board.constant import BOARD_SIZE
    spec = json.load(open(spec_path))
    size = spec["size"]
    assert BOARD_SIZE == size, (BOARD_SIZE, size)
    work = tempfile.mkdtemp(prefix="dg_")
    try:
        kifu = os.path.join(work, "kifu")
        os.makedirs(kifu)
        for name, text in spec["games"].items():
            with open(os.path.join(kifu, name + ".sgf"), "w", encoding="utf-8") as f:
                f.write(text)
        dg.BATCH_SIZE, dg.DATA_SET_SIZE = LARGE_BATCH_SIZE, LARGE_DATA_SET_SIZE
        prog = os.path.join(work, "prog")
        os.makedirs(os.path.join(prog, "data"))
        dg.generate_supervised_learning_data(prog, kifu, size)
        meta = {"size": size, "seeds": spec["seeds"], "games": spec["games"], "sl_batch_size": LARGE_BATCH_SIZE,
                "sl_data_set_size": LARGE_DATA_SET_SIZE, "sl_files": {}}
        out = {}
        for f in sorted(glob.glob(os.path.join(prog, "data", "sl_data_*.npz"))):
            z = np.load(f)
            meta["sl_files"][os.path.basename(f)] = {
                key: {"shape": list(z[key].shape), "dtype": str(z[key].dtype), "sha256": digest(z[key])}
                for key in ("input", "policy", "value", "kifu_count")}
            name = os.path.basename(f)[:-4]
            out[f"{name}_input_head"] = z["input"][:16]
            out[f"{name}_policy_head"] = z["policy"][:16]
            out[f"{name}_value_head"] = z["value"][:16]
        np.savez_compressed(os.path.join(GOLD, f"datagen_s{size}.npz"), **out)
        json.dump(meta, open(os.path.join(GOLD, f"datagen_s{size}.json"), "w"), indent=1)
        print(f"wrote datagen_s{size}.npz / .json:", list(meta["sl_files"]))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    if "--large-worker" in sys.argv:
        sys.exit(large_worker(sys.argv[sys.argv.index("--large-worker") + 1]))
    sys.exit(large_orchestrate() if "--large" in sys.argv else main())
