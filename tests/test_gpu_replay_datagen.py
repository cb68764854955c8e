"""device_replay=True of the data generators (tg_replay_run: the records are replayed on the device, the targets built as
one table look-up per chunk) against the reference-written files and against the host path of the same checkout; the
in-memory chunks against the files as the trainer loads them; the errors of the C ABI.  Every comparison is exact."""
import ctypes
import functools
import glob
import hashlib
import os
import random

import numpy as np
import pytest

from tamago_amd.board.go_board import GoBoard
from tests._replay_records import events, random_record, sgf_text
from tests.helpers import load_json, load_npz

pytestmark = pytest.mark.gpu

# board size -> (moves per game, seeds): seeds for which the records hold what the replay can get wrong (asserted below)
RECORDS = {9: (200, (6, 18, 36)), 13: (150, (6, 21, 59)), 19: (250, (44, 33))}


@functools.lru_cache(maxsize=None)
def _records(size):
    n_moves, seeds = RECORDS[size]
    return tuple(tuple(random_record(size, n_moves, seed)) for seed in seeds)


def _write(root, texts, one_dir_per_game):
    dirs = []
    for i, text in enumerate(texts):
        d = os.path.join(root, f"g{i:03d}") if one_dir_per_game else os.path.join(root, "all")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"{i + 1:04d}.sgf"), "w", encoding="utf-8") as f:
            f.write(text)
        dirs.append(d)
    return dirs


def _generate(dg, tmp_path, name, kind, dirs, size, device_replay, seed=3):
    prog = tmp_path / name
    os.makedirs(prog / "data")
    random.seed(seed)
    np.random.seed(seed)
    if kind == "rl":
        dg.generate_reinforcement_learning_data(str(prog), dirs, size, device_replay=device_replay)
    else:
        dg.generate_supervised_learning_data(str(prog), dirs[0], size, device_replay=device_replay)
    return prog / "data"


def _assert_same_files(got_dir, want_dir, prefix):
    got = sorted(os.path.basename(f) for f in glob.glob(str(got_dir / f"{prefix}_*.npz")))
    want = sorted(os.path.basename(f) for f in glob.glob(str(want_dir / f"{prefix}_*.npz")))
    assert got == want and want
    rows = 0
    for name in want:
        a, b = np.load(got_dir / name), np.load(want_dir / name)
        assert sorted(a.files) == sorted(b.files) == ["input", "kifu_count", "policy", "value"]
        for key in b.files:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (name, key)
            assert np.array_equal(a[key], b[key]), (name, key)
        rows += len(b["value"])
    return rows


# ---- 1. the reference-written files -------------------------------------------------------------------------------------
def _write_golden_games(root, one_dir_per_game):
    games = load_json("selfplay_games.json")
    dirs = []
    for key in sorted(games):
        d = os.path.join(root, "g" + key.replace(",", "_")) if one_dir_per_game else os.path.join(root, "all")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, key.split(",")[0] + ".sgf"), "w", encoding="utf-8") as f:
            f.write(games[key])
        dirs.append(d)
    return dirs


def test_rl_data_files_equal_reference_with_device_replay(tmp_path, monkeypatch):
    import tamago_amd.nn.data_generator as dg
    meta = load_json("datagen_s9.json")
    fix = load_npz("datagen_s9.npz")
    monkeypatch.setattr(dg, "BATCH_SIZE", meta["rl_batch_size"])
    monkeypatch.setattr(dg, "DATA_SET_SIZE", meta["rl_data_set_size"])
    dirs = _write_golden_games(str(tmp_path), True)
    os.makedirs(tmp_path / "prog" / "data")
    random.seed(meta["rl_seed"])
    np.random.seed(meta["rl_seed"])
    flagged = dg.REPLAY_STATS["flagged"]
    dg.generate_reinforcement_learning_data(str(tmp_path / "prog"), dirs, 9, device_replay=True)
    assert dg.REPLAY_STATS["flagged"] == flagged
    files = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "prog" / "data" / "rl_data_*.npz")))
    assert files == meta["rl_files"]
    for name in files:
        got = np.load(tmp_path / "prog" / "data" / name)
        stem = name[:-4]
        for key in ("input", "policy", "value", "kifu_count"):
            want = fix[f"{stem}_{key}"]
            assert got[key].dtype == want.dtype and got[key].shape == want.shape, (name, key)
            assert np.array_equal(got[key], want), (name, key)


def _assert_sl_files_equal_fixture(dg, tmp_path, monkeypatch, meta, fix, kifu_dir, size):
    monkeypatch.setattr(dg, "BATCH_SIZE", meta["sl_batch_size"])
    monkeypatch.setattr(dg, "DATA_SET_SIZE", meta["sl_data_set_size"])
    os.makedirs(tmp_path / "prog" / "data")
    flagged = dg.REPLAY_STATS["flagged"]
    dg.generate_supervised_learning_data(str(tmp_path / "prog"), kifu_dir, size, device_replay=True)
    assert dg.REPLAY_STATS["flagged"] == flagged
    files = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "prog" / "data" / "sl_data_*.npz")))
    assert files == sorted(meta["sl_files"])
    for name in files:
        got = np.load(tmp_path / "prog" / "data" / name)
        for key, want in meta["sl_files"][name].items():
            a = np.ascontiguousarray(got[key])
            assert list(got[key].shape) == want["shape"] and str(a.dtype) == want["dtype"], (name, key)
            assert hashlib.sha256(a.tobytes()).hexdigest() == want["sha256"], (name, key)
        stem = name[:-4]
        assert np.array_equal(got["input"][:16], fix[f"{stem}_input_head"])
        assert np.array_equal(got["policy"][:16], fix[f"{stem}_policy_head"])
        assert np.array_equal(got["value"][:16], fix[f"{stem}_value_head"])


def test_sl_data_files_equal_reference_with_device_replay(tmp_path, monkeypatch):
    import tamago_amd.nn.data_generator as dg
    dirs = _write_golden_games(str(tmp_path), False)
    _assert_sl_files_equal_fixture(dg, tmp_path, monkeypatch, load_json("datagen_s9.json"), load_npz("datagen_s9.npz"),
                                   dirs[0], 9)


@pytest.mark.parametrize("size", (13, 19))
def test_sl_data_files_equal_reference_on_larger_boards(tmp_path, monkeypatch, size):
    """tests/golden/datagen_s13 / _s19: the reference's SL generator on two 40-move records (tools/gen_golden_datagen.py
    --large); the records are in the JSON."""
    import tamago_amd.nn.data_generator as dg
    meta = load_json(f"datagen_s{size}.json")
    kifu = tmp_path / "kifu"
    os.makedirs(kifu)
    for name, text in meta["games"].items():
        with open(kifu / f"{name}.sgf", "w", encoding="utf-8") as f:
            f.write(text)
    _assert_sl_files_equal_fixture(dg, tmp_path, monkeypatch, meta, load_npz(f"datagen_s{size}.npz"), str(kifu), size)


# ---- 2. device path against host path at 9, 13 and 19 -------------------------------------------------------------------
@pytest.mark.parametrize("size", (9, 13, 19))
def test_device_path_equals_host_path(tmp_path, monkeypatch, size):
    import tamago_amd.nn.data_generator as dg
    records = _records(size)
    seen = [events(size, moves) for moves in records]
    assert sum(e["big_captures"] for e in seen) >= 1, "no capture of a string of two or more stones"
    assert sum(e["ko_captures"] for e in seen) >= 1, "no ko capture"
    assert sum(e["pass_then_move"] for e in seen) >= 1, "no pass followed by a board move"
    # SL samples every ply, so a pass at ply >= 1 is itself a sample (target PASS) and so is the position after it
    assert any(e["passes"] for e in seen), "no pass at ply >= 1"
    texts = [sgf_text(size, moves, ("B+0.5", "W+R", "0")[i], seed=1000 * size + i) for i, moves in enumerate(records)]
    before = dict(dg.REPLAY_STATS)

    monkeypatch.setattr(dg, "BATCH_SIZE", 64)
    monkeypatch.setattr(dg, "DATA_SET_SIZE", 1024)          # chunks end in the middle of a game
    dirs = _write(str(tmp_path / "sl"), texts, False)
    want = _generate(dg, tmp_path, "sl_host", "sl", dirs, size, False)
    got = _generate(dg, tmp_path, "sl_dev", "sl", dirs, size, True)
    rows = _assert_same_files(got, want, "sl_data")
    assert rows == sum(len(m) for m in records) * 8 // 64 * 64

    monkeypatch.setattr(dg, "BATCH_SIZE", 4)
    monkeypatch.setattr(dg, "DATA_SET_SIZE", 12)
    dirs = _write(str(tmp_path / "rl"), texts, True)
    want = _generate(dg, tmp_path, "rl_host", "rl", dirs, size, False, seed=size)
    got = _generate(dg, tmp_path, "rl_dev", "rl", dirs, size, True, seed=size)
    assert _assert_same_files(got, want, "rl_data") == len(records) * 8
    assert dg.REPLAY_STATS["flagged"] == before["flagged"], "a legal record was flagged"
    assert dg.REPLAY_STATS["games"] > before["games"]


# ---- 3. edge records -----------------------------------------------------------------------------------------------------
def _edge_texts(size=9):
    w = size + 2
    at = lambda x, y: x + y * w                                           # noqa: E731
    short = [[], [at(5, 5)], list(random_record(size, 7, 70)),
             [at(3, 3), at(4, 4), 0, 0],                                  # ends in two passes
             [0, at(2, 2), 0, at(3, 2), 0, 0]]                            # (RL samples its passes at ply >= 1 too)
    short += [list(random_record(size, 3 + i % 5, 500 + i)) for i in range(300)]
    return [sgf_text(size, moves, ("B+1.5", "W+2.5")[i % 2], seed=i) for i, moves in enumerate(short)], short


def test_edge_records_in_one_call(tmp_path, monkeypatch):
    """Games of 0, 1 and 7 moves (RL takes every ply of a game of at most 8), a game that ends in two passes, samples at
    ply 0 and at the last ply (SL takes them all), and more games than the device has compute units - in one launch."""
    import tamago_amd.nn.data_generator as dg
    texts, moves = _edge_texts()
    assert len(texts) > 256
    monkeypatch.setattr(dg, "BATCH_SIZE", 8)
    monkeypatch.setattr(dg, "DATA_SET_SIZE", 1 << 20)
    dirs = _write(str(tmp_path / "rl"), texts, True)
    want = _generate(dg, tmp_path, "rl_host", "rl", dirs, 9, False)
    before = dict(dg.REPLAY_STATS)
    got = _generate(dg, tmp_path, "rl_dev", "rl", dirs, 9, True)
    assert dg.REPLAY_STATS["calls"] == before["calls"] + 1 and dg.REPLAY_STATS["flagged"] == before["flagged"]
    assert _assert_same_files(got, want, "rl_data") == sum(min(len(m), 8) for m in moves) // 8 * 8

    dirs = _write(str(tmp_path / "sl"), texts, False)
    want = _generate(dg, tmp_path, "sl_host", "sl", dirs, 9, False)
    before = dict(dg.REPLAY_STATS)
    got = _generate(dg, tmp_path, "sl_dev", "sl", dirs, 9, True)
    assert dg.REPLAY_STATS["calls"] == before["calls"] + 1 and dg.REPLAY_STATS["flagged"] == before["flagged"]
    assert _assert_same_files(got, want, "sl_data") == sum(len(m) for m in moves) * 8 // 8 * 8


def test_move_on_an_occupied_point_flags_that_game_only(tmp_path, monkeypatch):
    import tamago_amd.nn.data_generator as dg
    size, w = 9, 11
    games = [list(random_record(size, 30, 900 + i)) for i in range(5)]
    bad = games[2]
    bad[4] = next(m for m in bad[:4] if m != 0)                          # the fifth move lands on a stone
    board = GoBoard(size)
    for ply, pos in enumerate(bad[:4]):
        board.put_stone(pos, 1 + ply % 2)
    assert board.cells[bad[4]] in (1, 2)
    texts = [sgf_text(size, moves, "W+R", seed=40 + i) for i, moves in enumerate(games)]
    monkeypatch.setattr(dg, "BATCH_SIZE", 16)
    monkeypatch.setattr(dg, "DATA_SET_SIZE", 1 << 20)
    dirs = _write(str(tmp_path / "sl"), texts, False)
    want = _generate(dg, tmp_path, "sl_host", "sl", dirs, size, False)
    before = dict(dg.REPLAY_STATS)
    got = _generate(dg, tmp_path, "sl_dev", "sl", dirs, size, True)
    assert dg.REPLAY_STATS["flagged"] == before["flagged"] + 1
    assert _assert_same_files(got, want, "sl_data") == 5 * 30 * 8 // 16 * 16
    # which game: the same records straight through the C ABI
    flags, _ = _run_replay(size, games, [list(range(len(g))) for g in games])
    assert flags.tolist() == [0, 0, 1, 0, 0]
    # ... and a coordinate that is none of this board
    games[0][3] = w * w + 5
    games[4][0] = 3                                                      # a border cell
    flags, _ = _run_replay(size, games, [list(range(len(g))) for g in games])
    assert flags.tolist() == [1, 0, 1, 0, 1]


def _run_replay(size, games, plies, sym=0):
    import torch
    from tamago_amd import lib as tl
    lib = tl.load()
    handle = ctypes.c_void_p()
    tl.check(lib.tg_replay_create(size, 0, ctypes.byref(handle)), "tg_replay_create")
    try:
        offsets = np.zeros(len(games) + 1, dtype=np.int64)
        np.cumsum([len(g) for g in games], out=offsets[1:])
        s_off = np.zeros(len(games) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in plies], out=s_off[1:])
        moves = np.array([m for g in games for m in g], dtype=np.int32)
        ply = np.array([p for ps in plies for p in ps], dtype=np.int32)
        syms = np.full(len(ply), sym, dtype=np.int8)
        flags = np.full(len(games), -1, dtype=np.int32)
        planes = torch.zeros((len(ply), 6, size, size), dtype=torch.float32, device="cuda:0")
        tl.check(lib.tg_replay_run(handle, moves.ctypes.data, offsets.ctypes.data, len(games), ply.ctypes.data,
                                   syms.ctypes.data, s_off.ctypes.data, planes.data_ptr(), flags.ctypes.data,
                                   torch.cuda.current_stream().cuda_stream), "tg_replay_run")
        return flags, planes.cpu().numpy()
    finally:
        lib.tg_replay_destroy(handle)


# ---- 4. chunks in device memory ------------------------------------------------------------------------------------------
def test_in_memory_chunks_equal_loaded_files(tmp_path, monkeypatch):
    """iter_reinforcement_learning_chunks + the trainer's shuffle = np.load of the files + load_data_set, row for row,
    when both start from the same seeds: the batches HipTrainer.step sees are the same."""
    import torch
    import tamago_amd.nn.data_generator as dg
    from tamago_amd.nn import learn
    games = load_json("selfplay_games_400.json")
    texts = [games[k] for k in sorted(games)]
    texts += [sgf_text(9, moves, "B+3.5", seed=7 + i) for i, moves in enumerate(_records(9))]
    monkeypatch.setattr(dg, "BATCH_SIZE", 8)
    monkeypatch.setattr(dg, "DATA_SET_SIZE", 16)
    dirs = _write(str(tmp_path / "rl"), texts, True)
    data = _generate(dg, tmp_path, "files", "rl", dirs, 9, False, seed=21)
    files = sorted(glob.glob(str(data / "rl_data_*.npz")))
    assert len(files) >= 3
    want = [learn.load_data_set(path) for path in files]

    random.seed(21)
    np.random.seed(21)
    got = []
    for chunk in dg.iter_reinforcement_learning_chunks(dirs, 9, torch.device("cuda", 0)):
        assert all(t.is_cuda for t in chunk)
        assert chunk[0].dtype == torch.float32 and chunk[1].dtype == torch.float32 and chunk[2].dtype == torch.int64
        got.append(tuple(t.cpu().numpy() for t in learn.permute_chunk_on_device(*chunk)))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape
            assert np.array_equal(x, y)


# ---- 5. the C ABI's errors ------------------------------------------------------------------------------------------------
def test_replay_abi_errors():
    from tamago_amd import lib as tl
    lib = tl.load()
    handle = ctypes.c_void_p()
    assert lib.tg_replay_create(11, 0, ctypes.byref(handle)) == -1 and handle.value is None
    assert b"board size 11" in lib.tg_last_error()
    assert lib.tg_replay_create(9, 0, None) == -1
    assert lib.tg_replay_destroy(None) == 0
    tl.check(lib.tg_replay_create(9, 0, ctypes.byref(handle)), "tg_replay_create")
    try:
        offsets = np.array([0, 2], dtype=np.int64)
        moves = np.array([12, 13], dtype=np.int32)
        ply = np.array([0], dtype=np.int32)
        sym = np.array([0], dtype=np.int8)
        s_off = np.array([0, 1], dtype=np.int64)
        flags = np.zeros(1, dtype=np.int32)
        args = [moves.ctypes.data, offsets.ctypes.data, 1, ply.ctypes.data, sym.ctypes.data, s_off.ctypes.data, None,
                flags.ctypes.data, None]
        assert lib.tg_replay_run(handle, *args) == -1 and b"null" in lib.tg_last_error()          # no planes
        assert lib.tg_replay_run(None, *args) == -1
        args[1] = None
        assert lib.tg_replay_run(handle, *args) == -1 and b"null" in lib.tg_last_error()
        import torch
        planes = torch.zeros((1, 6, 9, 9), device="cuda:0")
        ply[0] = 2                                                        # a sample beyond the game's moves
        assert lib.tg_replay_run(handle, moves.ctypes.data, offsets.ctypes.data, 1, ply.ctypes.data, sym.ctypes.data,
                                 s_off.ctypes.data, planes.data_ptr(), flags.ctypes.data, None) == -1
        assert b"beyond" in lib.tg_last_error()
    finally:
        lib.tg_replay_destroy(handle)


# ---- 6. tools/rl_loop.py with device_data ---------------------------------------------------------------------------------
def test_generation_with_device_data_trains_without_files(tmp_path, monkeypatch):
    """self-play -> tg_replay_run -> chunks in device memory -> training steps: no rl_data file is written, and the trainer
    takes the batches the records hold (8 sampled positions per game)."""
    import sys
    import torch
    import tamago_amd.nn.data_generator as dg
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import rl_loop
    monkeypatch.setattr(dg, "BATCH_SIZE", 32)
    torch.manual_seed(11)
    np.random.seed(11)
    random.seed(11)
    prog = str(tmp_path)
    lines = []
    before = dict(dg.REPLAY_STATS)
    stats, loss = rl_loop.run_generation(prog, 0, 24, 16, 16, 32, log=lines.append, device_data=True)
    assert stats["games"] == 24 and len(glob.glob(os.path.join(prog, "archive", "0", "*.sgf"))) == 24
    assert glob.glob(os.path.join(prog, "data", "rl_data_*.npz")) == []
    assert dg.REPLAY_STATS["games"] == before["games"] + 24 and dg.REPLAY_STATS["flagged"] == before["flagged"]
    assert np.isfinite(loss["loss"]) and loss["loss"] > 0
    ck = torch.load(os.path.join(prog, "model", "rl-state.ckpt"), map_location="cpu")
    assert ck["num_trained_batches"] == 24 * 8 // 32
    assert "data" in lines[-1] and "train" in lines[-1]
