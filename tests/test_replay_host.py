"""Host half of the device_replay data path (no GPU): the whole-chunk target builders of nn/feature.py against the
per-sample functions they replace, for all 8 symmetries at 9, 13 and 19, and the symmetry tables they index with."""
import numpy as np
import pytest

from tamago_amd.board.constant import PASS
from tamago_amd.board.go_board import GoBoard
from tamago_amd.nn import feature

SIZES = (9, 13, 19)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want)


@pytest.mark.parametrize("size", SIZES)
def test_symmetry_tables_are_permutations(size):
    index = feature.symmetry_index_table(size)
    assert index.shape == (8, size * size) and index.dtype == np.int64
    board = GoBoard(size)
    pos = feature.symmetry_pos_table(size)
    assert pos.shape == (8, size * size + 1) and pos.dtype == np.int64
    for sym in range(8):
        assert sorted(index[sym]) == list(range(size * size))
        assert [int(v) for v in index[sym]] == [feature.symmetric_index(size, q, sym) for q in range(size * size)]
        assert [int(v) for v in pos[sym][:-1]] == [board.onboard_pos[i] for i in index[sym]]
        assert pos[sym][-1] == PASS
    assert np.array_equal(index[0], np.arange(size * size))
    assert len({index[sym].tobytes() for sym in range(8)}) == 8


@pytest.mark.parametrize("size", SIZES)
def test_sl_targets_equal_per_sample_function(size):
    board = GoBoard(size)
    rs = np.random.RandomState(size)
    # corners, an edge point, the centre, random points, and PASS as the move played
    w = size + 2
    moves = [PASS, w + 1, w + size, size * w + 1, size * w + size, w + 2, (size // 2 + 1) * w + size // 2 + 1]
    moves += [board.onboard_pos[i] for i in rs.randint(0, size * size, size=5)]
    pos = np.repeat(moves, 8)
    sym = np.tile(np.arange(8), len(moves))
    want = np.array([feature.generate_target_data(board, int(p), int(s)) for p, s in zip(pos, sym)])
    got = feature.generate_target_data_batch(size, pos, sym)
    assert want.dtype == np.int64
    _same(got, want)
    assert (got.sum(axis=1) == 1).all() and (got[:8, -1] == 1).all()


@pytest.mark.parametrize("size", SIZES)
def test_rl_targets_equal_per_sample_function(size):
    board = GoBoard(size)
    rs = np.random.RandomState(100 + size)
    coord = board.coordinate

    def comment(points, with_pass):
        names = [coord.convert_to_gtp_format(board.onboard_pos[i]) for i in points] + (["PASS"] if with_pass else [])
        probs = rs.dirichlet(np.ones(len(names)))
        return " ".join([str(len(names))] + [f"{n}:{float(p)!r}" for n, p in zip(names, probs)])

    comments = ["",                                                    # a ply without a comment: no candidates
                comment([0, size - 1, size * size - size, size * size - 1], True),     # the corners and PASS
                comment([], True),                                     # PASS alone
                comment(list(rs.choice(size * size, size=16, replace=False)), False),
                comment(list(rs.choice(size * size, size=5, replace=False)), True),
                "2 A1:0.25 A1:0.75"]                                   # a later entry replaces an earlier one
    texts = [c for c in comments for _ in range(8)]
    sym = np.tile(np.arange(8), len(comments))
    want = np.array([feature.generate_rl_target_data(board, t, int(s)) for t, s in zip(texts, sym)])
    got = feature.generate_rl_target_data_batch(size, texts, sym)
    assert want.dtype == np.float64
    _same(got, want)
    assert (got[:8] == 1e-18).all()
    assert (got[16:24, -1] > 0.99).all()                               # "1 PASS:1.0"
    assert (got[8:16, -1] != 1e-18).all() and (got[24:32, -1] == 1e-18).all()


def test_empty_batches_keep_shape_and_dtype():
    got = feature.generate_target_data_batch(9, [], [])
    assert got.shape == (0, 82) and got.dtype == np.int64
    got = feature.generate_rl_target_data_batch(9, [], [])
    assert got.shape == (0, 82) and got.dtype == np.float64


# ---- everything of the device_replay path but the planes: records, random-call order, chunking, targets, value labels ----
def _stub_planes(monkeypatch, dg):
    """No GPU here: both paths get planes of zeros (host: _Samples.planes; device: _ReplayPending._replay)."""
    import torch
    monkeypatch.setattr(dg._Samples, "planes",
                        lambda self, device_index=0: np.zeros((len(self), 6, self.size, self.size), dtype=np.float32))
    monkeypatch.setattr(dg._ReplayPending, "_replay",
                        lambda self, records: torch.zeros((sum(len(r.ply) for r in records), 6, self.size, self.size)))


def _golden_games(root, one_dir_per_game):
    import os
    from tests.helpers import load_json
    games = load_json("selfplay_games.json")
    dirs = []
    for key in sorted(games):
        d = os.path.join(root, "g" + key.replace(",", "_")) if one_dir_per_game else os.path.join(root, "all")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, key.split(",")[0] + ".sgf"), "w", encoding="utf-8") as f:
            f.write(games[key])
        dirs.append(d)
    return dirs


def test_rl_policy_value_and_chunking_equal_reference_files(tmp_path, monkeypatch):
    import glob
    import os
    import random
    import tamago_amd.nn.data_generator as dg
    from tests.helpers import load_json, load_npz
    meta, fix = load_json("datagen_s9.json"), load_npz("datagen_s9.npz")
    _stub_planes(monkeypatch, dg)
    monkeypatch.setattr(dg, "BATCH_SIZE", meta["rl_batch_size"])
    monkeypatch.setattr(dg, "DATA_SET_SIZE", meta["rl_data_set_size"])
    dirs = _golden_games(str(tmp_path), True)
    states = []
    for device_replay in (False, True):
        prog = tmp_path / f"prog{int(device_replay)}"
        os.makedirs(prog / "data")
        random.seed(meta["rl_seed"])
        np.random.seed(meta["rl_seed"])
        dg.generate_reinforcement_learning_data(str(prog), dirs, 9, device_replay=device_replay)
        states.append((random.random(), float(np.random.random_sample())))      # the generators are left where they were
        files = sorted(os.path.basename(f) for f in glob.glob(str(prog / "data" / "rl_data_*.npz")))
        assert files == meta["rl_files"]
        for name in files:
            got = np.load(prog / "data" / name)
            assert got["input"].shape == fix[f"{name[:-4]}_input"].shape and got["input"].dtype == np.float32
            for key in ("policy", "value", "kifu_count"):
                _same(got[key], fix[f"{name[:-4]}_{key}"])
    assert states[0] == states[1]


def test_sl_policy_value_and_chunking_equal_reference_files(tmp_path, monkeypatch):
    import glob
    import hashlib
    import os
    import tamago_amd.nn.data_generator as dg
    from tests.helpers import load_json, load_npz
    meta, fix = load_json("datagen_s9.json"), load_npz("datagen_s9.npz")
    _stub_planes(monkeypatch, dg)
    monkeypatch.setattr(dg, "BATCH_SIZE", meta["sl_batch_size"])
    monkeypatch.setattr(dg, "DATA_SET_SIZE", meta["sl_data_set_size"])
    dirs = _golden_games(str(tmp_path), False)
    os.makedirs(tmp_path / "prog" / "data")
    dg.generate_supervised_learning_data(str(tmp_path / "prog"), dirs[0], 9, device_replay=True)
    files = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "prog" / "data" / "sl_data_*.npz")))
    assert files == sorted(meta["sl_files"])
    for name in files:
        got = np.load(tmp_path / "prog" / "data" / name)
        for key in ("policy", "value", "kifu_count"):
            want = meta["sl_files"][name][key]
            a = np.ascontiguousarray(got[key])
            assert list(got[key].shape) == want["shape"] and str(a.dtype) == want["dtype"], (name, key)
            assert hashlib.sha256(a.tobytes()).hexdigest() == want["sha256"], (name, key)
        assert list(got["input"].shape) == meta["sl_files"][name]["input"]["shape"]
        _same(got["policy"][:16], fix[f"{name[:-4]}_policy_head"])
