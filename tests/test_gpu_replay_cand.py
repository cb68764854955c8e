"""tg_replay_run_cand (replay_cand_kernel, csrc/search.hip): the candidate masks of replayed records against the reference-written
candidate lists of the rule corpus (tests/golden/rule_corpus_s*.npz) and against the host board's filter, with superko off and
on; the planes of the same call against tg_replay_run's bytes; flags, untouched rows and launch sizes.  Every comparison is
exact."""
import ctypes
import functools

import numpy as np
import pytest

from tests import _eval_cases as ec
from tests import _rule_corpus as rc
from tests._replay_records import random_record

pytestmark = pytest.mark.gpu

UNTOUCHED = 0xDEADBEEF


def _arrays(games, plies, sym):
    offsets = np.zeros(len(games) + 1, dtype=np.int64)
    np.cumsum([len(g) for g in games], out=offsets[1:])
    s_off = np.zeros(len(games) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in plies], out=s_off[1:])
    moves = np.array([m for g in games for m in g], dtype=np.int32)
    ply = np.array([p for ps in plies for p in ps], dtype=np.int32)
    syms = np.array([sym(i) for i in range(len(ply))], dtype=np.int8)
    return offsets, s_off, moves, ply, syms


def _run(size, games, plies, superko, planes="cand", sym=lambda i: 0):
    """planes: "cand" = tg_replay_run_cand with planes, "none" = with planes_dev NULL, "plain" = tg_replay_run.
    -> (flags [games], masks uint32 [samples, W] (rows nothing wrote: UNTOUCHED), planes [samples, 6, S, S] or None)"""
    import torch
    from tamago_amd import lib as tl
    lib = tl.load()
    handle = ctypes.c_void_p()
    tl.check(lib.tg_replay_create(size, 0, ctypes.byref(handle)), "tg_replay_create")
    try:
        offsets, s_off, moves, ply, syms = _arrays(games, plies, sym)
        flags = np.full(len(games), -1, dtype=np.int32)
        n = len(ply)
        plane_t = torch.full((n, 6, size, size), 7.0, dtype=torch.float32, device="cuda:0") if planes != "none" else None
        masks = torch.from_numpy(np.full((n, ec.mask_words(size)), UNTOUCHED, dtype=np.uint32).view(np.int32)).to("cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        head = [handle, moves.ctypes.data, offsets.ctypes.data, len(games), ply.ctypes.data, syms.ctypes.data, s_off.ctypes.data,
                plane_t.data_ptr() if plane_t is not None else None, flags.ctypes.data]
        if planes == "plain":
            tl.check(lib.tg_replay_run(*head, stream), "tg_replay_run")
        else:
            tl.check(lib.tg_replay_run_cand(*head, int(superko), masks.data_ptr(), stream), "tg_replay_run_cand")
        torch.cuda.synchronize()
        return flags, masks.cpu().numpy().view(np.uint32), plane_t.cpu().numpy() if plane_t is not None else None
    finally:
        lib.tg_replay_destroy(handle)


# ---- 1. the rule corpus: the reference's lists, the host board's filter ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus_run(size, superko):
    """Every entry as a record with one PASS appended, the ply behind its last move sampled: one launch."""
    fx = rc.load_fixture(size)
    games = [list(e.moves) + [rc.PASS] for e in fx.entries]
    return _run(size, games, [[len(e.moves)] for e in fx.entries], superko)


@pytest.mark.parametrize("superko", [False, True], ids=["superko_off", "superko_on"])
@pytest.mark.parametrize("size", rc.SIZES)
def test_masks_equal_the_reference_lists(size, superko):
    fx = rc.load_fixture(size)
    flags, masks, _ = _corpus_run(size, superko)
    # a record longer than the board's move record (the late plies of the 9x9 fights, the history-limit entries beyond the
    # limit) is flagged and nothing of it is written - tg_replay_run's rule; every other entry is replayed
    too_long = np.array([len(e.moves) + 1 > rc.hmax(size) for e in fx.entries])
    assert flags.tolist() == too_long.astype(int).tolist() and too_long.any() and too_long.sum() < len(fx.entries) // 4
    P = size * size
    checked_superko_only = 0
    for i, entry in enumerate(fx.entries):
        if too_long[i]:
            assert (masks[i] == UNTOUCHED).all(), entry.name
            continue
        want = ec.words_of_list(size, fx.cand[int(superko)][i])
        assert np.array_equal(masks[i], want), (entry.name, superko)
        assert (int(masks[i][P >> 5]) >> (P & 31)) & 1 and int(masks[i][-1]) >> ((P & 31) + 1) == 0      # PASS set, tail bits zero
        checked_superko_only += fx.cand[0][i] != fx.cand[1][i]
    assert checked_superko_only >= 5                                           # the two settings differ on the corpus


@pytest.mark.parametrize("superko", [False, True], ids=["superko_off", "superko_on"])
@pytest.mark.parametrize("size", rc.SIZES)
def test_masks_equal_the_host_board(size, superko):
    """GoBoard.get_all_legal_pos, check_self_atari_stone < 7, not is_complete_eye, PASS (tamago_amd/board/candidates.py) - the
    filter a flagged game is redone with."""
    fx = rc.load_fixture(size)
    flags, masks, _ = _corpus_run(size, superko)
    for i, entry in enumerate(fx.entries):
        if flags[i] == 0:
            assert np.array_equal(masks[i], ec.words_of_list(size, ec.host_candidates(size, i, superko))), (entry.name, superko)


# ---- 2. whole records: every ply, planes in the same call ------------------------------------------------------------------
RECORDS = {9: (120, 6), 13: (90, 21), 19: (120, 44)}        # board size -> (moves, seed): seeds of tests/test_gpu_replay_datagen.py


@functools.lru_cache(maxsize=None)
def _record(size):
    n_moves, seed = RECORDS[size]
    return tuple(random_record(size, n_moves, seed))


@pytest.mark.parametrize("size", rc.SIZES)
def test_planes_equal_tg_replay_run_and_masks_need_no_planes(size):
    """Two records, every ply twice under two symmetries: the planes are tg_replay_run's bytes, the masks do not depend on the
    planes pointer or the symmetry, and on every ply they are the host board's."""
    games = [list(_record(size)), list(_record(size))[:37]]
    plies = [[p for p in range(len(g)) for _ in (0, 1)] for g in games]
    sym = lambda i: (3 * i + i // 2) % 8                                   # noqa: E731
    flags_a, _, planes_a = _run(size, games, plies, False, planes="plain", sym=sym)
    flags_b, masks_b, planes_b = _run(size, games, plies, False, planes="cand", sym=sym)
    flags_c, masks_c, _ = _run(size, games, plies, False, planes="none", sym=sym)
    assert flags_a.tolist() == flags_b.tolist() == flags_c.tolist() == [0, 0]
    assert planes_a.tobytes() == planes_b.tobytes()
    assert masks_b.tobytes() == masks_c.tobytes()
    want = np.concatenate([np.repeat(ec.record_masks(size, g, False), 2, axis=0) for g in games])
    assert np.array_equal(masks_b, want)
    _, masks_s, _ = _run(size, games, plies, True, planes="none", sym=sym)
    want_s = np.concatenate([np.repeat(ec.record_masks(size, g, True), 2, axis=0) for g in games])
    assert np.array_equal(masks_s, want_s)


# ---- 3. flags, untouched rows, launch sizes --------------------------------------------------------------------------------
def test_a_move_onto_an_occupied_point_flags_the_game():
    size = 9
    good = list(_record(size))[:30]
    bad = list(good)
    k = 20
    from tamago_amd.board.go_board import GoBoard
    board = GoBoard(size)
    for ply, pos in enumerate(good[:k]):
        board.put_stone(pos, 1 + ply % 2)
    bad[k] = next(p for p in board.onboard_pos if board.cells[p] != 0)        # a point that holds a stone at ply k
    games = [good, bad, good[:11]]
    plies = [list(range(len(g))) for g in games]
    flags, masks, planes = _run(size, games, plies, False)
    assert flags.tolist() == [0, 1, 0]
    off = np.cumsum([0] + [len(p) for p in plies])
    host = [ec.record_masks(size, g, False) for g in (good, good[:k + 1], good[:11])]
    assert np.array_equal(masks[off[0]:off[1]], host[0]) and np.array_equal(masks[off[2]:off[3]], host[2])
    # the rows up to and including the ply of the bad move are written (the position in front of it exists) ...
    assert np.array_equal(masks[off[1]:off[1] + k + 1], host[1])
    # ... the later rows are as they were: masks and planes
    assert (masks[off[1] + k + 1:off[2]] == UNTOUCHED).all()
    assert (planes[off[1] + k + 1:off[2]] == 7.0).all() and not (planes[off[1]:off[1] + k + 1] == 7.0).any()


@pytest.mark.parametrize("n_games", [1, 63, 64, 65])
def test_games_of_one_move_and_launch_sizes(n_games):
    """Games of 1 .. 24 moves (the first ones of one move: a stone, a pass), the last ply of each sampled."""
    size = 9
    base = list(_record(size))
    games = [[base[0]], [0]] + [base[:1 + g % 24] for g in range(2, 65)]
    games = games[:n_games]
    plies = [[len(g) - 1] for g in games]
    flags, masks, _ = _run(size, games, plies, True)
    assert flags.tolist() == [0] * n_games
    for g, game in enumerate(games):
        assert np.array_equal(masks[g], ec.record_masks(size, game, True)[-1]), g
    assert bin(int(masks[0][0])).count("1") + bin(int(masks[0][1])).count("1") + bin(int(masks[0][2])).count("1") == 82   # the empty board


def test_refusals():
    import torch
    from tamago_amd import lib as tl
    lib = tl.load()
    handle = ctypes.c_void_p()
    tl.check(lib.tg_replay_create(9, 0, ctypes.byref(handle)), "tg_replay_create")
    try:
        offsets, s_off, moves, ply, syms = _arrays([[12, 13]], [[0]], lambda i: 0)
        flags = np.zeros(1, dtype=np.int32)
        masks = torch.zeros((1, 3), dtype=torch.int32, device="cuda:0")
        args = [moves.ctypes.data, offsets.ctypes.data, 1, ply.ctypes.data, syms.ctypes.data, s_off.ctypes.data, None,
                flags.ctypes.data, 0, None, None]
        assert lib.tg_replay_run_cand(handle, *args) == -1 and b"tg_replay_run_cand: null" in lib.tg_last_error()    # no masks
        args[9] = masks.data_ptr()
        assert lib.tg_replay_run_cand(None, *args) == -1
        assert lib.tg_replay_run_cand(handle, *args) == 0                                                            # no planes: fine
        ply[0] = 2
        assert lib.tg_replay_run_cand(handle, *args) == -1 and b"beyond" in lib.tg_last_error()
    finally:
        lib.tg_replay_destroy(handle)
