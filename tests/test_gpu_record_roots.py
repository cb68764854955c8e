"""Search roots written on the device from game records (tg_search_set_roots_from_records, tg_search_seed_streams,
tg_search_read_root_state; SearchEngine.set_roots_from_records / seed_trees / read_root_state) and the layers over them:
reanalyse_records, iter_reanalysed_chunks(device_roots=True), analyze_game(device_roots=True).

The expected root is always the host GoBoard read the way SearchEngine.set_root reads it, under the engine's Zobrist table
(GoBoard's own: zobrist_keys).  Every record is a tests/_replay_records.random_record whose seed was kept because events()
reports a ko capture, a capture of two or more stones and a pass followed by a move (checked again here, on the CPU)."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import _reanalyse_cases as rc
from tests._replay_records import events, random_record, sgf_text
from tests._root_state import assert_root as _assert_root, expected as _expected, host_states as _host_states

pytestmark = pytest.mark.gpu

# (size, moves, seed, pass_rate) of the records: seeds found by a CPU search over events()
REC9 = [(9, 80, 5, 0.04), (9, 80, 6, 0.04), (9, 80, 15, 0.04)]
REC13 = (13, 40, 77310, 0.04)
REC19 = (19, 120, 1640, 0.04)
REC9_SHORT = (9, 20, 6879, 0.04)


def _record(spec):
    size, n, seed, rate = spec
    moves = random_record(size, n, seed, rate)
    ev = events(size, moves)
    assert ev["ko_captures"] >= 1 and ev["big_captures"] >= 1 and ev["pass_then_move"] >= 1, (spec, ev)
    return moves


def _engine(size, trees, superko):
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    return SearchEngine(size, trees, 24, 8, HostEvaluator(StubNet(3), torch.device("cuda:0")), False, superko)


def _every_ply(size, moves, colors, superko, trees):
    """Each ply of the record, 0 and the final one included, is one tree; launches of `trees` trees."""
    want = _host_states(size, moves, colors, superko)
    record = moves if colors is None else (moves, colors)
    engine = _engine(size, trees, superko)
    try:
        for lo in range(0, len(want), trees):
            plies = list(range(lo, min(lo + trees, len(want))))
            flags = engine.set_roots_from_records([record], [(0, p) for p in plies] + [None] * (trees - len(plies)))
            assert flags.dtype == np.int32 and flags.shape == (trees,) and not flags.any()
            positions = engine.read_positions()
            for k, ply in enumerate(plies):
                _assert_root(engine, k, want[ply], positions, f"{size}x{size} ply {ply}")
    finally:
        engine.close()


@pytest.mark.parametrize("superko", [True, False])
def test_every_ply_9x9(superko):
    _every_ply(9, _record(REC9[0]), None, superko, 16)            # 81 positions: six launches, the last with one tree


def test_every_ply_13x13():
    _every_ply(13, _record(REC13), None, True, 16)


def test_every_ply_19x19():
    _every_ply(19, _record(REC19), None, True, 32)


def _playable(size, moves, colors):
    """The record under other colours than it was generated with: a move whose point is no longer empty then (the
    captures differ) becomes a pass, so that the replay has no move it would flag."""
    from tamago_amd.board.go_board import GoBoard
    board, out = GoBoard(size), []
    for pos, color in zip(moves, colors):
        pos = int(pos) if board.cells[pos] == 0 else 0
        board.put_stone(pos, color)
        out.append(pos)
    return out


def test_explicit_colours():
    """Two consecutive moves of one colour, and a record that starts with white, against host put_stone with those
    colours; the side to move is the tag's, and after the last move its opponent."""
    moves = _record(REC9[1])[:40]
    twice = [1 + i % 2 for i in range(40)]
    twice[7] = twice[6]
    white_first = [2 - i % 2 for i in range(40)]
    for colors in (twice, white_first):
        _every_ply(9, _playable(9, moves, colors), colors, True, 41)
    from tamago_amd.board.stone import Stone
    _every_ply(9, _playable(9, moves[:9], white_first[:9]), [Stone(c) for c in white_first[:9]], False, 10)


def _marker_boards(size, trees, superko):
    """One distinct one-stone position per tree, staged with set_root before a call: what a flagged tree must still hold."""
    from tamago_amd.board.go_board import GoBoard
    boards = []
    for t in range(trees):
        board = GoBoard(size, check_superko=superko)
        board.put_stone(board.onboard_pos[t % (size * size)], 1)
        boards.append(board)
    return boards


def _occupied_move(size, moves, at):
    """The record with move `at` replaced by a point that holds a stone of the mover's own colour at that time."""
    board = rc.played(size, moves[:at])[0]
    own = [p for p in board.onboard_pos if board.cells[p] == 1 + at % 2]
    assert own
    return moves[:at] + [own[len(own) // 2]] + moves[at + 1:]


def test_flags_for_a_move_onto_an_occupied_point():
    k = 23
    moves = _occupied_move(9, _record(REC9[2])[:40], k)
    trees = 41
    want = _host_states(9, moves, None, True, upto=k)
    markers = _marker_boards(9, trees, True)
    engine = _engine(9, trees, True)
    try:
        for t, board in enumerate(markers):
            engine.set_root(t, board, 2)
        flags = engine.set_roots_from_records([moves], [(0, p) for p in range(trees)])
        assert flags.tolist() == [0] * (k + 1) + [1] * (trees - k - 1)
        positions = engine.read_positions()
        for t in range(trees):
            _assert_root(engine, t, want[t] if t <= k else _expected(markers[t], 2, True), positions, f"ply {t}")
    finally:
        engine.close()


def test_flags_at_the_move_record_boundary():
    """max_records = 3 * S * S = 243 at 9x9.  A record of exactly 243 moves gives every position but its final one (the
    host board has no record of move 243: prev_move and get_to_move have nothing to read); one of 244 gives none."""
    from tamago_amd.board.constant import max_records
    hmax = max_records(9)
    assert hmax == 243
    exact, over = [0] * hmax, [0] * (hmax + 1)
    want = _host_states(9, exact, None, True, upto=hmax - 1)
    markers = _marker_boards(9, 8, True)
    engine = _engine(9, 8, True)
    try:
        for t, board in enumerate(markers):
            engine.set_root(t, board, 2)
        members = [(0, 0), (0, 100), (0, hmax - 1), (0, hmax), (1, 0), (1, 7), (1, hmax), (1, hmax + 1)]
        flags = engine.set_roots_from_records([exact, over], members)
        assert flags.tolist() == [0, 0, 0, 1, 1, 1, 1, 1]
        positions = engine.read_positions()
        for t, (rec, ply) in enumerate(members):
            _assert_root(engine, t, _expected(markers[t], 2, True) if flags[t] else want[ply], positions, f"tree {t}")
        assert engine.read_root_state(2)["hist_len"] == hmax and engine.read_root_state(2)["moves"] == hmax
    finally:
        engine.close()


def test_ordering():
    """set_root then the call on the same tree: the record's root wins; the call then set_root: the host's wins; a tree
    with game -1 keeps its root - a staged one, and one already on the device."""
    moves = _record(REC9[0])
    want = _host_states(9, moves, None, True)
    markers = _marker_boards(9, 4, True)
    engine = _engine(9, 4, True)
    try:
        for t in range(4):
            engine.set_root(t, markers[t], 2)
        flags = engine.set_roots_from_records([moves], [(0, 30), (0, 31), None, None])
        assert not flags.any()
        engine.set_root(1, markers[3], 1)
        positions = engine.read_positions()
        _assert_root(engine, 0, want[30], positions, "set_root, then the record")
        _assert_root(engine, 1, _expected(markers[3], 1, True), positions, "the record, then set_root")
        _assert_root(engine, 2, _expected(markers[2], 2, True), positions, "left alone (staged)")
        flags = engine.set_roots_from_records([moves], [None, (0, 80), None, (0, 12)])
        assert not flags.any()
        positions = engine.read_positions()
        _assert_root(engine, 0, want[30], positions, "left alone (on the device)")
        _assert_root(engine, 1, want[80], positions, "the record again")
        _assert_root(engine, 2, _expected(markers[2], 2, True), positions, "left alone")
        _assert_root(engine, 3, want[12], positions, "the record")
    finally:
        engine.close()


def test_argument_errors():
    from tamago_amd import lib as tl
    engine = _engine(9, 2, True)
    try:
        lib = engine.lib
        moves = np.array([12, 13, 14], dtype=np.int32)
        colors = np.array([1, 2, 1], dtype=np.int8)
        offsets = np.array([0, 3], dtype=np.int64)
        game = np.array([0, -1], dtype=np.int32)
        ply = np.array([3, 0], dtype=np.int32)
        flags = np.full(2, 7, dtype=np.int32)

        def call(moves=moves, colors=colors, offsets=offsets, games=1, game=game, ply=ply, flags=flags):
            ptr = lambda a: None if a is None else a.ctypes.data                     # noqa: E731
            return lib.tg_search_set_roots_from_records(engine.handle, ptr(moves), ptr(colors), ptr(offsets), games,
                                                        ptr(game), ptr(ply), ptr(flags), None)

        assert call() == 0 and flags.tolist() == [0, 0]
        assert call(colors=None) == 0
        for bad, text in ((dict(flags=None), b"null"), (dict(offsets=None), b"null"), (dict(moves=None), b"null"),
                          (dict(offsets=np.array([1, 3], dtype=np.int64)), b"start at 0"),
                          (dict(offsets=np.array([0, 3, 2], dtype=np.int64), games=2), b"decrease"),
                          (dict(game=np.array([1, -1], dtype=np.int32)), b"game 1 of 1"),
                          (dict(ply=np.array([4, 0], dtype=np.int32)), b"ply 4 outside"),
                          (dict(ply=np.array([-1, 0], dtype=np.int32)), b"ply -1 outside"),
                          (dict(colors=np.array([1, 3, 1], dtype=np.int8)), b"colour 3")):
            assert call(**bad) == -1 and text in lib.tg_last_error(), bad
        assert lib.tg_search_seed_streams(engine.handle, None) == -1
        assert lib.tg_search_read_root_state(engine.handle, 2, None, None, None, 0) == -1
        with pytest.raises(ValueError):
            engine.set_roots_from_records([[12]], [(0, 2), None])
        with pytest.raises(tl.TamagoHipError):
            tl.check(call(flags=None), "tg_search_set_roots_from_records")
    finally:
        engine.close()


def test_seed_trees():
    """tg_search_stream_state after tg_search_seed_streams is numpy's state for the seed - as seeded, and after a root
    evaluation and a noise draw have consumed from the device-resident streams (against set_stream's)."""
    from tamago_amd.board.go_board import GoBoard
    seeds = [0, 1, 12345, 2 ** 32 - 1]
    one_by_one, at_once = _engine(9, 4, True), _engine(9, 4, True)
    try:
        at_once.seed_trees(seeds)
        for t, seed in enumerate(seeds):
            want = np.random.RandomState(seed).get_state()
            got = at_once.streams[t].final_state()
            assert np.array_equal(got[1], want[1]) and got[2] == want[2] == 624, seed
        for engine in (one_by_one, at_once):
            for t in range(4):
                engine.set_root(t, GoBoard(9, check_superko=True), 1)
        for t, seed in enumerate(seeds):
            one_by_one.set_stream(t, np.random.RandomState(seed).get_state())
        noise = []
        for engine in (one_by_one, at_once):
            engine.root_eval(use_logit=True)
            noise.append(engine.set_gumbel_noise().copy())
        assert np.array_equal(noise[0].view(np.uint64), noise[1].view(np.uint64))
        for t in range(4):
            a, b = one_by_one.streams[t].final_state(), at_once.streams[t].final_state()
            assert np.array_equal(a[1], b[1]) and a[2] == b[2], t
        with pytest.raises(ValueError):
            at_once.seed_trees([0, 1, 2, 2 ** 32])
    finally:
        one_by_one.close()
        at_once.close()


# ---- reanalysis ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net9():
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), 9)
    net.load_state_dict(make_state_dict(9, 11, 1.4))
    return net


def _assert_same_reanalysis(got, want):
    assert got.range_fallbacks == 0 and want.range_fallbacks == 0
    assert got.rows.shape == want.rows.shape and torch.equal(got.rows.view(torch.int32), want.rows.view(torch.int32))
    assert got.moves == want.moves and got.visits == want.visits
    assert np.array_equal(np.array(got.values).view(np.uint64), np.array(want.values).view(np.uint64))
    assert np.array_equal(np.array(got.raw_values).view(np.uint64), np.array(want.raw_values).view(np.uint64))
    assert got.forward_positions == want.forward_positions


@pytest.fixture(scope="module")
def reanalysis_case(net9):
    """Three records, 40 sampled positions (a record spans chunks of max_trees=16; the last chunk is short), and the host
    path's result: the boards replayed on the host, reanalyse_positions."""
    from tamago_amd.mcts.reanalyse import reanalyse_positions
    records = [_record(spec) for spec in REC9]
    members = [(0, p) for p in range(0, 81, 6)] + [(1, p) for p in range(2, 80, 6)] + [(2, p) for p in range(4, 81, 6)]
    assert len(members) == 40 and (0, 0) in members
    members[-1] = (2, 80)                                           # a final position
    seeds = [500 + 3 * k for k in range(40)]
    boards = [rc.played(9, records[r][:ply]) for r, ply in members]
    return records, members, seeds, boards, reanalyse_positions(net9, boards, 16, seeds=seeds, max_trees=16)


@pytest.mark.parametrize("unique", [False, True])
def test_reanalyse_records(net9, reanalysis_case, unique):
    from tamago_amd.mcts.reanalyse import reanalyse_positions, reanalyse_records
    records, members, seeds, boards, want = reanalysis_case
    if unique:
        want = reanalyse_positions(net9, boards, 16, seeds=seeds, max_trees=16, unique_leaves=True)
    got = reanalyse_records(net9, records, members, 16, seeds=seeds, max_trees=16, unique_leaves=unique)
    _assert_same_reanalysis(got, want)
    assert got.host_roots == 0 and got.visits == [16] * 40


def test_reanalyse_records_with_a_flagged_record(net9, reanalysis_case):
    """A fourth record with a move onto an occupied point at ply 20: its positions beyond are staged from one host replay
    of that record, and every row is still the host path's."""
    from tamago_amd.mcts.reanalyse import reanalyse_positions, reanalyse_records
    records, members, seeds, boards, _ = reanalysis_case
    bad = _occupied_move(9, records[1][:40], 20)
    records = records + [bad]
    members = members[:10] + [(3, 5), (3, 20), (3, 21), (3, 33), (3, 40)] + members[30:37]
    seeds = seeds[:len(members)]
    boards = [rc.played(9, records[r][:ply]) for r, ply in members]
    want = reanalyse_positions(net9, boards, 16, seeds=seeds, max_trees=16)
    got = reanalyse_records(net9, records, members, 16, seeds=seeds, max_trees=16)
    _assert_same_reanalysis(got, want)
    assert got.host_roots == 3
    with pytest.raises(ValueError):
        reanalyse_records(net9, records, [(4, 0)], 16)


def test_reanalysed_chunks_with_device_roots(net9, tmp_path, monkeypatch):
    """iter_reanalysed_chunks(device_roots=True) against the default from one saved global random state: the same chunks,
    the generators left in the same state; REANALYSE_STATS counts the positions set up each way."""
    import tamago_amd.nn.data_generator as dg
    monkeypatch.setattr(dg, "BATCH_SIZE", 8)
    monkeypatch.setattr(dg, "DATA_SET_SIZE", 16)
    kifu = str(tmp_path / "kifu")
    os.makedirs(kifu)
    for k, spec in enumerate(REC9):
        with open(os.path.join(kifu, f"{k + 1}.sgf"), "w") as f:
            f.write(sgf_text(9, _record(spec), result=("B+1.5", "W+R", "B+R")[k], seed=k))
    np.random.seed(17)
    random.seed(17)
    np_state, py_state = np.random.get_state(), random.getstate()
    runs, after, counted = [], [], []
    for device_roots in (False, True):
        np.random.set_state(np_state)
        random.setstate(py_state)
        before = dict(dg.REANALYSE_STATS)
        runs.append(list(dg.iter_reanalysed_chunks(net9, [kifu], 9, 8, device=0, seed=100, max_trees=5,
                                                   device_roots=device_roots)))
        after.append((np.random.get_state(), random.getstate()))
        counted.append({k: dg.REANALYSE_STATS[k] - before[k] for k in before})
    assert after[0][1] == after[1][1] and np.array_equal(after[0][0][1], after[1][0][1]) and after[0][0][2:] == after[1][0][2:]
    assert [int(c[0].shape[0]) for c in runs[0]] == [int(c[0].shape[0]) for c in runs[1]] == [16, 8]
    for host, dev in zip(*runs):
        for a, b in zip(host, dev):
            assert a.dtype == b.dtype and torch.equal(a, b)
    assert (counted[0]["positions"], counted[0]["host_roots"], counted[0]["device_roots"]) == (24, 24, 0)
    assert (counted[1]["positions"], counted[1]["host_roots"], counted[1]["device_roots"]) == (24, 0, 24)
    assert counted[0]["range_fallbacks"] == counted[1]["range_fallbacks"] == 0
    assert counted[0]["forward_positions"] == counted[1]["forward_positions"]


# ---- analysis ------------------------------------------------------------------------------------------------------------
def _tagged_sgf(size, moves, colors):
    w = size + 2
    letters = "abcdefghijklmnopqrs"
    body = "".join(f";{'BW'[c - 1]}[{'' if p == 0 else letters[p % w - 1] + letters[p // w - 1]}]" for p, c in zip(moves, colors))
    return f"(;FF[4]GM[1]SZ[{size}]PB[b]PW[w]KM[7.0]{body})\n"


@pytest.mark.parametrize("variant", ["alternating", "same colour twice"])
def test_analyze_game_with_device_roots(tmp_path, variant):
    """A 20-move 9x9 record at 32 visits: JSONL records, lz lines and the annotated SGF are the default path's."""
    from oracle.stubnet import StubNet
    from tamago_amd import analyze
    from tamago_amd.mcts.analysis import analyze_game, annotated_sgf
    from tamago_amd.sgf.reader import SGFReader
    moves = _record(REC9_SHORT)
    colors = [1 + i % 2 for i in range(20)]
    if variant != "alternating":
        colors[3] = colors[2]
        moves = _playable(9, moves, colors)
    path = str(tmp_path / "game.sgf")
    with open(path, "w") as f:
        f.write(_tagged_sgf(9, moves, colors))
    superko = variant == "alternating"
    kw = dict(seed=4, superko=superko, batch_size=8, max_trees=6)
    host = analyze_game(StubNet(2), path, 32, **kw)
    dev = analyze_game(StubNet(2), path, 32, device_roots=True, **kw)
    assert len(host) == len(dev) == 21
    assert [json.dumps(g.record()) for g in dev] == [json.dumps(g.record()) for g in host]
    assert [g.analysis.lz() for g in dev] == [g.analysis.lz() for g in host]
    assert [g.analysis.cgos() for g in dev if g.analysis.visits] == [g.analysis.cgos() for g in host if g.analysis.visits]
    sgf = SGFReader(path, 9)
    assert annotated_sgf(dev, sgf) == annotated_sgf(host, sgf)
    assert [g.position.color for g in dev] == [g.position.color for g in host]
    if variant == "alternating":                                      # the command line: the same lines either way
        lines = []
        for extra in ([], ["--device-roots"]):
            out = tmp_path / f"a{len(extra)}.jsonl"
            args = [path, "--visits", "32", "--batch-size", "8", "--trees", "6", "--seed", "4", "--superko", "true"] + extra
            with open(out, "w") as f:
                analyze.run(analyze.parser().parse_args(args), out=f, network_for=lambda size: StubNet(2))
            lines.append(open(out).read())
        assert lines[0] == lines[1] and lines[0].splitlines() == [json.dumps(g.record()) for g in host]
