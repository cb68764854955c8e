"""Every writer of a tree's root yields the same root (DESIGN.md 3 "Root positions"): the host's set_root, the record
replay on the device, tg_search_play move by move and a played policy move, each against the host GoBoard replayed to
the same ply - the whole state tg_search_read_root_state and read_positions return (hash, moves, ko point and move, the
last two moves, side to move, num_nodes, hist_len, the history words, the cells).

Every record is a tests/_replay_records.random_record whose seed was kept because events() reports a ko capture, a capture
of two or more stones and a pass followed by a move, and because every move is legal under positional superko as well
(the policy path only plays legal moves); both are checked again here, on the CPU."""
import random

import numpy as np
import pytest
import torch

from tests._replay_records import events, random_record
from tests._root_state import PolicyRoots, assert_root, host_states

pytestmark = pytest.mark.gpu

# (size, moves, seed, pass_rate): seeds found by a CPU search over events() and superko legality
RECORDS = {"9x9 a": (9, 30, 15638, 0.06), "9x9 b": (9, 20, 6879, 0.04), "13x13": (13, 40, 77310, 0.04), "19x19": (19, 93, 1640, 0.04)}
CASES = [("9x9 a", True), ("9x9 a", False), ("9x9 b", True), ("9x9 b", False), ("13x13", True), ("19x19", False)]
MAX_TREES = 8


def _record(spec):
    from tamago_amd.board.go_board import GoBoard
    size, n, seed, rate = spec
    moves = random_record(size, n, seed, rate)
    ev = events(size, moves)
    assert ev["ko_captures"] >= 1 and ev["big_captures"] >= 1 and ev["pass_then_move"] >= 1, (spec, ev)
    board = GoBoard(size, check_superko=True)
    for ply, pos in enumerate(moves):
        assert pos == 0 or board.is_legal(pos, 1 + ply % 2), (spec, ply)
        board.put_stone(pos, 1 + ply % 2)
    return moves


def _plies(moves, want):
    """Ply 0, the plies right after the first ko capture and one later (the ko point set, then stale), right after the
    first pass, the middle and the last one."""
    n = len(moves)
    ko = next(p for p in range(1, n + 1) if want[p]["ko_pos"] != 0 and want[p]["ko_move"] == want[p]["moves"] - 1)
    after_pass = next(p for p in range(1, n + 1) if moves[p - 1] == 0)
    plies = sorted({0, ko, min(ko + 1, n), after_pass, n // 2, n})
    assert len(plies) <= MAX_TREES
    return plies


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]} superko {'on' if c[1] else 'off'}")
def case(request):
    name, superko = request.param
    size = RECORDS[name][0]
    moves = _record(RECORDS[name])
    want = host_states(size, moves, None, superko)
    return size, moves, superko, want, _plies(moves, want)


def _engine(size, trees, superko):
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    return SearchEngine(size, trees, 24, 8, HostEvaluator(StubNet(3), torch.device("cuda:0")), False, superko)


def _check(engine, want, plies, what):
    positions = engine.read_positions()
    for tree, ply in enumerate(plies):
        assert_root(engine, tree, want[ply], positions, f"{what}, ply {ply}")


def test_set_root(case):
    """(a) the host board replayed to the ply, staged and flushed.

    The three superko-off cases failed on the library before the writers were unified (every other field, the cells and
    history[0] agreed): tg_search_set_root took hist_len from the PRESENCE of hash_history, which SearchEngine.set_root
    always passes, not from the handle's superko flag - the first tree behind ply 0 read back hist_len 8 (9x9 a, ply 7),
    11 (9x9 b, ply 10) and 47 (19x19, ply 46) where the three device writers give 1.  It now takes the handle's flag as
    they do; without superko no kernel uses the history (and flush_roots does not upload it), so no search changed."""
    from tamago_amd.mcts.record_roots import host_record_positions
    size, moves, superko, want, plies = case
    engine = _engine(size, len(plies), superko)
    try:
        for tree, (board, color) in enumerate(host_record_positions(moves, plies, size, superko)):
            engine.set_root(tree, board, color)
        _check(engine, want, plies, "set_root")
    finally:
        engine.close()


def test_roots_from_records(case):
    """(b) the record replayed on the device, one tree per ply."""
    size, moves, superko, want, plies = case
    engine = _engine(size, len(plies), superko)
    try:
        flags = engine.set_roots_from_records([moves], [(0, ply) for ply in plies])
        assert not flags.any()
        _check(engine, want, plies, "set_roots_from_records")
    finally:
        engine.close()


def test_play(case):
    """(c) the empty board, then tg_search_play of the first `ply` moves, one launch per move (a tree that has reached
    its ply skips the launch)."""
    from tamago_amd.board.go_board import GoBoard
    size, moves, superko, want, plies = case
    engine = _engine(size, len(plies), superko)
    try:
        for tree in range(len(plies)):
            engine.set_root(tree, GoBoard(size, check_superko=superko), 1)
        for at in range(max(plies)):
            engine.play([moves[at] if at < ply else -1 for ply in plies])
        _check(engine, want, plies, "tg_search_play")
    finally:
        engine.close()


def test_played_policy_moves(case):
    """(d) the empty board on a PolicyBoards handle, then one moves(policy, play=True) launch per move with a one-hot
    policy on the record's move: the only candidate above the tenth-of-the-maximum cut.  Both boards play the record;
    their roots are read at each chosen ply on the way."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.nn.policy_player import PolicyBoards
    size, moves, superko, want, plies = case
    w = size + 2
    boards = PolicyBoards(size, 2, superko)
    reader = PolicyRoots(boards)
    try:
        for t in range(2):
            boards.set_root(t, GoBoard(size, check_superko=superko), 1)
            boards.seed(t, random.Random(t).getstate())
        policy = np.zeros((2, size * size + 1), dtype=np.float32)
        for at in range(len(moves) + 1):
            if at in plies:
                positions = reader.read_positions()
                for t in range(2):
                    assert_root(reader, t, want[at], positions, f"played policy move, ply {at}")
            if at == len(moves):
                break
            pos = moves[at]
            policy[:] = 0.0
            policy[:, size * size if pos == 0 else (pos // w - 1) * size + pos % w - 1] = 1.0
            played = boards.moves(torch.from_numpy(policy).to(boards.device), play=True)
            assert played.tolist() == [pos, pos], at
    finally:
        boards.close()
