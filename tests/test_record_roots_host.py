"""The host half of SearchEngine.set_roots_from_records (tamago_amd/mcts/record_roots.py): the packing of records and
members into the arrays of tg_search_set_roots_from_records, and the host replay of a flagged record.  No GPU, no native
library."""
import sys

import numpy as np
import pytest

from tamago_amd.board.go_board import GoBoard
from tamago_amd.board.stone import Stone
from tamago_amd.mcts.record_roots import (alternating_colors, host_record_positions, pack_record_roots, to_move_at)


def test_the_module_does_not_load_the_native_library():
    import os
    import subprocess
    code = ("import sys; import tamago_amd.mcts.record_roots; "
            "sys.exit(1 if 'tamago_amd.lib' in sys.modules or 'torch' in sys.modules else 0)")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=repo).returncode == 0


def test_packing():
    records = [[12, 13, 0, 14], [20, 21], [], ([30, 31, 32], [2, 2, 1])]
    #          tree:    0       1       2     3       4       5      6        7
    members = [(0, 3), (0, 0), None, (0, 3), (3, 1), (0, 4), (3, 3), (0, 1)]
    p = pack_record_roots(records, members, 8)
    assert p.record_index == [0, 3] and p.games == 2                 # only the records that have a member, in their order
    assert p.offsets.dtype == np.int64 and p.offsets.tolist() == [0, 4, 7]
    assert p.moves.dtype == np.int32 and p.moves.tolist() == [12, 13, 0, 14, 30, 31, 32]
    # one record has colours: the other's alternating colours are spelled out
    assert p.colors.dtype == np.int8 and p.colors.tolist() == [1, 2, 1, 2, 2, 2, 1]
    assert p.root_game.dtype == p.root_ply.dtype == np.int32
    assert p.root_game.tolist() == [0, 0, -1, 0, 1, 0, 1, 0]
    assert [ply for g, ply in zip(p.root_game, p.root_ply) if g >= 0] == [3, 0, 3, 1, 4, 3, 1]
    # the trees of one record by non-decreasing ply; duplicates (trees 0 and 3) side by side; a final-position ply (4 of 4, 3 of 3)
    assert p.by_record == [[(0, 1), (1, 7), (3, 0), (3, 3), (4, 5)], [(1, 4), (3, 6)]]
    for rows in p.by_record:
        assert [ply for ply, _ in rows] == sorted(ply for ply, _ in rows)
    assert sorted(t for rows in p.by_record for _, t in rows) == [t for t, m in enumerate(members) if m is not None]


def test_packing_without_colours_and_without_members():
    p = pack_record_roots([np.array([5, 6], dtype=np.int32), [7]], [(1, 1), (0, 2)])
    assert p.colors is None and p.moves.tolist() == [5, 6, 7] and p.offsets.tolist() == [0, 2, 3]
    assert p.root_game.tolist() == [1, 0] and p.root_ply.tolist() == [1, 2]
    empty = pack_record_roots([[1, 2]], [None, None], 2)
    assert empty.games == 0 and empty.offsets.tolist() == [0] and empty.moves.size == 0 and empty.colors is None
    assert empty.root_game.tolist() == [-1, -1] and empty.by_record == []
    stones = pack_record_roots([([3, 4], [Stone.WHITE, Stone.BLACK])], [(0, 0)])
    assert stones.colors.tolist() == [2, 1]
    only_final = pack_record_roots([[]], [(0, 0)])                     # an empty record has its final position
    assert only_final.offsets.tolist() == [0, 0] and only_final.root_ply.tolist() == [0]


@pytest.mark.parametrize("records, members, trees, text", [
    ([[1, 2]], [(0, 0)], 2, "members for 2 trees"),
    ([[1, 2]], [(1, 0)], None, "names record 1 of 1"),
    ([[1, 2]], [(-1, 0)], None, "names record -1"),
    ([[1, 2]], [(0, 3)], None, r"ply 3 outside \[0, 2\]"),
    ([[1, 2]], [(0, -1)], None, "ply -1 outside"),
    ([([1, 2], [1])], [(0, 0)], None, "1 colours for 2 moves"),
    ([([1, 2], [1, 3])], [(0, 0)], None, "neither 1"),
    ([([1, 2], [0, 1])], [(0, 0)], None, "neither 1"),
    ([[1.5, 2.0]], [(0, 0)], None, "not integers"),
    ([[1, 2 ** 40]], [(0, 0)], None, "32 bits"),
    ([([1], [1], [1])], [(0, 0)], None, "pair"),
])
def test_bad_input_raises_before_any_native_call(records, members, trees, text):
    with pytest.raises(ValueError, match=text):
        pack_record_roots(records, members, trees)


def test_a_bad_record_without_members_is_not_looked_at():
    p = pack_record_roots([[1.5], [4]], [(1, 0)])
    assert p.record_index == [1]


def test_side_to_move():
    assert alternating_colors(5).tolist() == [1, 2, 1, 2, 1]
    assert [to_move_at(None, 3, k) for k in range(4)] == [1, 2, 1, 2]
    assert to_move_at(None, 0, 0) == 1 and to_move_at([], 0, 0) == 1
    colors = [2, 2, 1]
    assert [to_move_at(colors, 3, k) for k in range(4)] == [2, 2, 1, 2]
    # the final position: GoBoard.get_to_move
    for col in ([1, 2, 1], [2, 2], [1, 1, 2, 2]):
        board = GoBoard(9)
        for i, c in enumerate(col):
            board.put_stone(12 + i, c)
        assert to_move_at(col, len(col), len(col)) == board.get_to_move().value


def test_host_replay_of_one_record():
    from tests._replay_records import random_record
    moves = random_record(9, 30, 3)
    want = GoBoard(9, check_superko=True)
    boards = host_record_positions(moves, [0, 7, 7, 30], 9, True)
    assert [b.moves for b, _ in boards] == [1, 8, 8, 31] and [c for _, c in boards] == [Stone.BLACK, Stone.WHITE, Stone.WHITE, Stone.BLACK]
    for i, pos in enumerate(moves):
        want.put_stone(pos, 1 + i % 2)
    final = boards[3][0]
    assert final.check_superko and np.array_equal(final.cells, want.cells) and final.hash == want.hash
    assert np.array_equal(final.rec_hash, want.rec_hash) and (final.ko_pos, final.ko_move) == (want.ko_pos, want.ko_move)
    assert boards[1][0] is not boards[2][0]
    white_first = host_record_positions(([12, 13], [2, 2]), [2], 9, False)[0]
    assert white_first[0].cells[12] == 2 and white_first[0].cells[13] == 2 and white_first[1] == Stone.BLACK
    with pytest.raises(ValueError):
        host_record_positions(moves, [5, 4], 9, True)
