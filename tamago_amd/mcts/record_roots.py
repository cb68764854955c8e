"""Search roots from game records: the host half of tg_search_set_roots_from_records (include/tamago_hip.h).

A record is a list of moves (padded coordinates, PASS 0: colours alternate from black) or a pair (moves, colours) with one
colour (1 black / 2 white, or a Stone) per move.  A member is (record index, ply): the position BEFORE move `ply`
(0-based), ply == the record's length being the final position; None leaves its tree alone.

Nothing here touches the native library: pack_record_roots is the pure function SearchEngine.set_roots_from_records hands
to the C call, host_record_positions the host-board replay of ONE record for the trees a launch flags."""
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tamago_amd.board.go_board import GoBoard
from tamago_amd.board.stone import Stone, color_value

BLACK, WHITE = 1, 2


@dataclass
class PackedRecordRoots:
    """The arrays of one tg_search_set_roots_from_records call.  Only the records that have a member are packed:
    record_index[g] is the index in the caller's `records` of packed record g.  colors is None when no packed record has
    colours (a record without colours beside one with them gets its alternating colours spelled out).  by_record[g] lists
    the (ply, tree) pairs of packed record g by non-decreasing ply (trees ascending within a ply) - the order the kernel
    meets them in."""
    moves: np.ndarray                  # int32, the packed records' moves concatenated
    colors: Optional[np.ndarray]       # int8, same length, or None
    offsets: np.ndarray                # int64 [games + 1]
    root_game: np.ndarray              # int32 [T]: packed record of tree t, -1 = leave the tree alone
    root_ply: np.ndarray               # int32 [T]
    record_index: List[int]
    by_record: List[List[Tuple[int, int]]]

    @property
    def games(self) -> int:
        return len(self.record_index)


def split_record(record):
    """(moves, colours or None) of a record."""
    if isinstance(record, tuple):
        if len(record) != 2:
            raise ValueError("a record with colours is a pair (moves, colours)")
        return record[0], record[1]
    return record, None


def _checked_moves(moves, what: str) -> np.ndarray:
    arr = np.asarray(moves)
    if arr.ndim != 1 and arr.size:
        raise ValueError(f"{what}: moves are not a flat list")
    arr = arr.reshape(-1)
    if arr.size and not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"{what}: moves are not integers")
    if arr.size and (arr.min() < np.iinfo(np.int32).min or arr.max() > np.iinfo(np.int32).max):
        raise ValueError(f"{what}: a move does not fit 32 bits")
    return arr.astype(np.int32)


def _checked_colors(colors, length: int, what: str) -> np.ndarray:
    values = [color_value(c) for c in colors]
    if len(values) != length:
        raise ValueError(f"{what}: {len(values)} colours for {length} moves")
    if any(v not in (BLACK, WHITE) for v in values):
        raise ValueError(f"{what}: a colour is neither 1 (black) nor 2 (white)")
    return np.asarray(values, dtype=np.int8).reshape(-1)


def alternating_colors(length: int) -> np.ndarray:
    return np.where(np.arange(length) % 2 == 0, BLACK, WHITE).astype(np.int8)


def to_move_at(colors, length: int, ply: int) -> int:
    """The side to move before move `ply`: that move's colour where colours are given, else alternating from black; for
    the final position GoBoard.get_to_move() - the opponent of the last move's colour, black for an empty record.
    (The device's statement of this rule is record_to_move in csrc/root_position.h.)"""
    if ply < length:
        return color_value(colors[ply]) if colors is not None else (BLACK if ply % 2 == 0 else WHITE)
    if length == 0:
        return BLACK
    last = color_value(colors[length - 1]) if colors is not None else (BLACK if (length - 1) % 2 == 0 else WHITE)
    return 3 - last


def pack_record_roots(records: Sequence, members: Sequence[Optional[Tuple[int, int]]],
                      num_trees: Optional[int] = None) -> PackedRecordRoots:
    """members[t] = (record index, ply) or None for tree t -> the call's arrays.  Raises ValueError for: a member count
    other than num_trees (if given), a record index outside `records`, a ply outside [0, length], moves that are no
    32-bit integers, colours that are not one per move or neither 1 nor 2."""
    members = list(members)
    if num_trees is not None and len(members) != num_trees:
        raise ValueError(f"{len(members)} members for {num_trees} trees")
    used = sorted({int(m[0]) for m in members if m is not None})
    if used and (used[0] < 0 or used[-1] >= len(records)):
        raise ValueError(f"a member names record {used[0] if used[0] < 0 else used[-1]} of {len(records)}")
    packed_of = {rec: g for g, rec in enumerate(used)}
    moves, colors = [], []
    for rec in used:
        mv, col = split_record(records[rec])
        mv = _checked_moves(mv, f"record {rec}")
        moves.append(mv)
        colors.append(None if col is None else _checked_colors(col, len(mv), f"record {rec}"))
    lengths = [len(mv) for mv in moves]
    root_game = np.full(len(members), -1, dtype=np.int32)
    root_ply = np.zeros(len(members), dtype=np.int32)
    by_record: List[List[Tuple[int, int]]] = [[] for _ in used]
    for t, m in enumerate(members):
        if m is None:
            continue
        rec, ply = int(m[0]), int(m[1])
        g = packed_of[rec]
        if ply < 0 or ply > lengths[g]:
            raise ValueError(f"tree {t}: ply {ply} outside [0, {lengths[g]}] of record {rec}")
        root_game[t], root_ply[t] = g, ply
        by_record[g].append((ply, t))
    for rows in by_record:
        rows.sort()
    offsets = np.zeros(len(used) + 1, dtype=np.int64)
    if used:
        offsets[1:] = np.cumsum(lengths)
    all_moves = np.concatenate(moves).astype(np.int32) if used else np.zeros(0, np.int32)
    all_colors = None
    if any(c is not None for c in colors):
        all_colors = np.concatenate([alternating_colors(n) if c is None else c for c, n in zip(colors, lengths)]).astype(np.int8)
    return PackedRecordRoots(np.ascontiguousarray(all_moves), None if all_colors is None else np.ascontiguousarray(all_colors),
                             offsets, root_game, root_ply, used, by_record)


def host_record_positions(record, plies: Sequence[int], board_size: int, check_superko: bool):
    """[(board, colour to move)] before each of `plies` (non-decreasing) of ONE record, replayed on a host GoBoard the way
    analysis.game_positions and data_generator._sampled_positions replay it: what a flagged tree is staged from."""
    import copy
    moves, colors = split_record(record)
    length = len(moves)
    board = GoBoard(board_size=board_size, check_superko=check_superko)
    out, played = [], 0
    for ply in plies:
        if ply < played or ply > length:
            raise ValueError(f"ply {ply} out of order or outside [0, {length}]")
        while played < ply:
            board.put_stone(int(moves[played]), to_move_at(colors, length, played))
            played += 1
        out.append((copy.deepcopy(board), Stone(to_move_at(colors, length, ply))))
    return out
