"""The candidate filter of MCTSTree.expand_node (mcts/tree.py:260-264) on the host board: legal (go_board.py:260-304), no
self-atari of seven or more stones (check_self_atari_stone, :327-365), no complete eye of the mover (:367-397), PASS last.
The search runs this filter on the device (gen_candidates, csrc/search.hip); this is the host statement the evaluation of game
records falls back to for a game the device replay flags (tamago_amd/nn/evaluate.py)."""
from typing import List

from tamago_amd.board.go_board import GoBoard
from tamago_amd.board.stone import color_value

EMPTY, BLACK, WHITE, OOB = 0, 1, 2, 3
PASS = 0


def check_self_atari_stone(board: GoBoard, pos: int, color: int) -> int:
    """go_board.py:327-365: the size of the string the stone would make if it ends with fewer than three liberties and takes
    nothing, else 0."""
    cells = board.cells
    libs = set(n for n in board.get_neighbor4(pos) if cells[n] == EMPTY)
    if len(libs) > 1:
        return 0
    other = 3 - color
    seen: List[set] = []
    size = 0
    for n in board.get_neighbor4(pos):
        c = cells[n]
        if c == color:
            if any(n in stones for stones in seen):
                continue
            stones, string_libs = board._string(n)
            libs |= string_libs
            if len(libs) >= 3:
                return 0
            size += len(stones)
            seen.append(stones)
        elif c == other and len(board._string(n)[1]) == 1:
            return 0
    return size + 1


def is_eye_of(board: GoBoard, pos: int, color: int) -> bool:
    """pattern.py:52-98,153-162 as the rule the reference's table equals on real boards (csrc/search.hip is_eye_of): every
    orthogonal neighbour own or border; of four on-board diagonals at most one the opponent's, or two with two own; of two
    (side) one own or both the opponent's; one (corner): always."""
    cells, w = board.cells, board.board_size_with_ob
    if any(cells[n] != color and cells[n] != OOB for n in board.get_neighbor4(pos)):
        return False
    diag = [int(cells[pos + d]) for d in (-w - 1, -w + 1, w - 1, w + 1)]
    n_free = sum(1 for v in diag if v != OOB)
    n_own, n_opp = diag.count(color), diag.count(3 - color)
    if n_free == 4:
        return n_opp <= 1 or (n_opp == 2 and n_own == 2)
    if n_free == 2:
        return n_own >= 1 or n_opp == 2
    return True


def is_complete_eye(board: GoBoard, pos: int, color: int) -> bool:
    """go_board.py:367-397."""
    if not is_eye_of(board, pos, color):
        return False
    cells, w = board.cells, board.board_size_with_ob
    count, edge = 0, False
    for c in (pos - w - 1, pos - w + 1, pos + w - 1, pos + w + 1):
        v = cells[c]
        if v == color or v == OOB:
            count += 1
        elif v == EMPTY and is_eye_of(board, c, color):
            count += 1
        if v == OOB:
            edge = True
    return (edge and count == 4) or (not edge and count >= 3)


def search_candidates(board: GoBoard, color) -> List[int]:
    """Padded coordinates in row-major order, PASS (0) last; superko as the board's check_superko says."""
    color = color_value(color)
    out = [p for p in board.get_all_legal_pos(color)
           if check_self_atari_stone(board, p, color) < 7 and not is_complete_eye(board, p, color)]
    out.append(PASS)
    return out
