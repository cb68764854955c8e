"""Game records for the device_replay tests: seeded random legal play on the Python board, written as SGF text with
improved-policy comments in the self-play record's format, and the events a record has to contain to be a test."""
import numpy as np

from tamago_amd.board.constant import PASS
from tamago_amd.board.go_board import BLACK, EMPTY, WHITE, GoBoard

_LETTERS = "abcdefghijklmnopqrs"


def random_record(size: int, n_moves: int, seed: int, pass_rate: float = 0.04):
    """n_moves legal moves from the empty board, colours alternating from black; about pass_rate of them are passes.
    Half of the board moves are drawn next to one of the last four stones, the others anywhere: fights (captures of whole
    strings, ko) are what the replay has to get right, and uniform play on a large board rarely has any."""
    rs = np.random.RandomState(seed)
    board = GoBoard(size)
    w = size + 2
    moves, recent, color = [], [], BLACK
    for _ in range(n_moves):
        pos = PASS
        if rs.random_sample() >= pass_rate:
            for _ in range(64):
                if recent and rs.random_sample() < 0.5:
                    base = recent[rs.randint(len(recent))]
                    cand = base + (rs.randint(3) - 1) * w + rs.randint(3) - 1
                else:
                    cand = board.onboard_pos[rs.randint(size * size)]
                if board.cells[cand] == EMPTY and board.is_legal(cand, color):
                    pos = cand
                    break
            else:                                        # a crowded board: take any legal point there is
                legal = board.get_all_legal_pos(color)
                if legal:
                    pos = legal[rs.randint(len(legal))]
        board.put_stone(pos, color)
        moves.append(int(pos))
        if pos != PASS:
            recent = (recent + [int(pos)])[-4:]
        color = 3 - color
    return moves


def events(size: int, moves):
    """What happens when the record is replayed: {"big_captures": moves that take a string of two or more stones off,
    "ko_captures": moves that set the ko point, "pass_then_move": passes followed by a board move, "passes": plies (>= 1)
    whose move is a pass}."""
    board = GoBoard(size)
    out = {"big_captures": 0, "ko_captures": 0, "pass_then_move": 0, "passes": []}
    color = BLACK
    for ply, pos in enumerate(moves):
        before = {c: int((board.cells == c).sum()) for c in (BLACK, WHITE)}
        at = board.moves
        board.put_stone(pos, color)
        if pos == PASS:
            if ply >= 1:
                out["passes"].append(ply)
            if ply + 1 < len(moves) and moves[ply + 1] != PASS:
                out["pass_then_move"] += 1
        else:
            other = 3 - color
            # a stone neighbouring two strings can take both: count stones, then ask the board whether one string had two
            taken = before[other] - int((board.cells == other).sum())
            if taken >= 2:
                out["big_captures"] += 1
            if board.ko_move == at and board.ko_pos != 0 and taken == 1:
                out["ko_captures"] += 1
        color = 3 - color
    return out


def policy_comment(size: int, rs, board_coordinate, onboard_pos) -> str:
    """An improved-policy comment as the self-play records carry it: "<n> <gtp>:<p> ...", sometimes with PASS."""
    k = int(rs.randint(1, 6))
    names = [board_coordinate.convert_to_gtp_format(onboard_pos[i]) for i in rs.choice(size * size, size=k, replace=False)]
    if rs.random_sample() < 0.3:
        names.append("PASS")
    probs = rs.dirichlet(np.ones(len(names)))
    return " ".join([str(len(names))] + [f"{n}:{p:.3e}" for n, p in zip(names, probs)])


def sgf_text(size: int, moves, result: str = "B+1.5", seed=None) -> str:
    """The record as SGF text (colour tags alternating from black); seed: a comment on every move."""
    board = GoBoard(size)
    rs = np.random.RandomState(seed) if seed is not None else None
    w = size + 2
    out = [f"(;FF[4]GM[1]SZ[{size}]\nAP[test]PB[b]PW[w]RE[{result}]KM[7.0]"]
    for ply, pos in enumerate(moves):
        point = "" if pos == PASS else _LETTERS[pos % w - 1] + _LETTERS[pos // w - 1]
        text = f";{'BW'[ply % 2]}[{point}]"
        if rs is not None:
            text += f"C[{policy_comment(size, rs, board.coordinate, board.onboard_pos)}]"
        out.append(text)
    out.append(")\n")
    return "".join(out)
