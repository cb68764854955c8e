"""The root position's rules on the CPU: csrc/root_position.h, compiled alone into tests/root_position_driver.cpp with the
host compiler, against the Python boards and mcts/record_roots.py (DESIGN.md 3 "Root positions")."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (9, 13, 19)
EMPTY, BLACK, WHITE, OOB, PASS = 0, 1, 2, 3, 0
RECORDS = {"empty": (0, None), "alternating": (5, None), "tagged": (6, [1, 2, 2, 1, 2, 2]), "white_first": (3, [2, 1, 2])}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("root_position") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(HERE, "root_position_driver.cpp"), "-o", exe])
    return [line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]


def rows(listing, kind, size=None):
    return [r[1:] if size is None else r[2:] for r in listing if r[0] == kind and (size is None or int(r[1]) == size)]


def test_geometry_and_codes(listing):
    (codes,) = rows(listing, "codes")
    assert [int(x) for x in codes] == [EMPTY, BLACK, WHITE, OOB, PASS]
    for s in SIZES:
        (geo,) = rows(listing, "geo", s)
        assert [int(x) for x in geo] == [s + 2, (s + 2) ** 2, s * s, s * s + 1, 3 * s * s]


def test_root_meta_layout_and_fill(listing):
    (meta,) = rows(listing, "meta")
    # an 8-byte hash, then eight int32: moves, ko_pos, ko_move, prev, prevprev, to_move, num_nodes, hist_len; 40 bytes
    assert [int(x) for x in meta] == [40, 0, 8, 12, 16, 20, 24, 28, 32, 36]
    for s in SIZES:
        (fill,) = rows(listing, "fill", s)
        # the driver's scalars {hash, moves 7, ko_pos 30, ko_move 5, prev 41, prevprev 0}, white to move, 3 words: no tree yet
        assert [int(x) for x in fill] == [0x0123456789abcdef + s, 7, 30, 5, 41, 0, WHITE, 0, 3]


def test_empty_board_is_the_boards(listing):
    from oracle.board import GoBoard as OracleBoard
    from tamago_amd.board.go_board import GoBoard
    for s in SIZES:
        (cells,) = rows(listing, "cells", s)
        cells = [int(x) for x in cells]
        assert cells == [int(c) for c in OracleBoard(s).board]
        assert cells == [int(c) for c in GoBoard(s).cells]
        assert cells.count(EMPTY) == s * s and cells.count(OOB) == 4 * s + 4


def test_history_length(listing):
    from tamago_amd.board.go_board import GoBoard
    for s in SIZES:
        hmax = GoBoard(s).max_records
        got = {(int(m), int(k)): int(v) for m, k, v in rows(listing, "hist_len", s)}
        assert sorted(got) == sorted((m, k) for k in (0, 1) for m in (1, 2, hmax - 1, hmax, hmax + 1))
        for (moves, keeps), value in got.items():
            assert value == (min(moves, hmax) if keeps else 1), (s, moves, keeps)
        assert {int(n): int(v) for n, v in rows(listing, "too_long", s)} == {0: 0, hmax - 1: 0, hmax: 0, hmax + 1: 1}


def test_move_check(listing):
    for s in SIZES:
        w, nc = s + 2, (s + 2) ** 2
        got = {name: (int(mv), int(v)) for name, mv, v in rows(listing, "playable", s)}
        # the driver's board: empty but for a white stone at (1, 2); (2, 1) is empty, 4 * W lies on the left border
        assert got == {"pass": (PASS, 1), "negative": (-1, 0), "beyond": (nc, 0), "last_cell": (nc - 1, 0),
                       "empty": (2 * w + 3, 1), "occupied": (3 * w + 2, 0), "border": (4 * w, 0)}


def test_side_to_move_is_to_move_at(listing):
    from tamago_amd.mcts.record_roots import to_move_at
    for s in SIZES:
        got = {r[0]: [int(x) for x in r[1:]] for r in rows(listing, "to_move", s)}
        assert sorted(got) == sorted(RECORDS)
        for name, (length, colors) in RECORDS.items():
            assert got[name] == [to_move_at(colors, length, ply) for ply in range(length + 1)], (s, name)
    # ply 0, an inner ply behind two moves of one colour, the final position; the empty record: black
    assert got["tagged"][0] == BLACK and got["tagged"][2] == WHITE and got["tagged"][6] == BLACK
    assert got["white_first"] == [WHITE, BLACK, WHITE, BLACK] and got["alternating"][5] == WHITE and got["empty"] == [BLACK]
