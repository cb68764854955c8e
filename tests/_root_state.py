"""The whole root position of a search tree as the host GoBoard states it, and the assertion that a device-resident root
equals it: shared by the tests of the root's writers (test_gpu_record_roots.py, test_gpu_root_writers.py)."""
import numpy as np


def expected(board, to_move, superko):
    """The root SearchEngine.set_root hands over for this board (engine.py set_root), hist_len by the device's rule."""
    hl = min(board.moves, board.max_records) if superko else 1
    return {"cells": np.array(board.cells, dtype=np.uint8), "hash": int(board.hash), "moves": int(board.moves),
            "ko_pos": int(board.ko_pos), "ko_move": int(board.ko_move), "prev": int(board.prev_move(1)),
            "prevprev": int(board.prev_move(2)), "to_move": int(to_move), "num_nodes": 0, "hist_len": hl,
            "history": np.array(board.rec_hash[:hl], dtype=np.uint64)}


def host_states(size, moves, colors, superko, upto=None):
    """expected() before every ply 0 .. upto (default: the final position included) of the record."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.record_roots import to_move_at
    board = GoBoard(size, check_superko=superko)
    n = len(moves)
    out = []
    for ply in range((n if upto is None else upto) + 1):
        out.append(expected(board, to_move_at(colors, n, ply), superko))
        if ply < n:
            board.put_stone(int(moves[ply]), to_move_at(colors, n, ply))
    return out


def assert_root(engine, tree, want, positions, what):
    """`engine`: anything with SearchEngine's read_root_state; positions: its read_positions()."""
    cells, moves, to_move = positions
    got = engine.read_root_state(tree)
    for name in ("hash", "moves", "ko_pos", "ko_move", "prev", "prevprev", "to_move", "num_nodes", "hist_len"):
        assert got[name] == want[name], (what, tree, name, got[name], want[name])
    assert np.array_equal(got["history"], want["history"]), (what, tree, "history")
    assert np.array_equal(cells[tree], want["cells"]), (what, tree, "cells")
    assert (int(moves[tree]), int(to_move[tree])) == (want["moves"], want["to_move"]), (what, tree)


class PolicyRoots:
    """read_root_state / read_positions of the search handle under a PolicyBoards."""

    def __init__(self, boards):
        self.lib, self.handle, self.P = boards.lib, boards.search, boards.S * boards.S
        self.read_positions = boards.read_positions

    def read_root_state(self, tree):
        from tamago_amd.mcts.engine import SearchEngine
        return SearchEngine.read_root_state(self, tree)
