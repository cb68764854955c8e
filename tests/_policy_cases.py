"""The recorded policy-player cases (tests/golden/policy_moves_s*.{json,npz}, tools/gen_golden_policy.py) for the host and
the device tests: each file is read once per process."""
import functools
import hashlib
import random

import numpy as np

from helpers import load_json, load_npz

CATEGORIES = "abcdefghij"


@functools.lru_cache(maxsize=None)
def load(size):
    """(label file, {array name: array}) of one board size."""
    data = load_npz(f"policy_moves_s{size}.npz")
    return load_json(f"policy_moves_s{size}.json"), {name: data[name] for name in data.files}


def replay(size, case):
    """(GoBoard after the case's moves, colour value to move)."""
    from tamago_amd.board.go_board import GoBoard
    board = GoBoard(size, 7.0, case["superko"])
    color = 1
    for pos in case["moves"]:
        board.put_stone(int(pos), color)
        color = 3 - color
    assert color == case["color"]
    return board, color


def prepared_rng(case):
    """A random.Random in the state the reference's global generator was in before the case's call."""
    rng = random.Random()
    rng.seed(case["seed"])
    for _ in range(case["n_bits"]):
        rng.getrandbits(32)
    assert rng.getstate()[1][624] == case["start_pos"]
    return rng


def digest(words):
    """(position, sha256 of the 624 key words) of random.getstate()[1], as the label files record a state."""
    words = np.asarray(words, dtype=np.uint32)
    return int(words[624]), hashlib.sha256(words[:624].tobytes()).hexdigest()
