"""Shared by the evaluation tests (tests/test_evaluate_host.py, tests/test_gpu_replay_cand.py, tests/test_gpu_evaluate.py): the
host boards of the rule corpus, candidate lists as bit images, the golden game records per board size, and the host pipeline
evaluate_records is held to."""
import functools

import numpy as np

from tests import _row_score_cases as rs
from tests import _rule_corpus as rc
from tests.helpers import load_json


def mask_words(size):
    return (size * size + 1 + 31) // 32


def words_of_list(size, cand):
    """A candidate list (padded coordinates, PASS = 0) -> uint32 [ceil(A / 32)]."""
    w, P = size + 2, size * size
    bits = np.zeros(P + 1, dtype=bool)
    for pos in cand:
        bits[P if pos == 0 else (pos // w - 1) * size + pos % w - 1] = True
    return rs.pack_mask(bits)


@functools.lru_cache(maxsize=None)
def host_boards(size):
    """The package's host board behind every entry of the rule corpus (check_superko on; is_legal reads the switch per call)."""
    from tamago_amd.board.go_board import GoBoard
    boards = []
    for entry in rc.load_fixture(size).entries:
        board = GoBoard(size, 7.0, True)
        color = 1
        for pos in entry.moves:
            board.put_stone(int(pos), color)
            color = 3 - color
        assert color == entry.to_move
        boards.append(board)
    return boards


def host_candidates(size, index, superko):
    from tamago_amd.board.candidates import search_candidates
    board = host_boards(size)[index]
    board.check_superko = bool(superko)
    try:
        return search_candidates(board, rc.load_fixture(size).entries[index].to_move)
    finally:
        board.check_superko = True


def record_masks(size, moves, superko):
    """uint32 [len(moves), W]: the host candidate mask in front of every move of a record (colours alternating from black)."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.nn.evaluate import candidate_words
    board = GoBoard(size, 7.0, bool(superko))
    out, color = [], 1
    for pos in moves:
        out.append(candidate_words(board, color, size))
        board.put_stone(int(pos), color)
        color = 3 - color
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def golden_games(size):
    """[(name, sgf text)]: the games of the datagen_s* fixtures - 9x9: the three self-play records datagen_s9 was written from."""
    if size == 9:
        games = load_json("selfplay_games.json")
        return tuple((key.split(",")[0], games[key]) for key in sorted(games))
    games = load_json(f"datagen_s{size}.json")["games"]
    return tuple((key, games[key]) for key in sorted(games))


def write_games(root, size, extra=()):
    """The golden games (and `extra` (name, text) pairs) as root/<name>.sgf; returns the sorted paths."""
    import os
    os.makedirs(root, exist_ok=True)
    paths = []
    for name, text in tuple(golden_games(size)) + tuple(extra):
        path = os.path.join(str(root), f"{name}.sgf")
        with open(path, "w", encoding="utf-8") as f:
            f.write(text)
        paths.append(path)
    return sorted(paths)


def host_pipeline(network, paths, size, *, stride=1, first_ply=0, bucket_width=10, n_buckets=32, superko=False, chunk_rows=65536):
    """GoBoard replay, generate_input_planes, tg_net_forward_host on the same rows in the same chunking, the numpy restatement.
    -> (records: restate()'s list in row order, row_game, row_ply)"""
    import torch
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.board.stone import Stone
    from tamago_amd.nn import evaluate as ev
    from tamago_amd.nn.feature import generate_input_planes
    records = ev.as_records(paths, size)
    out, row_game, row_ply = [], [], []
    for g0, count in ev.chunk_games(records, stride, first_ply, chunk_rows):
        planes, masks, move, cls, ply = [], [], [], [], []
        for g in range(g0, g0 + count):
            rec = records[g]
            board = GoBoard(size, 7.0, bool(superko))
            color = Stone.BLACK
            actions = ev.move_actions(rec.moves, size)
            for i, pos in enumerate(rec.moves):
                if i >= first_ply and (i - first_ply) % stride == 0:
                    planes.append(np.asarray(generate_input_planes(board, color, 0), dtype=np.float32).reshape(6, size, size))
                    masks.append(ev.candidate_words(board, color, size))
                    move.append(int(actions[i]))
                    cls.append(rec.value_label if i % 2 == 0 else 2 - rec.value_label)
                    ply.append(i)
                    row_game.append(g)
                board.put_stone(int(pos), color)
                color = Stone.get_opponent_color(color)
        if not planes:
            continue
        policy, value = network.inference(torch.from_numpy(np.stack(planes)))
        arrays = (policy.numpy(), value.numpy(), np.stack(masks), np.array(move, np.int32), np.array(cls, np.int32),
                  np.array(ply, np.int32))
        out += rs.restate(arrays, bucket_width, n_buckets)
        row_ply += ply
    return out, np.array(row_game), np.array(row_ply)
