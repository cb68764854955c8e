"""Move generation from the policy network alone (mirror of nn/policy_player.py:13-46).

One forward pass; the legal moves whose policy exceeds a tenth of the best are kept and one of them is drawn
with ``random.choices``.  ``choose_from_policy`` states the rule on the host; for a ``DualNet`` the whole move -
planes, forward pass, candidates, cut, draw - runs on the device (``tg_policy_*``, csrc/search.hip) from the
state of Python's global ``random`` generator, which is put back advanced by exactly the one ``random()`` the
reference consumes.  ``policy_moves`` does many positions in one launch set, ``policy_games`` plays whole games
policy against policy on device-resident boards.
"""
import ctypes
import itertools
import random
import time
from bisect import bisect_right
from typing import List, Optional, Sequence

import numpy as np
import torch

from tamago_amd import lib as _lib
from tamago_amd.board.constant import PASS
from tamago_amd.board.go_board import GoBoard, zobrist_keys
from tamago_amd.board.stone import color_value

MT_WORDS = 625                     # random.getstate()[1]: 624 key words + the position


def choose_from_policy(policy: Sequence[float], board: GoBoard, color, rng=random) -> int:
    """policy_player.py:29-46 for policy probabilities ``policy`` (float32 [S*S+1], index S*S = PASS): one
    ``rng.random()`` is consumed.  ``random.choices`` is restated as CPython 3.10 computes it (Lib/random.py:
    sequential running sum, ``bisect_right(cum, random() * total, 0, n - 1)``)."""
    policy = [float(p) for p in policy]              # float32 -> Python floats, like .numpy().tolist()
    size = board.get_board_size()
    legal = [(p, policy[i]) for i, p in enumerate(board.onboard_pos) if board.is_legal(p, color)]
    pos = [p for p, _ in legal] + [PASS]
    weights = [w for _, w in legal] + [policy[size ** 2]]
    cut = max(weights) * 0.1
    kept = [(p, w) for p, w in zip(pos, weights) if w > cut]
    cum = list(itertools.accumulate(w for _, w in kept))
    total = cum[-1] + 0.0
    return kept[bisect_right(cum, rng.random() * total, 0, len(kept) - 1)][0]


def _state_words(state) -> np.ndarray:
    """random.getstate() (or its [1]) -> uint32 [625]."""
    words = state[1] if len(state) == 3 else state
    out = np.asarray(words, dtype=np.uint32)
    if out.shape != (MT_WORDS,):
        raise ValueError("expected the 625 words of random.getstate()[1]")
    return out


def seed_states(seeds: Sequence[int]) -> np.ndarray:
    """uint32 [n, 625]: random.Random(seed).getstate()[1] for every seed.  Seeds in [0, 2^32) are expanded by the library
    (tg_policy_seed_states: CPython's init_by_array on the one-word key), any other seed goes through a Random object."""
    seeds = list(seeds)
    if not all(isinstance(v, (int, np.integer)) and 0 <= int(v) < 2 ** 32 for v in seeds):
        return np.stack([_state_words(random.Random(seed).getstate()) for seed in seeds])
    words = np.asarray(seeds, dtype=np.uint32)
    out = np.empty((len(seeds), MT_WORDS), dtype=np.uint32)
    _lib.check(_lib.load().tg_policy_seed_states(words.ctypes.data, len(seeds), out.ctypes.data), "tg_policy_seed_states")
    return out


class PolicyBoards:
    """T device-resident boards with one `random` stream each: a tg_search (for the boards) and the tg_policy on it."""

    def __init__(self, board_size: int, boards: int, superko: bool, device_index: int = 0):
        self.lib = _lib.load()
        self.S, self.T, self.A = board_size, boards, board_size * board_size + 1
        self.superko = bool(superko)
        self.device = torch.device("cuda", device_index)
        self.search = ctypes.c_void_p()
        self.handle = ctypes.c_void_p()
        cfg = _lib.SearchConfig(board_size, boards, 2, 1, 0, int(self.superko), device_index, 0)
        _lib.check(self.lib.tg_search_create(ctypes.byref(cfg), ctypes.byref(self.search)), "tg_search_create")
        keys = zobrist_keys(board_size)
        _lib.check(self.lib.tg_search_set_zobrist(self.search, keys.ctypes.data, keys.size), "tg_search_set_zobrist")
        _lib.check(self.lib.tg_policy_create(self.search, ctypes.byref(self.handle)), "tg_policy_create")
        self._plain = set()                          # boards without the superko check on a handle that checks
        self.planes = torch.empty((boards, 6, board_size, board_size), dtype=torch.float32, device=self.device)
        self.policy = torch.empty((boards, self.A), dtype=torch.float32, device=self.device)
        self.value = torch.empty((boards, 3), dtype=torch.float32, device=self.device)

    def close(self):
        if self.handle:
            self.lib.tg_policy_destroy(self.handle)
            self.handle = ctypes.c_void_p()
        if self.search:
            self.lib.tg_search_destroy(self.search)
            self.search = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def set_root(self, t: int, board: GoBoard, color):
        """The position of board t, as MCTSTree hands it to its engine (SearchEngine.set_root)."""
        assert board.board_size == self.S
        check = bool(board.check_superko)
        if check and not self.superko:
            raise ValueError("a board that checks superko needs PolicyBoards(superko=True)")
        if self.superko and (not check or t in self._plain):          # a board of the other kind on a checking handle
            _lib.check(self.lib.tg_policy_set_superko(self.handle, t, int(check)), "tg_policy_set_superko")
            (self._plain.discard if check else self._plain.add)(t)
        cells = np.ascontiguousarray(board.cells, dtype=np.uint8)
        hist = np.ascontiguousarray(board.rec_hash[:min(board.moves, board.max_records)])
        pos = _lib.RootPosition(cells.ctypes.data, hist.ctypes.data, ctypes.c_uint64(int(board.hash)), board.moves,
                                board.ko_pos, board.ko_move, board.prev_move(1), board.prev_move(2), color_value(color))
        _lib.check(self.lib.tg_search_set_root(self.search, t, ctypes.byref(pos)), "tg_search_set_root")

    def seed(self, t: int, state):
        words = _state_words(state)
        _lib.check(self.lib.tg_policy_seed(self.handle, t, words.ctypes.data, int(words[624])), "tg_policy_seed")

    def state(self, t: int) -> tuple:
        """The 625 words to put back with random.setstate((3, words, gauss_next))."""
        words = np.empty(MT_WORDS, dtype=np.uint32)
        pos = ctypes.c_int(0)
        _lib.check(self.lib.tg_policy_state(self.handle, t, words.ctypes.data, ctypes.byref(pos)), "tg_policy_state")
        words[624] = pos.value
        return tuple(int(w) for w in words)

    def write_planes(self) -> torch.Tensor:
        _lib.check(self.lib.tg_policy_planes(self.handle, self.planes.data_ptr(), self._stream()), "tg_policy_planes")
        return self.planes

    def moves(self, policy: torch.Tensor, play: bool = False, answer_pass: bool = False) -> np.ndarray:
        """One move per board from a device policy [T, A] (tg_policy_moves)."""
        assert policy.is_cuda and policy.dtype == torch.float32 and policy.is_contiguous()
        assert tuple(policy.shape) == (self.T, self.A)
        out = np.empty(self.T, dtype=np.int32)
        _lib.check(self.lib.tg_policy_moves(self.handle, policy.data_ptr(), int(play), int(answer_pass), None,
                                            out.ctypes.data, self._stream()), "tg_policy_moves")
        return out

    def moves_with(self, network, play: bool = False, answer_pass: bool = False) -> np.ndarray:
        """Planes, the forward pass of `network` (a DualNet) and the move of every board."""
        network.forward_device(self.write_planes(), False, out=(self.policy, self.value))
        return self.moves(self.policy, play, answer_pass)

    def read_positions(self):
        """(cells uint8 [T, (S+2)^2], GoBoard.moves [T], side to move [T]) of the boards as they stand."""
        w = (self.S + 2) ** 2
        cells = np.empty((self.T, w), dtype=np.uint8)
        moves = np.empty(self.T, dtype=np.int32)
        to_move = np.empty(self.T, dtype=np.int32)
        _lib.check(self.lib.tg_search_read_positions(self.search, cells.ctypes.data, moves.ctypes.data,
                                                     to_move.ctypes.data), "tg_search_read_positions")
        return cells, moves, to_move


_single = {}                      # (board size, superko, device) -> PolicyBoards of one board


def _single_board(size: int, superko: bool, device_index: int) -> PolicyBoards:
    key = (size, bool(superko), device_index)
    if key not in _single:
        _single[key] = PolicyBoards(size, 1, superko, device_index)
    return _single[key]


def generate_move_from_policy(network, board: GoBoard, color) -> int:
    """nn/policy_player.py:13-46.  A DualNet runs on the device from the state of the global ``random``
    generator, which is left where the reference's one ``random.choices`` call leaves it; any other network
    object goes through its ``inference`` and ``choose_from_policy``."""
    from tamago_amd.nn.network.dual_net import DualNet
    if not isinstance(network, DualNet):
        size = board.get_board_size()
        policy, _ = network.inference(torch.tensor(_host_planes(board, color).reshape(1, 6, size, size)))
        return choose_from_policy(policy[0].numpy().tolist(), board, color)
    boards = _single_board(board.get_board_size(), board.check_superko, network.device_index)
    version, _, gauss_next = state = random.getstate()
    boards.set_root(0, board, color)
    boards.seed(0, state)
    move = int(boards.moves_with(network)[0])
    random.setstate((version, boards.state(0), gauss_next))
    return move


def _host_planes(board: GoBoard, color) -> np.ndarray:
    """nn/feature.py:10-57 in numpy, for network objects used where there is no device."""
    size = board.get_board_size()
    data = np.array(board.get_board_data(), dtype=np.int64)
    if color_value(color) == 2:
        data = np.where(data == 0, 0, 3 - data)
    planes = np.zeros((6, size * size), dtype=np.float32)
    for c in range(3):
        planes[c] = data == c
    prev = board.prev_move(1)
    if board.moves > 1 and prev == PASS:
        planes[4] = 1.0
    elif board.moves > 1:
        planes[3, board.onboard_pos.index(prev)] = 1.0
    planes[5] = 1.0 if color_value(color) == 1 else -1.0
    return planes.reshape(6, size, size)


def policy_moves(network, positions, states, superko: Optional[bool] = None, play: bool = False,
                 answer_pass: bool = False):
    """The policy move of many positions in one launch set.  positions: [(GoBoard, colour)] of one board size
    (mixed colours allowed), states: one ``random.getstate()`` (or its 625 words) per position.  Returns
    (moves int32 [n], [the 625 words after the draw per position])."""
    if len(positions) != len(states) or not positions:
        raise ValueError("one stream state per position")
    first = positions[0][0]
    superko = any(board.check_superko for board, _ in positions) if superko is None else superko
    boards = PolicyBoards(first.get_board_size(), len(positions), superko, network.device_index)
    try:
        for t, ((board, color), state) in enumerate(zip(positions, states)):
            boards.set_root(t, board, color)
            boards.seed(t, state)
        moves = boards.moves_with(network, play, answer_pass)
        return moves, [boards.state(t) for t in range(len(positions))]
    finally:
        boards.close()


END_REASONS = {0: "unfinished", 1: "two_passes", 2: "max_moves"}


def policy_games(black, white, games: int, size: int = 9, komi: float = 7.0, seeds: Optional[Sequence[int]] = None,
                 max_moves: Optional[int] = None, boards: Optional[int] = None, superko: bool = True,
                 answer_pass: bool = True, keep_policy: bool = False, device_index: int = 0) -> dict:
    """`games` games from the empty board, DualNet `black` against DualNet `white`, every move by
    generate_move_from_policy (and, with answer_pass, the rule of gtp/client.py:209-211), all on the device.
    Game g draws from the stream of ``random.Random(seeds[g])`` (default seed g); it ends after two passes or
    max_moves moves (default 2 S^2, selfplay/worker.py:44).  Slot t of the `boards` boards plays the games t,
    t + boards, ...  Returns a dict: games = [{moves, length, end, score, winner}] with score = count_score - komi
    and winner by worker.py:80-87 ("black" / "white" / "draw"; None for a game that reached max_moves), positions =
    positions forwarded, plies, seconds (set-up, plies enqueued, device drained + results copied, results as Python
    objects), and with keep_policy policies = float32 [plies, boards, A]."""
    seeds = list(range(games)) if seeds is None else list(seeds)
    if len(seeds) != games:
        raise ValueError("one seed per game")
    max_moves = 2 * size * size if max_moves is None else max_moves
    boards = min(games, 4096) if boards is None else boards
    clock = [time.perf_counter()]
    states = np.ascontiguousarray(seed_states(seeds))
    pb = PolicyBoards(size, boards, superko, device_index)
    lib = pb.lib
    try:
        _lib.check(lib.tg_policy_games_begin(pb.handle, games, max_moves, int(answer_pass), states.ctypes.data),
                   "tg_policy_games_begin")
        clock.append(time.perf_counter())
        rounds = -(-games // boards)
        max_plies = (max_moves + (max_moves & 1)) * rounds + 1
        kept: List[torch.Tensor] = []
        finished = ctypes.c_int32(0)
        plies = 0
        while plies < max_plies:
            net = black if plies % 2 == 0 else white
            keep = torch.empty_like(pb.policy) if keep_policy else None
            _lib.check(lib.tg_policy_games_ply(pb.handle, net.handle, pb.planes.data_ptr(), pb.policy.data_ptr(),
                                               pb.value.data_ptr(), keep.data_ptr() if keep_policy else None,
                                               pb._stream()), "tg_policy_games_ply")
            if keep_policy:
                kept.append(keep)
            plies += 1
            if plies % 8 == 0:                       # the counter is host-mapped: a look costs no synchronisation
                _lib.check(lib.tg_policy_games_finished(pb.handle, ctypes.byref(finished)), "tg_policy_games_finished")
                if finished.value >= games:
                    break
        clock.append(time.perf_counter())
        log = np.zeros((games, max_moves), dtype=np.int32)
        length = np.zeros(games, dtype=np.int32)
        reason = np.zeros(games, dtype=np.int32)
        score = np.zeros(games, dtype=np.int32)
        total = ctypes.c_int64(0)
        _lib.check(lib.tg_policy_games_results(pb.handle, log.ctypes.data, length.ctypes.data, reason.ctypes.data,
                                               score.ctypes.data, None, ctypes.byref(total)), "tg_policy_games_results")
        clock.append(time.perf_counter())            # (tg_policy_games_results has waited for the last ply)
        if int((reason == 0).sum()):
            raise _lib.TamagoHipError(f"{int((reason == 0).sum())} games still running after {plies} plies")
        out = []
        for moves, n, why, points in zip(log.tolist(), length.tolist(), reason.tolist(), score.tolist()):
            result = {"moves": moves[:n], "length": n, "end": END_REASONS[why], "score": 0.0, "winner": None}
            if why == 1:
                result["score"] = float(points) - komi
                result["winner"] = "black" if result["score"] > 0.1 else "white" if result["score"] < -0.1 else "draw"
            out.append(result)
        clock.append(time.perf_counter())
        # seconds: streams and handles set up | plies enqueued | the device finished, results copied | results as Python objects
        res = {"games": out, "plies": plies, "positions": plies * boards,
               "seconds": [b - a for a, b in zip(clock, clock[1:])]}
        if keep_policy:
            res["policies"] = torch.stack(kept).cpu().numpy() if kept else np.zeros((0, boards, pb.A), np.float32)
        return res
    finally:
        pb.close()
