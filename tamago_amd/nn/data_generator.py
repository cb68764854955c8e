"""Training-data generation from game records (mirror of nn/data_generator.py:17-149):
``sl_data_<k>.npz`` (every position x 8 symmetries, one-hot move targets) and
``rl_data_<k>.npz`` (8 random positions per self-play game, one random symmetry each,
improved-policy targets from the SGF comments) with the reference's keys, dtypes, chunking
and random-number call order (``random.shuffle`` of the file list, two
``np.random.permutation`` calls per game) - the files ``train.py`` consumes.

MI355X form: games are replayed on the host board only to collect position descriptors
(cells, side to move, previous move, move count, symmetry); the input planes of a whole
chunk are then produced by ONE launch of the featurise kernel (tg_featurize_sym_dev)
instead of one Python ``generate_input_planes`` per sample.

``device_replay=True`` (opt-in; the files are the same byte for byte) moves the replay itself to the device: the host only
parses the records and decides which plies and symmetries are sampled (so the random-number call order above stays where
it is), ``tg_replay_run`` replays every game of a chunk on the LDS board and writes the planes of the sampled plies, and
the targets of the chunk are built with one table look-up (``generate_target_data_batch`` /
``generate_rl_target_data_batch``).  A game with a move the device engine is not specified for (onto a point that is not
empty, or no coordinate of the board) comes back flagged and is redone with the Python board.
``iter_reinforcement_learning_chunks`` hands the same chunks to the trainer in device memory, without a file;
``iter_reanalysed_chunks`` (no reference counterpart) hands over the same planes and value labels with policy targets that
the given network searches afresh (tamago_amd/mcts/reanalyse.py) instead of the ones frozen in the records' comments."""
import glob
import os
import random
from typing import List

import numpy as np
import torch

from tamago_amd import lib as _lib
from tamago_amd.board.go_board import GoBoard
from tamago_amd.board.stone import Stone, color_value
from tamago_amd.nn.feature import (featurize_batch, generate_rl_target_data, generate_rl_target_data_batch, generate_target_data,
                                   generate_target_data_batch)
from tamago_amd.sgf.reader import SGFReader

BATCH_SIZE = 256                       # learning_param.py:11
DATA_SET_SIZE = BATCH_SIZE * 4000      # learning_param.py:31


class _Samples:
    """Position descriptors + targets waiting to be written."""

    def __init__(self, size: int):
        self.size = size
        self.cells: List[np.ndarray] = []
        self.to_move: List[int] = []
        self.prev_move: List[int] = []
        self.moves: List[int] = []
        self.sym: List[int] = []
        self.policy: List[np.ndarray] = []
        self.value: List[int] = []

    def __len__(self):
        return len(self.value)

    def add(self, board: GoBoard, color, sym: int, policy: np.ndarray, value: int):
        self.cells.append(np.array(board.get_board_data(), dtype=np.uint8))
        self.to_move.append(color_value(color))
        self.prev_move.append(board.prev_move(1))
        self.moves.append(board.moves)
        self.sym.append(int(sym))
        self.policy.append(policy)
        self.value.append(value)

    def take(self, count: int) -> "_Samples":
        head = _Samples(self.size)
        for name in ("cells", "to_move", "prev_move", "moves", "sym", "policy", "value"):
            values = getattr(self, name)
            setattr(head, name, values[:count])
            setattr(self, name, values[count:])
        return head

    def planes(self, device_index: int = 0) -> np.ndarray:
        out = featurize_batch(self.size, np.stack(self.cells), np.array(self.to_move), np.array(self.prev_move),
                              np.array(self.moves), np.array(self.sym), device_index)
        return out.cpu().numpy()


def _save_data(save_file_path: str, samples: _Samples, kifu_counter: int) -> None:
    """nn/data_generator.py:17-34 (np.savez_compressed; value int32, kifu_count 0-d)."""
    np.savez_compressed(save_file_path, input=samples.planes(), policy=np.array(samples.policy),
                        value=np.array(samples.value, dtype=np.int32), kifu_count=np.array(kifu_counter))


def _write_chunks(program_dir: str, prefix: str, games, board_size: int, per_game) -> None:
    """Chunking of nn/data_generator.py:70-86 / :133-149: a full DATA_SET_SIZE chunk is written
    as soon as enough samples exist, the tail in whole mini-batches."""
    pending = _Samples(board_size)
    kifu_counter, data_counter = 1, 0
    for path in games:
        per_game(path, pending)
        if len(pending) >= DATA_SET_SIZE:
            _save_data(os.path.join(program_dir, "data", f"{prefix}_{data_counter}"),
                       pending.take(DATA_SET_SIZE), kifu_counter)
            kifu_counter = 1
            data_counter += 1
        kifu_counter += 1
    n_batches = len(pending) // BATCH_SIZE
    if n_batches > 0:
        _save_data(os.path.join(program_dir, "data", f"{prefix}_{data_counter}"),
                   pending.take(n_batches * BATCH_SIZE), kifu_counter)


def generate_supervised_learning_data(program_dir: str, kifu_dir: str, board_size: int = 9,
                                      device_replay: bool = False) -> None:
    """nn/data_generator.py:37-86.  device_replay: the same files through tg_replay_run (module docstring)."""
    if device_replay:
        paths = sorted(glob.glob(os.path.join(kifu_dir, "*.sgf")))
        _write_replay_chunks(program_dir, "sl_data", (_sl_record(path, board_size) for path in paths), board_size, "sl")
        return
    board = GoBoard(board_size=board_size)

    def per_game(path: str, pending: _Samples):
        board.clear()
        sgf = SGFReader(path, board_size)
        color = Stone.BLACK
        value_label = sgf.get_value_label()
        for pos in sgf.get_moves():
            for sym in range(8):
                pending.add(board, color, sym, generate_target_data(board, pos, sym), value_label)
            board.put_stone(pos, color)
            color = Stone.get_opponent_color(color)
            value_label = 2 - value_label                # label is from the mover's point of view

    _write_chunks(program_dir, "sl_data", sorted(glob.glob(os.path.join(kifu_dir, "*.sgf"))), board_size, per_game)


def generate_reinforcement_learning_data(program_dir: str, kifu_dir_list: List[str], board_size: int = 9,
                                         device_replay: bool = False) -> None:
    """nn/data_generator.py:89-149.  device_replay: the same files through tg_replay_run (module docstring)."""
    board = GoBoard(board_size=board_size)
    kifu_list = []
    for kifu_dir in kifu_dir_list:
        kifu_list.extend(glob.glob(os.path.join(kifu_dir, "*.sgf")))
    random.shuffle(kifu_list)
    if device_replay:
        _write_replay_chunks(program_dir, "rl_data", (_rl_record(path, board_size) for path in kifu_list), board_size, "rl")
        return

    def per_game(path: str, pending: _Samples):
        board.clear()
        sgf = SGFReader(path, board_size)
        color = Stone.BLACK
        value_label = sgf.get_value_label()
        targets = set(int(i) for i in np.random.permutation(np.arange(sgf.get_n_moves()))[:8])
        sym_order = np.random.permutation(np.arange(8))
        taken = 0
        for i, pos in enumerate(sgf.get_moves()):
            if i in targets:
                sym = int(sym_order[taken])
                pending.add(board, color, sym, generate_rl_target_data(board, sgf.get_comment(i), sym), value_label)
                taken += 1
            board.put_stone(pos, color)
            color = Stone.get_opponent_color(color)
            value_label = 2 - value_label

    _write_chunks(program_dir, "rl_data", kifu_list, board_size, per_game)


# ---- device_replay: the replay and the planes on the device, the targets as one table look-up per chunk ------------------
# what the device_replay path has done in this process: tg_replay_run calls, games replayed, games redone on the host
REPLAY_STATS = {"calls": 0, "games": 0, "flagged": 0}


class _Record:
    """One parsed game and its samples: moves int32 [n] (padded coordinates, 0 = PASS), the sampled plies in increasing
    order with one symmetry each, the value label of every sample and what its policy target is made from (SL: the move
    played at the ply; RL: the improved-policy comment of the ply)."""
    __slots__ = ("moves", "ply", "sym", "value", "target", "komi")

    def __init__(self, moves, ply, sym, value_label, target, komi=7.0):
        self.moves = moves
        self.komi = komi
        self.ply = np.ascontiguousarray(ply, dtype=np.int32)
        self.sym = np.ascontiguousarray(sym, dtype=np.int8)
        # the label is from the mover's point of view: it flips with every ply (data_generator.py:64 / :134)
        self.value = np.where(self.ply % 2 == 0, value_label, 2 - value_label).astype(np.int32)
        self.target = target


def _sl_record(path: str, board_size: int) -> _Record:
    """data_generator.py:50-64: every ply under the eight symmetries, the move played as the target."""
    sgf = SGFReader(path, board_size)
    n = sgf.get_n_moves()
    moves = np.fromiter(sgf.get_moves(), dtype=np.int32, count=n)
    return _Record(moves, np.repeat(np.arange(n), 8), np.tile(np.arange(8), n), sgf.get_value_label(), np.repeat(moves, 8))


def _rl_record(path: str, board_size: int) -> _Record:
    """data_generator.py:105-134: eight random plies, the k-th of them (in game order) under the k-th entry of a random
    order of the symmetries - the two np.random.permutation calls of the host path, made before anything is replayed."""
    sgf = SGFReader(path, board_size)
    n = sgf.get_n_moves()
    moves = np.fromiter(sgf.get_moves(), dtype=np.int32, count=n)
    ply = np.sort(np.random.permutation(np.arange(n))[:8])
    sym_order = np.random.permutation(np.arange(8))
    return _Record(moves, ply, sym_order[:len(ply)], sgf.get_value_label(), [sgf.get_comment(int(i)) for i in ply], sgf.komi)


def _host_planes(size: int, record: _Record, device_index: int) -> torch.Tensor:
    """The planes of one record's samples by the host path (Python board, featurise kernel): what a flagged game gets."""
    board = GoBoard(board_size=size)
    samples = _Samples(size)
    color, k = Stone.BLACK, 0
    for i, pos in enumerate(record.moves):
        while k < len(record.ply) and record.ply[k] == i:
            samples.add(board, color, int(record.sym[k]), None, 0)
            k += 1
        if k == len(record.ply):
            break
        board.put_stone(int(pos), color)
        color = Stone.get_opponent_color(color)
    return featurize_batch(size, np.stack(samples.cells), np.array(samples.to_move), np.array(samples.prev_move),
                           np.array(samples.moves), np.array(samples.sym), device_index)


class _ReplayPending:
    """Samples waiting to be written, device_replay form: games queue as records; their rows (planes in device memory,
    policy and value on the host) are made by ONE tg_replay_run when a chunk is taken."""

    def __init__(self, size: int, mode: str, device_index: int = 0):
        self.size, self.mode, self.device_index = size, mode, device_index
        self.device = torch.device("cuda", device_index)
        self.lib = _lib.load()
        self.handle = None
        self.queue: List[_Record] = []
        self.queued = 0
        self.planes = self.policy = None     # rows made and not yet taken: planes on the device, policy / value on the host
        self.value = np.zeros(0, dtype=np.int32)

    def __len__(self):
        return len(self.value) + self.queued

    def close(self):
        if self.handle is not None:
            self.lib.tg_replay_destroy(self.handle)
            self.handle = None

    def add(self, record: _Record):
        self.queue.append(record)
        self.queued += len(record.ply)

    def _replay(self, records: List[_Record]) -> torch.Tensor:
        """planes [samples,6,S,S] of the records' samples, in device memory."""
        import ctypes
        if self.handle is None:
            handle = ctypes.c_void_p()
            _lib.check(self.lib.tg_replay_create(self.size, self.device_index, ctypes.byref(handle)), "tg_replay_create")
            self.handle = handle
        offsets = np.zeros(len(records) + 1, dtype=np.int64)
        np.cumsum([len(r.moves) for r in records], out=offsets[1:])
        sample_offsets = np.zeros(len(records) + 1, dtype=np.int64)
        np.cumsum([len(r.ply) for r in records], out=sample_offsets[1:])
        moves = np.ascontiguousarray(np.concatenate([r.moves for r in records]), dtype=np.int32)
        ply = np.ascontiguousarray(np.concatenate([r.ply for r in records]), dtype=np.int32)
        sym = np.ascontiguousarray(np.concatenate([r.sym for r in records]), dtype=np.int8)
        flags = np.zeros(len(records), dtype=np.int32)
        with torch.cuda.device(self.device):
            planes = torch.empty((len(ply), 6, self.size, self.size), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.tg_replay_run(self.handle, moves.ctypes.data, offsets.ctypes.data, len(records),
                                              ply.ctypes.data, sym.ctypes.data, sample_offsets.ctypes.data,
                                              planes.data_ptr(), flags.ctypes.data,
                                              torch.cuda.current_stream(self.device).cuda_stream), "tg_replay_run")
        for g in np.nonzero(flags)[0]:
            if sample_offsets[g + 1] > sample_offsets[g]:
                planes[sample_offsets[g]:sample_offsets[g + 1]] = _host_planes(self.size, records[g], self.device_index)
        REPLAY_STATS["calls"] += 1
        REPLAY_STATS["games"] += len(records)
        REPLAY_STATS["flagged"] += int(np.count_nonzero(flags))
        return planes

    def _targets(self, records: List[_Record]) -> np.ndarray:
        sym = np.concatenate([r.sym for r in records])
        if self.mode == "sl":
            return generate_target_data_batch(self.size, np.concatenate([r.target for r in records]), sym)
        return generate_rl_target_data_batch(self.size, [text for r in records for text in r.target], sym)

    def _make_rows(self):
        records = [r for r in self.queue if len(r.ply)]
        self.queue, self.queued = [], 0
        if not records:
            return
        planes, policy = self._replay(records), self._targets(records)
        self.planes = torch.cat([self.planes, planes]) if len(self.value) else planes
        self.policy = np.concatenate([self.policy, policy]) if len(self.value) else policy
        self.value = np.concatenate([self.value] + [r.value for r in records])

    def take(self, count: int):
        """The first `count` rows: (planes on the device, policy, value int32)."""
        self._make_rows()
        assert 0 < count <= len(self.value)
        head = (self.planes[:count], self.policy[:count], self.value[:count])
        self.planes, self.policy, self.value = self.planes[count:], self.policy[count:], self.value[count:]
        return head


def _replay_chunks(records, board_size: int, mode: str, device_index: int = 0):
    """The chunking of _write_chunks over game records: yields (planes on the device, policy, value, kifu_count)."""
    pending = _ReplayPending(board_size, mode, device_index)
    kifu_counter = 1
    try:
        for record in records:
            pending.add(record)
            if len(pending) >= DATA_SET_SIZE:
                yield pending.take(DATA_SET_SIZE) + (kifu_counter,)
                kifu_counter = 1
            kifu_counter += 1
        n_batches = len(pending) // BATCH_SIZE
        if n_batches > 0:
            yield pending.take(n_batches * BATCH_SIZE) + (kifu_counter,)
    finally:
        pending.close()


def _planes_to_host(planes: torch.Tensor) -> np.ndarray:
    return planes.cpu().numpy()


def _save_arrays(save_file_path: str, planes: torch.Tensor, policy: np.ndarray, value: np.ndarray, kifu_counter: int) -> None:
    """_save_data for rows that already exist."""
    np.savez_compressed(save_file_path, input=_planes_to_host(planes), policy=policy,
                        value=np.array(value, dtype=np.int32), kifu_count=np.array(kifu_counter))


def _write_replay_chunks(program_dir: str, prefix: str, records, board_size: int, mode: str) -> None:
    for data_counter, (planes, policy, value, kifu_counter) in enumerate(_replay_chunks(records, board_size, mode)):
        _save_arrays(os.path.join(program_dir, "data", f"{prefix}_{data_counter}"), planes, policy, value, kifu_counter)


def iter_reinforcement_learning_chunks(kifu_dir_list: List[str], board_size: int, device=0):
    """The chunks generate_reinforcement_learning_data(..., device_replay=True) writes as rl_data_<k>.npz, in the same
    order with the same rows, as device-resident (planes float32, policy float32, value int64) - what load_data_set makes
    of a file, before its shuffle - for train_with_gumbel_alphazero_on_gpu(..., chunks=...).  Every random call (the
    shuffle of the list, two permutations per game) is made before the first chunk is yielded, so a consumer that draws
    from the global generators between chunks, as the trainer does, sees the stream it would see after the files."""
    device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    index = device.index if device.index is not None else 0
    kifu_list = []
    for kifu_dir in kifu_dir_list:
        kifu_list.extend(glob.glob(os.path.join(kifu_dir, "*.sgf")))
    random.shuffle(kifu_list)
    records = [_rl_record(path, board_size) for path in kifu_list]
    for planes, policy, value, _ in _replay_chunks(records, board_size, "rl", index):
        yield (planes, torch.from_numpy(policy.astype(np.float32)).to(planes.device),
               torch.from_numpy(value.astype(np.int64)).to(planes.device))


def _sampled_positions(records, board_size: int):
    """(board, colour to move) before every sampled ply of the records, in row order: a host replay of each record as
    analysis.game_positions does it (a fresh board of the record's komi with self-play's superko setting, the moves in
    order, colours alternating from black as in the record paths above).  A generator: nothing is replayed before it is
    asked for."""
    import copy
    from tamago_amd.mcts.reanalyse import SELFPLAY_CHECK_SUPERKO
    for record in records:
        if not len(record.ply):
            continue
        board = GoBoard(board_size=board_size, komi=record.komi, check_superko=SELFPLAY_CHECK_SUPERKO)
        color, k = Stone.BLACK, 0
        for i, pos in enumerate(record.moves):
            while k < len(record.ply) and record.ply[k] == i:
                yield copy.deepcopy(board), color
                k += 1
            if k == len(record.ply):
                break
            board.put_stone(int(pos), color)
            color = Stone.get_opponent_color(color)


def iter_reanalysed_chunks(network, kifu_dir_list: List[str], board_size: int, visits: int, device=0, seed: int = 0,
                           max_trees=None, device_roots: bool = False):
    """iter_reinforcement_learning_chunks with fresh policy targets (no reference counterpart): the same records, sample
    choice and order of global random calls - all made before the first chunk is yielded - so planes and value labels are
    that function's byte for byte; the policy row of a sample is the improved policy `network` finds with a Gumbel search
    of `visits` simulations on the position before the sampled ply (mcts.reanalyse.reanalyse_positions: one tree per
    position, at most max_trees in lock-step), in the order of the sample's symmetry (symmetry_pos_table).  Row i of the
    whole run searches with seed `seed + i`; the searches draw from those private streams only.  Games the replay kernel
    flags get their planes from the host path as ever and are reanalysed like the others.  REANALYSE_STATS counts.
    device_roots: _sampled_positions is not run - the search roots are written on the device from the records already
    parsed (mcts.reanalyse.reanalyse_records, colours alternating from black and self-play's superko setting, as that
    replay has them); same chunks.  REANALYSE_STATS["device_roots"] / ["host_roots"] count the positions set up each way
    (host: every position of the default path, and the ones a launch flagged)."""
    import itertools
    import time
    from tamago_amd.mcts.reanalyse import reanalyse_positions, reanalyse_records, symmetric_rows
    device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    index = device.index if device.index is not None else 0
    kifu_list = []
    for kifu_dir in kifu_dir_list:
        kifu_list.extend(glob.glob(os.path.join(kifu_dir, "*.sgf")))
    random.shuffle(kifu_list)
    records = [_rl_record(path, board_size) for path in kifu_list]
    sym = np.concatenate([r.sym for r in records if len(r.ply)]) if any(len(r.ply) for r in records) else np.zeros(0, np.int8)
    if device_roots:
        moves = [r.moves for r in records]
        members = [(g, int(ply)) for g, r in enumerate(records) for ply in r.ply]
    else:
        positions = _sampled_positions(records, board_size)
    done = 0
    for planes, _, value, _ in _replay_chunks(records, board_size, "rl", index):
        n = int(planes.shape[0])
        t0 = time.perf_counter()
        boards = None if device_roots else list(itertools.islice(positions, n))
        t1 = time.perf_counter()
        seeds = range(seed + done, seed + done + n)
        if device_roots:
            result = reanalyse_records(network, moves, members[done:done + n], visits, seeds=seeds, max_trees=max_trees,
                                       device_index=index)
        else:
            result = reanalyse_positions(network, boards, visits, seeds=seeds, max_trees=max_trees, device_index=index)
        policy = symmetric_rows(board_size, result.rows, sym[done:done + n])
        done += n
        REANALYSE_STATS["positions"] += n
        REANALYSE_STATS["host_roots"] += result.host_roots if device_roots else n
        REANALYSE_STATS["device_roots"] += n - result.host_roots if device_roots else 0
        REANALYSE_STATS["board_seconds"] += t1 - t0
        REANALYSE_STATS["search_seconds"] += time.perf_counter() - t1
        REANALYSE_STATS["forward_positions"] += result.forward_positions
        REANALYSE_STATS["range_fallbacks"] += result.range_fallbacks
        yield planes, policy, torch.from_numpy(value.astype(np.int64)).to(planes.device)


# what iter_reanalysed_chunks has done in this process
REANALYSE_STATS = {"positions": 0, "board_seconds": 0.0, "search_seconds": 0.0, "forward_positions": 0, "range_fallbacks": 0,
                   "device_roots": 0, "host_roots": 0}
