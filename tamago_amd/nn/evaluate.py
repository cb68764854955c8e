"""Evaluate a network on game records, on the device (no reference counterpart): how well it predicts the moves
and the results of held-out games, and how much of its policy lies on the points the tree expands.

``evaluate_records`` reads the records with the reader the supervised data generator uses (SGFReader: the moves, and the value
label from the result, flipped with every ply), samples every ``stride``-th ply from ``first_ply`` at symmetry 0, and runs per
chunk of whole games

    tg_replay_run_cand   the records replayed on the LDS board: input planes and expand_node's candidate mask of every sampled ply
    the forward pass     tg_net_forward_dev (DeviceEvaluator), behind an evaluation cache when ``eval_cache`` is given
    tg_score_rows        a row record per position, added into a table of ply buckets

with planes, outputs, masks and row records in device memory.  Per chunk only the replay's flags come back; the table comes back
once at the end, the row records only with ``rows=True``.  A game the replay flags (a move onto a point that is not empty, a
record longer than the board's move record) is redone on the host board, as the data generators do, and the report names it.

MCTSNode.update_policy (mcts/node.py:86-93) copies the network's probabilities onto the candidates expand_node kept, without
masking or renormalising, so the policy mass outside the candidate mask is prior the search loses: ``prior_mass_lost``."""
import ctypes
import glob
import math
import os
from typing import List, Sequence

import numpy as np
import torch

from tamago_amd import lib as _lib
from tamago_amd.board.candidates import search_candidates
from tamago_amd.board.go_board import GoBoard
from tamago_amd.board.stone import Stone, color_value

ROW_DTYPE = np.dtype([("cand_mass", "<f8"), ("brier", "<f8"), ("p_move", "<u4"), ("rank", "<i4"), ("v_label", "<u4"),
                      ("flags", "<u4"), ("bucket", "<i4"), ("reserved", "<i4")])          # tg_score_row
BUCKET_DTYPE = np.dtype([("count", "<u8", 6), ("sum", "<f8", 4)])                          # tg_score_bucket
MOVE_IS_CANDIDATE, VALUE_HIT, INVALID, HAS_MASK = 1, 2, 4, 8


class EvalRecord:
    """One game: moves int32 [n] (padded coordinates, 0 = PASS), the value label of the record's result from BLACK's side at
    ply 0 (nn/data_generator.py: 2 - label for the plies white moves at) and a name for the report."""
    __slots__ = ("moves", "value_label", "name")

    def __init__(self, moves, value_label: int, name: str = ""):
        self.moves = np.ascontiguousarray(moves, dtype=np.int32)
        self.value_label = int(value_label)
        self.name = name


def read_record(path: str, board_size: int) -> EvalRecord:
    from tamago_amd.sgf.reader import SGFReader
    sgf = SGFReader(path, board_size)
    n = sgf.get_n_moves()
    return EvalRecord(np.fromiter(sgf.get_moves(), dtype=np.int32, count=n), sgf.get_value_label(), path)


def as_records(records_or_paths, board_size: int) -> List[EvalRecord]:
    """A directory (its *.sgf, sorted), or a sequence of paths, EvalRecords and (moves, value_label) pairs."""
    if isinstance(records_or_paths, str):
        records_or_paths = sorted(glob.glob(os.path.join(records_or_paths, "*.sgf")))
    out = []
    for i, item in enumerate(records_or_paths):
        if isinstance(item, EvalRecord):
            out.append(item)
        elif isinstance(item, str):
            out.append(read_record(item, board_size))
        else:
            moves, label = item
            out.append(EvalRecord(moves, label, f"record {i}"))
    return out


def sampled_plies(n_moves: int, stride: int, first_ply: int) -> np.ndarray:
    return np.arange(first_ply, n_moves, stride, dtype=np.int32)


def move_actions(moves: np.ndarray, board_size: int) -> np.ndarray:
    """Padded coordinates -> action indices: row-major board points 0 .. P - 1, PASS = P; no point of the board: -1 (the row
    is invalid)."""
    w = board_size + 2
    x, y = moves % w - 1, moves // w - 1
    on_board = (x >= 0) & (x < board_size) & (y >= 0) & (y < board_size)
    return np.where(moves == 0, board_size * board_size, np.where(on_board, y * board_size + x, -1)).astype(np.int32)


def chunk_games(records: Sequence[EvalRecord], stride: int, first_ply: int, chunk_rows: int):
    """Whole games per chunk, as many as fit in chunk_rows rows (one game at least): yields (first game, game count)."""
    start, rows = 0, 0
    for g, rec in enumerate(records):
        n = len(sampled_plies(len(rec.moves), stride, first_ply))
        if g > start and rows + n > chunk_rows:
            yield start, g - start
            start, rows = g, 0
        rows += n
    if len(records) > start:
        yield start, len(records) - start


def candidate_words(board: GoBoard, color, board_size: int) -> np.ndarray:
    """expand_node's candidate list on the host board as tg_replay_run_cand's bit image."""
    w = board_size + 2
    words = np.zeros((board_size * board_size + 1 + 31) // 32, dtype=np.uint32)
    for pos in search_candidates(board, color):
        a = board_size * board_size if pos == 0 else (pos // w - 1) * board_size + pos % w - 1
        words[a >> 5] |= np.uint32(1 << (a & 31))
    return words


def host_rows(record: EvalRecord, plies: np.ndarray, board_size: int, superko: bool, device_index: int = 0):
    """The planes (device tensor) and candidate masks of one record's sampled plies by the host path: the Python board and the
    featurise kernel - what a flagged game gets."""
    from tamago_amd.nn.feature import featurize_batch
    board = GoBoard(board_size, 7.0, superko)
    cells, to_move, prev, n_moves, masks = [], [], [], [], []
    color, k = Stone.BLACK, 0
    for i, pos in enumerate(record.moves):
        if k < len(plies) and plies[k] == i:
            cells.append(np.array(board.get_board_data(), dtype=np.uint8))
            to_move.append(color_value(color))
            prev.append(board.prev_move(1))
            n_moves.append(board.moves)
            masks.append(candidate_words(board, color, board_size))
            k += 1
        if k == len(plies):
            break
        board.put_stone(int(pos), color)
        color = Stone.get_opponent_color(color)
    planes = featurize_batch(board_size, np.stack(cells), np.array(to_move), np.array(prev), np.array(n_moves),
                             np.zeros(len(cells), dtype=np.int64), device_index)
    return planes, np.stack(masks)


def report_from_table(table: np.ndarray, bucket_width: int) -> dict:
    """Totals and per-bucket statistics from the table of tg_score_rows (BUCKET_DTYPE [n_buckets])."""
    def stats(count, sums):
        rows = int(count[0])
        mean = (lambda v: float(v) / rows) if rows else (lambda v: None)
        return {"rows": rows, "invalid_rows": int(count[5]),
                "top1": mean(count[1]), "top5": mean(count[2]),
                "policy_loss": mean(sums[0]), "value_loss": mean(sums[2]),
                "value_hit_rate": mean(count[4]), "brier": mean(sums[3]),
                "prior_mass_on_candidates": mean(sums[1]),
                "prior_mass_lost": (1.0 - mean(sums[1])) if rows else None,
                "moves_never_expanded": mean(count[3])}
    buckets = []
    for b in range(len(table)):
        entry = {"first_ply": b * bucket_width, "last_ply": (b + 1) * bucket_width - 1 if b + 1 < len(table) else None}
        entry.update(stats(table["count"][b], table["sum"][b]))
        buckets.append(entry)
    total_count = table["count"].sum(axis=0)
    total_sums = [math.fsum(float(v) for v in table["sum"][:, s]) for s in range(4)]
    return {"totals": stats(total_count, total_sums), "buckets": buckets}


def evaluate_records(network, records_or_paths, board_size: int, *, stride: int = 1, first_ply: int = 0, bucket_width: int = 10,
                     n_buckets: int = 32, superko: bool = False, chunk_rows: int = 65536, device: int = 0, rows: bool = False,
                     eval_cache=None, timing: dict = None) -> dict:
    """See the module docstring.  network: a DualNet of ``board_size`` on ``cuda:device``.  Returns the report: ``totals`` and
    ``buckets`` (rows, top1, top5, policy_loss, value_loss, value_hit_rate, brier, prior_mass_on_candidates, prior_mass_lost,
    moves_never_expanded, invalid_rows), ``games``, ``positions``, ``host_games`` (the names of the games redone on the host),
    ``range_fallbacks`` and the settings; with ``rows=True`` also ``rows`` (ROW_DTYPE [positions], in record order) and
    ``row_game`` / ``row_ply``.  timing (measurement only): a dict that receives the milliseconds between timed events around
    the three stages, added up over the chunks - ``replay_ms`` (upload, replay_cand_kernel, flags back, flagged games on the host, the rows' moves and classes going up), ``forward_ms``,
    ``score_ms``."""
    from tamago_amd.mcts.engine import evaluator_for
    if stride < 1 or first_ply < 0 or chunk_rows < 1:
        raise ValueError("stride >= 1, first_ply >= 0 and chunk_rows >= 1")
    if bucket_width < 1 or n_buckets < 1:
        raise ValueError("bucket_width >= 1 and n_buckets >= 1")
    records = as_records(records_or_paths, board_size)
    lib = _lib.load()
    dev = torch.device("cuda", device)
    A = board_size * board_size + 1
    mask_words = (A + 31) // 32
    evaluator = evaluator_for(network, device, eval_cache)
    fallbacks_before = network.range_fallbacks() if hasattr(network, "range_fallbacks") else 0
    handle = ctypes.c_void_p()
    _lib.check(lib.tg_replay_create(board_size, device, ctypes.byref(handle)), "tg_replay_create")
    host_games, kept_rows, row_game, row_ply = [], [], [], []
    positions = 0
    marks = []

    def mark():
        if timing is not None:
            marks.append(torch.cuda.Event(enable_timing=True))
            marks[-1].record(torch.cuda.current_stream(dev))
    try:
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            table = torch.zeros(n_buckets * BUCKET_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            first = True
            for g0, count in chunk_games(records, stride, first_ply, chunk_rows):
                chunk = records[g0:g0 + count]
                plies = [sampled_plies(len(r.moves), stride, first_ply) for r in chunk]
                offsets = np.zeros(count + 1, dtype=np.int64)
                np.cumsum([len(r.moves) for r in chunk], out=offsets[1:])
                s_off = np.zeros(count + 1, dtype=np.int64)
                np.cumsum([len(p) for p in plies], out=s_off[1:])
                n = int(s_off[-1])
                if n == 0:
                    continue
                moves = np.ascontiguousarray(np.concatenate([r.moves for r in chunk]), dtype=np.int32)
                ply = np.ascontiguousarray(np.concatenate(plies), dtype=np.int32)
                sym = np.zeros(n, dtype=np.int8)
                flags = np.zeros(count, dtype=np.int32)
                planes = torch.empty((n, 6, board_size, board_size), dtype=torch.float32, device=dev)
                cand = torch.empty((n, mask_words), dtype=torch.int32, device=dev)
                mark()
                _lib.check(lib.tg_replay_run_cand(handle, moves.ctypes.data, offsets.ctypes.data, count, ply.ctypes.data,
                                                  sym.ctypes.data, s_off.ctypes.data, planes.data_ptr(), flags.ctypes.data,
                                                  int(bool(superko)), cand.data_ptr(), stream), "tg_replay_run_cand")
                for g in np.nonzero(flags)[0]:
                    host_games.append(chunk[g].name or f"record {g0 + g}")
                    if s_off[g + 1] > s_off[g]:
                        h_planes, h_masks = host_rows(chunk[g], plies[g], board_size, superko, device)
                        planes[s_off[g]:s_off[g + 1]] = h_planes
                        cand[s_off[g]:s_off[g + 1]] = torch.from_numpy(h_masks.view(np.int32)).to(dev)
                # what the record says of every row: the move played, the result from the mover's side, the ply
                move = np.concatenate([move_actions(r.moves[p], board_size) for r, p in zip(chunk, plies)])
                cls = np.concatenate([np.where(p % 2 == 0, r.value_label, 2 - r.value_label) for r, p in zip(chunk, plies)])
                meta = torch.from_numpy(np.ascontiguousarray(np.stack([move, cls, ply]), dtype=np.int32)).to(dev)
                mark()
                policy, value = evaluator(planes, False)
                mark()
                row_buf = torch.empty(n * ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                _lib.check(lib.tg_score_rows(policy.data_ptr(), value.data_ptr(), cand.data_ptr(), meta[0].data_ptr(),
                                             meta[1].data_ptr(), meta[2].data_ptr(), n, A, bucket_width, n_buckets,
                                             row_buf.data_ptr(), table.data_ptr(), 1 if first else 0, stream), "tg_score_rows")
                mark()
                first = False
                positions += n
                if rows:
                    kept_rows.append(row_buf.cpu().numpy().view(ROW_DTYPE))
                    row_game.append(np.repeat(np.arange(g0, g0 + count), np.diff(s_off)))
                    row_ply.append(ply)
            table_host = table.cpu().numpy().view(BUCKET_DTYPE)
            if timing is not None:
                torch.cuda.synchronize(dev)
                for k, name in enumerate(("replay_ms", "forward_ms", "score_ms")):      # four marks a chunk
                    timing[name] = timing.get(name, 0.0) + sum(marks[i + k].elapsed_time(marks[i + k + 1])
                                                               for i in range(0, len(marks), 4))
    finally:
        lib.tg_replay_destroy(handle)
    report = report_from_table(table_host, bucket_width)
    report.update({"board_size": board_size, "games": len(records), "positions": positions, "stride": stride, "first_ply": first_ply,
                   "bucket_width": bucket_width, "n_buckets": n_buckets, "superko": bool(superko),
                   "host_games": host_games,
                   "range_fallbacks": (network.range_fallbacks() - fallbacks_before) if hasattr(network, "range_fallbacks") else 0})
    if rows:
        report["rows"] = np.concatenate(kept_rows) if kept_rows else np.zeros(0, dtype=ROW_DTYPE)
        report["row_game"] = np.concatenate(row_game) if row_game else np.zeros(0, dtype=np.int64)
        report["row_ply"] = np.concatenate(row_ply) if row_ply else np.zeros(0, dtype=np.int32)
        report["table"] = table_host
    return report


def format_report(report: dict) -> str:
    """The totals and the buckets that hold rows, as a table."""
    def cell(v, fmt):
        return "-" if v is None else format(v, fmt)
    head = f"{'plies':>9} {'rows':>8} {'top1':>6} {'top5':>6} {'p-loss':>7} {'v-loss':>7} {'v-hit':>6} {'brier':>6} " \
           f"{'on-cand':>8} {'lost':>8} {'unexp':>6} {'invalid':>7}"
    lines = [f"{report['games']} games, {report['positions']} positions at {report['board_size']}x{report['board_size']}, "
             f"stride {report['stride']} from ply {report['first_ply']}, superko {'on' if report['superko'] else 'off'}; "
             f"{len(report['host_games'])} games redone on the host", head]
    entries = [("all", report["totals"])]
    for b in report["buckets"]:
        if b["rows"] or b["invalid_rows"]:
            entries.append((f"{b['first_ply']}-{'' if b['last_ply'] is None else b['last_ply']}", b))
    for name, e in entries:
        lines.append(f"{name:>9} {e['rows']:>8} {cell(e['top1'], '6.3f')} {cell(e['top5'], '6.3f')} {cell(e['policy_loss'], '7.4f')} "
                     f"{cell(e['value_loss'], '7.4f')} {cell(e['value_hit_rate'], '6.3f')} {cell(e['brier'], '6.4f')} "
                     f"{cell(e['prior_mass_on_candidates'], '8.5f')} {cell(e['prior_mass_lost'], '8.5f')} "
                     f"{cell(e['moves_never_expanded'], '6.4f')} {e['invalid_rows']:>7}")
    return "\n".join(lines)
