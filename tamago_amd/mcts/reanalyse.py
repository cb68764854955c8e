"""Reanalysis: stored positions searched again, every position as its own Gumbel tree, many trees in lock-step on one
SearchEngine; the result is each root's improved policy as a training target (tg_search_read_improved_policy).

No reference counterpart: the reference searches a position once, in self-play, and keeps the improved policy of that
search as "%.3e" text in the game record (sgf/selfplay_record.py:56 -> nn/feature.py:80-102).  The equivalence contract
(the analysis module's, for Gumbel): position k reanalysed with seed s_k gives the root of

    np.random.set_state(np.random.RandomState(s_k).get_state())
    tree = MCTSTree(network, tree_size=visits + 16)
    tree.generate_move_with_sequential_halving(board_k, color_k, TimeManager(TimeControl.STRICT_PLAYOUT, visits), True)
    tree.get_root()

whatever the number of trees per engine (max_trees) and whatever else shares the launch:
- every tree draws from its own stream, np.random.RandomState(s_k).get_state(): the root's Dirichlet prior, its Gumbel
  noise, the priors of the nodes its descents expand;
- every tree follows its own schedule get_candidates_and_visit_pairs(min(children, MAX_CONSIDERED_NODES), visits); a tree
  whose schedule is shorter than the longest of its chunk sits the later phases out ((0, 0): no descent, no draw), the way
  tg_selfplay_schedule handles boards with fewer candidates;
- the row of position k is calculate_improved_policy (node.py:281-321) of that root, float64 rounded once to float32, in
  the network's output order, np.float32(1e-18) where the root has no child - an rl_data row without the text round trip.
It holds provided the DualNet takes no f16 range fallback (a hot position's exact redo covers the positions launched with
it): Reanalysis.range_fallbacks reports the count, 0 for a healthy network.  unique_leaves=True evaluates each distinct
leaf of a phase once (SearchEngine.gumbel_phase(unique=True)): same trees, same rows, under the same caveat."""
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from tamago_amd.board.go_board import GoBoard
from tamago_amd.mcts.analysis import default_max_trees, plan_chunks, tree_size_for
from tamago_amd.mcts.constant import MAX_CONSIDERED_NODES, PLAYOUTS
from tamago_amd.mcts.engine import SearchEngine, evaluator_for
from tamago_amd.mcts.sequential_halving import get_candidates_and_visit_pairs

# what selfplay_shard gives its boards (selfplay/worker.py: GoBoard(..., check_superko=True))
SELFPLAY_CHECK_SUPERKO = True


@dataclass
class Reanalysis:
    """rows: float32 [n, S * S + 1] in device memory, one improved-policy row per position.  moves [n]: the move
    select_move_by_sequential_halving_for_root(PLAYOUTS) picks (padded coordinate, PASS 0).  visits [n]: the root's
    node_visits.  values [n]: calculate_value_evaluation of that move's child (what generate_move_with_sequential_halving
    tests for resignation).  raw_values [n]: the network's value of the root.  forward_positions: positions handed to the
    network; range_fallbacks: forward launches redone in exact fp32 meanwhile (module docstring).  seconds: host wall time
    of root set-up / search / read-out, summed over the chunks."""
    rows: torch.Tensor
    moves: List[int]
    visits: List[int]
    values: List[float]
    raw_values: List[float]
    forward_positions: int = 0
    range_fallbacks: int = 0
    seconds: Optional[dict] = None
    host_roots: int = 0           # reanalyse_records: positions a launch flagged, staged from a host board instead


def tree_schedules(children: Sequence[int], visits: int) -> Tuple[List[List[int]], List[List[int]]]:
    """Per-phase (num_considered, max_count) lists over trees with `children` root children each: tree t follows
    get_candidates_and_visit_pairs(min(children[t], MAX_CONSIDERED_NODES), visits) (tree.py:337-343); phases past the end of
    its schedule are (0, 0)."""
    pairs = [list(get_candidates_and_visit_pairs(min(int(c), MAX_CONSIDERED_NODES), visits).items()) for c in children]
    phases = max((len(p) for p in pairs), default=0)
    considered = [[p[ph][0] if ph < len(p) else 0 for p in pairs] for ph in range(phases)]
    counts = [[p[ph][1] if ph < len(p) else 0 for p in pairs] for ph in range(phases)]
    return considered, counts


def symmetric_rows(size: int, rows: torch.Tensor, sym) -> torch.Tensor:
    """rows [n, S * S + 1] (symmetry 0) -> the rows a sample under symmetry sym[k] has: slot q holds the value of the move
    symmetry_pos_table(size)[sym[k]][q], as generate_rl_target_data orders a target."""
    from tamago_amd.nn.feature import symmetry_pos_table
    w = size + 2
    pos = symmetry_pos_table(size)[np.asarray(sym, dtype=np.int64).reshape(-1)]
    slot = np.where(pos == 0, size * size, (pos // w - 1) * size + pos % w - 1)
    return torch.gather(rows, 1, torch.from_numpy(slot).to(rows.device))


def _check(network, positions, visits, seeds):
    size = positions[0][0].board_size
    if any(board.board_size != size for board, _ in positions):
        raise ValueError("reanalyse_positions: positions of several board sizes")
    net_size = getattr(network, "board_size", None)
    if net_size is not None and net_size != size:
        raise ValueError(f"network is built for {net_size}x{net_size}, boards are {size}x{size}")
    if visits < 1:
        raise ValueError("reanalyse_positions: visits must be at least 1")
    seeds = list(range(len(positions))) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != len(positions):
        raise ValueError("reanalyse_positions: one seed per position")
    return size, seeds


def set_chunk_roots(engine, positions, indices, seeds, records=None, check_superko: bool = SELFPLAY_CHECK_SUPERKO):
    """The one place where a chunk's roots and streams are set: tree k gets position indices[k] and the stream of
    seeds[indices[k]].  records None: positions are (board, colour) pairs, one set_root each.  Otherwise positions are
    (record index, ply) members of `records` and the roots are written on the device (SearchEngine.set_roots_from_records,
    seed_trees); the trees a launch flags are staged from a host board replayed for their record only (one replay per
    flagged record).  Returns the trees that were set up from a host board."""
    if records is None:
        for k, index in enumerate(indices):
            board, color = positions[index]
            engine.set_root(k, board, color, np.random.RandomState(seeds[index]).get_state())
        return list(range(len(indices)))
    from tamago_amd.mcts.record_roots import host_record_positions
    flags = engine.set_roots_from_records(records, [positions[index] for index in indices])
    engine.seed_trees([seeds[index] for index in indices])
    flagged = {}
    for k in np.nonzero(flags)[0]:
        record, ply = positions[indices[k]]
        flagged.setdefault(int(record), []).append((int(ply), int(k)))
    for record, rows in flagged.items():
        rows.sort()
        replayed = host_record_positions(records[record], [ply for ply, _ in rows], engine.S, check_superko)
        for (_, k), (board, color) in zip(rows, replayed):
            engine.set_root(k, board, color)
    return [int(k) for k in np.nonzero(flags)[0]]


def searched_chunks(network, positions, visits: int, seeds, max_trees: Optional[int] = None,
                    check_superko: bool = SELFPLAY_CHECK_SUPERKO, unique_leaves: bool = False, device_index: int = 0,
                    seconds: Optional[dict] = None, records=None, board_size: Optional[int] = None,
                    host_roots: Optional[list] = None):
    """The lock-step searches behind reanalyse_positions, chunk by chunk: yields (engine, first, end) with the trees
    0 .. end - first - 1 of `engine` searched for positions[first:end] (the spare trees of a short last chunk hold copies of
    its last position).  The engine is reused from chunk to chunk and closed when the generator ends; `seconds`, if given,
    collects the host wall time of "setup" and "search".
    records: positions are (record index, ply) members of these records of size board_size (reanalyse_records);
    host_roots, if given, collects the indices of the positions that were set up from a host board."""
    import time
    size = positions[0][0].board_size if records is None else board_size
    trees, chunks = plan_chunks(len(positions), max_trees or default_max_trees(size, visits))
    # every phase is one mini-batch of num_considered * max_count <= visits leaves per tree
    engine = SearchEngine(size, trees, tree_size_for(visits), visits, evaluator_for(network, device_index), False,
                          check_superko, device_index)
    try:
        for lo, hi in chunks:
            t0 = time.perf_counter()
            indices = [lo + min(k, hi - lo - 1) for k in range(trees)]
            by_host = set_chunk_roots(engine, positions, indices, seeds, records, check_superko)
            if host_roots is not None:
                host_roots.extend(lo + k for k in by_host if k < hi - lo)
            engine.root_eval(use_logit=True)
            engine.set_gumbel_noise()
            t1 = time.perf_counter()
            for considered, counts in zip(*tree_schedules(engine.root_children, visits)):
                engine.ensure_capacity(max(a * b for a, b in zip(considered, counts)))
                engine.gumbel_phase(considered, counts, unique=unique_leaves)
            if seconds is not None:
                torch.cuda.synchronize(engine.device)
                seconds["setup"] = seconds.get("setup", 0.0) + t1 - t0
                seconds["search"] = seconds.get("search", 0.0) + time.perf_counter() - t1
            yield engine, lo, hi
    finally:
        engine.close()


def reanalyse_positions(network, positions: Sequence[Tuple[GoBoard, object]], visits: int,
                        seeds: Optional[Sequence[int]] = None, max_trees: Optional[int] = None,
                        check_superko: bool = SELFPLAY_CHECK_SUPERKO, unique_leaves: bool = False,
                        device_index: int = 0) -> Reanalysis:
    """Reanalyse (board, colour to move) pairs of one board size, one Gumbel tree of `visits` simulations per position (see
    the module docstring for the contract).  seeds default to 0, 1, 2, ...; max_trees defaults to default_max_trees.
    check_superko must match the boards' own setting (as MCTSTree takes it from the board)."""
    positions = list(positions)
    if not positions:
        return _no_positions(device_index)
    size, seeds = _check(network, positions, visits, seeds)
    return _reanalyse(network, positions, size, visits, seeds, max_trees, check_superko, unique_leaves, device_index)


def reanalyse_records(network, records: Sequence, members: Sequence[Tuple[int, int]], visits: int,
                      seeds: Optional[Sequence[int]] = None, max_trees: Optional[int] = None,
                      check_superko: bool = SELFPLAY_CHECK_SUPERKO, unique_leaves: bool = False,
                      device_index: int = 0) -> Reanalysis:
    """reanalyse_positions with position k given as members[k] = (record index, ply) in place of a board: the position
    before move `ply` of records[record index] (a move list, colours alternating from black, or (moves, colours):
    mcts/record_roots.py; ply == the record's length: the final position), on a board of the network's size.  One Gumbel
    tree of `visits` simulations per position (see the module docstring for the contract); seeds default to 0, 1, 2, ...;
    max_trees defaults to default_max_trees.  No position is replayed or copied on the host: the roots are written on the
    device from the records, chunk by chunk (SearchEngine.set_roots_from_records), and a chunk's streams are seeded in one
    call.  A position a launch flags (a record with a move onto an occupied point, or one longer than a board records) is
    staged from a host board replayed for that record only - Reanalysis.host_roots counts them - so its row is the host
    path's as well."""
    members = [(int(r), int(p)) for r, p in members]
    if not members:
        return _no_positions(device_index)
    size = getattr(network, "board_size", None)
    if size is None:
        raise ValueError("reanalyse_records: the network does not say its board size")
    if visits < 1:
        raise ValueError("reanalyse_records: visits must be at least 1")
    seeds = list(range(len(members))) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != len(members):
        raise ValueError("reanalyse_records: one seed per position")
    from tamago_amd.mcts.record_roots import pack_record_roots
    pack_record_roots(records, members)               # (bad input raises here, before an engine exists)
    return _reanalyse(network, members, size, visits, seeds, max_trees, check_superko, unique_leaves, device_index, records)


def _no_positions(device_index: int) -> Reanalysis:
    device = torch.device("cuda", device_index)
    return Reanalysis(torch.empty((0, 0), dtype=torch.float32, device=device), [], [], [], [], 0, 0,
                      {"setup": 0.0, "search": 0.0, "readout": 0.0})


def _reanalyse(network, positions, size, visits, seeds, max_trees, check_superko, unique_leaves, device_index,
               records=None) -> Reanalysis:
    """The read-out loop over searched_chunks that reanalyse_positions (records None) and reanalyse_records share."""
    import time
    device = torch.device("cuda", device_index)
    seconds = {"setup": 0.0, "search": 0.0, "readout": 0.0}
    fallbacks0 = network.range_fallbacks() if hasattr(network, "range_fallbacks") else 0
    rows = torch.empty((len(positions), size * size + 1), dtype=torch.float32, device=device)
    chunk_rows = None
    moves, root_visits, values, raw_values = [], [], [], []
    forwarded = 0
    host_roots = [] if records is not None else None
    for engine, lo, hi in searched_chunks(network, positions, visits, seeds, max_trees, check_superko, unique_leaves,
                                          device_index, seconds, records, size, host_roots):
        t0 = time.perf_counter()
        chunk_rows = engine.read_improved_policy(chunk_rows)
        rows[lo:hi] = chunk_rows[:hi - lo]
        stats = engine.read_root_stats()
        for k in range(hi - lo):
            root = engine.root_view(stats, k)
            index = root.select_move_by_sequential_halving_for_root(PLAYOUTS)
            moves.append(int(root.get_child_move(index)))
            root_visits.append(int(root.node_visits))
            values.append(float(root.calculate_value_evaluation(index)))
            raw_values.append(float(root.raw_value))
        torch.cuda.synchronize(device)
        seconds["readout"] += time.perf_counter() - t0
        forwarded = engine.forward_positions
    fallbacks = (network.range_fallbacks() - fallbacks0) if hasattr(network, "range_fallbacks") else 0
    return Reanalysis(rows, moves, root_visits, values, raw_values, forwarded, fallbacks, seconds,
                      len(host_roots) if host_roots is not None else 0)
