"""Lock-step driver of T device-resident search trees (host side of the C ABI in
include/tamago_hip.h).  MCTSTree (one tree, the reference's API) and the self-play worker
(many boards per GPU) are thin layers over this class.

Random streams: the reference consumes numpy's legacy MT19937 stream in program order -
n doubles per node expansion (Dirichlet(1..1) prior, mcts/tree.py:509-519) and A doubles
per Gumbel move (mcts/node.py:275-278).  ``ExpStream`` reproduces that stream position by
position with ``RandomState.standard_exponential`` / ``gumbel`` (the very C functions
numpy's dirichlet / gumbel use, so the doubles are bit-identical) and hands windows of it
to the device, which consumes them with a cursor.
"""
import ctypes
import math
import os
from typing import List, Optional

import numpy as np
import torch

from tamago_amd import lib as _lib
from tamago_amd.board.go_board import GoBoard, zobrist_keys
from tamago_amd.board.stone import color_value
from tamago_amd.mcts.node import MCTSNode


# tg_best_move (include/tamago_hip.h), one per tree out of SearchEngine.best_moves; the bits of its status
BEST_MOVE = np.dtype([("num_children", "<i4"), ("move", "<i4"), ("best", "<i4"), ("visits", "<i4"), ("value_sum", "<f8"),
                      ("node_visits", "<i4"), ("status", "<i4")])
assert BEST_MOVE.itemsize == 32
BEST_SAT_OUT, BEST_NO_ROOT, BEST_TREE_ERROR = 1, 2, 4
# tg_advance_record (include/tamago_hip.h): what became of a tree whose root was advanced by a move
ADVANCE = np.dtype([("kept_visits", "<i4"), ("kept_nodes", "<i4"), ("num_children", "<i4"), ("status", "<i4")])
assert ADVANCE.itemsize == 16
ADVANCE_LEFT_ALONE, ADVANCE_OCCUPIED = 1, 2


class ExpStream:
    """Position-addressable view of a legacy numpy stream as exponentials e_i = -log(1-u_i).

    Gumbel noise comes from the same values: numpy's legacy gumbel is
    ``loc - scale*log(-log(1-u))`` = ``-log(e_i)`` with the same libm ``log`` (verified
    bit-for-bit in tests/test_host_rng.py), so no second generator has to be positioned."""

    def __init__(self, state):
        self.origin = state                       # RandomState state at position 0
        self.gen = np.random.RandomState()        # generator at position buf0 + len(buf)
        self.gen.set_state(state)
        self.buf = np.empty(0, dtype=np.float64)  # exponentials for positions [buf0, buf0+len)
        self.buf0 = 0
        self.pos = 0                              # next unconsumed position

    def window(self, need: int) -> np.ndarray:
        have = self.buf0 + len(self.buf) - self.pos
        if have < need:
            extra = self.gen.standard_exponential(need - have)
            self.buf = np.concatenate([self.buf[self.pos - self.buf0:], extra])
            self.buf0 = self.pos
        off = self.pos - self.buf0
        return self.buf[off:off + need]

    def consume(self, count: int):
        self.pos += int(count)

    def gumbel(self, size: int) -> np.ndarray:
        """Next `size` positions as Gumbel(0,1) noise (node.py:278)."""
        noise = np.array([-math.log(v) for v in self.window(size)], dtype=np.float64)
        self.pos += size
        return noise

    def final_state(self):
        """Generator state after everything consumed so far (O(pos): per-move streams only)."""
        g = np.random.RandomState()
        g.set_state(self.origin)
        if self.pos:
            g.random_sample(self.pos)             # one double per position
        return g.get_state()


class LibStream:
    """Handle on a library-owned legacy stream (tg_search_seed_stream): the C side generates,
    stages and uploads the draws; Python only seeds it and reads the state back."""

    def __init__(self, engine, tree: int, state):
        """state None: the stream has been seeded already (SearchEngine.seed_trees)."""
        self.engine = engine
        self.tree = tree
        if state is None:
            return
        key = np.ascontiguousarray(state[1], dtype=np.uint32)
        assert state[0] == "MT19937" and key.shape == (624,)
        _lib.check(engine.lib.tg_search_seed_stream(engine.handle, tree, key.ctypes.data, int(state[2])),
                   "tg_search_seed_stream")

    def final_state(self):
        """numpy state after everything this tree has consumed so far."""
        key = np.zeros(624, dtype=np.uint32)
        pos = ctypes.c_int(0)
        _lib.check(self.engine.lib.tg_search_stream_state(self.engine.handle, self.tree, key.ctypes.data,
                                                          ctypes.byref(pos)), "tg_search_stream_state")
        return ("MT19937", key, int(pos.value), 0, 0.0)


class LibrarySource:
    """Where an engine's draws come from: the library-owned streams.  The C side generates and windows the draws
    (tg_search_feed_streams / advance_streams / draw_noise); Python seeds them and says when a new window is due."""
    chainable = True                              # one window for a whole chained search: tg_search_puct_chain feeds it

    def __init__(self, engine):
        self.engine = engine
        self.invalid = True                       # the next feed starts a new window whatever is left of the last

    def seed(self, tree: int, state):
        self.engine.streams[tree] = LibStream(self.engine, tree, state)
        self.invalid = True

    def seed_all(self, seeds):
        eng = self.engine
        words = np.asarray(seeds, dtype=np.uint32)
        _lib.check(eng.lib.tg_search_seed_streams(eng.handle, words.ctypes.data), "tg_search_seed_streams")
        eng.streams = [LibStream(eng, k, None) for k in range(eng.T)]
        self.invalid = True

    def invalidate(self):
        self.invalid = True

    def take_invalid(self) -> int:
        """The force flag of the feed that goes out now (the library tracks the window from there on)."""
        force, self.invalid = int(self.invalid), False
        return force

    def feed(self, need: int):
        eng = self.engine
        _lib.check(eng.lib.tg_search_feed_streams(eng.handle, need, self.take_invalid()), "tg_search_feed_streams")

    def collect(self):
        eng = self.engine
        delta = np.zeros(eng.T, dtype=np.int64)
        _lib.check(eng.lib.tg_search_advance_streams(eng.handle, delta.ctypes.data), "tg_search_advance_streams")
        return delta

    def noise(self):
        eng = self.engine
        noise = np.empty((eng.T, eng.A), dtype=np.float64)
        _lib.check(eng.lib.tg_search_draw_noise(eng.handle, noise.ctypes.data), "tg_search_draw_noise")
        return noise


class HostSource:
    """Where an engine's draws come from: numpy on the host (ExpStream per tree), handed over with tg_search_set_rng /
    tg_search_rng_consumed / tg_search_set_noise - the calls a numpy-side host would make."""
    chainable = False

    def __init__(self, engine):
        self.engine = engine
        self.left = 0                             # draws of the uploaded window no tree has read (0: the next feed uploads)
        self.cap = 0
        self.used = np.zeros(engine.T, dtype=np.int64)
        self.pool = None

    def seed(self, tree: int, state):
        self.engine.streams[tree] = ExpStream(state)
        self.left = 0

    def seed_all(self, seeds):
        for k, seed in enumerate(seeds):
            self.seed(k, np.random.RandomState(seed).get_state())

    def invalidate(self):
        self.left = 0

    def take_invalid(self) -> int:
        return int(self.left == 0)

    def feed(self, need: int):
        eng = self.engine
        if self.left >= need:
            return
        self.left = self.cap = need
        self.used = np.zeros(eng.T, dtype=np.int64)
        win = np.empty((eng.T, need), dtype=np.float64)

        def fill(t):
            win[t] = eng.streams[t].window(need)

        if eng.T >= 8:
            # numpy's legacy generators release the GIL while filling, so threads scale
            if self.pool is None:
                from concurrent.futures import ThreadPoolExecutor
                self.pool = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))
            list(self.pool.map(fill, range(eng.T)))
        else:
            for t in range(eng.T):
                fill(t)
        _lib.check(eng.lib.tg_search_set_rng(eng.handle, win.ctypes.data, need, need), "tg_search_set_rng")

    def collect(self):
        eng = self.engine
        used = np.zeros(eng.T, dtype=np.int64)
        _lib.check(eng.lib.tg_search_rng_consumed(eng.handle, used.ctypes.data), "tg_search_rng_consumed")
        # the device cursor is cumulative within the active window
        delta = used - self.used
        self.used = used
        for s, c in zip(eng.streams, delta):
            s.consume(int(c))
        self.left = self.cap - int(used.max()) if len(used) else 0
        return delta

    def noise(self):
        eng = self.engine
        self.left = 0                             # the noise sits between two windows
        noise = np.empty((eng.T, eng.A), dtype=np.float64)
        for t, s in enumerate(eng.streams):
            noise[t] = s.gumbel(eng.A)
        _lib.check(eng.lib.tg_search_set_noise(eng.handle, noise.ctypes.data), "tg_search_set_noise")
        return noise


class HostEvaluator:
    """Adapter for any object with the DualNet host API (inference /
    inference_with_policy_logits on CPU tensors): planes are copied to the host, results
    back to the device.  Used for stand-in evaluators in the parity tests and for drop-in
    compatibility with arbitrary networks."""

    def __init__(self, network, device):
        self.network = network
        self.device = device
        self.batches: List[int] = []

    def __call__(self, planes: torch.Tensor, want_logits: bool):
        x = planes.cpu()
        self.batches.append(x.shape[0])
        if want_logits:
            policy, value = self.network.inference_with_policy_logits(x)
        else:
            policy, value = self.network.inference(x)
        return (policy.to(self.device, torch.float32).contiguous(),
                value.to(self.device, torch.float32).contiguous())


class DeviceEvaluator:
    """DualNet forward without a host hop (tg_net_forward_dev)."""

    def __init__(self, network):
        self.network = network
        self.batches: List[int] = []

    def __call__(self, planes: torch.Tensor, want_logits: bool):
        self.batches.append(planes.shape[0])
        return self.network.forward_device(planes, want_logits)


def evaluator_for(network, device_index: int = 0, eval_cache=None):
    """DualNet -> DeviceEvaluator (no host hop); any other network -> HostEvaluator.  eval_cache (an nn.eval_cache.EvalCache
    of this network's outputs): the evaluator behind that cache - a CachedEvaluator, which the chained calls do
    not take (can_chain), so the drivers go mini-batch by mini-batch."""
    from tamago_amd.nn.network.dual_net import DualNet
    if isinstance(network, DualNet):
        inner = DeviceEvaluator(network)
    else:
        inner = HostEvaluator(network, torch.device("cuda", device_index))
    if eval_cache is None:
        return inner
    from tamago_amd.nn.eval_cache import CachedEvaluator
    return CachedEvaluator(inner, eval_cache)


def continue_pv(pv_list, index: int, read_node):
    """mcts/tree.py:462-473 get_best_move_sequence from node `index` on, one read_node(index) -> MCTSNode per node: the host
    end of a principal variation that tg_search_read_analysis cut at its max_depth."""
    while True:
        node = read_node(index)
        if node.node_visits == 0:
            return pv_list
        best = node.get_best_move_index()
        pv_list.append(node.action[best])
        index = int(node.children_index[best])
        if index == -1:
            return pv_list


class SearchEngine:
    def __init__(self, board_size: int, num_trees: int, tree_size: int, batch_size: int,
                 evaluator, cgos_mode: bool = False, check_superko: bool = False,
                 device_index: int = 0, host_streams: bool = False):
        """host_streams: generate the random draws in Python (ExpStream + tg_search_set_rng /
        tg_search_rng_consumed / tg_search_set_noise - the calls a numpy-side host would make)
        instead of the library-owned streams; same results, kept for that boundary's tests."""
        self.lib = _lib.load()
        self.S = board_size
        self.P = board_size * board_size
        self.A = self.P + 1
        self.T = num_trees
        self.N = tree_size
        self.K = batch_size
        self.device = torch.device("cuda", device_index)
        self.evaluator = evaluator
        cfg = _lib.SearchConfig(board_size, num_trees, tree_size, batch_size, int(cgos_mode),
                                int(check_superko), device_index, 0)
        handle = ctypes.c_void_p()
        _lib.check(self.lib.tg_search_create(ctypes.byref(cfg), ctypes.byref(handle)),
                   "tg_search_create")
        self.handle = handle
        keys = zobrist_keys(board_size)
        _lib.check(self.lib.tg_search_set_zobrist(self.handle, keys.ctypes.data, keys.size),
                   "tg_search_set_zobrist")
        self.planes = torch.empty((num_trees * batch_size, 6, board_size, board_size),
                                  dtype=torch.float32, device=self.device)
        self.host_streams = host_streams or bool(os.environ.get("TG_HOST_STREAMS"))
        self.streams: List[Optional[ExpStream]] = [None] * num_trees      # per tree, what the source seeded: final_state()
        self.source = HostSource(self) if self.host_streams else LibrarySource(self)
        self.node_bound = 0                       # upper bound of nodes in use in any tree
        self.forward_positions = 0                # positions handed to the evaluator by _evaluate_and_backup
        self.forward_positions_by_group = {}      # group -> positions its evaluator was handed by the grouped calls
        self.group_counts = self.group_offsets = None     # the segments of the last group_live()
        self.unique_caps = None                   # plane range per tree of the last unique gumbel_phase
        self._halting = False                     # halt words have been used (the planes buffer was zero-filled then)
        self.live_count = None                    # trees the last compact_live() found live
        self._budget = None                       # the visit totals in force (set_budget)
        self._kept = None                         # (nodes [T], root visits [T]) each tree held after the last advance: what a
                                                  # budgeted search can still add to it is total - visits nodes (_budget_need)

    def close(self):
        if self.handle is not None:
            self.lib.tg_search_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---------------------------------------------------------------------------------
    def set_root(self, tree: int, board: GoBoard, color, rng_state=None):
        """Position + (optionally) the legacy-RNG state this tree draws from."""
        assert board.board_size == self.S
        cells = np.ascontiguousarray(board.cells, dtype=np.uint8)
        hist = np.ascontiguousarray(board.rec_hash[:min(board.moves, board.max_records)])
        pos = _lib.RootPosition(cells.ctypes.data, hist.ctypes.data,
                                ctypes.c_uint64(int(board.hash)), board.moves, board.ko_pos,
                                board.ko_move, board.prev_move(1), board.prev_move(2),
                                color_value(color))
        _lib.check(self.lib.tg_search_set_root(self.handle, tree, ctypes.byref(pos)),
                   "tg_search_set_root")
        if self._kept is not None:                # (a new position: the tree is fresh)
            self._kept[0][tree] = self._kept[1][tree] = 0
        if rng_state is not None:
            self.set_stream(tree, rng_state)

    def set_stream(self, tree: int, rng_state):
        """(Re)seed the legacy stream tree `tree` draws from (np.random.get_state() layout)."""
        self.source.seed(tree, rng_state)

    def set_roots_from_records(self, records, members) -> np.ndarray:
        """Roots written on the device from game records (tg_search_set_roots_from_records): members[k] = (record index,
        ply) - the position before move `ply` of records[...], ply == its length the final one - or None to leave tree k
        alone; a record is a move list or (moves, colours) (mcts/record_roots.py).  Returns the flags [T]: 1 = the tree's
        root was NOT written (stage it from a host board with set_root), 0 otherwise.  The streams are not touched
        (seed_trees)."""
        from tamago_amd.mcts.record_roots import pack_record_roots
        packed = pack_record_roots(records, members, self.T)
        self._kept = None
        flags = np.zeros(self.T, dtype=np.int32)
        _lib.check(self.lib.tg_search_set_roots_from_records(
            self.handle, packed.moves.ctypes.data, None if packed.colors is None else packed.colors.ctypes.data,
            packed.offsets.ctypes.data, packed.games, packed.root_game.ctypes.data, packed.root_ply.ctypes.data,
            flags.ctypes.data, self._stream()), "tg_search_set_roots_from_records")
        return flags

    def seed_trees(self, seeds):
        """Tree k draws from np.random.RandomState(seeds[k]).get_state() from now on: set_stream for every tree, in one
        call (tg_search_seed_streams) where the library owns the streams."""
        seeds = [int(s) for s in seeds]
        assert len(seeds) == self.T
        if any(s < 0 or s >= 2 ** 32 for s in seeds):
            raise ValueError("seed_trees: seeds must be between 0 and 2**32 - 1")
        self.source.seed_all(seeds)

    def read_root_state(self, tree: int) -> dict:
        """The device-resident root of `tree` beyond read_positions (tg_search_read_root_state): hash, moves, ko_pos,
        ko_move, prev, prevprev, to_move, num_nodes, hist_len and the hist_len words of hash history (uint64)."""
        cap = 3 * self.P
        value = ctypes.c_uint64(0)
        meta = np.zeros(8, dtype=np.int32)
        hist = np.zeros(cap, dtype=np.uint64)
        _lib.check(self.lib.tg_search_read_root_state(self.handle, tree, ctypes.byref(value), meta.ctypes.data,
                                                      hist.ctypes.data, cap), "tg_search_read_root_state")
        names = ("moves", "ko_pos", "ko_move", "prev", "prevprev", "to_move", "num_nodes", "hist_len")
        out = {name: int(v) for name, v in zip(names, meta)}
        out["hash"] = int(value.value)
        out["history"] = hist[:min(out["hist_len"], cap)].copy()
        return out

    def _feed_rng(self, need: int):
        """Upload the next `need` stream positions of every tree (window becomes active at the
        next root / select launch).  Skipped when an earlier (pre-fetched) window still covers
        `need` positions for every tree."""
        self.source.feed(need)

    def _collect_rng(self):
        return self.source.collect()

    def _evaluate_and_backup(self, n_slots: int, use_logit: bool, packed_total: int = 0, unique_total: int = 0,
                             compact_trees: Optional[int] = None):
        """Forward pass over the queued leaves + write-back / backup.  `packed_total` > 0: the
        leaves of the trees lie back to back (n_slots is ignored, 0 is passed to the library).
        `unique_total` > 0: the UNIQUE layout - that many planes hold the distinct leaves (-1 is passed).
        `compact_trees`: the COMPACT layout - the leaves of that many ranked trees, n_slots each; 0: no forward pass."""
        if compact_trees is not None:
            assert not packed_total and not unique_total
            planes = self.planes[:compact_trees * n_slots]
            if compact_trees > 0:
                self.forward_positions += int(planes.shape[0])
                policy, value = self.evaluator(planes, use_logit)
            else:                                 # (no tree is live: nothing to evaluate, and the backup reads no row)
                policy = torch.zeros((1, self.A), dtype=torch.float32, device=self.device)
                value = torch.zeros((1, 3), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.tg_search_backup_compact(self.handle, policy.data_ptr(), value.data_ptr(), n_slots,
                                                         int(use_logit), self._stream()), "tg_search_backup_compact")
            self._keep = (policy, value)
            return
        if unique_total:
            planes, layout = self.planes[:unique_total], -1
        elif packed_total:
            planes, layout = self.planes[:packed_total], 0
        else:
            planes, layout = self.planes[:self.T * n_slots], n_slots
        self.forward_positions += int(planes.shape[0])
        policy, value = self.evaluator(planes, use_logit)
        _lib.check(self.lib.tg_search_backup(self.handle, policy.data_ptr(), value.data_ptr(),
                                             layout, int(use_logit), self._stream()),
                   "tg_search_backup")
        self._keep = (policy, value)        # keep alive until the stream has consumed them

    def root_eval(self, use_logit: bool = False, first_batch: int = 0):
        """tree.py:49-54: expand + evaluate the root of every tree (one leaf each).  With
        `first_batch` the random window also covers the first mini-batch of that many leaves,
        so no upload sits between the (tiny) root evaluation and the first selection."""
        self.node_bound = 1
        self._kept = None
        self._queue_stride = 1
        self._feed_rng(self.A * (1 + first_batch))
        _lib.check(self.lib.tg_search_root_planes(self.handle, self.planes.data_ptr(),
                                                  self._stream()), "tg_search_root_planes")
        # a Dirichlet prior takes one draw per child (mcts/tree.py:509-519): what the root expansion consumed IS the roots'
        # child counts - known as soon as the expansion kernel is done, without waiting for the root's forward pass and backup
        self.root_children = np.asarray(self._collect_rng(), dtype=np.int64).copy()
        self._evaluate_and_backup(1, use_logit)

    def prefetch_rng(self, leaves: int):
        """Generate + upload the window for the NEXT root evaluation and its first mini-batch
        now (e.g. while the last forward pass of the current search is still running)."""
        self.source.invalidate()
        self._feed_rng(self.A * (1 + leaves))

    def compact_live(self) -> int:
        """The live ranks of the trees as the halt words stand (tg_search_compact_live): what puct_batch(compact=True) lays
        its leaves out by.  Returns the number of live trees (the host waits for the launch stream)."""
        live = ctypes.c_int32(-1)
        self._halting_used()
        _lib.check(self.lib.tg_search_compact_live(self.handle, ctypes.byref(live), self._stream()), "tg_search_compact_live")
        self.live_count = int(live.value)
        return self.live_count

    def read_live_rank(self) -> np.ndarray:
        """rank [T] int32 of the last compact_live() (tg_search_read_live_rank): -1 for a tree that was not live."""
        rank = np.zeros(self.T, dtype=np.int32)
        _lib.check(self.lib.tg_search_read_live_rank(self.handle, rank.ctypes.data), "tg_search_read_live_rank")
        return rank

    # ---- the trees of several networks in one lock-step launch ------------------
    def group_live(self, groups) -> np.ndarray:
        """Grouped ranks as the halt words stand (tg_search_group_live): groups [T], tree t's group in [0, G) with G =
        max(groups) + 1 or, where given as (groups, G), G itself.  The live trees are sorted by group - group g's count[g]
        trees take the ranks from offset[g] on, in tree order.  Returns count [G]; group_counts / group_offsets keep it (the
        host waits for the launch stream)."""
        if isinstance(groups, tuple):
            groups, n_groups = groups
        else:
            n_groups = int(np.max(groups)) + 1 if len(groups) else 0
        arr = np.ascontiguousarray(groups, dtype=np.int32)
        assert arr.shape == (self.T,)
        count = np.zeros(max(int(n_groups), 1), dtype=np.int32)
        self._halting_used()
        _lib.check(self.lib.tg_search_group_live(self.handle, arr.ctypes.data, int(n_groups), count.ctypes.data, self._stream()),
                   "tg_search_group_live")
        self.group_counts = count.astype(np.int64)
        self.group_offsets = np.cumsum(self.group_counts) - self.group_counts
        self.live_count = None                    # (a plain puct_batch(compact=True) takes its own ranks)
        return self.group_counts.copy()

    def _rows_by_rank(self, gather: bool, src: torch.Tensor, dst: torch.Tensor):
        assert src.dtype == dst.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous()
        assert src.shape[0] >= self.T and dst.shape[0] >= self.T and src.shape[1:] == dst.shape[1:]
        name = "tg_search_gather_rows_by_rank" if gather else "tg_search_scatter_rows_by_rank"
        _lib.check(getattr(self.lib, name)(self.handle, src.data_ptr(), dst.data_ptr(), int(src[0].numel()), self._stream()), name)

    def gather_rows_by_rank(self, src: torch.Tensor, dst: torch.Tensor):
        """dst[rank[t]] = src[t] for every ranked tree t (tg_search_gather_rows_by_rank): float32 rows, T of them at least."""
        self._rows_by_rank(True, src, dst)

    def scatter_rows_by_rank(self, src: torch.Tensor, dst: torch.Tensor):
        """dst[t] = src[rank[t]] for every ranked tree t (tg_search_scatter_rows_by_rank); the other rows of dst are left alone."""
        self._rows_by_rank(False, src, dst)

    def _segments(self, evaluators):
        counts = self.group_counts
        if len(evaluators) != len(counts):
            raise ValueError(f"{len(evaluators)} evaluators for ranks of {len(counts)} groups")
        return [(g, int(self.group_offsets[g]), int(counts[g])) for g in range(len(counts)) if counts[g] > 0]

    def root_eval_groups(self, evaluators, groups, halt=None, use_logit: bool = False):
        """root_eval with tree t's root evaluated by evaluators[groups[t]]: the root planes (tree t at row t), halt words for the
        trees with a true flag in `halt` (slots without a game: they get rank -1 and no evaluation), the grouped ranks, a
        gather of the planes to rows by rank, ONE evaluator call per group that has live trees on its segment, a scatter of
        the outputs back to rows by tree, the strided root backup.  The grouped ranks stay in force for puct_chain_groups."""
        self.node_bound = 1
        self._kept = None
        self._queue_stride = 1
        self._halting_used()                         # (before the root planes are written: the first use zero-fills the buffer)
        self._feed_rng(self.A)
        _lib.check(self.lib.tg_search_root_planes(self.handle, self.planes.data_ptr(), self._stream()), "tg_search_root_planes")
        self.root_children = np.asarray(self._collect_rng(), dtype=np.int64).copy()
        if halt is not None and np.any(halt):
            self.set_halt(halt)
        self.group_live((groups, len(evaluators)))
        if getattr(self, "_group_rows", None) is None:
            # rows by tree of the outputs (zeros where no evaluation has ever been scattered: a halted tree's root backup
            # reads its row) and the gathered planes
            self._group_rows = (torch.zeros((self.T, self.A), dtype=torch.float32, device=self.device),
                                torch.zeros((self.T, 3), dtype=torch.float32, device=self.device),
                                torch.zeros((self.T, 6, self.S, self.S), dtype=torch.float32, device=self.device))
        policy_t, value_t, planes_r = self._group_rows
        self.gather_rows_by_rank(self.planes, planes_r)
        policy_r = torch.zeros((self.T, self.A), dtype=torch.float32, device=self.device)      # (rows by rank: T at most)
        value_r = torch.zeros((self.T, 3), dtype=torch.float32, device=self.device)
        for g, offset, count in self._segments(evaluators):
            policy, value = evaluators[g](planes_r[offset:offset + count], use_logit)
            policy_r[offset:offset + count] = policy
            value_r[offset:offset + count] = value
            self.forward_positions += count
            self.forward_positions_by_group[g] = self.forward_positions_by_group.get(g, 0) + count
        self.scatter_rows_by_rank(policy_r, policy_t)
        self.scatter_rows_by_rank(value_r, value_t)
        _lib.check(self.lib.tg_search_backup(self.handle, policy_t.data_ptr(), value_t.data_ptr(), 1, int(use_logit), self._stream()),
                   "tg_search_backup")
        self._keep = (policy_r, value_r)

    def can_chain_groups(self, total_leaves: int, evaluators) -> bool:
        """can_chain for every evaluator: all exactly DeviceEvaluator on a network handle, library streams, a pool that holds
        the search."""
        return total_leaves > 0 and self.source.chainable and self.node_bound + total_leaves <= self.N and \
            all(type(e) is DeviceEvaluator and hasattr(e.network, "handle") for e in evaluators)

    def puct_chain_groups(self, batches, evaluators) -> int:
        """puct_chain(compact=True) of a strict search by the grouped ranks in force (group_live / root_eval_groups): per
        mini-batch ONE compact selection of every live tree, evaluators[g] on group g's segment of the plane rows for every
        group that has live trees, ONE compact backup.  Where can_chain_groups allows, one call of the library
        (tg_search_puct_chain_groups); otherwise mini-batch by mini-batch - the puct_batch(compact=True) path with a loop
        over the segments, which any evaluator can take.  Returns the mini-batches queued."""
        arr = np.ascontiguousarray(batches, dtype=np.int32)
        total, kmax = int(arr.sum()), int(arr.max())
        segments = self._segments(evaluators)
        live = int(self.group_counts.sum())
        if self.can_chain_groups(total, evaluators):
            self.node_bound += total
            self._queue_stride = int(arr[-1])
            policy = torch.empty((max(live, 1) * kmax, self.A), dtype=torch.float32, device=self.device)
            value = torch.empty((max(live, 1) * kmax, 3), dtype=torch.float32, device=self.device)
            nets = (ctypes.c_void_p * len(evaluators))(*[e.network.handle for e in evaluators])
            launched = ctypes.c_int64(0)
            self._halting_used()
            _lib.check(self.lib.tg_search_puct_chain_groups(
                self.handle, nets, len(evaluators), arr.ctypes.data, len(arr), self.source.take_invalid(), self.planes.data_ptr(),
                policy.data_ptr(), value.data_ptr(), self._stream(), ctypes.byref(launched)), "tg_search_puct_chain_groups")
            assert int(launched.value) == live * total
            for g, _, count in segments:
                evaluators[g].batches.append(count * total)   # (one entry for the call, as puct_chain(compact=True) records it)
                self.forward_positions_by_group[g] = self.forward_positions_by_group.get(g, 0) + count * total
            self.forward_positions += int(launched.value)
            self._keep = (policy, value)
            self._collect_rng()
            return len(arr)
        if live == 0:
            return 0
        for leaves in (int(k) for k in arr):
            self.ensure_capacity(leaves)
            self.node_bound += leaves
            self._queue_stride = leaves
            self._feed_rng(leaves * self.A)
            _lib.check(self.lib.tg_search_select_puct_compact(self.handle, leaves, 0, self.planes.data_ptr(), None, self._stream()),
                       "tg_search_select_puct_compact")
            policy = torch.empty((live * leaves, self.A), dtype=torch.float32, device=self.device)
            value = torch.empty((live * leaves, 3), dtype=torch.float32, device=self.device)
            for g, offset, count in segments:
                rows = slice(offset * leaves, (offset + count) * leaves)
                policy[rows], value[rows] = evaluators[g](self.planes[rows], False)
                self.forward_positions += count * leaves
                self.forward_positions_by_group[g] = self.forward_positions_by_group.get(g, 0) + count * leaves
            _lib.check(self.lib.tg_search_backup_compact(self.handle, policy.data_ptr(), value.data_ptr(), leaves, 0, self._stream()),
                       "tg_search_backup_compact")
            self._keep = (policy, value)
            self._collect_rng()
        return len(arr)

    def puct_batch(self, leaves: int, compact: bool = False, shrunk_ok: bool = False, n_leaves: Optional[torch.Tensor] = None):
        """`leaves` PUCT descents per tree + one evaluation + backup (tree.py:146-152 with
        the flush of :240-241).  compact: in the COMPACT layout - the evaluator gets the leaves of the trees
        the last compact_live() ranked and no other tree's; the library refuses ranks that are not fresh (shrunk_ok: ranks
        since which halt words were only SET are taken - a tree halted since keeps an idle slot).  n_leaves: an int32 [T]
        device tensor that receives the leaves each tree queued (under visit budgets: its descents), in stream order."""
        counts = None
        if n_leaves is not None:
            assert n_leaves.dtype == torch.int32 and n_leaves.shape == (self.T,) and n_leaves.is_contiguous() and n_leaves.device == self.device
            counts = n_leaves.data_ptr()
        if compact:
            if self.live_count is None:
                self.compact_live()
            self.node_bound += leaves
            self._queue_stride = leaves
            self._feed_rng(leaves * self.A)
            _lib.check(self.lib.tg_search_select_puct_compact(self.handle, leaves, int(shrunk_ok), self.planes.data_ptr(),
                                                              counts, self._stream()), "tg_search_select_puct_compact")
            self._evaluate_and_backup(leaves, False, compact_trees=self.live_count)
            self._collect_rng()
            return
        # order matters for overlap: the random window of THIS batch is generated and
        # uploaded (private copy stream) while the forward pass of the PREVIOUS batch is
        # still running; the cursor read-back waits for the selection kernel only
        self.node_bound += leaves
        self._queue_stride = leaves
        self._feed_rng(leaves * self.A)
        _lib.check(self.lib.tg_search_select_puct(self.handle, leaves, self.planes.data_ptr(),
                                                  counts, self._stream()), "tg_search_select_puct")
        # forward + backup are queued BEFORE the cursor read-back: that read waits for the selection kernel only
        # (its own event on the copy stream), so the host is back while the forward pass runs
        self._evaluate_and_backup(leaves, False)
        self._collect_rng()

    def _halting_used(self):
        """A halted tree's plane slots are still part of a mini-batch's forward pass and hold whatever was there: the planes
        buffer starts from zeros (once), so that no stale slot can be out of the f16 kernels' range."""
        if not self._halting:
            self._halting = True
            self.planes.zero_()

    def set_halt(self, halt):
        """Halt the trees with a true flag (tg_search_set_halt): the PUCT selection passes them by - no descent, no draw, no
        plane, no leaf - until root_eval clears every word, or set_root, set_roots_from_records or reroot the words of the
        trees they give a root.  False: left alone."""
        flags = np.ascontiguousarray(halt, dtype=np.uint8)
        assert flags.shape == (self.T,)
        self._halting_used()
        _lib.check(self.lib.tg_search_set_halt(self.handle, flags.ctypes.data, self._stream()), "tg_search_set_halt")

    def read_halt(self):
        """(halted [T] bool, stopped_at [T] int32: the root's visits when the stop rule halted the tree, else 0)."""
        halted = np.zeros(self.T, dtype=np.uint8)
        stopped = np.zeros(self.T, dtype=np.int32)
        _lib.check(self.lib.tg_search_read_halt(self.handle, halted.ctypes.data, stopped.ctypes.data), "tg_search_read_halt")
        return halted.astype(bool), stopped

    def stop_rule(self, totals, wait: bool = True):
        """One launch of the early-stop rule (tg_search_stop_rule); wait: returns the number of trees left running."""
        arr = np.ascontiguousarray(np.broadcast_to(np.asarray(totals, dtype=np.int32), (self.T,)))
        live = ctypes.c_int32(-1)
        self._halting_used()
        _lib.check(self.lib.tg_search_stop_rule(self.handle, arr.ctypes.data, ctypes.byref(live) if wait else None,
                                                self._stream()), "tg_search_stop_rule")
        return int(live.value) if wait else None

    DEFAULT_POLL_EVERY = 4                          # mini-batches between two looks at the live count: the fastest single-tree
                                                    # setting at batch 256 in profiles/early_stop_bench.json

    def puct_chain(self, batches, early_total=None, poll_every=None, compact: bool = False, budget=None):
        """Several mini-batches queued in one go: ONE random window for all of them (the device cursor runs on from launch to
        launch), every selection / forward / backup launch enqueued back to back, one cursor read-back at the end - for searches
        whose course does not depend on what a mini-batch found (STRICT_PLAYOUT: no early stop, time_manager.py:160-161).  Same
        launches on the same data as puct_batch called once per mini-batch; what goes is the host's round trip between them
        (the selection launch of mini-batch k + 1 used to be queued only after the cursor of mini-batch k had been read back).

        early_total (an int, or one per tree): the CONSTANT_PLAYOUT search instead - the early-stop rule runs on the device
        behind every full mini-batch that has descents to follow and halts the trees it decides (tg_search_puct_chain_early);
        every poll_every mini-batches (None: DEFAULT_POLL_EVERY; 0: never) the host looks whether a tree is still running
        and stops queueing when none is.  An engine that cannot chain (can_chain: a host evaluator, host streams, a pool
        that may have to grow) sends these mini-batches one by one, puct_batch each, with the same rule launches and polls
        in between.

        compact: the forward passes cover the live trees only - those that were live when the call began
        and, with early_total, at its last poll (the live ranks are taken where the host looks, never in between: a tree
        halted since keeps an idle slot until the next look).  Same trees, streams and halt words; forward_positions and
        evaluator.batches record the positions really launched.  Returns the mini-batches queued.

        budget (not together with early_total): per-tree visit budgets bound every tree's descents and the
        budget rule halts a tree behind the backup that spends its budget (tg_search_puct_chain_budget) - `batches` is what
        a fresh tree needs, a tree that kept visits stops sooner, the call ends at the first look that finds no tree
        live.  Totals (an int, or one per tree): set_budget first; True: the budgets already in force."""
        arr = np.ascontiguousarray(batches, dtype=np.int32)
        total, kmax = int(arr.sum()), int(arr.max())
        if budget is not None and budget is not False:
            if early_total is not None:
                raise ValueError("puct_chain: budget and early_total exclude each other")
            if budget is not True:
                self.set_budget(budget)
            return self._budget_chain(arr, poll_every, compact)
        if (early_total is not None or compact) and not self.can_chain(total):
            poll = (self.DEFAULT_POLL_EVERY if poll_every is None else int(poll_every)) or len(arr)
            if compact and self.compact_live() == 0:
                return 0                                         # (no tree is live: nothing to queue)
            for b, leaves in enumerate(int(k) for k in arr):
                self.ensure_capacity(leaves)
                self.puct_batch(leaves, compact=compact, shrunk_ok=True)
                if early_total is not None and leaves == int(arr[0]) and b + 1 < len(arr):
                    wait = (b + 1) % poll == 0
                    live = self.stop_rule(early_total, wait=wait)
                    if compact and wait:
                        live = self.compact_live()               # (the rule's count, over every tree: the same predicate)
                    if live == 0:
                        return b + 1
            return len(arr)
        self.node_bound += total
        self._queue_stride = int(arr[-1])
        policy = torch.empty((self.T * kmax, self.A), dtype=torch.float32, device=self.device)
        value = torch.empty((self.T * kmax, 3), dtype=torch.float32, device=self.device)
        run = len(arr)
        positions = None
        if compact:
            totals = None if early_total is None else \
                np.ascontiguousarray(np.broadcast_to(np.asarray(early_total, dtype=np.int32), (self.T,)))
            poll = (self.DEFAULT_POLL_EVERY if poll_every is None else int(poll_every)) or len(arr)
            ran, launched = ctypes.c_int32(0), ctypes.c_int64(0)
            self._halting_used()
            _lib.check(self.lib.tg_search_puct_chain_compact(
                self.handle, self.evaluator.network.handle, arr.ctypes.data, len(arr), None if totals is None else totals.ctypes.data,
                poll, self.source.take_invalid(), self.planes.data_ptr(), policy.data_ptr(), value.data_ptr(), self._stream(),
                ctypes.byref(ran), ctypes.byref(launched)), "tg_search_puct_chain_compact")
            run, positions = int(ran.value), int(launched.value)
            self.live_count = None                   # (the call's own looks: the next puct_batch(compact=True) takes its own)
        elif early_total is None:
            _lib.check(self.lib.tg_search_puct_chain(self.handle, self.evaluator.network.handle, arr.ctypes.data, len(arr),
                                                     self.source.take_invalid(), self.planes.data_ptr(), policy.data_ptr(),
                                                     value.data_ptr(), self._stream()), "tg_search_puct_chain")
        else:
            totals = np.ascontiguousarray(np.broadcast_to(np.asarray(early_total, dtype=np.int32), (self.T,)))
            poll = self.DEFAULT_POLL_EVERY if poll_every is None else int(poll_every)
            if poll == 0:
                poll = len(arr)
            ran = ctypes.c_int32(0)
            self._halting_used()
            _lib.check(self.lib.tg_search_puct_chain_early(
                self.handle, self.evaluator.network.handle, arr.ctypes.data, len(arr), totals.ctypes.data, poll,
                self.source.take_invalid(), self.planes.data_ptr(), policy.data_ptr(), value.data_ptr(), self._stream(),
                ctypes.byref(ran)), "tg_search_puct_chain_early")
            run = int(ran.value)
        if positions is None:
            self.evaluator.batches.extend(int(self.T * k) for k in arr[:run])
        else:
            self.evaluator.batches.append(positions)  # (one entry for the call: the library chose each launch's size)
            self.forward_positions += positions
        self._keep = (policy, value)                 # keep alive until the stream has consumed them
        self._collect_rng()
        return run

    def _budget_need(self, total_leaves: int) -> int:
        """Nodes the pool must hold for a budgeted search of at most total_leaves descents per tree: a descent adds at most
        one node, and a tree makes no more than its budget leaves of its total - kept nodes + (total - kept root visits)
        where the last advance said what each tree kept, the engine's bound + total_leaves otherwise."""
        if self._kept is None or self._budget is None:
            return int(self.node_bound) + total_leaves
        nodes, visits = self._kept
        owed = np.minimum(np.maximum(self._budget.astype(np.int64) - visits, 0), total_leaves)
        return int((np.maximum(nodes, 1) + owed).max())

    def _budget_chain(self, arr, poll_every, compact: bool) -> int:
        total, kmax = int(arr.sum()), int(arr.max())
        poll = (self.DEFAULT_POLL_EVERY if poll_every is None else int(poll_every)) or len(arr)
        self._halting_used()
        need = self._budget_need(total)
        if not self.can_chain(total, need):
            if compact and self.compact_live() == 0:
                return 0
            for b, leaves in enumerate(int(k) for k in arr):
                if need > self.N:                     # (else the whole search fits: no mini-batch has to look at the pool)
                    self.ensure_capacity(leaves)
                self.puct_batch(leaves, compact=compact, shrunk_ok=True)
                wait = (b + 1) % poll == 0 and b + 1 < len(arr)
                live = self.budget_rule(wait=wait)
                if compact and wait:
                    live = self.compact_live()
                if wait and live == 0:
                    return b + 1
            return len(arr)
        self.node_bound = max(int(self.node_bound), need)
        self._queue_stride = int(arr[-1])
        policy = torch.empty((self.T * kmax, self.A), dtype=torch.float32, device=self.device)
        value = torch.empty((self.T * kmax, 3), dtype=torch.float32, device=self.device)
        ran, launched = ctypes.c_int32(0), ctypes.c_int64(0)
        _lib.check(self.lib.tg_search_puct_chain_budget(
            self.handle, self.evaluator.network.handle, arr.ctypes.data, len(arr), poll, int(bool(compact)),
            self.source.take_invalid(), self.planes.data_ptr(), policy.data_ptr(), value.data_ptr(), self._stream(),
            ctypes.byref(ran), ctypes.byref(launched)), "tg_search_puct_chain_budget")
        self.live_count = None
        self.evaluator.batches.append(int(launched.value))
        self.forward_positions += int(launched.value)
        self._keep = (policy, value)
        self._collect_rng()
        return int(ran.value)

    def can_chain(self, total_leaves: int, need: Optional[int] = None) -> bool:
        """puct_chain needs the library's streams (one window for the whole search), the device evaluator (the forward pass is
        queued by the library) and a pool that holds the whole search without growing (the reference doubles its node list
        between mini-batches, mcts/tree.py:254-258: that stays there)."""
        # (exactly DeviceEvaluator: the chained forward passes are launched by the library on the network handle and never go
        # through evaluator.__call__ - a subclass that wraps the forward pass keeps the per-mini-batch loop)
        return total_leaves > 0 and self.source.chainable and type(self.evaluator) is DeviceEvaluator and \
            hasattr(self.evaluator.network, "handle") and (self.node_bound + total_leaves if need is None else need) <= self.N

    def puct_select(self, leaves: int):
        """The selection half of puct_batch: afterwards the device queue holds `leaves` leaves per
        tree (read_queue) until puct_flush() evaluates and backs them up."""
        self.node_bound += leaves
        self._queue_stride = leaves
        self._feed_rng(leaves * self.A)
        _lib.check(self.lib.tg_search_select_puct(self.handle, leaves, self.planes.data_ptr(),
                                                  None, self._stream()), "tg_search_select_puct")
        self._collect_rng()

    def puct_flush(self):
        """process_mini_batch (tree.py:273-315) for the leaves queued by puct_select."""
        self._evaluate_and_backup(self._queue_stride, False)

    def ensure_capacity(self, leaves: int) -> bool:
        """Make room for `leaves` more descents (each allocates at most one node) in every tree:
        the reference doubles its node list when it fills up (mcts/tree.py:254-258), the device
        pool is grown in place the same way (tg_search_grow keeps the trees).  The host-side
        bound makes this free while the pool is far from full.  Returns True if the pool grew."""
        if self.node_bound + leaves <= self.N:
            return False
        self.node_bound = int(self.num_nodes().max())
        if self.node_bound + leaves <= self.N:
            return False
        new_size = self.N
        while self.node_bound + leaves > new_size:
            import sys
            sys.stderr.write(f"Tree is full. Allocate new space {new_size} -> {new_size * 2}\n")
            new_size *= 2
        _lib.check(self.lib.tg_search_grow(self.handle, new_size), "tg_search_grow")
        self.N = new_size
        return True

    def read_queue(self, tree: int = 0):
        """The device leaf queue of `tree` as a BatchQueue (mcts/batch_data.py:7-34): input planes,
        root-first paths and node indices of the leaves the last selection launch queued.  Empty
        once the mini-batch has been backed up (the reference clears its queue there, tree.py:315)."""
        from tamago_amd.mcts.batch_data import BatchQueue
        idx = np.zeros(self.K, dtype=np.int32)
        n = ctypes.c_int32(0)
        _lib.check(self.lib.tg_search_read_queue(self.handle, tree, idx.ctypes.data, self.K, ctypes.byref(n)),
                   "tg_search_read_queue")
        queue = BatchQueue()
        if n.value:
            planes = self.planes[tree * self._queue_stride:tree * self._queue_stride + n.value].cpu().numpy()
            for k in range(n.value):
                queue.push(planes[k], self.read_path(tree, k), int(idx[k]))
        return queue

    def play(self, moves):
        """Play one move per tree on the device-resident root positions (-1 = skip, -2 = the most visited root child's
        move, chosen on the device)."""
        mv = np.ascontiguousarray(moves, dtype=np.int32)
        assert mv.shape == (self.T,)
        _lib.check(self.lib.tg_search_play(self.handle, mv.ctypes.data, self._stream()), "tg_search_play")

    def best_moves(self, resign_threshold: float, play: bool, sit_out=None) -> np.ndarray:
        """The PUCT move of every tree, decided on the device (tg_search_best_moves: the end of search_best_move - PASS for
        a one-child root, else the first most visited child's move, RESIGN (-1) when its value is < resign_threshold) as
        one BEST_MOVE record per tree; play: the moves are played on the root positions as play() would.  sit_out [T]
        (optional): trees with a true flag are left alone (status BEST_SAT_OUT)."""
        out = np.zeros(self.T, dtype=BEST_MOVE)
        flags = None
        if sit_out is not None:
            flags = np.ascontiguousarray(sit_out, dtype=np.uint8)
            assert flags.shape == (self.T,)
        _lib.check(self.lib.tg_search_best_moves(self.handle, float(resign_threshold), int(bool(play)),
                                                 None if flags is None else flags.ctypes.data, out.ctypes.data,
                                                 self._stream()), "tg_search_best_moves")
        return out

    def count_scores(self, cells) -> np.ndarray:
        """GoBoard.count_score of padded boards [n][(S+2)^2] as read_positions returns them (tg_search_count_scores)."""
        cells = np.ascontiguousarray(cells, dtype=np.uint8).reshape(-1, (self.S + 2) ** 2)
        out = np.zeros(len(cells), dtype=np.int32)
        _lib.check(self.lib.tg_search_count_scores(cells.ctypes.data, self.S, len(cells), out.ctypes.data),
                   "tg_search_count_scores")
        return out

    def find_child(self, tree: int, node: int, move: int) -> int:
        """Index of the EXPANDED child of `node` reached by `move` (padded coordinate, PASS = 0), -1 if there is none."""
        view = self.read_node(tree, node)
        for i in range(view.num_children):
            if view.action[i] == move:
                return int(view.children_index[i])
        return -1

    def reroot(self, new_roots):
        """Tree reuse (tg_search_reroot, no reference counterpart): for every tree with new_roots[t] >= 0 the subtree under
        that node becomes the whole tree - compacted in place on the device, new root = node 0, creation order kept - and a
        position staged by set_root becomes its root position without the reset / root evaluation of root_eval.  -1 leaves
        a tree alone.  Queued on the launch stream; the next puct_batch feeds its random window as usual."""
        roots = np.ascontiguousarray(new_roots, dtype=np.int32)
        assert roots.shape == (self.T,)
        _lib.check(self.lib.tg_search_reroot(self.handle, roots.ctypes.data, self._stream()), "tg_search_reroot")
        # (node_bound stays an upper bound: a compacted tree only shrinks)
        self._queue_stride = 1
        self._kept = None

    # ---- tree reuse in lock-step matches ---------------------------------------
    def advance(self, moves, wait: bool = True):
        """Every tree's root advanced by one move on the device (tg_search_advance): moves [T] padded coordinates, 0 = PASS,
        -1 leaves a tree alone.  The move is played on the root position; the subtree under the move's root child becomes
        the tree (as reroot makes it) or, where that child is not expanded, the tree becomes fresh (no nodes: the next
        root_eval_fresh expands it).  Returns the ADVANCE records [T] (kept_visits -1: fresh), or None without wait.
        node_bound and root_children follow the records."""
        mv = np.ascontiguousarray(moves, dtype=np.int32)
        assert mv.shape == (self.T,)
        out = np.zeros(self.T, dtype=ADVANCE) if wait else None
        _lib.check(self.lib.tg_search_advance(self.handle, mv.ctypes.data, None if out is None else out.ctypes.data,
                                              self._stream()), "tg_search_advance")
        self._queue_stride = 1
        if out is None:
            self._kept = None
            return None                               # (node_bound stays an upper bound: an advanced tree only shrinks)
        moved = mv >= 0
        # (a tree left alone may have searched since its entry was made: its visits and its nodes grew alike, and what it can
        # still add under a total did not; a tree nothing is known of: as many nodes as the engine's bound, no visits)
        nodes, visits = self._kept if self._kept is not None else \
            (np.full(self.T, min(int(self.node_bound), self.N), dtype=np.int64), np.zeros(self.T, dtype=np.int64))
        self._kept = (np.where(moved, out["kept_nodes"], nodes).astype(np.int64),
                      np.where(moved, np.maximum(out["kept_visits"], 0), visits).astype(np.int64))
        if moved.any():
            still = int(self.node_bound) if not moved.all() else 0
            self.node_bound = max(still, int(out["kept_nodes"][moved].max()))
            children = getattr(self, "root_children", None)
            if children is None or len(children) != self.T:
                children = np.zeros(self.T, dtype=np.int64)
            children = np.asarray(children, dtype=np.int64).copy()
            children[moved] = out["num_children"][moved]
            self.root_children = children
        return out

    def root_eval_fresh(self, use_logit: bool = False, first_batch: int = 0):
        """root_eval for the fresh trees only (tg_search_root_planes_fresh): a tree without nodes is expanded and evaluated
        as root_eval does it, a tree that kept a subtree is not touched - no draw, no node, no plane.  root_children of the
        fresh trees comes off the draw cursors as in root_eval, of the kept trees from the advance record."""
        self.node_bound = max(1, int(self.node_bound))
        self._queue_stride = 1
        self._halting_used()                         # (a kept tree's plane row is not written: it must hold something in range)
        self._feed_rng(self.A * (1 + first_batch))
        _lib.check(self.lib.tg_search_root_planes_fresh(self.handle, self.planes.data_ptr(), self._stream()),
                   "tg_search_root_planes_fresh")
        drawn = np.asarray(self._collect_rng(), dtype=np.int64)
        children = getattr(self, "root_children", None)
        if children is None or len(children) != self.T:
            children = np.zeros(self.T, dtype=np.int64)
        # (an expansion draws once per child and a root has at least PASS: a tree drew iff it was expanded)
        self.root_children = np.where(drawn > 0, drawn, np.asarray(children, dtype=np.int64))
        self._evaluate_and_backup(1, use_logit)

    def set_budget(self, totals):
        """Per-tree visit budgets (tg_search_set_budget): from the next PUCT selection on, tree t makes
        clamp(totals[t] - root visits, 0, leaves) descents per mini-batch.  An int serves every tree; None switches the
        budgets off."""
        if totals is None:
            _lib.check(self.lib.tg_search_set_budget(self.handle, None, self._stream()), "tg_search_set_budget")
            self._budget = None
            return
        arr = np.ascontiguousarray(np.broadcast_to(np.asarray(totals, dtype=np.int32), (self.T,)))
        _lib.check(self.lib.tg_search_set_budget(self.handle, arr.ctypes.data, self._stream()), "tg_search_set_budget")
        self._budget = arr

    def budget_rule(self, wait: bool = True):
        """Halt the trees whose budget is spent (tg_search_budget_rule); wait: returns the number of trees left running."""
        live = ctypes.c_int32(-1)
        self._halting_used()
        _lib.check(self.lib.tg_search_budget_rule(self.handle, ctypes.byref(live) if wait else None, self._stream()),
                   "tg_search_budget_rule")
        return int(live.value) if wait else None

    def read_node_links(self, tree: int, node: int):
        """(parent, parent's child slot) of a node; (-1, -1) for the root."""
        parent = ctypes.c_int32(0)
        pedge = ctypes.c_int32(0)
        _lib.check(self.lib.tg_search_read_node_links(self.handle, tree, node, ctypes.byref(parent), ctypes.byref(pedge)),
                   "tg_search_read_node_links")
        return int(parent.value), int(pedge.value)

    def read_positions(self):
        """(cells [T][(S+2)^2], moves [T], to_move [T]) of the current root positions."""
        cells = np.zeros((self.T, (self.S + 2) ** 2), dtype=np.uint8)
        moves = np.zeros(self.T, dtype=np.int32)
        to_move = np.zeros(self.T, dtype=np.int32)
        _lib.check(self.lib.tg_search_read_positions(self.handle, cells.ctypes.data, moves.ctypes.data,
                                                     to_move.ctypes.data), "tg_search_read_positions")
        return cells, moves, to_move

    def set_gumbel_noise(self):
        """node.py:275-278 for every root: A doubles from each tree's stream, drawn after the
        root's Dirichlet prior and NN evaluation (tree.py:332-336)."""
        self.noise = self.source.noise()
        return self.noise

    def gumbel_phase(self, num_considered, max_count, packed: bool = True, unique: bool = False):
        """One sequential-halving phase for every tree (tree.py:375-384): per-tree
        (num_considered, max_count), one evaluation of all queued leaves, backup.
        unique: the UNIQUE layout (tg_search_select_gumbel with slots_per_tree -1) - the descents of a phase
        through one root child end on the same leaf; each distinct leaf is evaluated once (same trees)."""
        nc = np.ascontiguousarray(num_considered, dtype=np.int32)
        mc = np.ascontiguousarray(max_count, dtype=np.int32)
        per_tree = nc.astype(np.int64) * mc
        slots = int(per_tree.max())
        if slots == 0:
            return
        # packed leaf layout (slots_per_tree = 0): the forward pass covers exactly the queued
        # leaves - a tree whose root has one candidate runs 1 x `visits` levels and would
        # otherwise stretch every tree's slot range to `visits`
        self.node_bound += slots
        self._feed_rng(slots * self.A)
        _lib.check(self.lib.tg_search_select_gumbel(self.handle, nc.ctypes.data, mc.ctypes.data,
                                                    -1 if unique else (0 if packed else slots),
                                                    self.planes.data_ptr(), self._stream()),
                   "tg_search_select_gumbel")
        # forward + backup are queued before the cursor read-back (which waits for the selection kernel only)
        if unique:
            total = ctypes.c_int64(0)
            caps = np.zeros(self.T, dtype=np.int32)
            _lib.check(self.lib.tg_search_unique_planes(self.handle, ctypes.byref(total), caps.ctypes.data),
                       "tg_search_unique_planes")
            self.unique_caps = caps
            self._evaluate_and_backup(slots, True, unique_total=int(total.value))
        else:
            self._evaluate_and_backup(slots, True, packed_total=int(per_tree.sum()) if packed else 0)
        self._collect_rng()

    # ---------------------------------------------------------------------------------
    def num_nodes(self) -> np.ndarray:
        out = np.zeros(self.T, dtype=np.int32)
        _lib.check(self.lib.tg_search_num_nodes(self.handle, out.ctypes.data), "tg_search_num_nodes")
        return out

    def read_path(self, tree: int, slot: int):
        """[(node index, child index), ...] root first for queued leaf `slot` (tree.py:199-244 path)."""
        cap = 4 * self.P + 8
        nodes = np.zeros(cap, dtype=np.int32)
        edges = np.zeros(cap, dtype=np.int32)
        n = ctypes.c_int32(0)
        _lib.check(self.lib.tg_search_read_path(self.handle, tree, slot, nodes.ctypes.data, edges.ctypes.data,
                                                cap, ctypes.byref(n)), "tg_search_read_path")
        return [(int(nodes[i]), int(edges[i])) for i in range(n.value)]

    def read_roots(self):
        """(num_children [T], action [T][A], children_visits [T][A]) of every root."""
        nc = np.zeros(self.T, dtype=np.int32)
        action = np.zeros((self.T, self.A), dtype=np.int32)
        visits = np.zeros((self.T, self.A), dtype=np.int32)
        _lib.check(self.lib.tg_search_read_roots(self.handle, nc.ctypes.data, action.ctypes.data,
                                                 visits.ctypes.data), "tg_search_read_roots")
        return nc, action, visits

    def read_root_stats(self):
        """dict of root arrays for all trees ([T] / [T][A]) in one call."""
        t, a = self.T, self.A
        out = {"num_children": np.zeros(t, np.int32), "node_visits": np.zeros(t, np.int32),
               "raw_value": np.zeros(t, np.float32), "action": np.zeros((t, a), np.int32),
               "children_visits": np.zeros((t, a), np.int32),
               "children_virtual_loss": np.zeros((t, a), np.int32),
               "children_value_sum": np.zeros((t, a), np.float64),
               "children_policy": np.zeros((t, a), np.float64)}
        _lib.check(self.lib.tg_search_read_root_stats(
            self.handle, out["num_children"].ctypes.data, out["node_visits"].ctypes.data,
            out["raw_value"].ctypes.data, out["action"].ctypes.data,
            out["children_visits"].ctypes.data, out["children_virtual_loss"].ctypes.data,
            out["children_value_sum"].ctypes.data, out["children_policy"].ctypes.data),
            "tg_search_read_root_stats")
        return out

    def root_view(self, stats, tree: int) -> MCTSNode:
        """MCTSNode view of one root out of read_root_stats() (no further device access)."""
        view = MCTSNode(self.A)
        view.num_children = int(stats["num_children"][tree])
        view.node_visits = int(stats["node_visits"][tree])
        view.raw_value = np.float32(stats["raw_value"][tree])
        view.action = [int(x) for x in stats["action"][tree]]
        view.children_visits = stats["children_visits"][tree]
        view.children_virtual_loss = stats["children_virtual_loss"][tree]
        view.children_value_sum = stats["children_value_sum"][tree]
        view.children_policy = stats["children_policy"][tree]
        noise = getattr(self, "noise", None)
        if noise is not None:
            view.noise = noise[tree]
        return view

    def read_improved_policy(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """calculate_improved_policy (node.py:281-321) of every root as a dense float32 row in the network's output order,
        [T][A] in device memory (tg_search_read_improved_policy: float64 arithmetic on the device, np.float32(1e-18) where a
        root has no child).  Every root must be expanded.  `out`: a contiguous float32 [T][A] tensor to write into."""
        if out is None:
            out = torch.empty((self.T, self.A), dtype=torch.float32, device=self.device)
        assert out.shape == (self.T, self.A) and out.dtype == torch.float32 and out.is_contiguous() and out.device == self.device
        _lib.check(self.lib.tg_search_read_improved_policy(self.handle, out.data_ptr(), self._stream()),
                   "tg_search_read_improved_policy")
        return out

    def read_analysis(self, max_depth: int = 32):
        """Analysis read-out of every tree in one launch (tg_search_read_analysis): per tree (root, pv_lists) - an MCTSNode
        view of the root with what get_analysis reads (num_children, node_visits, node_value_sum, action, children_visits,
        children_value_sum, children_policy; children_index is not read) and a pv_lists(root, coord) callable that returns
        MCTSTree.get_pv_lists's {gtp move: [gtp moves]}.  PVs longer than max_depth are completed on the host with
        read_node, so pv_lists must be called before the trees change.  A tree with its error flags set raises."""
        t, a = self.T, self.A
        head = np.zeros((t, 4), np.int32)
        action = np.zeros((t, a), np.int32)
        visits = np.zeros((t, a), np.int32)
        value_sum = np.zeros((t, a), np.float64)
        policy = np.zeros((t, a), np.float64)
        pv = np.zeros((t, a, max_depth), np.int16)
        pv_len = np.zeros((t, a), np.int32)
        resume = np.zeros((t, a), np.int32)
        _lib.check(self.lib.tg_search_read_analysis(
            self.handle, int(max_depth), head.ctypes.data, action.ctypes.data, visits.ctypes.data, value_sum.ctypes.data,
            policy.ctypes.data, pv.ctypes.data, pv_len.ctypes.data, resume.ctypes.data, self._stream()),
            "tg_search_read_analysis")
        for tree, err in enumerate(head[:, 3]):
            if err:                              # (bit 0: kErrPoolFull of csrc/readout.h, the home of the flags and their text)
                raise _lib.TamagoHipError(f"tg_search_read_analysis: tree {tree}: error flags 0x{int(err):x}"
                                          f"{' (node pool full)' if err & 1 else ''}")
        out = []
        for tree in range(t):
            view = MCTSNode(a)
            view.num_children = int(head[tree, 0])
            view.node_visits = int(head[tree, 1])
            view.node_value_sum = head[tree, 2:3].view(np.float32)[0]
            view.action = [int(x) for x in action[tree]]
            view.children_visits = visits[tree]
            view.children_value_sum = value_sum[tree]
            view.children_policy = policy[tree]
            out.append((view, self._pv_lists_func(tree, pv[tree], pv_len[tree], resume[tree])))
        return out

    def _pv_lists_func(self, tree, pv, pv_len, resume):
        def pv_lists(root: MCTSNode, coord):
            lists = {}
            for i in range(root.num_children):
                if root.children_visits[i] > 0:
                    seq = [int(m) for m in pv[i, :pv_len[i]]]
                    if resume[i] >= 0:
                        seq = continue_pv(seq, int(resume[i]), lambda node: self.read_node(tree, node))
                    lists[coord.convert_to_gtp_format(root.action[i])] = [coord.convert_to_gtp_format(p) for p in seq]
            return lists
        return pv_lists

    def read_node(self, tree: int, node: int) -> MCTSNode:
        a = self.A
        view = MCTSNode(a)
        nc = ctypes.c_int32()
        nv = ctypes.c_int32()
        nvl = ctypes.c_int32()
        nvs = ctypes.c_float()
        raw = ctypes.c_float()
        action = np.zeros(a, dtype=np.int32)
        _lib.check(self.lib.tg_search_read_node(
            self.handle, tree, node, ctypes.byref(nc), ctypes.byref(nv), ctypes.byref(nvl),
            action.ctypes.data,
            view.children_index.ctypes.data, view.children_visits.ctypes.data,
            view.children_virtual_loss.ctypes.data, view.children_value_sum.ctypes.data,
            view.children_policy.ctypes.data, view.children_value.ctypes.data,
            ctypes.byref(nvs), ctypes.byref(raw)), "tg_search_read_node")
        view.num_children = nc.value
        view.node_visits = nv.value
        view.virtual_loss = nvl.value
        view.node_value_sum = np.float32(nvs.value)
        view.raw_value = np.float32(raw.value)
        view.action = [int(v) for v in action]
        n = ctypes.c_int32(0)
        _lib.check(self.lib.tg_search_node_record_num_nodes(self.handle, ctypes.byref(n)), "tg_search_node_record_num_nodes")
        view.tree_num_nodes = int(n.value)           # num_nodes of the tree, read with the node
        return view

    # ---- whole-tree read-out ------------------------------------------------------------------------------
    def _tree_list(self, trees):
        """(int32 array or None, its address or None, the number of listed trees): None lists every tree in order."""
        if trees is None:
            return None, None, self.T
        arr = np.ascontiguousarray(trees, dtype=np.int32).reshape(-1)
        return arr, arr.ctypes.data, int(arr.size)

    def dump_sizes(self, trees=None):
        """(num_nodes [n], children [n]) int64 of the listed trees (tg_search_dump_sizes): what a dump of them holds."""
        arr, ptr, n = self._tree_list(trees)
        nodes = np.zeros(max(n, 1), dtype=np.int64)
        children = np.zeros(max(n, 1), dtype=np.int64)
        _lib.check(self.lib.tg_search_dump_sizes(self.handle, ptr, n, nodes.ctypes.data, children.ctypes.data, self._stream()),
                   "tg_search_dump_sizes")
        return nodes[:n], children[:n]

    def dump_trees(self, trees=None, check: bool = True):
        """Every node of the listed trees (None: all; any subset in any order, no duplicates) in a fixed number of launches and
        one copy (tg_search_dump_trees): one packed tree per listed tree (tamago_amd/mcts/dump.py: a dict of numpy arrays).
        check: a tree whose sticky error word is set raises (False: the word is the packed tree's "err")."""
        from tamago_amd.mcts import dump as _dump
        arr, ptr, n = self._tree_list(trees)
        nodes, children = self.dump_sizes(trees)
        capacity = sum(_dump.record_bytes(int(a), int(b)) for a, b in zip(nodes, children))
        records = np.zeros(capacity, dtype=np.uint8)
        offsets = np.zeros(n + 1, dtype=np.int64)
        _lib.check(self.lib.tg_search_dump_trees(self.handle, ptr, n, records.ctypes.data, capacity, offsets.ctypes.data,
                                                 self._stream()), "tg_search_dump_trees")
        out = [_dump.parse_record(records[offsets[j]:offsets[j + 1]]) for j in range(n)]
        if check and any(tree["err"] for tree in out):
            self.num_nodes()                     # (raises with the tree's error text, csrc/readout.h error_text)
            raise _lib.TamagoHipError("tg_search_dump_trees: a listed tree's error word is set")
        return out

    def tree_digests(self, trees=None) -> np.ndarray:
        """[n, 2] uint64: the digest of every listed tree, computed on the device without packing anything
        (tg_search_tree_digests; dump.digest_of restates it for a dumped tree)."""
        arr, ptr, n = self._tree_list(trees)
        out = np.zeros((max(n, 1), 2), dtype=np.uint64)
        _lib.check(self.lib.tg_search_tree_digests(self.handle, ptr, n, out.ctypes.data, self._stream()), "tg_search_tree_digests")
        return out[:n]

    # ---- whole-tree write-in ------------------------------------------------------------------------------
    def check_records(self, records, offsets):
        """tg_search_check_records for this engine's board and pool: raises TamagoHipError with the first violated rule."""
        _lib.check(self.lib.tg_search_check_records(self.S, self.N, records.ctypes.data, offsets.ctypes.data, len(offsets) - 1),
                   "tg_search_check_records")

    def load_trees(self, packed_list, trees=None, check: bool = True) -> np.ndarray:
        """Packed trees (tamago_amd/mcts/dump.py) written into the listed trees' pool rows (tg_search_load_trees; trees as in
        dump_trees, None: all).  Every record is checked on the host first (csrc/tree_load.h): one inadmissible record refuses
        the whole call and nothing is launched.  A tree's root position (set_root; a staged one goes up ahead of the load),
        stream, budget and rank table are not touched; its noise row, error word and halt word are cleared.  Returns the flags
        [n]: 1 = the record's side to move is not that of the tree's root position, the tree was left as it was.  check: a
        flag raises."""
        from tamago_amd.mcts import dump as _dump
        arr, ptr, n = self._tree_list(trees)
        if len(packed_list) != n:
            raise ValueError(f"load_trees: {len(packed_list)} packed trees for {n} listed trees")
        records = [_dump.make_record(packed) for packed in packed_list]
        offsets = np.zeros(n + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([r.size for r in records])
        blob = np.concatenate(records) if records else np.zeros(0, dtype=np.uint8)
        flags = np.zeros(max(n, 1), dtype=np.int32)
        _lib.check(self.lib.tg_search_load_trees(self.handle, ptr, n, blob.ctypes.data, offsets.ctypes.data, flags.ctypes.data,
                                                 self._stream()), "tg_search_load_trees")
        flags = flags[:n]
        listed = np.arange(self.T) if arr is None else arr
        nodes = np.array([int(p["num_nodes"]) for p in packed_list], dtype=np.int64)
        loaded = flags == 0
        if loaded.any():
            # node_bound: an upper bound of the nodes in use in any tree; root_children and _kept follow the loaded roots
            self.node_bound = max(int(self.node_bound), int(nodes[loaded].max()))
            children = getattr(self, "root_children", None)
            if children is None or len(children) != self.T:
                children = np.zeros(self.T, dtype=np.int64)
            children = np.asarray(children, dtype=np.int64).copy()
            for j in np.flatnonzero(loaded):
                packed = packed_list[j]
                children[listed[j]] = int(packed["num_children"][0]) if packed["num_nodes"] else 0
                if self._kept is not None:
                    self._kept[0][listed[j]] = int(packed["num_nodes"])
                    self._kept[1][listed[j]] = int(packed["node_visits"][0]) if packed["num_nodes"] else 0
            self.root_children = children
            noise = getattr(self, "noise", None)
            if noise is not None:
                noise[listed[loaded]] = 0.0
        self._queue_stride = 1
        self.live_count = None
        if check and flags.any():
            raise _lib.TamagoHipError(f"tg_search_load_trees: list entries {np.flatnonzero(flags).tolist()}: the record's side to "
                                      "move is not the root position's")
        return flags

    def snapshot(self, trees=None):
        """Per listed tree, everything a continuation needs, as a dict of numpy arrays and ints: the packed tree ("tree"), the
        root position ("cells", "root": read_root_state's scalars, "history"), the stream's state ("stream_key" [624],
        "stream_pos"), the root noise row ("noise") and the halt word ("halt").  NOT in a snapshot: an evaluation cache, visit
        budgets, the live-rank table, a pending leaf queue (take it between mini-batches)."""
        arr, _, n = self._tree_list(trees)
        listed = np.arange(self.T) if arr is None else arr
        packed = self.dump_trees(trees)
        cells = self.read_positions()[0]
        halted, _ = self.read_halt()
        noise = getattr(self, "noise", None)
        out = []
        for j, t in enumerate(int(v) for v in listed):
            root = self.read_root_state(t)
            history = root.pop("history")
            stream = self.streams[t].final_state() if self.streams[t] is not None else None
            out.append({"tree": packed[j], "cells": cells[t].copy(), "root": root, "history": history,
                        "stream_key": None if stream is None else np.asarray(stream[1], dtype=np.uint32).copy(),
                        "stream_pos": -1 if stream is None else int(stream[2]),
                        "noise": np.zeros(self.A) if noise is None else np.asarray(noise[t], dtype=np.float64).copy(),
                        "halt": int(halted[t])})
        return out

    def _set_root_arrays(self, tree: int, snap):
        root = snap["root"]
        cells = np.ascontiguousarray(snap["cells"], dtype=np.uint8)
        assert cells.size == (self.S + 2) ** 2
        hist = np.zeros(max(1, len(snap["history"])), dtype=np.uint64)
        hist[:len(snap["history"])] = snap["history"]
        pos = _lib.RootPosition(cells.ctypes.data, hist.ctypes.data, ctypes.c_uint64(int(root["hash"])), int(root["moves"]),
                                int(root["ko_pos"]), int(root["ko_move"]), int(root["prev"]), int(root["prevprev"]), int(root["to_move"]))
        _lib.check(self.lib.tg_search_set_root(self.handle, tree, ctypes.byref(pos)), "tg_search_set_root")
        if self._kept is not None:
            self._kept[0][tree] = self._kept[1][tree] = 0

    def restore(self, snapshots, trees=None):
        """snapshot()'s inverse, into any listed trees of any engine of the same board size and superko setting whose pool
        holds the trees: the root positions (set_root from the saved arrays), the trees (load_trees), the streams, the noise
        rows and the halt words.  The next puct_batch / puct_chain / gumbel_phase continues as the source engine would have."""
        arr, _, n = self._tree_list(trees)
        listed = [int(v) for v in (np.arange(self.T) if arr is None else arr)]
        if len(snapshots) != n:
            raise ValueError(f"restore: {len(snapshots)} snapshots for {n} listed trees")
        from tamago_amd.mcts import dump as _dump
        records = [_dump.make_record(snap["tree"]) for snap in snapshots]
        offsets = np.zeros(n + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([r.size for r in records])
        self.check_records(np.concatenate(records), offsets)           # (refused before any root is staged)
        for t, snap in zip(listed, snapshots):
            self._set_root_arrays(t, snap)
        self.load_trees([snap["tree"] for snap in snapshots], trees)
        for t, snap in zip(listed, snapshots):
            if snap["stream_key"] is not None and snap["stream_pos"] >= 0:
                self.set_stream(t, ("MT19937", np.asarray(snap["stream_key"], dtype=np.uint32), int(snap["stream_pos"]), 0, 0.0))
        if any(np.any(snap["noise"] != 0.0) for snap in snapshots) or getattr(self, "noise", None) is not None:
            noise = getattr(self, "noise", None)
            noise = np.zeros((self.T, self.A), dtype=np.float64) if noise is None else np.array(noise, dtype=np.float64)
            for t, snap in zip(listed, snapshots):
                noise[t] = snap["noise"]
            _lib.check(self.lib.tg_search_set_noise(self.handle, noise.ctypes.data), "tg_search_set_noise")
            self.noise = noise
        if any(snap["halt"] for snap in snapshots):
            halt = np.zeros(self.T, dtype=np.uint8)
            for t, snap in zip(listed, snapshots):
                halt[t] = 1 if snap["halt"] else 0
            self.set_halt(halt)
