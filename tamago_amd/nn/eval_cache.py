"""Evaluation cache: network outputs served from a hash table in device memory, keyed by the exact input planes.

``EvalCache`` owns the table (tg_evalcache_*: csrc/eval_cache.hip, the rules in csrc/eval_cache.h); ``CachedEvaluator`` wraps ANY
evaluator of the search engine - DeviceEvaluator or HostEvaluator - at the evaluator boundary: probe, the inner evaluator on
the rows that missed, commit.  A hit returns the bits that were committed for an equal row, so trees, moves, records and
stream positions are those of the run without a cache (under the forward kernels' own caveat: bit for bit across launch
shapes only while no f16 range fallback is taken).  Opt-in everywhere; there is no fallback: without the library's kernels
the calls raise."""
import ctypes
from typing import List

import numpy as np
import torch

from tamago_amd import lib as _lib

STAT_NAMES = ("lookups", "hits", "uncacheable", "inserts", "twin_skips", "evictions", "dropped", "tag_only_matches")
DEFAULT_WAYS = 8


def key_words(board_size: int) -> int:
    """Words of a key: the bit image of planes 0-4, ceil(P / 32) words a plane, and the colour / want_logits word."""
    return 5 * ((board_size * board_size + 31) // 32) + 1


class _DeviceRows:
    """A borrowed device buffer [rows, 6, S, S] fp32 as torch sees it (``__cuda_array_interface__``): no copy."""

    def __init__(self, ptr: int, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "version": 2,
                                         "strides": None}


class EvalCache:
    """``entries`` entries in buckets of ``ways`` ways for ``board_size`` (9, 13, 19) on ``cuda:device_index``.  One cache
    belongs to ONE network's outputs and is used from one stream at a time; ``clear()`` when the weights change
    (CachedEvaluator does that for a DualNet)."""

    def __init__(self, board_size: int, entries: int, ways: int = DEFAULT_WAYS, device_index: int = 0):
        self.lib = _lib.load()
        self.board_size, self.ways, self.device_index = int(board_size), int(ways), int(device_index)
        # (whole buckets: a request is rounded down to a multiple of the ways, and up to one bucket - `--eval-cache 1` is a
        # valid, tiny table; zero, negative or oversized requests the library refuses)
        self.entries = max(int(entries) // self.ways, 1) * self.ways if self.ways > 0 and int(entries) > 0 else int(entries)
        # whose outputs the table holds: (id(network), its weight_version) as of the last use (None: nobody's yet).  Kept HERE,
        # not in an evaluator: evaluators come and go with engines while the table lives on
        self.filled_under = None
        self.device = torch.device("cuda", device_index)
        handle = ctypes.c_void_p()
        _lib.check(self.lib.tg_evalcache_create(self.board_size, self.device_index, self.entries, self.ways, ctypes.byref(handle)),
                   "tg_evalcache_create")
        self.handle = handle

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def close(self):
        if self.handle is not None:
            self.lib.tg_evalcache_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def claim(self, network):
        """The table is about to serve and take `network`'s outputs: cleared first if what it holds was filled under another
        network object or other weights of this one (DualNet.weight_version)."""
        key = (id(network), getattr(network, "weight_version", None))
        if self.filled_under is not None and self.filled_under != key:
            self.clear()
        self.filled_under = key

    def set_timing(self, on: bool):
        """Measurement only: timed events around every launch of the following probes and commits (tg_evalcache_set_timing)."""
        _lib.check(self.lib.tg_evalcache_set_timing(self.handle, int(bool(on))), "tg_evalcache_set_timing")

    def read_timing(self) -> dict:
        """Kernel times (ms) of the last timed probe and of its commit (0.0 when none was launched); waits for them."""
        ms = np.zeros(4, dtype=np.float32)
        _lib.check(self.lib.tg_evalcache_read_timing(self.handle, ms.ctypes.data), "tg_evalcache_read_timing")
        return dict(zip(("probe_ms", "rank_ms", "gather_ms", "commit_ms"), (float(v) for v in ms)))

    def clear(self):
        _lib.check(self.lib.tg_evalcache_clear(self.handle, self._stream()), "tg_evalcache_clear")

    def stats(self, reset: bool = False) -> dict:
        """The device counters (STAT_NAMES; evictions are part of inserts).  Synchronises the device."""
        out = np.zeros(8, dtype=np.uint64)
        _lib.check(self.lib.tg_evalcache_stats(self.handle, out.ctypes.data, int(reset)), "tg_evalcache_stats")
        return {name: int(v) for name, v in zip(STAT_NAMES, out)}

    def _check_planes(self, planes) -> int:
        s = self.board_size
        if not (planes.is_cuda and planes.dtype == torch.float32 and planes.is_contiguous()):
            raise ValueError("expected a contiguous float32 CUDA tensor of planes")
        if tuple(planes.shape[1:]) != (6, s, s):
            raise ValueError(f"expected [B,6,{s},{s}], got {tuple(planes.shape)}")
        return s

    def probe(self, planes: torch.Tensor, want_logits: bool, policy: torch.Tensor, value: torch.Tensor):
        """Fills the hit rows of policy / value; returns (n_miss, miss_planes [n_miss,6,S,S] - the cache's own buffer, valid
        until the next probe; None when nothing missed).  Waits for the stream once."""
        s = self._check_planes(planes)
        n_miss, ptr = ctypes.c_int32(0), ctypes.c_void_p()
        _lib.check(self.lib.tg_evalcache_probe(self.handle, planes.data_ptr(), planes.shape[0], int(bool(want_logits)), policy.data_ptr(),
                                               value.data_ptr(), self._stream(), ctypes.byref(n_miss), ctypes.byref(ptr)),
                   "tg_evalcache_probe")
        n = int(n_miss.value)
        if n == 0:
            return 0, None
        return n, torch.as_tensor(_DeviceRows(ptr.value, (n, 6, s, s)), device=self.device)

    def commit(self, miss_policy, miss_value, policy: torch.Tensor, value: torch.Tensor):
        _lib.check(self.lib.tg_evalcache_commit(self.handle, None if miss_policy is None else miss_policy.data_ptr(),
                                                None if miss_value is None else miss_value.data_ptr(), policy.data_ptr(),
                                                value.data_ptr(), self._stream()), "tg_evalcache_commit")

    def forward(self, network, planes: torch.Tensor, want_logits: bool, policy: torch.Tensor, value: torch.Tensor) -> int:
        """tg_evalcache_forward on a DualNet: probe, the network over the rows that missed, commit - one library call.
        Returns how many rows the network evaluated."""
        s = self._check_planes(planes)
        _lib.check(self.lib.tg_evalcache_forward(self.handle, network.handle, planes.data_ptr(), planes.shape[0], int(bool(want_logits)),
                                                 policy.data_ptr(), value.data_ptr(), self._stream()), "tg_evalcache_forward")
        n_miss = ctypes.c_int32(0)
        _lib.check(self.lib.tg_evalcache_last_misses(self.handle, ctypes.byref(n_miss)), "tg_evalcache_last_misses")
        return int(n_miss.value)

    def debug_read(self, index: int):
        """Entry `index` (bucket * ways + way): (tag word, key words uint32 [K], policy float32 [A], value float32 [3])."""
        a = self.board_size ** 2 + 1
        tag = ctypes.c_uint64(0)
        key = np.zeros(key_words(self.board_size), dtype=np.uint32)
        policy, value = np.zeros(a, dtype=np.float32), np.zeros(3, dtype=np.float32)
        _lib.check(self.lib.tg_evalcache_debug_read(self.handle, int(index), ctypes.byref(tag), key.ctypes.data, policy.ctypes.data,
                                                    value.ctypes.data), "tg_evalcache_debug_read")
        return int(tag.value), key, policy, value


def caches_for(networks, board_size: int, entries: int, device_index: int = 0, ways: int = DEFAULT_WAYS) -> dict:
    """{id(network): EvalCache} - one cache of `entries` entries per DISTINCT network object: two setups on the same network
    share one, two networks never do."""
    out = {}
    for network in networks:
        if id(network) not in out:
            out[id(network)] = EvalCache(board_size, entries, ways, device_index)
    return out


def total_stats(caches) -> dict:
    """The counters of several caches added up, and the entries they hold room for."""
    out = {name: 0 for name in STAT_NAMES}
    for cache in caches:
        for name, v in cache.stats().items():
            out[name] += v
    out["entries"] = sum(c.entries for c in caches)
    out["caches"] = len(caches)
    return out


class CachedEvaluator:
    """``inner`` (a DeviceEvaluator, a HostEvaluator, anything with their call) behind ``cache``.  ``batches`` records the
    positions really evaluated; ``handed`` what the engine handed over.  A wrapped DeviceEvaluator goes through
    tg_evalcache_forward (one library call: probe, forward over the misses, commit).  Not exactly DeviceEvaluator, so
    SearchEngine.can_chain is false and every driver takes its mini-batch by mini-batch path: the miss count needs a host
    look per forward pass anyway."""

    def __init__(self, inner, cache: EvalCache):
        self.inner, self.cache = inner, cache
        self.network = getattr(inner, "network", None)
        self.batches: List[int] = []
        self.handed = 0

    def __call__(self, planes: torch.Tensor, want_logits: bool):
        from tamago_amd.mcts.engine import DeviceEvaluator
        self.cache.claim(self.network)            # (new weights, or another network's table: cleared before it serves)
        cache, b = self.cache, int(planes.shape[0])
        a = cache.board_size ** 2 + 1
        policy = torch.empty((b, a), dtype=torch.float32, device=planes.device)
        value = torch.empty((b, 3), dtype=torch.float32, device=planes.device)
        self.handed += b
        if type(self.inner) is DeviceEvaluator:
            n_miss = cache.forward(self.network, planes, want_logits, policy, value)
            if n_miss:
                self.batches.append(n_miss)
                self.inner.batches.append(n_miss)
            return policy, value
        n_miss, miss_planes = cache.probe(planes, want_logits, policy, value)
        if n_miss:
            miss_policy, miss_value = self.inner(miss_planes, want_logits)
            self.batches.append(n_miss)
            cache.commit(miss_policy.contiguous(), miss_value.contiguous(), policy, value)
        else:
            cache.commit(None, None, policy, value)
        return policy, value
