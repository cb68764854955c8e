"""Shared cases of the evaluation-cache tests (test_eval_cache_host.py, test_gpu_eval_cache.py): numpy restatements of the
key and the hash of csrc/eval_cache.h, the model of what a cache without overflow serves, rows, and the oracle's evaluated-row
logs of the games the GPU tests play."""
import functools

import numpy as np

from oracle.stubnet import StubNet, plane_hash
from tests import _puct_match_cases as pc
from tests._match_cases import make_net

ONE, ZERO, MINUS_ONE = 0x3f800000, 0x00000000, 0xbf800000
HIT, MISS, UNCACHED = 0, 1, 2
M64 = (1 << 64) - 1


def words_per_plane(P):
    return (P + 31) // 32


def key_words(P):
    return 5 * words_per_plane(P) + 1


def entry_words(P):
    return (2 + key_words(P) + (P + 1) + 3 + 3) // 4 * 4


def canonical(row: np.ndarray) -> bool:
    """The issue's words: every value of planes 0-4 is exactly 0.0f or 1.0f, plane 5 uniformly +1.0f or uniformly -1.0f.
    row: float32 [6, P] (compared by bit pattern: -0.0f is not 0.0f)."""
    bits = np.ascontiguousarray(row, dtype=np.float32).view(np.uint32).reshape(6, -1)
    body = np.isin(bits[:5], (ZERO, ONE)).all()
    return bool(body and ((bits[5] == ONE).all() or (bits[5] == MINUS_ONE).all()))


def pack(row: np.ndarray, want_logits: bool) -> np.ndarray:
    """Key words of a canonical row: one bit per point of planes 0-4, ceil(P / 32) words a plane, tail bits zero, and the word
    colour | want_logits << 1."""
    bits = np.ascontiguousarray(row, dtype=np.float32).view(np.uint32).reshape(6, -1)
    P = bits.shape[1]
    wpp = words_per_plane(P)
    key = np.zeros(key_words(P), dtype=np.uint64)
    for pl in range(5):
        padded = np.zeros(wpp * 32, dtype=np.uint64)
        padded[:P] = bits[pl] == ONE
        key[pl * wpp:(pl + 1) * wpp] = (padded.reshape(wpp, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1)
    key[5 * wpp] = (1 if bits[5][0] == ONE else 0) | (2 if want_logits else 0)
    return key.astype(np.uint32)


def mix(x: int) -> int:
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def hash_key(key) -> int:
    total = 0
    for i, w in enumerate(key):
        total = (total + mix(((i + 1) << 32) | int(w))) & M64
    return mix((total + 0x9E3779B97F4A7C15) & M64)


def placement(h: int, n_buckets: int, ways: int):
    """(bucket, tag, victim way) of a hash."""
    tag = h >> 32
    return (h & 0xffffffff) % n_buckets, tag if tag else 1, (h >> 40) % ways


def random_rows(rnd, S: int, n: int, density: float = 0.3) -> np.ndarray:
    """n random canonical rows float32 [n, 6, S, S]: planes 0-4 of zeros and ones, plane 5 of the row's colour."""
    rows = (rnd.random_sample((n, 6, S, S)) < density).astype(np.float32)
    rows[:, 5] = np.where(rnd.random_sample(n) < 0.5, 1.0, -1.0).astype(np.float32)[:, None, None]
    return rows


class DictModel:
    """What a cache that never overflows serves: a row hits iff an equal row (and want_logits) was committed in an EARLIER
    call since the last clear; in-call twins all miss and are inserted once; a row that is not canonical always misses."""

    def __init__(self):
        self.known = set()
        self.stats = dict(lookups=0, hits=0, uncacheable=0, inserts=0, twin_skips=0)

    def clear(self):
        self.known = set()

    def call(self, rows: np.ndarray, want_logits: bool):
        """-> flags [n] (HIT / MISS / UNCACHED)."""
        flags, fresh = [], set()
        for row in rows:
            self.stats["lookups"] += 1
            if not canonical(row):
                flags.append(UNCACHED)
                self.stats["uncacheable"] += 1
                continue
            k = (row.astype(np.float32).tobytes(), bool(want_logits))
            if k in self.known:
                flags.append(HIT)
                self.stats["hits"] += 1
            else:
                flags.append(MISS)
                self.stats["twin_skips" if k in fresh else "inserts"] += 1
                fresh.add(k)
        self.known |= fresh
        return np.array(flags)


# ---- the oracle's evaluated rows ---------------------------------------------------------------------------------------------
class LoggingNet:
    """An evaluator that logs (want_logits, oracle.stubnet.plane_hash of every row) per call before it forwards."""

    def __init__(self, inner, log):
        self.inner, self.log = inner, log

    def inference(self, planes):
        self.log.append((False, [int(h) for h in plane_hash(planes.numpy())]))
        return self.inner.inference(planes)

    def inference_with_policy_logits(self, planes):
        self.log.append((True, [int(h) for h in plane_hash(planes.numpy())]))
        return self.inner.inference_with_policy_logits(planes)


def repeats(log):
    """(rows, rows a cache without overflow serves) of one network's call log: a row is served iff an identical row (and
    want_logits) came in an EARLIER call."""
    known, total, served = set(), 0, 0
    for want_logits, hashes in log:
        keys = [(want_logits, h) for h in hashes]
        total += len(keys)
        served += sum(1 for k in keys if k in known)
        known.update(keys)
    return total, served


MATCH_SEED = 1


@functools.lru_cache(maxsize=None)
def oracle_match_logs(shared: bool):
    """The evaluator call logs of oracle game MATCH_SEED (tests/_puct_match_cases: black 26 visits x 8, white 20 x 6) and its
    record.  shared False: StubNet(301) black, StubNet(302) white, a log - a cache - each; True: StubNet(301) on both sides,
    one log.  With ONE board a lock-step match makes exactly the oracle's calls."""
    if shared:
        log = []
        net = LoggingNet(make_net(pc.S301), log)
        text, (moves, ending), state = pc.oracle_puct_match_game(MATCH_SEED, net, net)
        return text, moves, ending, state, (log,)
    black_log, white_log = [], []
    text, (moves, ending), state = pc.oracle_puct_match_game(MATCH_SEED, LoggingNet(make_net(pc.S301), black_log),
                                                             LoggingNet(make_net(pc.S302), white_log))
    return text, moves, ending, state, (black_log, white_log)


def oracle_match_counts(shared: bool):
    """(rows handed to the networks, rows served from the caches) of that game."""
    logs = oracle_match_logs(shared)[4]
    pairs = [repeats(log) for log in logs]
    return sum(p[0] for p in pairs), sum(p[1] for p in pairs)


TWO_MOVES = (3, 60, 8)            # (seed, visits, batch) of the two consecutive single-tree searches


@functools.lru_cache(maxsize=None)
def oracle_two_moves():
    """Two consecutive searches of one oracle tree from the empty 9x9 board under StubNet(7): search, play the best move,
    search again for the other colour.  -> (first move, [(rows, served)] after each search, cumulative over one cache)."""
    from oracle.board import GoBoard, BLACK
    from oracle.tree import MCTSTree, TimeControl, TimeManager
    seed, visits, batch = TWO_MOVES
    log = []
    tree = MCTSTree(LoggingNet(StubNet(7), log), 9, tree_size=visits + 16, batch_size=batch)
    saved = np.random.get_state()
    np.random.seed(seed)
    try:
        board = GoBoard(9, 7.0, False)
        first = tree.search_best_move(board, BLACK, TimeManager(TimeControl.STRICT_PLAYOUT, visits))
        after_first = repeats(log)
        board.put_stone(first, BLACK)
        second = tree.search_best_move(board, 3 - BLACK, TimeManager(TimeControl.STRICT_PLAYOUT, visits))
        return first, second, [after_first, repeats(log)]
    finally:
        np.random.set_state(saved)
