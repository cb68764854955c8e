"""Rows for the row-scoring checks (csrc/row_score.h, tg_score_rows) and the numpy / Python restatement they are held to: rank by
a stable argsort, sums by math.fsum, the logarithm Python's (= libm, which tests/test_host_rng.py holds tg_glibc_log to).  Shared
by tests/test_row_score_host.py (the header on the CPU), tests/test_gpu_row_score.py (the kernels) and
tests/test_gpu_evaluate.py (the pipeline)."""
import math

import numpy as np

ACTIONS = (82, 170, 362)
MOVE_IS_CANDIDATE, VALUE_HIT, INVALID, HAS_MASK = 1, 2, 4, 8
COUNTS = ("rows", "rank0", "rank5", "move_not_candidate", "value_hits", "invalid")
SUMS = ("policy_term", "cand_mass", "value_term", "brier")

ROW_DTYPE = np.dtype([("cand_mass", "<f8"), ("brier", "<f8"), ("p_move", "<u4"), ("rank", "<i4"), ("v_label", "<u4"),
                      ("flags", "<u4"), ("bucket", "<i4"), ("reserved", "<i4")])
BUCKET_DTYPE = np.dtype([("count", "<u8", 6), ("sum", "<f8", 4)])
assert ROW_DTYPE.itemsize == 40 and BUCKET_DTYPE.itemsize == 80


def mask_words(A):
    return (A + 31) // 32


def pack_mask(bits):
    """bool [A] -> uint32 [ceil(A / 32)], bit a of word a // 32; tail bits zero."""
    A = len(bits)
    words = np.zeros(mask_words(A), dtype=np.uint32)
    for a in np.nonzero(bits)[0]:
        words[a >> 5] |= np.uint32(1 << (a & 31))
    return words


def unpack_mask(words, A):
    return np.array([(int(words[a >> 5]) >> (a & 31)) & 1 for a in range(A)], dtype=bool)


class Rows:
    """n rows: policy float32 [n, A], value float32 [n, 3], mask uint32 [n, W], move / cls / ply int32 [n]."""

    def __init__(self, A):
        self.A = A
        self.policy, self.value, self.mask, self.move, self.cls, self.ply = [], [], [], [], [], []

    def add(self, policy, value, move, cls, ply, bits=None):
        policy = np.asarray(policy, dtype=np.float32)
        assert policy.shape == (self.A,)
        if bits is None:                                                     # a plausible mask: the larger half and PASS
            bits = policy >= np.median(policy[~np.isnan(policy)]) if not np.isnan(policy).all() else np.ones(self.A, bool)
            bits = np.array(bits)
            bits[self.A - 1] = True
        self.policy.append(policy)
        self.value.append(np.asarray(value, dtype=np.float32))
        self.mask.append(pack_mask(np.asarray(bits, dtype=bool)))
        self.move.append(move)
        self.cls.append(cls)
        self.ply.append(ply)

    def arrays(self, n=None):
        n = len(self.move) if n is None else n
        assert n <= len(self.move)
        return (np.ascontiguousarray(np.stack(self.policy[:n])), np.ascontiguousarray(np.stack(self.value[:n])),
                np.ascontiguousarray(np.stack(self.mask[:n])), np.array(self.move[:n], dtype=np.int32),
                np.array(self.cls[:n], dtype=np.int32), np.array(self.ply[:n], dtype=np.int32))


def softmax32(x):
    e = np.exp(x - x.max())
    return (e / e.sum()).astype(np.float32)


def corpus(A, n_random=230, seed=0, bucket_width=10, n_buckets=32):
    """Crafted rows first, random rows behind them (more than 257 in all)."""
    rnd = np.random.RandomState(1000 * A + seed)
    P = A - 1
    rows = Rows(A)
    third = (np.float32(1) / 3,) * 3
    last = bucket_width * n_buckets

    def rand_policy():
        return softmax32(rnd.standard_normal(A) * 2.0)

    def rand_value():
        return softmax32(rnd.standard_normal(3))

    # a plain row first (n = 1 scores this one)
    rows.add(rand_policy(), rand_value(), 17, 2, 3)
    # the move at index 0, 63, 64 and P (PASS), with ties equal to p_move before and after it
    for move in (0, 63, 64, P):
        pol = rand_policy()
        rows.add(pol, rand_value(), move, int(rnd.randint(3)), int(rnd.randint(400)))
        tied = pol.copy()
        others = [a for a in (1, 62, 65, 70, P - 1) if a != move]
        tied[others] = tied[move]
        rows.add(tied, rand_value(), move, int(rnd.randint(3)), int(rnd.randint(400)))
        top = pol.copy()                                                      # ... and tied for the maximum
        top[[move] + others] = top.max() * np.float32(1.5)
        rows.add(top, rand_value(), move, int(rnd.randint(3)), int(rnd.randint(400)))
    # an all-equal row: the rank is the index
    for move in (0, 5, 64, P):
        rows.add(np.full(A, 1.0 / A, np.float32), third, move, move % 3, 7)
    # a one-hot row: the move on it, before it and behind it (p_move == 0, tied with every other zero)
    hot = np.zeros(A, np.float32)
    hot[40] = 1.0
    for move in (40, 3, 41, P):
        rows.add(hot, (0, 0, 1), move, 2, 11)
    # value ties: the FIRST maximum is the hit
    for value in ((0.5, 0.5, 0.0), (0.0, 0.5, 0.5), (0.5, 0.0, 0.5), third):
        for cls in (0, 1, 2):
            rows.add(rand_policy(), value, int(rnd.randint(A)), cls, int(rnd.randint(400)))
    # NaN rows, moves and classes out of range: invalid, whatever else they hold
    nan_pol = rand_policy()
    nan_pol[A - 2] = np.nan
    rows.add(nan_pol, rand_value(), 4, 1, 20)
    rows.add(rand_policy(), (0.5, np.nan, 0.5), 4, 1, 25)
    rows.add(np.full(A, np.nan, np.float32), third, 4, 1, 25)
    for move, cls in ((-1, 1), (A, 1), (5, -1), (5, 3), (1 << 20, 0)):
        rows.add(rand_policy(), rand_value(), move, cls, 30)
    # masks with only PASS set, and with every bit set; the move in and out of the mask
    only_pass = np.zeros(A, bool)
    only_pass[P] = True
    for move in (0, P):
        rows.add(rand_policy(), rand_value(), move, 0, 33, only_pass)
        rows.add(rand_policy(), rand_value(), move, 0, 34, np.ones(A, bool))
    # the bucket rule at its edge: the last ply of the last regular bucket, the first ply beyond, far beyond
    for ply in (0, bucket_width - 1, bucket_width, last - bucket_width - 1, last - bucket_width, last - 1, last, last + 1, 100000):
        rows.add(rand_policy(), rand_value(), int(rnd.randint(A)), int(rnd.randint(3)), ply)
    # random rows: peaked and flat policies, random masks
    for _ in range(n_random):
        pol = softmax32(rnd.standard_normal(A) * rnd.choice([0.1, 1.0, 4.0]))
        bits = rnd.random_sample(A) < rnd.choice([0.2, 0.6, 0.95])
        bits[P] = True
        move = int(np.argmax(pol)) if rnd.random_sample() < 0.4 else int(rnd.randint(A))
        rows.add(pol, rand_value(), move, int(rnd.randint(3)), int(rnd.randint(last + 40)), bits)
    return rows


# ---- the restatement ------------------------------------------------------------------------------------------------------
def bucket_of(ply, bucket_width, n_buckets):
    return min(max(int(ply), 0) // bucket_width, n_buckets - 1)


def restate_row(policy, value, words, move, cls, ply, bucket_width, n_buckets):
    """-> dict: the record's members (p_move / v_label as uint32 bits) and `mass_terms`, the addends of cand_mass."""
    A = len(policy)
    move, cls = int(move), int(cls)
    rec = {"cand_mass": 0.0, "brier": 0.0, "p_move": 0, "rank": -1, "v_label": 0, "flags": HAS_MASK if words is not None else 0,
           "bucket": bucket_of(ply, bucket_width, n_buckets), "mass_terms": []}
    if not (0 <= move < A and 0 <= cls <= 2) or np.isnan(policy).any() or np.isnan(value).any():
        rec["flags"] |= INVALID
        return rec
    order = np.argsort(-policy, kind="stable")                                # descending, equal probabilities in index order
    rec["rank"] = int(np.nonzero(order == move)[0][0])
    rec["p_move"] = int(policy[move:move + 1].view(np.uint32)[0])
    rec["v_label"] = int(value[cls:cls + 1].view(np.uint32)[0])
    if words is not None:
        bits = unpack_mask(words, A)
        rec["mass_terms"] = [float(p) for p in policy[bits]]
        rec["cand_mass"] = math.fsum(rec["mass_terms"])
        if bits[move]:
            rec["flags"] |= MOVE_IS_CANDIDATE
    if int(np.argmax(value)) == cls:
        rec["flags"] |= VALUE_HIT
    d = 0.5 * cls - (float(value[2]) + 0.5 * float(value[1]))
    rec["brier"] = d * d
    return rec


def restate(arrays, bucket_width, n_buckets, with_mask=True):
    policy, value, mask, move, cls, ply = arrays
    return [restate_row(policy[i], value[i], mask[i] if with_mask else None, move[i], cls[i], ply[i], bucket_width, n_buckets)
            for i in range(len(move))]


def row_terms(rec, cand_mass=None):
    """The four fp64 addends of a valid row; cand_mass: the mass to use in place of the restatement's (a device record's)."""
    pm = float(np.array([rec["p_move"]], dtype=np.uint32).view(np.float32)[0])
    vl = float(np.array([rec["v_label"]], dtype=np.uint32).view(np.float32)[0])
    return (-math.log(pm + 1e-8), rec["cand_mass"] if cand_mass is None else cand_mass, -math.log(vl + 1e-8), rec["brier"])


def restate_table(records, n_buckets, cand_mass=None):
    """-> counts int [n_buckets, 6], terms: [n_buckets][4] lists of addends.  cand_mass: per-row masses to sum instead."""
    counts = np.zeros((n_buckets, 6), dtype=np.int64)
    terms = [[[] for _ in SUMS] for _ in range(n_buckets)]
    for i, rec in enumerate(records):
        b = rec["bucket"]
        if rec["flags"] & INVALID:
            counts[b, 5] += 1
            continue
        counts[b, 0] += 1
        counts[b, 1] += rec["rank"] == 0
        counts[b, 2] += rec["rank"] < 5
        counts[b, 3] += bool(rec["flags"] & HAS_MASK) and not rec["flags"] & MOVE_IS_CANDIDATE
        counts[b, 4] += bool(rec["flags"] & VALUE_HIT)
        for s, term in enumerate(row_terms(rec, None if cand_mass is None else float(cand_mass[i]))):
            terms[b][s].append(term)
    return counts, terms


def sum_bound(terms):
    """k * 2^-52 * sum |term|: the standard bound for an fp64 sum of k terms in any order."""
    return len(terms) * 2.0 ** -52 * math.fsum(abs(t) for t in terms)


def check_records(got, want, arrays=None):
    """got: structured array (ROW_DTYPE) or list of dicts with the same keys; want: restate()'s list.  Bit for bit in p_move,
    rank, v_label, flags, bucket and brier; cand_mass within the summation bound of its addends."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert int(g["flags"]) == w["flags"] and int(g["bucket"]) == w["bucket"], (i, int(g["flags"]), w["flags"], int(g["bucket"]), w["bucket"])
        if w["flags"] & INVALID:
            continue
        assert int(g["p_move"]) == w["p_move"] and int(g["rank"]) == w["rank"] and int(g["v_label"]) == w["v_label"], \
            (i, int(g["rank"]), w["rank"], int(g["p_move"]), w["p_move"])
        assert float(g["brier"]) == w["brier"], (i, float(g["brier"]), w["brier"])
        assert abs(float(g["cand_mass"]) - w["cand_mass"]) <= sum_bound(w["mass_terms"]), (i, float(g["cand_mass"]), w["cand_mass"])


def check_table(got, records, n_buckets, masses):
    """got: structured array (BUCKET_DTYPE) [n_buckets]; counts exact, every sum within the bound of its addends (cand_mass:
    the addends are the rows' own masses, `masses`)."""
    counts, terms = restate_table(records, n_buckets, masses)
    assert np.array_equal(np.asarray(got["count"], dtype=np.int64), counts), (np.asarray(got["count"]).tolist(), counts.tolist())
    for b in range(n_buckets):
        for s in range(len(SUMS)):
            assert abs(float(got["sum"][b][s]) - math.fsum(terms[b][s])) <= sum_bound(terms[b][s]), (b, SUMS[s])
