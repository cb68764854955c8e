// Row scoring: what one evaluated position of a game record contributes to an evaluation report - the probability
// and the rank of the move played, the prior mass on the candidates the tree would expand, the value of the record's result - and
// how the rows add up into a table of ply buckets.  Pure arithmetic, no HIP: row_score.hip compiles this text for the device,
// tests/row_score_driver.cpp for the host (tests/test_row_score_host.py), so the CPU checks the very rules the kernels apply, in
// the kernels' order of operations (one wavefront per row; one workgroup per bucket).  The logarithm is a parameter: the kernels
// pass tg_rng::glibc_log, the host driver libm's.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define TG_SCORE_FN __host__ __device__ inline
#else
#define TG_SCORE_FN inline
#endif

namespace tg_score {

constexpr int kLanes = 64;                 // one wavefront per row: ceil(A / 64) lane passes
constexpr int kReduceThreads = 256;        // one workgroup per bucket in the table launch
constexpr int kReduceWaves = kReduceThreads / kLanes;

// flag bits of a row record
constexpr uint32_t kMoveIsCandidate = 1u;  // the move played is in the candidate mask (never set without masks)
constexpr uint32_t kValueHit = 2u;         // the first maximum of the three values is the record's class
constexpr uint32_t kInvalid = 4u;          // move or class out of range, or a NaN in the row: counts as invalid and nothing else
constexpr uint32_t kHasMask = 8u;          // the call had candidate masks: cand_mass and kMoveIsCandidate mean something

// One row, 40 bytes.  Of an invalid row only `flags` and `bucket` are specified (the other members are zero, rank -1).
struct RowRecord {
    double cand_mass;                      // sum of (double)policy[a] over the set mask bits (0 without masks)
    double brier;                          // (score - expected)^2 of the value head (brier_term)
    uint32_t p_move;                       // the bits of policy[move]
    int32_t rank;                          // position of the move in a stable descending sort of the policy
    uint32_t v_label;                      // the bits of value[class]
    uint32_t flags;
    int32_t bucket;                        // min(ply / bucket_width, n_buckets - 1)
    int32_t reserved;
};
static_assert(sizeof(RowRecord) == 40, "RowRecord is part of the ABI (tg_score_row)");

// One ply bucket, 80 bytes.
enum { kRows = 0, kRank0, kRank5, kMoveNotCandidate, kValueHits, kInvalidRows, kCounts };
enum { kPolicyTerm = 0, kCandMass, kValueTerm, kBrier, kSums };
struct Bucket {
    uint64_t count[kCounts];
    double sum[kSums];
};
static_assert(sizeof(Bucket) == 80, "Bucket is part of the ABI (tg_score_bucket)");

TG_SCORE_FN float bits_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
TG_SCORE_FN uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// The rules (the tests put wrong ones here).
struct Rule {
    // action a (probability p) stands before the move (probability pm) in a stable descending sort
    static TG_SCORE_FN bool ahead(float p, int a, float pm, int move) { return p > pm || (p == pm && a < move); }
    // numpy's argmax of the three values: the first maximum
    static TG_SCORE_FN int value_argmax(float v0, float v1, float v2) {
        int best = 0;
        float m = v0;
        if (v1 > m) { m = v1; best = 1; }
        if (v2 > m) { best = 2; }
        return best;
    }
};

// A ply before the first counts into the first bucket (records have none; the table has no other place for it).
TG_SCORE_FN int32_t bucket_of(int32_t ply, int32_t bucket_width, int32_t n_buckets) {
    if (ply < 0) return 0;
    const int32_t b = ply / bucket_width;
    return b < n_buckets - 1 ? b : n_buckets - 1;
}

TG_SCORE_FN bool mask_bit(const uint32_t *mask, int a) { return (mask[a >> 5] >> (a & 31)) & 1u; }

// What one lane brings to its row: the actions a = lane, lane + 64, ... in that order.
struct LanePart {
    int32_t ahead;
    int32_t nan;
    double mass;
};
template <class R = Rule>
TG_SCORE_FN LanePart lane_part(const float *policy, const uint32_t *mask, int A, int lane, bool move_ok, float pm, int move) {
    LanePart part{0, 0, 0.0};
    for (int a = lane; a < A; a += kLanes) {
        const float p = policy[a];
        part.nan |= p != p;
        if (move_ok && R::ahead(p, a, pm, move)) ++part.ahead;
        if (mask && mask_bit(mask, a)) part.mass += (double)p;
    }
    return part;
}

// (score - expected)^2: score 1 / 0.5 / 0 for class 2 / 1 / 0, expected = value[2] + 0.5 * value[1]
TG_SCORE_FN double brier_term(int cls, float v1, float v2) {
    const double d = 0.5 * (double)cls - ((double)v2 + 0.5 * (double)v1);
    return d * d;
}

// The record from the wavefront's totals: `ahead` and `nan` summed over the lanes, `mass` by the butterfly (wave_sum_host).
template <class R = Rule>
TG_SCORE_FN RowRecord finish_row(const float *policy, const float *value, const uint32_t *mask, int A, int move, int cls, int32_t ply,
                                 int32_t bucket_width, int32_t n_buckets, int32_t ahead, bool any_nan, double mass) {
    RowRecord rec{0.0, 0.0, 0u, -1, 0u, mask ? kHasMask : 0u, bucket_of(ply, bucket_width, n_buckets), 0};
    const float v0 = value[0], v1 = value[1], v2 = value[2];
    const bool ok = move >= 0 && move < A && cls >= 0 && cls <= 2 && !any_nan && v0 == v0 && v1 == v1 && v2 == v2;
    if (!ok) { rec.flags |= kInvalid; return rec; }
    rec.p_move = float_bits(policy[move]);
    rec.rank = ahead;
    rec.cand_mass = mask ? mass : 0.0;
    rec.v_label = float_bits(value[cls]);
    rec.brier = brier_term(cls, v1, v2);
    if (mask && mask_bit(mask, move)) rec.flags |= kMoveIsCandidate;
    if (R::value_argmax(v0, v1, v2) == cls) rec.flags |= kValueHit;
    return rec;
}

// The cross-lane sum of the table launch and of cand_mass: an xor butterfly, steps 1, 2, ... 32 (a + b == b + a, so every lane
// ends with the same bits).  On the host over an array of kLanes values.
inline double wave_sum_host(double *v) {
    for (int step = 1; step < kLanes; step <<= 1) {
        double next[kLanes];
        for (int l = 0; l < kLanes; ++l) next[l] = v[l] + v[l ^ step];
        for (int l = 0; l < kLanes; ++l) v[l] = next[l];
    }
    return v[0];
}

// The kernel's order of operations for one row, on the host.
template <class R = Rule>
inline RowRecord score_row(const float *policy, const float *value, const uint32_t *mask, int A, int move, int cls, int32_t ply,
                           int32_t bucket_width, int32_t n_buckets) {
    const bool move_ok = move >= 0 && move < A;
    const float pm = move_ok ? policy[move] : 0.f;
    int32_t ahead = 0;
    bool any_nan = false;
    double mass[kLanes];
    for (int lane = 0; lane < kLanes; ++lane) {
        const LanePart part = lane_part<R>(policy, mask, A, lane, move_ok, pm, move);
        ahead += part.ahead;
        any_nan |= part.nan != 0;
        mass[lane] = part.mass;
    }
    return finish_row<R>(policy, value, mask, A, move, cls, ply, bucket_width, n_buckets, ahead, any_nan, wave_sum_host(mass));
}

// What a row adds to its bucket: six counts and four fp64 terms.
struct Terms {
    uint32_t count[kCounts];
    double sum[kSums];
};
template <class Log>
TG_SCORE_FN Terms row_terms(const RowRecord &rec, Log log_fn) {
    Terms t{};
    if (rec.flags & kInvalid) { t.count[kInvalidRows] = 1; return t; }
    t.count[kRows] = 1;
    t.count[kRank0] = rec.rank == 0;
    t.count[kRank5] = rec.rank < 5;
    t.count[kMoveNotCandidate] = (rec.flags & kHasMask) && !(rec.flags & kMoveIsCandidate);
    t.count[kValueHits] = (rec.flags & kValueHit) != 0;
    const double pm = (double)bits_float(rec.p_move), vl = (double)bits_float(rec.v_label);
    t.sum[kPolicyTerm] = -log_fn(pm + 1e-8);          // calculate_policy_loss (nn/loss.py:9-19) with a one-hot target
    t.sum[kCandMass] = rec.cand_mass;
    t.sum[kValueTerm] = -log_fn(vl + 1e-8);
    t.sum[kBrier] = rec.brier;
    return t;
}

// The table launch for bucket b, on the host: thread t of kReduceThreads takes the rows t, t + 256, ... in that order, the 64
// threads of a wavefront are summed by the butterfly, the wavefronts in their order, and the result is added to the bucket.
template <class Log>
inline void reduce_bucket(const RowRecord *rec, int64_t n, int32_t b, Bucket &acc, Log log_fn) {
    uint64_t count[kCounts] = {};
    double sum[kSums] = {};
    for (int w = 0; w < kReduceWaves; ++w) {
        double part[kSums][kLanes];
        for (int l = 0; l < kLanes; ++l) {
            for (int s = 0; s < kSums; ++s) part[s][l] = 0.0;
            for (int64_t r = w * kLanes + l; r < n; r += kReduceThreads) {
                if (rec[r].bucket != b) continue;
                const Terms t = row_terms(rec[r], log_fn);
                for (int c = 0; c < kCounts; ++c) count[c] += t.count[c];
                if (rec[r].flags & kInvalid) continue;
                for (int s = 0; s < kSums; ++s) part[s][l] += t.sum[s];
            }
        }
        for (int s = 0; s < kSums; ++s) sum[s] += wave_sum_host(part[s]);
    }
    for (int c = 0; c < kCounts; ++c) acc.count[c] += count[c];
    for (int s = 0; s < kSums; ++s) acc.sum[s] += sum[s];
}

}  // namespace tg_score
