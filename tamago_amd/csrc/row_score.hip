// Row scoring (the rules: row_score.h): network outputs on the positions of game records become evaluation
// statistics without leaving device memory.  Two kernels behind each other on the caller's stream:
//   rows    a wavefront per row: ceil(A / 64) lane passes over the policy (coalesced reads; a partial last pass), the rank of the
//           move played from per-lane counts, the candidate mass as per-lane fp64 sums and one xor butterfly, one 40-byte record
//   table   a workgroup per ply bucket: thread t takes the records t, t + 256, ... that fall in its bucket in that order, a
//           butterfly per wavefront, the four wavefronts in their order through LDS, and thread 0 - the bucket's only writer -
//           adds the result to the caller's table
// No floating-point atomics and no wavefront waits for another: the order of every sum is a function of (n, workgroup size)
// alone, so equal rows give equal table bits.  The logarithm is tg_rng::glibc_log, the function behind tg_glibc_log.
#include <hip/hip_runtime.h>

#include "common.h"
#include "legacy_rng_device.h"
#include "row_score.h"

namespace sc = tg_score;

namespace {

constexpr int kRowBlock = 256;
constexpr int kRowsPerBlock = kRowBlock / sc::kLanes;

struct ScoreDev {
    const float *policy;        // [n][A]
    const float *value;         // [n][3]
    const uint32_t *cand;       // [n][ceil(A / 32)] or null
    const int32_t *move, *cls, *ply;
    sc::RowRecord *rows;        // [n]
    sc::Bucket *table;          // [n_buckets]
    int32_t n, A, mask_words, bucket_width, n_buckets;
};

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int step = 1; step < sc::kLanes; step <<= 1) v += __shfl_xor(v, step);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {          // row_score.h wave_sum_host: steps 1, 2, ... 32
#pragma unroll
    for (int step = 1; step < sc::kLanes; step <<= 1) v += __shfl_xor(v, step);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int step = 1; step < sc::kLanes; step <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, step), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), step);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(kRowBlock) void score_rows_kernel(ScoreDev D) {
    const int lane = threadIdx.x & (sc::kLanes - 1);
    const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= D.n) return;                                          // (wave-uniform: a wavefront owns one row)
    const float *policy = D.policy + (size_t)row * D.A;
    const float *value = D.value + (size_t)row * 3;
    const uint32_t *mask = D.cand ? D.cand + (size_t)row * D.mask_words : nullptr;
    const int move = D.move[row], cls = D.cls[row];
    const bool move_ok = move >= 0 && move < D.A;
    const float pm = move_ok ? policy[move] : 0.f;
    const sc::LanePart part = sc::lane_part<sc::Rule>(policy, mask, D.A, lane, move_ok, pm, move);
    const int ahead = wave_sum_i32(part.ahead);
    const bool any_nan = __ballot(part.nan != 0) != 0ull;
    const double mass = wave_sum_f64(part.mass);
    if (lane == 0)
        D.rows[row] = sc::finish_row<sc::Rule>(policy, value, mask, D.A, move, cls, D.ply[row], D.bucket_width, D.n_buckets, ahead,
                                               any_nan, mass);
}

__global__ __launch_bounds__(sc::kReduceThreads) void score_table_kernel(ScoreDev D) {
    __shared__ unsigned long long wave_count[sc::kReduceWaves][sc::kCounts];
    __shared__ double wave_sums[sc::kReduceWaves][sc::kSums];
    const int b = blockIdx.x;                                        // grid = n_buckets
    const int lane = threadIdx.x & (sc::kLanes - 1), wave = threadIdx.x >> 6;
    unsigned long long count[sc::kCounts] = {};
    double sum[sc::kSums] = {};
    auto log_fn = [](double x) { return tg_rng::glibc_log(x, tg_rng::kLogTab); };
    for (int r = threadIdx.x; r < D.n; r += sc::kReduceThreads) {
        if (D.rows[r].bucket != b) continue;
        const sc::RowRecord rec = D.rows[r];
        const sc::Terms t = sc::row_terms(rec, log_fn);
#pragma unroll
        for (int c = 0; c < sc::kCounts; ++c) count[c] += t.count[c];
#pragma unroll
        for (int s = 0; s < sc::kSums; ++s) sum[s] += t.sum[s];
    }
#pragma unroll
    for (int c = 0; c < sc::kCounts; ++c) {
        const unsigned long long total = wave_sum_u64(count[c]);
        if (lane == 0) wave_count[wave][c] = total;
    }
#pragma unroll
    for (int s = 0; s < sc::kSums; ++s) {
        const double total = wave_sum_f64(sum[s]);
        if (lane == 0) wave_sums[wave][s] = total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sc::Bucket &acc = D.table[b];
        for (int c = 0; c < sc::kCounts; ++c) {
            unsigned long long total = 0;
            for (int w = 0; w < sc::kReduceWaves; ++w) total += wave_count[w][c];
            acc.count[c] += total;
        }
        for (int s = 0; s < sc::kSums; ++s) {
            double total = 0.0;
            for (int w = 0; w < sc::kReduceWaves; ++w) total += wave_sums[w][s];
            acc.sum[s] += total;
        }
    }
}

}  // namespace

static_assert(sizeof(tg_score_row) == sizeof(sc::RowRecord) && sizeof(tg_score_bucket) == sizeof(sc::Bucket),
              "include/tamago_hip.h and csrc/row_score.h describe the same records");

extern "C" int tg_score_rows(const float *policy_dev, const float *value_dev, const uint32_t *cand_dev, const int32_t *move_dev,
                             const int32_t *class_dev, const int32_t *ply_dev, int n, int actions, int bucket_width, int n_buckets,
                             tg_score_row *rows_dev, tg_score_bucket *table_dev, int clear, void *stream) {
    if (!table_dev) return tg::fail(TG_ERR_ARG, "tg_score_rows: null argument (table)");
    if (n < 0) return tg::fail(TG_ERR_ARG, "tg_score_rows: negative number of rows");
    if (n_buckets < 1) return tg::fail(TG_ERR_ARG, "tg_score_rows: n_buckets %d < 1", n_buckets);
    if (bucket_width < 1) return tg::fail(TG_ERR_ARG, "tg_score_rows: bucket_width %d < 1", bucket_width);
    if (actions < 2) return tg::fail(TG_ERR_ARG, "tg_score_rows: %d actions (a board has at least one point and PASS)", actions);
    if (n && (!policy_dev || !value_dev || !move_dev || !class_dev || !ply_dev || !rows_dev))
        return tg::fail(TG_ERR_ARG, "tg_score_rows: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (clear) TG_HIP(hipMemsetAsync(table_dev, 0, (size_t)n_buckets * sizeof(sc::Bucket), st));
    if (n == 0) return TG_OK;
    ScoreDev D{policy_dev, value_dev, cand_dev, move_dev, class_dev, ply_dev, reinterpret_cast<sc::RowRecord *>(rows_dev),
               reinterpret_cast<sc::Bucket *>(table_dev), n, actions, (actions + 31) / 32, bucket_width, n_buckets};
    hipLaunchKernelGGL(score_rows_kernel, dim3((n + kRowsPerBlock - 1) / kRowsPerBlock), dim3(kRowBlock), 0, st, D);
    TG_HIP(hipGetLastError());
    hipLaunchKernelGGL(score_table_kernel, dim3(n_buckets), dim3(sc::kReduceThreads), 0, st, D);
    TG_HIP(hipGetLastError());
    return TG_OK;
}
