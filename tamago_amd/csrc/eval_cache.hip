// Evaluation cache (the rules: eval_cache.h): a hash table in device memory that serves the network's outputs
// for input planes it has seen.  Four kernels, all behind each other on the caller's stream:
//   probe   a wavefront per row: the key's bit image from wave ballots over coalesced plane reads (the canonical test in the
//           same pass), the bucket's tag words a way per lane, the key words of a matching way a word per lane; a hit copies
//           the entry's outputs to the caller's row; every row gets its flag (hit / miss / uncacheable)
//   rank    ONE workgroup scans the flags of the rows that need the network (eval_cache.h's RankRule, live_rank.h's layout) and
//           leaves their number in a pinned word
//   gather  a wavefront per ranked row: its planes to miss_planes[rank], 16 bytes a lane
//   commit  a wavefront per rank: the outputs to the row, and a cacheable miss into the table by eval_cache.h's insert walk - one
//           64-bit compare-and-swap per way at most (lane 0), then the whole wavefront writes key and outputs
// No kernel waits for another wavefront: a claim is at most W + 1 compare-and-swaps and nothing spins.  Probe and commit of one
// cache are ordered by the stream, so no reader sees an entry that is being written.  Counters: added up per wavefront in
// registers, one atomic a counter at the wavefront's end.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>

#include "common.h"
#include "eval_cache.h"
#include "host_resources.h"

namespace ec = tg_ecache;

namespace {

struct CacheDev {
    uint32_t *table;
    unsigned long long *counters;
    uint32_t n_buckets, ways;
    int P, A, K, E, wpp;
};

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / ec::kLanes;
constexpr int kMaxGrid = 2048;
constexpr unsigned long long kAllLanes = ~0ull;

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int step = 1; step < ec::kLanes; step <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, step), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), step);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// The key of one row, a word per lane (lane i < K holds key word i, the others 0), and whether the row is canonical.  All 64
// lanes of the wavefront call this together; the reads of a plane are 64 consecutive floats.
__device__ __forceinline__ bool row_key(const CacheDev &C, const float *row, int want_logits, int lane, uint32_t *word) {
    const uint32_t *bits = reinterpret_cast<const uint32_t *>(row);
    const int chunks = (C.P + ec::kLanes - 1) / ec::kLanes;
    uint32_t my = 0;
    bool ok = true;
    for (int pl = 0; pl < ec::kKeyPlanes; ++pl)
        for (int c = 0; c < chunks; ++c) {
            const int p = c * ec::kLanes + lane;
            const bool valid = p < C.P;
            const uint32_t b = valid ? bits[pl * C.P + p] : ec::kBitsZero;
            ok = ok && __ballot(ec::point_ok(b)) == kAllLanes;
            const unsigned long long one = __ballot(b == ec::kBitsOne);
            const int w0 = pl * C.wpp + 2 * c;
            if (lane == w0) my = (uint32_t)one;
            if (2 * c + 1 < C.wpp && lane == w0 + 1) my = (uint32_t)(one >> 32);
        }
    bool pos = true, neg = true;
    for (int c = 0; c < chunks; ++c) {
        const int p = c * ec::kLanes + lane;
        const bool valid = p < C.P;
        const uint32_t b = valid ? bits[ec::kKeyPlanes * C.P + p] : 0u;
        pos = pos && __ballot(!valid || b == ec::kBitsOne) == kAllLanes;
        neg = neg && __ballot(!valid || b == ec::kBitsMinusOne) == kAllLanes;
    }
    if (lane == ec::kKeyPlanes * C.wpp) my = ec::meta_word(pos, want_logits != 0);
    *word = my;
    return ok && (pos || neg);
}

__device__ __forceinline__ uint64_t key_hash(const CacheDev &C, uint32_t word, int lane) {
    return ec::HashRule::finish(wave_sum64(lane < C.K ? ec::HashRule::term(lane, word) : 0ull));
}

__device__ __forceinline__ uint32_t *entry_of(const CacheDev &C, uint32_t bucket, uint32_t way) {
    return C.table + ((size_t)bucket * C.ways + way) * (size_t)C.E;
}
__device__ __forceinline__ uint64_t load_tag(const uint32_t *entry) {
    return __hip_atomic_load(reinterpret_cast<const unsigned long long *>(entry), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void count(const CacheDev &C, int which, unsigned long long n, int lane) {
    if (lane == 0 && n) atomicAdd(C.counters + which, n);
}

__global__ __launch_bounds__(kBlock) void evalcache_probe_kernel(CacheDev C, const float *planes, int batch, int want_logits,
                                                                  float *policy, float *value, uint8_t *flag) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), n_waves = gridDim.x * kWavesPerBlock;
    unsigned long long lookups = 0, hits = 0, uncacheable = 0, tag_only = 0;
    for (int row = wave; row < batch; row += n_waves) {
        ++lookups;
        uint32_t word;
        if (!row_key(C, planes + (size_t)row * ec::kPlanes * C.P, want_logits, lane, &word)) {
            if (lane == 0) flag[row] = ec::kUncached;
            ++uncacheable;
            continue;
        }
        const uint64_t h = key_hash(C, word, lane);
        const uint32_t bucket = ec::bucket_of(h, C.n_buckets), tag = ec::tag_of(h);
        const uint64_t tw = lane < (int)C.ways ? load_tag(entry_of(C, bucket, lane)) : 0ull;
        unsigned long long match = __ballot(tw != 0 && ec::word_tag(tw) == tag);
        bool hit = false;
        while (match) {                                             // (wave-uniform: at most one pass but for tag collisions)
            const int way = __ffsll((long long)match) - 1;
            match &= match - 1;
            const uint32_t *e = entry_of(C, bucket, way);
            const bool key_equal = __ballot(lane >= C.K || e[2 + lane] == word) == kAllLanes;
            if (ec::HitRule::hit(true, key_equal)) {
                const uint32_t *src = e + 2 + C.K;
                uint32_t *pol = reinterpret_cast<uint32_t *>(policy) + (size_t)row * C.A;
                for (int i = lane; i < C.A; i += ec::kLanes) pol[i] = src[i];
                if (lane < 3) reinterpret_cast<uint32_t *>(value)[(size_t)row * 3 + lane] = src[C.A + lane];
                hit = true;
                break;
            }
            ++tag_only;
        }
        if (lane == 0) flag[row] = hit ? ec::kHit : ec::kMiss;
        hits += hit ? 1 : 0;
    }
    count(C, ec::kLookups, lookups, lane);
    count(C, ec::kHits, hits, lane);
    count(C, ec::kUncacheable, uncacheable, lane);
    count(C, ec::kTagOnly, tag_only, lane);
}

// ONE workgroup of kChunk threads (live_rank_kernel's layout): rank[row] = the rows before `row` that need the network, -1 for
// a hit; miss_row[rank] = row; *n_miss (a pinned word) = their number
__global__ __launch_bounds__(ec::kChunk) void evalcache_rank_kernel(const uint8_t *flag, int batch, int32_t *rank, int32_t *miss_row,
                                                                     int32_t *n_miss) {
    using ec::RankRule;
    __shared__ int32_t wave_total[ec::kWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int32_t carry = 0;
    for (int c0 = 0; c0 < batch; c0 += ec::kChunk) {
        const int t = c0 + (int)threadIdx.x;
        const int32_t own = t < batch ? ec::needs_network(flag[t]) : 0;
        const unsigned long long owns = __ballot(own != 0);
        const int32_t inclusive = __popcll(owns & ((2ull << lane) - 1ull));
        if (lane == 63) wave_total[wid] = inclusive;
        __syncthreads();
        int32_t waves_before = 0, chunk_total = 0;
#pragma unroll
        for (int w = 0; w < ec::kWaves; ++w) {
            const int32_t n = wave_total[w];
            if (w < wid) waves_before += n;
            chunk_total += n;
        }
        if (t < batch) {
            const int32_t r = RankRule::rank(own, carry, waves_before, RankRule::before(inclusive, own));
            rank[t] = r;
            if (r >= 0) miss_row[r] = t;
        }
        carry = RankRule::next_carry(carry, chunk_total);
        __syncthreads();                                   // (wave_total is written again for the next chunk)
    }
    if (threadIdx.x == 0) *n_miss = carry;
}

// 16 bytes of a row: rows are 6 P floats - an odd number of 8-byte units at every board size - so a row starts on an 8-byte
// boundary and the 16-byte accesses are declared with that alignment
typedef float row16 __attribute__((ext_vector_type(4), aligned(8)));
typedef float row8 __attribute__((ext_vector_type(2), aligned(8)));

__global__ __launch_bounds__(kBlock) void evalcache_gather_kernel(const float *planes, const int32_t *rank, int batch, int row_floats,
                                                                   float *miss_planes) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), n_waves = gridDim.x * kWavesPerBlock;
    const int n16 = row_floats / 4, tail = row_floats - 4 * n16;           // (tail: 0 or 2 floats)
    for (int row = wave; row < batch; row += n_waves) {
        const int32_t r = rank[row];
        if (r < 0) continue;
        const float *src = planes + (size_t)row * row_floats;
        float *dst = miss_planes + (size_t)r * row_floats;
        for (int i = lane; i < n16; i += ec::kLanes) reinterpret_cast<row16 *>(dst)[i] = reinterpret_cast<const row16 *>(src)[i];
        if (tail && lane == 0) *reinterpret_cast<row8 *>(dst + 4 * n16) = *reinterpret_cast<const row8 *>(src + 4 * n16);
    }
}

__global__ __launch_bounds__(kBlock) void evalcache_commit_kernel(CacheDev C, const float *miss_planes, const int32_t *miss_row,
                                                                   const uint8_t *flag, const float *miss_policy, const float *miss_value,
                                                                   int n_miss, int want_logits, uint32_t epoch, float *policy, float *value) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), n_waves = gridDim.x * kWavesPerBlock;
    unsigned long long inserts = 0, twins = 0, evictions = 0, dropped = 0;
    for (int m = wave; m < n_miss; m += n_waves) {
        const int32_t row = miss_row[m];
        const uint32_t *mpol = reinterpret_cast<const uint32_t *>(miss_policy) + (size_t)m * C.A;
        const uint32_t *mval = reinterpret_cast<const uint32_t *>(miss_value) + (size_t)m * 3;
        uint32_t *pol = reinterpret_cast<uint32_t *>(policy) + (size_t)row * C.A;
        for (int i = lane; i < C.A; i += ec::kLanes) pol[i] = mpol[i];
        if (lane < 3) reinterpret_cast<uint32_t *>(value)[(size_t)row * 3 + lane] = mval[lane];
        if (flag[row] != ec::kMiss) continue;                        // (uncacheable: evaluated, never inserted)
        uint32_t word;
        (void)row_key(C, miss_planes + (size_t)m * ec::kPlanes * C.P, want_logits, lane, &word);
        const uint64_t h = key_hash(C, word, lane);
        const uint32_t bucket = ec::bucket_of(h, C.n_buckets), tag = ec::tag_of(h);
        // the walk runs wave-uniformly: the observed tag words come from one load a lane, lane 0 swaps and tells the others
        const uint64_t seen = lane < (int)C.ways ? load_tag(entry_of(C, bucket, lane)) : 0ull;
        uint32_t way = 0;
        const ec::Outcome o = ec::insert_walk<ec::InsertRule>(
            C.ways, ec::victim_of(h, C.ways), tag, epoch, [&](uint32_t w) { return shfl64(seen, (int)w); },
            [&](uint32_t w, uint64_t expected, uint64_t desired) {
                unsigned long long was = 0;
                if (lane == 0)
                    was = atomicCAS(reinterpret_cast<unsigned long long *>(entry_of(C, bucket, w)), (unsigned long long)expected,
                                    (unsigned long long)desired);
                return shfl64(was, 0);
            },
            &way);
        inserts += o == ec::kInserted || o == ec::kEvicted ? 1 : 0;
        evictions += o == ec::kEvicted ? 1 : 0;
        twins += o == ec::kTwin ? 1 : 0;
        dropped += o == ec::kDrop ? 1 : 0;
        if (o == ec::kInserted || o == ec::kEvicted) {
            uint32_t *e = entry_of(C, bucket, way);
            if (lane < C.K) e[2 + lane] = word;
            for (int i = lane; i < C.A; i += ec::kLanes) e[2 + C.K + i] = mpol[i];
            if (lane < 3) e[2 + C.K + C.A + lane] = mval[lane];
        }
    }
    count(C, ec::kInserts, inserts, lane);
    count(C, ec::kTwinSkips, twins, lane);
    count(C, ec::kEvictions, evictions, lane);
    count(C, ec::kDropped, dropped, lane);
}

int grid_for(int waves) {
    const int blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
    return blocks < 1 ? 1 : blocks > kMaxGrid ? kMaxGrid : blocks;
}

}  // namespace

struct tg_evalcache {
    int device = 0, S = 0;
    uint32_t entries = 0;
    CacheDev dev{};
    tg::DevBuf<uint32_t> table;
    tg::DevBuf<unsigned long long> counters;
    tg::DevBuf<uint8_t> flag;
    tg::DevBuf<int32_t> rank, miss_row;
    tg::DevBuf<float> miss_planes, miss_policy, miss_value;
    tg::PinBuf<int32_t> n_miss_pin;                // written by the rank kernel (mapped), read after the stream was waited for
    uint32_t epoch = 0;                            // commit launches so far: the epoch of the entries the next one writes, less 1
    // the probe in flight
    bool probed = false;
    int batch = 0, n_miss = 0, want_logits = 0;
    float *policy = nullptr, *value = nullptr;
    // timing-only path (tg_evalcache_set_timing): events around each launch of the last probe [0..3] and commit [4..5]
    bool timing = false, probe_timed = false, commit_timed = false;
    hipEvent_t ev[6] = {};
    ~tg_evalcache() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

static int stamp(tg_evalcache *c, int i, hipStream_t st) {
    if (!c->timing) return TG_OK;
    if (!c->ev[i]) TG_HIP(hipEventCreate(&c->ev[i]));
    TG_HIP(hipEventRecord(c->ev[i], st));
    return TG_OK;
}

extern "C" {

int tg_evalcache_create(int board_size, int device, long long entries, int ways, tg_evalcache **out) {
    if (!out) return tg::fail(TG_ERR_ARG, "tg_evalcache_create: null argument");
    *out = nullptr;
    if (board_size != 9 && board_size != 13 && board_size != 19)
        return tg::fail(TG_ERR_ARG, "tg_evalcache_create: board size %d (9, 13 and 19 are served)", board_size);
    if (ways < 1 || ways > ec::kMaxWays) return tg::fail(TG_ERR_ARG, "tg_evalcache_create: %d ways (1 to %d: the probe compares a bucket in one pass)", ways, ec::kMaxWays);
    if (entries < 1 || entries % ways != 0 || entries > (1ll << 31) - 1)
        return tg::fail(TG_ERR_ARG, "tg_evalcache_create: %lld entries (a positive multiple of the %d ways, below 2^31)", entries, ways);
    TG_HIP(hipSetDevice(device));
    std::unique_ptr<tg_evalcache> c(new (std::nothrow) tg_evalcache);
    if (!c) return tg::fail(TG_ERR_ARG, "tg_evalcache_create: out of host memory");
    const int P = board_size * board_size;
    c->device = device;
    c->S = board_size;
    c->entries = (uint32_t)entries;
    int rc;
    if ((rc = c->table.alloc_zeroed((size_t)entries * ec::entry_words(P))) || (rc = c->counters.alloc_zeroed(ec::kCounters)) ||
        (rc = c->n_miss_pin.alloc(1, hipHostMallocMapped)))
        return rc;
    c->dev = CacheDev{c->table.get(), c->counters.get(), (uint32_t)(entries / ways), (uint32_t)ways, P, P + 1, ec::key_words(P),
                      ec::entry_words(P), ec::words_per_plane(P)};
    *out = c.release();
    return TG_OK;
}

int tg_evalcache_destroy(tg_evalcache *c) {
    if (!c) return TG_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();                  // (a cache has no stream of its own: nothing queued may still use its buffers)
    delete c;
    return TG_OK;
}

int tg_evalcache_clear(tg_evalcache *c, void *stream) {
    if (!c) return tg::fail(TG_ERR_ARG, "tg_evalcache_clear: null argument");
    if (c->probed) return tg::fail(TG_ERR_STATE, "tg_evalcache_clear: a probe waits for its commit");
    TG_HIP(hipSetDevice(c->device));
    TG_HIP(hipMemsetAsync(c->table.get(), 0, (size_t)c->entries * c->dev.E * sizeof(uint32_t), (hipStream_t)stream));
    return TG_OK;
}

int tg_evalcache_probe(tg_evalcache *c, const float *planes_dev, int batch, int want_logits, float *policy_dev, float *value_dev,
                       void *stream, int32_t *n_miss, const float **miss_planes_dev) {
    if (!c || !planes_dev || !policy_dev || !value_dev || !n_miss || !miss_planes_dev)
        return tg::fail(TG_ERR_ARG, "tg_evalcache_probe: null argument");
    if (batch < 1 || batch > ec::kMaxBatch) return tg::fail(TG_ERR_ARG, "tg_evalcache_probe: batch %d (1 to %d)", batch, ec::kMaxBatch);
    if ((uintptr_t)planes_dev % 8 != 0) return tg::fail(TG_ERR_ARG, "tg_evalcache_probe: planes must be 8-byte aligned");
    if (c->probed) return tg::fail(TG_ERR_STATE, "tg_evalcache_probe: the last probe was not committed (tg_evalcache_commit)");
    TG_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t row_floats = (size_t)ec::kPlanes * c->dev.P;
    // Each buffer is held to its own capacity (a reserve that failed leaves the others grown: the next probe still asks for
    // this one).  Growing frees first, and hipFree waits for the device: a commit still queued has run before its buffers go.
    int rc;
    if ((rc = c->flag.reserve(batch)) || (rc = c->rank.reserve(batch)) || (rc = c->miss_row.reserve(batch)) ||
        (rc = c->miss_planes.reserve(batch * row_floats)))
        return rc;
    if ((rc = stamp(c, 0, st))) return rc;
    hipLaunchKernelGGL(evalcache_probe_kernel, dim3(grid_for(batch)), dim3(kBlock), 0, st, c->dev, planes_dev, batch, want_logits ? 1 : 0,
                       policy_dev, value_dev, c->flag.get());
    TG_HIP(hipGetLastError());
    if ((rc = stamp(c, 1, st))) return rc;
    hipLaunchKernelGGL(evalcache_rank_kernel, dim3(1), dim3(ec::kChunk), 0, st, c->flag.get(), batch, c->rank.get(), c->miss_row.get(),
                       c->n_miss_pin.dev());
    TG_HIP(hipGetLastError());
    if ((rc = stamp(c, 2, st))) return rc;
    hipLaunchKernelGGL(evalcache_gather_kernel, dim3(grid_for(batch)), dim3(kBlock), 0, st, planes_dev, c->rank.get(), batch, (int)row_floats,
                       c->miss_planes.get());
    TG_HIP(hipGetLastError());
    if ((rc = stamp(c, 3, st))) return rc;
    c->probe_timed = c->timing;
    TG_HIP(hipStreamSynchronize(st));
    const int32_t n = *c->n_miss_pin.get();
    if (n < 0 || n > batch) return tg::fail(TG_ERR_STATE, "tg_evalcache_probe: the device counted %d misses in %d rows", n, batch);
    c->probed = true;
    c->batch = batch;
    c->n_miss = n;
    c->want_logits = want_logits ? 1 : 0;
    c->policy = policy_dev;
    c->value = value_dev;
    *n_miss = n;
    *miss_planes_dev = c->miss_planes.get();
    return TG_OK;
}

int tg_evalcache_commit(tg_evalcache *c, const float *miss_policy_dev, const float *miss_value_dev, float *policy_dev, float *value_dev,
                        void *stream) {
    if (!c || !policy_dev || !value_dev) return tg::fail(TG_ERR_ARG, "tg_evalcache_commit: null argument");
    if (!c->probed) return tg::fail(TG_ERR_STATE, "tg_evalcache_commit: no probe waits for a commit (tg_evalcache_probe)");
    if (policy_dev != c->policy || value_dev != c->value)
        return tg::fail(TG_ERR_STATE, "tg_evalcache_commit: other output rows than the probe's");
    if (c->n_miss > 0 && (!miss_policy_dev || !miss_value_dev)) return tg::fail(TG_ERR_ARG, "tg_evalcache_commit: null argument");
    c->probed = false;
    c->commit_timed = false;
    if (c->n_miss == 0) return TG_OK;
    TG_HIP(hipSetDevice(c->device));
    if (int rc = stamp(c, 4, (hipStream_t)stream)) return rc;
    if (++c->epoch == 0) c->epoch = 1;             // (2^32 commits on: an entry of epoch 1 may be that old - it is only kept a call longer)
    hipLaunchKernelGGL(evalcache_commit_kernel, dim3(grid_for(c->n_miss)), dim3(kBlock), 0, (hipStream_t)stream, c->dev, c->miss_planes.get(),
                       c->miss_row.get(), c->flag.get(), miss_policy_dev, miss_value_dev, c->n_miss, c->want_logits, c->epoch, policy_dev,
                       value_dev);
    TG_HIP(hipGetLastError());
    if (int rc = stamp(c, 5, (hipStream_t)stream)) return rc;
    c->commit_timed = c->timing;
    return TG_OK;
}

int tg_evalcache_set_timing(tg_evalcache *c, int on) {
    if (!c) return tg::fail(TG_ERR_ARG, "tg_evalcache_set_timing: null argument");
    c->timing = on != 0;
    c->probe_timed = c->commit_timed = false;
    return TG_OK;
}

int tg_evalcache_read_timing(tg_evalcache *c, float *ms) {
    if (!c || !ms) return tg::fail(TG_ERR_ARG, "tg_evalcache_read_timing: null argument");
    if (!c->probe_timed) return tg::fail(TG_ERR_STATE, "tg_evalcache_read_timing: no probe was timed (tg_evalcache_set_timing)");
    TG_HIP(hipSetDevice(c->device));
    TG_HIP(hipEventSynchronize(c->ev[3]));
    for (int i = 0; i < 3; ++i) TG_HIP(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
    ms[3] = 0.0f;
    if (c->commit_timed) {
        TG_HIP(hipEventSynchronize(c->ev[5]));
        TG_HIP(hipEventElapsedTime(&ms[3], c->ev[4], c->ev[5]));
    }
    return TG_OK;
}

int tg_evalcache_forward(tg_evalcache *c, tg_net *net, const float *planes_dev, int batch, int want_logits, float *policy_dev,
                         float *value_dev, void *stream) {
    if (!c || !net) return tg::fail(TG_ERR_ARG, "tg_evalcache_forward: null argument");
    if (tg_net_board_size(net) != c->S)
        return tg::fail(TG_ERR_ARG, "tg_evalcache_forward: a %dx%d network on a %dx%d cache", tg_net_board_size(net), tg_net_board_size(net), c->S, c->S);
    int32_t n = 0;
    const float *miss_planes = nullptr;
    int rc;
    if ((rc = tg_evalcache_probe(c, planes_dev, batch, want_logits, policy_dev, value_dev, stream, &n, &miss_planes))) return rc;
    if (n > 0) {
        if ((rc = c->miss_policy.reserve((size_t)c->flag.capacity() * c->dev.A)) || (rc = c->miss_value.reserve((size_t)c->flag.capacity() * 3)) ||
            (rc = tg_net_forward_dev(net, miss_planes, n, want_logits, c->miss_policy.get(), c->miss_value.get(), stream))) {
            c->probed = false;                     // (nothing was evaluated: the hit rows stand, the caller sees the error)
            return rc;
        }
    }
    return tg_evalcache_commit(c, c->miss_policy.get(), c->miss_value.get(), policy_dev, value_dev, stream);
}

int tg_evalcache_last_misses(tg_evalcache *c, int32_t *n_miss) {
    if (!c || !n_miss) return tg::fail(TG_ERR_ARG, "tg_evalcache_last_misses: null argument");
    *n_miss = c->n_miss;
    return TG_OK;
}

int tg_evalcache_stats(tg_evalcache *c, uint64_t *out, int reset) {
    if (!c || !out) return tg::fail(TG_ERR_ARG, "tg_evalcache_stats: null argument");
    TG_HIP(hipSetDevice(c->device));
    TG_HIP(hipDeviceSynchronize());
    TG_HIP(hipMemcpy(out, c->counters.get(), ec::kCounters * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) {
        TG_HIP(hipMemset(c->counters.get(), 0, ec::kCounters * sizeof(uint64_t)));
        TG_HIP(hipDeviceSynchronize());
    }
    return TG_OK;
}

int tg_evalcache_debug_read(tg_evalcache *c, long long index, uint64_t *tag, uint32_t *key, float *policy, float *value) {
    if (!c || !tag || !key || !policy || !value) return tg::fail(TG_ERR_ARG, "tg_evalcache_debug_read: null argument");
    if (index < 0 || index >= (long long)c->entries) return tg::fail(TG_ERR_ARG, "tg_evalcache_debug_read: entry %lld of %u", index, c->entries);
    TG_HIP(hipSetDevice(c->device));
    TG_HIP(hipDeviceSynchronize());
    const uint32_t *e = c->table.get() + (size_t)index * c->dev.E;
    TG_HIP(hipMemcpy(tag, e, 8, hipMemcpyDeviceToHost));
    TG_HIP(hipMemcpy(key, e + 2, (size_t)c->dev.K * 4, hipMemcpyDeviceToHost));
    TG_HIP(hipMemcpy(policy, e + 2 + c->dev.K, (size_t)c->dev.A * 4, hipMemcpyDeviceToHost));
    TG_HIP(hipMemcpy(value, e + 2 + c->dev.K + c->dev.A, 12, hipMemcpyDeviceToHost));
    return TG_OK;
}

}  // extern "C"
