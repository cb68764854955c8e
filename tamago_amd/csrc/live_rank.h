// Live ranks: which trees of a lock-step PUCT launch still search, and where a live tree's leaves go when the idle
// ones are compacted out of the forward pass.  A live tree's rank is the number of live trees before it, a tree that is not
// live gets -1, and the live count is the total.  Pure arithmetic, no HIP: search.hip's live_rank_kernel compiles this text for
// the device, tests/live_rank_driver.cpp for the host (tests/test_live_rank_host.py), so the CPU checks the very rule the
// kernel applies - the carry from one chunk of trees to the next included.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TG_LIVE_FN __host__ __device__ inline
#else
#define TG_LIVE_FN inline
#endif

namespace tg_live {

// The PUCT selectors' own predicate (select_puct_kernel and its three siblings): no sticky error, no halt word, a root.
TG_LIVE_FN bool live(int32_t err, int32_t halt, int32_t num_nodes) { return err == 0 && halt == 0 && num_nodes > 0; }

constexpr int32_t kNotLive = -1;

// How the kernel lays the trees out: one workgroup of kChunk threads takes them kChunk at a time, a wavefront of kLanes lanes
// scans its 64 flags, the wave totals are scanned across the workgroup, and `carry` - the live trees of the chunks before -
// goes from one chunk to the next.
constexpr int kLanes = 64;
constexpr int kChunk = 1024;
constexpr int kWaves = kChunk / kLanes;

// The scan rule.  own: the tree's flag (0 / 1); inclusive: the flags up to and including the tree's within its wavefront;
// waves_before: the totals of the wavefronts before it in the chunk.
struct Rule {
    static TG_LIVE_FN int32_t before(int32_t inclusive, int32_t own) { return inclusive - own; }
    static TG_LIVE_FN int32_t rank(int32_t own, int32_t carry, int32_t waves_before, int32_t lanes_before) {
        return own ? carry + waves_before + lanes_before : kNotLive;
    }
    static TG_LIVE_FN int32_t next_carry(int32_t carry, int32_t chunk_total) { return carry + chunk_total; }
};

// The kernel's order of operations on the host, under rule R (the tests put wrong rules here): rank[T] from flag[T], the live
// count returned.
template <class R = Rule>
inline int32_t replay(const uint8_t *flag, int T, int32_t *rank) {
    int32_t carry = 0;
    for (int c0 = 0; c0 < T; c0 += kChunk) {
        int32_t wave_total[kWaves];
        int32_t inclusive[kChunk];
        for (int w = 0; w < kWaves; ++w) {
            int32_t run = 0;
            for (int l = 0; l < kLanes; ++l) {
                const int t = c0 + w * kLanes + l;
                run += t < T && flag[t] ? 1 : 0;
                inclusive[w * kLanes + l] = run;
            }
            wave_total[w] = run;
        }
        int32_t waves_before = 0;
        for (int w = 0; w < kWaves; ++w) {
            for (int l = 0; l < kLanes; ++l) {
                const int t = c0 + w * kLanes + l;
                if (t >= T) break;
                const int32_t own = flag[t] ? 1 : 0;
                rank[t] = R::rank(own, carry, waves_before, R::before(inclusive[w * kLanes + l], own));
            }
            waves_before += wave_total[w];
        }
        carry = R::next_carry(carry, waves_before);
    }
    return carry;
}

}  // namespace tg_live
