// Grouped ranks: the live trees of a lock-step PUCT launch sorted by the network that has to evaluate them, so
// that one compact selection serves the trees of every network and each network's forward pass runs over one contiguous
// segment of the plane rows.  Every tree carries a group id in [0, G); count[g] is the number of live trees of group g,
// offset[g] the sum of the counts of the groups laid out before g, and
//     rank[t] = offset[group[t]] + #{t' < t : live(t') and group[t'] == group[t]}          for a live tree, -1 otherwise
// - a stable counting sort of the live trees by group.  Pure arithmetic, no HIP: search.hip's group_rank_kernel compiles this
// text for the device, tests/group_rank_driver.cpp for the host (tests/test_group_rank_host.py), so the CPU checks the very
// rule the kernel applies - the per-group carry from one chunk of trees to the next included.
#pragma once
#include <cstdint>

#include "live_rank.h"

namespace tg_group {

using tg_live::kChunk;
using tg_live::kLanes;
using tg_live::kWaves;
constexpr int kMaxGroups = 64;
constexpr int32_t kNotLive = tg_live::kNotLive;

// A tree takes part under its group id when the selectors would search it and the id is one of the call's groups (the host
// refuses any other id before the launch; the kernel passes such a tree by, never indexes with it).
TG_LIVE_FN bool ranked(bool live, int32_t group, int n_groups) { return live && group >= 0 && group < n_groups; }

// How the kernel lays the trees out: one workgroup of kChunk threads takes them kChunk at a time, twice - a COUNTING pass that
// adds up every group's live trees, then the offsets, then an ASSIGNING pass.  Within a chunk a wavefront takes, for every
// distinct group among its 64 trees, the ballot of that group's live lanes: the lanes below a tree give its position within
// the group, the whole ballot the wave's total; the wave totals [kWaves][kMaxGroups] go through LDS and every thread adds up
// those of the wavefronts before its own for its own group; the chunk's per-group totals carry into the next chunk.
struct Rule {
    // where group g lies among the G segments of the plane rows
    static TG_LIVE_FN int place(int g, int /*n_groups*/) { return g; }
    // the offset of a segment from the scan of the counts in place order: inclusive up to and including its own count
    static TG_LIVE_FN int32_t offset(int32_t inclusive, int32_t own_count) { return inclusive - own_count; }
    // a tree's position within its group in its wavefront; lanes_upto: the group's live lanes up to and including the tree's
    static TG_LIVE_FN int32_t within(int32_t lanes_upto) { return lanes_upto - 1; }
    static TG_LIVE_FN int32_t rank(int32_t carry, int32_t waves_before, int32_t within) { return carry + waves_before + within; }
    // group g's carry into the next chunk (it starts at offset[g]); chunk_total[kMaxGroups]: this chunk's live trees per group
    static TG_LIVE_FN int32_t next_carry(int32_t carry, const int32_t *chunk_total, int g, int /*n_groups*/) {
        return carry + chunk_total[g];
    }
};

// The kernel's order of operations on the host, under rule R (the tests put wrong rules here).  flag[T]: the selectors'
// predicate; group[T]; G in [1, kMaxGroups].  rank[T], count[G], offset[G] out.
template <class R = Rule>
inline void replay(const uint8_t *flag, const int32_t *group, int T, int G, int32_t *rank, int32_t *count, int32_t *offset) {
    // one chunk's wave totals and positions, as the ballots give them
    int32_t wave_total[kWaves][kMaxGroups];
    int32_t upto[kChunk];
    auto ballots = [&](int c0) {
        for (int w = 0; w < kWaves; ++w) {
            for (int g = 0; g < kMaxGroups; ++g) wave_total[w][g] = 0;
            for (int l = 0; l < kLanes; ++l) {
                const int t = c0 + w * kLanes + l;
                upto[w * kLanes + l] = 0;
                if (t < T && ranked(flag[t] != 0, group[t], G)) upto[w * kLanes + l] = ++wave_total[w][group[t]];
            }
        }
    };
    // ---- counting pass
    int32_t total[kMaxGroups] = {};
    for (int c0 = 0; c0 < T; c0 += kChunk) {
        ballots(c0);
        for (int g = 0; g < G; ++g)
            for (int w = 0; w < kWaves; ++w) total[g] += wave_total[w][g];
    }
    // ---- offsets: the counts scanned in place order
    int32_t placed[kMaxGroups] = {}, start[kMaxGroups] = {};
    for (int g = 0; g < G; ++g) placed[R::place(g, G)] = total[g];
    int32_t run = 0;
    for (int p = 0; p < kMaxGroups; ++p) {
        run += placed[p];
        start[p] = R::offset(run, placed[p]);
    }
    int32_t carry[kMaxGroups] = {};
    for (int g = 0; g < G; ++g) {
        count[g] = total[g];
        offset[g] = carry[g] = start[R::place(g, G)];
    }
    // ---- assigning pass
    for (int c0 = 0; c0 < T; c0 += kChunk) {
        ballots(c0);
        int32_t chunk_total[kMaxGroups] = {};
        for (int w = 0; w < kWaves; ++w) {
            for (int l = 0; l < kLanes; ++l) {
                const int t = c0 + w * kLanes + l;
                if (t >= T) break;
                if (!ranked(flag[t] != 0, group[t], G)) { rank[t] = kNotLive; continue; }
                const int g = group[t];
                int32_t waves_before = 0;
                for (int v = 0; v < w; ++v) waves_before += wave_total[v][g];
                rank[t] = R::rank(carry[g], waves_before, R::within(upto[w * kLanes + l]));
            }
            for (int g = 0; g < kMaxGroups; ++g) chunk_total[g] += wave_total[w][g];
        }
        int32_t next[kMaxGroups];
        for (int g = 0; g < G; ++g) next[g] = R::next_carry(carry[g], chunk_total, g, G);
        for (int g = 0; g < G; ++g) carry[g] = next[g];
    }
}

}  // namespace tg_group
