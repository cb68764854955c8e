// Device-resident batched MCTS for gfx950 (MI355X).
//
// Replaces, for T independent search trees driven in lock-step:
//   mcts/tree.py:199-244   search_mcts        (PUCT descent, virtual loss, leaf queueing)
//   mcts/tree.py:247-270   expand_node        (+ :509-519 Dirichlet tentative prior)
//   mcts/tree.py:273-315   process_mini_batch (policy write-back, value backup)
//   mcts/tree.py:387-422   search_sequential_halving (Gumbel descent)
//   mcts/node.py:41-157, 275-361, mcts/pucb/pucb.py:8-29 (node math)
//   mcts/batch_data.py:7-34 (the leaf queue)
//   board/go_board.py:131-185, 237-304, 327-409 as called from the search (put_stone,
//   legality incl. positional superko, self-atari, complete-eye filter)
//   nn/feature.py:10-57 for the leaf boards.
//
// One workgroup owns one tree; inside it every WAVEFRONT has a role of its own (selector, board worker, value or
// policy backup) and works alone on its data - the one-wavefront kernels are the reference forms of the pipelined
// ones (select_puct_pipe / select_puct_mpipe / select_gumbel_pipe).  The node pool is a
// structure-of-arrays in HBM ([tree][node][child] per field); PUCB / Gumbel selection is
// a 64-lane arg-max reduction with lowest-index tie-break, in float64 exactly as numpy
// evaluates it; expansion tests all on-board points in parallel (one lane per point) on
// a board held in LDS; backup walks the recorded path (or parent links).  Boards use an O(1)-state
// representation (cell colour + string id = smallest stone coordinate); liberties,
// sizes and string hashes are recomputed with LDS atomics when a node is expanded, so
// nothing has to be copied per descent except 3 bytes per cell.
//
// Bit-exactness notes (verified against the oracle in tests/test_gpu_search.py):
//   * leaf values are float32; children_value_sum is accumulated in FLOAT32 and stored as
//     float64, node_value_sum is float32, "1 - v" is float32 (what numpy/torch do in
//     mcts/tree.py:297-313);
//   * PUCB is float64 with IEEE division and sqrt; this file is compiled with
//     -ffp-contract=off so no FMA is formed behind the source's back;
//   * the random draws are generated on the device (csrc/legacy_rng_device.h: MT19937 + glibc's log restated) or come from
//     the caller through tg_search_set_rng.
#include "common.h"
#define TG_RNG_DEVICE_KERNELS
#include "legacy_rng_device.h"
#include "leaf_queue.h"
#include "node_pool.h"
#include "readout.h"
#include "root_position.h"
#include "stop_rule.h"
#include "live_rank.h"
#include "group_rank.h"
#include "tree_dump.h"
#include "tree_load.h"
#include "visit_budget.h"
#include "forward_plan.h"                                             // tg::LaunchCapsScope: per-thread grid caps of the forward launches

#include <sched.h>

#include <cmath>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <chrono>
#include <thread>
#include <condition_variable>
#include <functional>
#include <atomic>
#include <future>
#include <vector>

namespace {

// Hand-offs between the LANES of one wavefront (every role in this file is one wavefront).  LDS and vector-memory
// operations of a wavefront execute in order, so they need no s_barrier (and no drain of the outstanding global
// loads / stores that the compiler puts in front of one): wavefront-scope fences order the accesses for the
// compiler and cost no instruction.  Hand-offs BETWEEN wavefronts go through LDS flags with workgroup-scope
// release / acquire (pipe_store / pipe_load below).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}


using tg_root::kEmpty, tg_root::kBlack, tg_root::kWhite, tg_root::kOob, tg_root::Geo, tg_root::RootMeta;
using tg_pool::kNotExpanded, tg_pool::NodeRec;

struct SearchDev {
    // node pool, [T][N][A]: the members node_pool.h's TG_NODE_POOL_ARRAYS lists
    int32_t *ch_index, *ch_visits, *ch_vl;
    double *ch_vsum, *ch_policy, *ch_value;
    int16_t *action;
    // node scalars, [T][N]: ONE 32-byte record per node (round 6; seven separate arrays until then - a path level of the backup
    // touched three 64-byte lines for visits / virtual loss / value sum, a selection step three for children / visits / virtual loss)
    NodeRec *node;
    double *noise;              // [T][A]   root Gumbel noise (0 for PUCT)
    // root position, per tree
    uint8_t *root_cells;        // [T][NC]
    uint64_t *root_hist;        // [T][HMAX]
    RootMeta *meta;             // [T]
    // leaf queue, [T][K]: the members leaf_queue.h's TG_LEAF_QUEUE_ARRAYS lists (q_src: below)
    int32_t *q_node, *q_pnode, *q_pedge;
    int32_t *q_depth, *q_path;
    int32_t *n_leaves;          // [T]
    // random stream
    const double *rng;          // [T][rng_cap]  e_i = -log(1-u_i)
    int64_t *rng_cursor;        // [T]
    int64_t *cursor_pub;        // [T] host-mapped mirror of rng_cursor (written with it: the host reads the cursors behind the
                                // selection launch's event without a copy kernel, which would queue for a CU behind the forward pass)
    int64_t rng_cap;
    const uint64_t *zob;        // [4][NC]
    int32_t *err;               // [T] sticky error flags
    long long *prof;            // optional [16] s_memtime cycle accumulators of tree 0 (tg_search_profile)
    int32_t T, N, K, cgos, superko;
    int32_t gumbel_one_by_one;  // test hook (TG_GUMBEL_ONE_BY_ONE): select_gumbel_pipe_kernel takes every entry through its job ring, as a phase with a long path does
    int32_t *q_src;             // the leaf queue's last array (UNIQUE leaf layout)
    int32_t *halt;              // [T] halt words: non-zero = the PUCT selectors pass the tree by, as they do one whose
                                // error word is set - no descent, no draw, no plane, n_leaves 0.  Not an error: the Gumbel selectors
                                // and every read-out ignore it.  Written between launches only (tg_search_set_halt, stop_rule_kernel,
                                // the clears of a root reset), so every wavefront of a launch reads the same word at kernel entry.
    const int32_t *rank;        // [T] live ranks, null in every launch but those of the COMPACT leaf layout: the PUCT
                                // selectors and the backup then find tree t's leaves at row rank[t] * max_leaves, not t * max_leaves
    const int32_t *budget;      // [T] visit totals, null unless tg_search_set_budget put budgets in force: a PUCT selector
                                // then makes tg_budget::descents(budget[t], root visits, max_leaves) descents for tree t, not max_leaves
};

// The descents of tree t in a PUCT selection launch of max_leaves slots per tree: read ONCE at kernel entry by every wavefront
// that needs it (the root's visits change in the backup only, never during a selection).
__device__ __forceinline__ int budget_descents(const SearchDev &D, int t, int max_leaves) {
    return D.budget ? tg_budget::descents(D.budget[t], D.node[(size_t)t * D.N].visits, max_leaves) : max_leaves;
}

// The planes of tree t's leaves, as the PUCT selectors index them: `planes + (t * max_leaves + k) * plane_floats` stays what a
// selector computes, and in the COMPACT layout the pointer is moved ONCE at kernel entry by the rows between the tree's rank
// and its index (wave-uniform scalar arithmetic in front of everything else: the descents' index arithmetic, whose place the
// register allocation of these kernels hangs on, is the strided layout's).  A tree without a rank (-1) writes no plane.
__device__ __forceinline__ float *compact_planes(const SearchDev &D, float *planes, int t, int max_leaves, int plane_floats) {
    if (D.rank) {
        const int r = D.rank[t];
        if (r >= 0) planes += (ptrdiff_t)(r - t) * max_leaves * plane_floats;
    }
    return planes;
}

__device__ __forceinline__ void set_cursor(const SearchDev &D, int t, long long v) {
    D.rng_cursor[t] = v;
    if (D.cursor_pub) D.cursor_pub[t] = v;
}

// The one writer of a queue entry (one lane): the slot gets the leaf to evaluate, its parent and the parent's edge, and how
// many levels of q_path the kernel recorded for it (kNoRecordedPath: none); UNIQUE: the plane of its position.
// The slot is its index t * K + k where the kernel holds that for the path's stores as well, a TreeSlot elsewhere: then every
// store indexes for itself, as these kernels always did (the index computed once in front of the stores moves the kernel's
// argument loads, and the register allocation of the one-wavefront kernels with them: profiles/leaf_queue_refactor.json).
struct TreeSlot { int t, k; };
__device__ __forceinline__ size_t queue_index(const SearchDev &, size_t qs) { return qs; }
__device__ __forceinline__ size_t queue_index(const SearchDev &D, TreeSlot s) { return (size_t)s.t * D.K + s.k; }
template <bool UNIQUE = false, class Slot>
__device__ __forceinline__ void write_queue_entry(const SearchDev &D, Slot slot, int node, int parent, int edge, int depth,
                                                  int src = 0) {
    D.q_node[queue_index(D, slot)] = node;
    D.q_pnode[queue_index(D, slot)] = parent;
    D.q_pedge[queue_index(D, slot)] = edge;
    D.q_depth[queue_index(D, slot)] = tg_queue::recorded_depth(depth, D.N);
    if constexpr (UNIQUE) D.q_src[queue_index(D, slot)] = src;
}

// UNIQUE leaf layout: the most root children one sequential-halving phase enters (node.py:324-346; DESIGN 4.4 says why) - a
// tree's plane range is min(descents, kUniqueE) slots when the pipelined Gumbel kernel runs
constexpr int kUniqueE = 17;
using tg_queue::kPathCap, tg_queue::kNoRecordedPath, tg_queue::path_entry, tg_queue::path_node, tg_queue::path_edge;
using tg_readout::kErrPoolFull, tg_readout::kErrRngEmpty, tg_readout::kErrPipeline, tg_readout::kErrReroot;

// ---- wave helpers ----------------------------------------------------------------------
// Cross-lane exchange for all-reduce butterflies.  Steps inside a row of 16 lanes use DPP
// (quad_perm for xor 1 / 2, row_half_mirror / row_mirror for the 8- and 16-lane steps: mirrors
// pair every lane with one from the other half, which is all an all-reduce needs); only the two
// cross-row steps go through ds_bpermute.  ~3x fewer LDS-crossbar round trips than six
// __shfl_xor rounds on a (double, int) pair.
template <int STEP>
__device__ __forceinline__ int lane_partner_i32(int v) {
    if constexpr (STEP == 0) return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    else if constexpr (STEP == 1) return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    else if constexpr (STEP == 2) return __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true);  // row_half_mirror
    else if constexpr (STEP == 3) return __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true);  // row_mirror
    else if constexpr (STEP == 4) return __shfl_xor(v, 16);
    else return __shfl_xor(v, 32);
}
template <int STEP>
__device__ __forceinline__ double lane_partner_f64(double v) {
    const long long bits = __double_as_longlong(v);
    const int lo = lane_partner_i32<STEP>((int)(unsigned)bits);
    const int hi = lane_partner_i32<STEP>((int)(unsigned)((unsigned long long)bits >> 32));
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// inclusive prefix sum over the wave's lanes: four row shifts, two row broadcasts (no LDS crossbar round trips)
__device__ __forceinline__ int wave_scan_add_i32(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);     // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);     // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);     // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);     // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);     // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);     // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
    v += lane_partner_i32<0>(v);
    v += lane_partner_i32<1>(v);
    v += lane_partner_i32<2>(v);
    v += lane_partner_i32<3>(v);
    v += lane_partner_i32<4>(v);
    v += lane_partner_i32<5>(v);
    return v;
}
__device__ __forceinline__ uint64_t wave_xor64(uint64_t v) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo ^= (unsigned)lane_partner_i32<0>((int)lo); hi ^= (unsigned)lane_partner_i32<0>((int)hi);
    lo ^= (unsigned)lane_partner_i32<1>((int)lo); hi ^= (unsigned)lane_partner_i32<1>((int)hi);
    lo ^= (unsigned)lane_partner_i32<2>((int)lo); hi ^= (unsigned)lane_partner_i32<2>((int)hi);
    lo ^= (unsigned)lane_partner_i32<3>((int)lo); hi ^= (unsigned)lane_partner_i32<3>((int)hi);
    lo ^= (unsigned)lane_partner_i32<4>((int)lo); hi ^= (unsigned)lane_partner_i32<4>((int)hi);
    lo ^= (unsigned)lane_partner_i32<5>((int)lo); hi ^= (unsigned)lane_partner_i32<5>((int)hi);
    return ((uint64_t)hi << 32) | lo;
}
// arg-max with lowest-index tie-break (np.argmax); idx < 0 marks "no candidate"
template <int STEP>
__device__ __forceinline__ void argmax_step(double &val, int &idx) {
    const double ov = lane_partner_f64<STEP>(val);
    const int oi = lane_partner_i32<STEP>(idx);
    const bool take = oi >= 0 && (idx < 0 || ov > val || (ov == val && oi < idx));
    if (take) { val = ov; idx = oi; }
}
__device__ __forceinline__ void wave_argmax(double &val, int &idx) {
    argmax_step<0>(val, idx);
    argmax_step<1>(val, idx);
    argmax_step<2>(val, idx);
    argmax_step<3>(val, idx);
    argmax_step<4>(val, idx);
    argmax_step<5>(val, idx);
}
// broadcast of a double from a wave-uniform lane (v_readlane: no LDS crossbar)
__device__ __forceinline__ double read_lane_f64(double v, int src_lane) {
    const long long bits = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)bits, src_lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)bits >> 32), src_lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// np.argmax over per-lane candidates (idx < 0: none): the maximum by a max butterfly inside each row of 16 lanes
// (DPP) and a v_readlane of the four row results, then the lowest index among the lanes that hold it the same
// way.  ~40 instructions and no branches; the compare-and-swap butterfly above costs ~150 with its exec-mask
// juggling.  Returns the wave-uniform winner (-1: no candidate).  All 64 lanes must be active.
__device__ __forceinline__ int wave_argmax_first(double val, int idx) {
    // (compare + select, not fmax: fmax quiets signalling NaNs first - a v_max_f64 x, x in front of every step; the scores
    // compared here are never NaN unless the network has diverged, and then any deterministic answer will do)
    auto mx2 = [](double a, double b) { return b > a ? b : a; };
    double m = idx >= 0 ? val : -__builtin_inf();
    m = mx2(m, lane_partner_f64<0>(m));
    m = mx2(m, lane_partner_f64<1>(m));
    m = mx2(m, lane_partner_f64<2>(m));
    m = mx2(m, lane_partner_f64<3>(m));
    const double mx = mx2(mx2(read_lane_f64(m, 0), read_lane_f64(m, 16)), mx2(read_lane_f64(m, 32), read_lane_f64(m, 48)));
    int c = (idx >= 0 && val == mx) ? idx : 0x7fffffff;
    c = min(c, lane_partner_i32<0>(c));
    c = min(c, lane_partner_i32<1>(c));
    c = min(c, lane_partner_i32<2>(c));
    c = min(c, lane_partner_i32<3>(c));
    const int w = min(min(__builtin_amdgcn_readlane(c, 0), __builtin_amdgcn_readlane(c, 16)),
                      min(__builtin_amdgcn_readlane(c, 32), __builtin_amdgcn_readlane(c, 48)));
    return w == 0x7fffffff ? -1 : w;
}

// ---- board in LDS ------------------------------------------------------------------------
struct BoardScalars {
    uint64_t hash;
    int moves, ko_pos, ko_move, prev, prevprev;
};
// the scalars of a tree's root (the other direction: tg_root::root_meta)
__device__ __forceinline__ BoardScalars scalars_of(const RootMeta &m) {
    return BoardScalars{m.hash, m.moves, m.ko_pos, m.ko_move, m.prev, m.prevprev};
}

// HALVING = false drops the two softmax scratch vectors that only the one-wave Gumbel kernel keeps in its board
template <int S, bool HALVING = true>
struct Lds {
    using G = Geo<S>;
    uint64_t hist[G::HMAX];
    double w1[HALVING ? G::A + 7 : 1];
    double w2[HALVING ? G::A + 7 : 1];
    uint64_t strhash[G::NC];
    uint32_t libcnt[G::NC];
    uint32_t strsize[G::NC];
    uint16_t root_sid[G::NC];
    uint16_t sid[G::NC];
    uint16_t cand[G::A + 3];
    uint8_t root_color[G::NC + 7];
    uint8_t color[G::NC + 7];
    int32_t scratch[8];
};

template <int S, typename LT>
__device__ __forceinline__ bool touches(const LT &L, int p, int id) {
    constexpr int W = Geo<S>::W;
    return L.sid[p - W] == id || L.sid[p - 1] == id || L.sid[p + 1] == id || L.sid[p + W] == id;
}

// go_board.py:131-185 on the LDS board.  All 64 lanes call it with wave-uniform arguments.
template <int S, typename LT>
__device__ void put_stone(LT &L, BoardScalars &b, int pos, int c, const uint64_t *zob, int lane) {
    using G = Geo<S>;
    constexpr int W = G::W, NC = G::NC;
    if (pos == 0) {                                   // PASS: record only (go_board.py:138-141)
        if (lane == 0 && b.moves < G::HMAX) L.hist[b.moves] = b.hash;
        b.prevprev = b.prev;
        b.prev = 0;
        b.moves += 1;
        wave_sync();
        return;
    }
    const int opp = 3 - c;
    if (lane == 0) L.color[pos] = (uint8_t)c;
    b.hash ^= zob[c * NC + pos];
    wave_sync();
    const int nb[4] = {pos - W, pos - 1, pos + 1, pos + W};
    int captured = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int n = nb[d];
        if (L.color[n] != opp) continue;               // wave-uniform
        const int id = L.sid[n];
        int cnt = 0;
        for (int p = lane; p < NC; p += 64)
            if (L.color[p] == kEmpty && touches<S>(L, p, id)) ++cnt;
        if (wave_sum(cnt) != 0) continue;
        // capture string `id` (string.py:292-325): clear stones, XOR their keys out
        uint64_t hx = 0;
        int removed = 0;
        for (int p = lane; p < NC; p += 64)
            if (L.sid[p] == id) { hx ^= zob[opp * NC + p]; ++removed; }
        wave_sync();
        for (int p = lane; p < NC; p += 64)
            if (L.sid[p] == id) { L.color[p] = kEmpty; L.sid[p] = 0; }
        b.hash ^= wave_xor64(hx);
        captured += wave_sum(removed);
        wave_sync();
    }
    // connect with friendly neighbours: string id = smallest stone coordinate
    int f[4];
    int newid = pos;
    bool any_friend = false;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        f[d] = (L.color[nb[d]] == c) ? L.sid[nb[d]] : 0;
        if (f[d]) { any_friend = true; newid = f[d] < newid ? f[d] : newid; }
    }
    if (any_friend) {
        for (int p = lane; p < NC; p += 64) {
            const int s = L.sid[p];
            if (s != 0 && (s == f[0] || s == f[1] || s == f[2] || s == f[3])) L.sid[p] = (uint16_t)newid;
        }
    } else if (captured == 1) {
        // ko, go_board.py:173-177: lone stone, exactly one capture, exactly one liberty
        int libs = 0, where = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if (L.color[nb[d]] == kEmpty) { ++libs; if (!where) where = nb[d]; }
        if (libs == 1) { b.ko_move = b.moves; b.ko_pos = where; }
    }
    wave_sync();
    if (lane == 0) {
        L.sid[pos] = (uint16_t)newid;
        if (b.moves < G::HMAX) L.hist[b.moves] = b.hash;
    }
    b.prevprev = b.prev;
    b.prev = pos;
    b.moves += 1;
    wave_sync();
}

// String ids from colours by min-label propagation (used once per root position).
template <int S>
__device__ void label_strings(uint8_t *color, uint16_t *sid, int lane) {
    using G = Geo<S>;
    constexpr int W = G::W, NC = G::NC;
    for (int p = lane; p < NC; p += 64) {
        const int c = color[p];
        sid[p] = (c == kBlack || c == kWhite) ? (uint16_t)p : 0;
    }
    wave_sync();
    for (int iter = 0; iter < NC; ++iter) {
        int changed = 0;
        for (int p = lane; p < NC; p += 64) {
            const int c = color[p];
            if (c != kBlack && c != kWhite) continue;
            int s = sid[p];
            const int nn[4] = {p - W, p - 1, p + 1, p + W};
#pragma unroll
            for (int d = 0; d < 4; ++d)
                if (color[nn[d]] == c && sid[nn[d]] < s) s = sid[nn[d]];
            if (s != sid[p]) { sid[p] = (uint16_t)s; changed = 1; }
        }
        wave_sync();
        if (wave_sum(changed) == 0) break;
    }
}

template <int S, typename LT>
__device__ __forceinline__ int pat3_at(const LT &L, int p) {
    constexpr int W = Geo<S>::W;
    return L.color[p - W - 1] | (L.color[p - W] << 2) | (L.color[p - W + 1] << 4) |
           (L.color[p - 1] << 6) | (L.color[p + 1] << 8) | (L.color[p + W - 1] << 10) |
           (L.color[p + W] << 12) | (L.color[p + W + 1] << 14);
}

// Eye colour of an empty point from its 3x3 neighbourhood (pattern.py:52-98,153-162) by the rule
// the reference's table is exactly equal to on real boards (tests/test_oracle_board.py::
// test_eye_table pins the rule to the reference's table entry by entry):
// orthogonals own or border; 4 on-board diagonals: <= 1 opponent, or 2 opponent + 2 own;
// 2 on-board diagonals (side): >= 1 own or both opponent; 1 on-board diagonal (corner): always.
__device__ __forceinline__ bool is_eye_of(int code, int me) {
    const int opp = 3 - me;
    const int n = (code >> 2) & 3, w = (code >> 6) & 3, e = (code >> 8) & 3, s = (code >> 12) & 3;
    if (!((n == me || n == kOob) && (w == me || w == kOob) && (e == me || e == kOob) && (s == me || s == kOob)))
        return false;
    const int d0 = code & 3, d1 = (code >> 4) & 3, d2 = (code >> 10) & 3, d3 = (code >> 14) & 3;
    const int n_free = (d0 != kOob) + (d1 != kOob) + (d2 != kOob) + (d3 != kOob);
    const int n_own = (d0 == me) + (d1 == me) + (d2 == me) + (d3 == me);
    const int n_opp = (d0 == opp) + (d1 == opp) + (d2 == opp) + (d3 == opp);
    if (n_free == 4) return n_opp <= 1 || (n_opp == 2 && n_own == 2);
    if (n_free == 2) return n_own >= 1 || n_opp == 2;
    return true;
}

// Candidate list of MCTSTree.expand_node (tree.py:260-264): legal (go_board.py:260-304),
// check_self_atari_stone < 7 (:327-365), not a complete eye (:367-397); row-major, PASS last.
// Returns the number of candidates (>= 1); L.cand[] holds their coordinates.
template <int S, typename LT>
__device__ int gen_candidates(LT &L, const BoardScalars &b, int me, const SearchDev &D, int lane) {
    using G = Geo<S>;
    constexpr int W = G::W, NC = G::NC, P = G::P;
    const int opp = 3 - me;
    for (int p = lane; p < NC; p += 64) { L.libcnt[p] = 0; L.strsize[p] = 0; L.strhash[p] = 0; }
    wave_sync();
    for (int p = lane; p < NC; p += 64) {
        const int c = L.color[p];
        if (c == kBlack || c == kWhite) {
            atomicAdd(&L.strsize[L.sid[p]], 1u);
            // superko quirk (go_board.py:292-296): keys of the mover's OPPONENT colour are
            // used for every adjacent one-liberty string, whatever its colour
            if (D.superko) atomicXor((unsigned long long *)&L.strhash[L.sid[p]],
                                     (unsigned long long)D.zob[opp * NC + p]);
        } else if (c == kEmpty) {
            const int s0 = L.sid[p - W], s1 = L.sid[p - 1], s2 = L.sid[p + 1], s3 = L.sid[p + W];
            if (s0) atomicAdd(&L.libcnt[s0], 1u);
            if (s1 && s1 != s0) atomicAdd(&L.libcnt[s1], 1u);
            if (s2 && s2 != s0 && s2 != s1) atomicAdd(&L.libcnt[s2], 1u);
            if (s3 && s3 != s0 && s3 != s1 && s3 != s2) atomicAdd(&L.libcnt[s3], 1u);
        }
    }
    wave_sync();

    int n = 0;
    for (int q0 = 0; q0 < P; q0 += 64) {
        const int q = q0 + lane;
        const int p = (q < P) ? (q / S + 1) * W + (q % S) + 1 : 0;
        bool keep = false;
        bool slow = false;          // self-atari needs the exact liberty-union count
        int fr[4] = {0, 0, 0, 0};
        int col[4] = {0, 0, 0, 0}, sid[4] = {0, 0, 0, 0}, lib[4] = {0, 0, 0, 0};
        int ne = 0;
        bool legal = false;
        uint64_t h = 0;
        if (q < P && L.color[p] == kEmpty) {
            const int nn[4] = {p - W, p - 1, p + 1, p + W};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                col[d] = L.color[nn[d]];
                sid[d] = L.sid[nn[d]];
                lib[d] = sid[d] ? (int)L.libcnt[sid[d]] : 0;
                ne += col[d] == kEmpty;
            }
            // suicide (go_board.py:237-258), only consulted when there is no empty neighbour
            bool suicide = true;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                if (col[d] == opp && lib[d] == 1) suicide = false;
                if (col[d] == me && lib[d] > 1) suicide = false;
            }
            legal = !(ne == 0 && suicide);
            if (b.ko_pos == p && b.ko_move == b.moves - 1) legal = false;
            if (legal && D.superko) {
                h = b.hash ^ D.zob[me * NC + p];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    bool dup = false;
#pragma unroll
                    for (int e = 0; e < d; ++e) dup |= sid[e] == sid[d];
                    if (sid[d] && !dup && lib[d] == 1) h ^= L.strhash[sid[d]];
                }
            }
        }
        if (D.superko) {
            // record.has_same_hash scans the whole fixed array; unused slots are 0 and slot 0 is never
            // written, so comparing with slots [0, moves) is equivalent.  Wave-uniform loop, four
            // uniform-address reads per round and no early exit: the reads pipeline (a per-lane loop
            // with a break paid one LDS round trip per history entry - 10 k cycles at move 100).
            const int hl = b.moves < G::HMAX ? b.moves : G::HMAX;
            bool seen = false;
            for (int i = 0; i < hl; i += 4) {
                const uint64_t a0 = L.hist[i];
                const uint64_t a1 = L.hist[i + 1 < G::HMAX ? i + 1 : i];
                const uint64_t a2 = L.hist[i + 2 < G::HMAX ? i + 2 : i];
                const uint64_t a3 = L.hist[i + 3 < G::HMAX ? i + 3 : i];
                seen |= a0 == h;
                seen |= i + 1 < hl && a1 == h;
                seen |= i + 2 < hl && a2 == h;
                seen |= i + 3 < hl && a3 == h;
            }
            if (seen) legal = false;
        }
        if (legal) {
            {
                // self-atari size (go_board.py:327-365); only "< 7" matters
                if (ne <= 1) {
                    int size = 0;
                    bool opp_atari = false, big_lib = false;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        if (col[d] == me) {
                            bool dup = false;
#pragma unroll
                            for (int e = 0; e < d; ++e) dup |= (col[e] == me && sid[e] == sid[d]);
                            if (!dup) { size += (int)L.strsize[sid[d]]; fr[d] = sid[d]; big_lib |= lib[d] >= 3; }
                        } else if (col[d] == opp && lib[d] == 1) {
                            opp_atari = true;
                        }
                    }
                    if (size + 1 >= 7 && !opp_atari && !big_lib) { slow = true; }
                }
                // complete eye (go_board.py:367-397)
                bool eye = false;
                if (is_eye_of(pat3_at<S>(L, p), me)) {
                    const int cr[4] = {p - W - 1, p - W + 1, p + W - 1, p + W + 1};
                    int count = 0;
                    bool edge = false;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int v = L.color[cr[d]];
                        if (v == me || v == kOob) ++count;
                        else if (v == kEmpty && is_eye_of(pat3_at<S>(L, cr[d]), me)) ++count;
                        if (v == kOob) edge = true;
                    }
                    eye = (edge && count == 4) || (!edge && count >= 3);
                }
                keep = !eye;
                if (eye) slow = false;
            }
        }
        // rare slow path: |{empty nbrs of p} U liberties of the friendly neighbour strings| >= 3 ?
        unsigned long long pending = __ballot(slow);
        while (pending) {
            const int src = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const int sp = __shfl(p, src);
            const int g0 = __shfl(fr[0], src), g1 = __shfl(fr[1], src), g2 = __shfl(fr[2], src),
                      g3 = __shfl(fr[3], src);
            int cnt = 0;
            for (int e = lane; e < NC; e += 64) {
                if (L.color[e] != kEmpty) continue;
                bool in = (e == sp) || e == sp - W || e == sp - 1 || e == sp + 1 || e == sp + W;
                if (!in) {
                    const int t0 = L.sid[e - W], t1 = L.sid[e - 1], t2 = L.sid[e + 1], t3 = L.sid[e + W];
                    const int ts[4] = {t0, t1, t2, t3};
#pragma unroll
                    for (int d = 0; d < 4; ++d)
                        if (ts[d] && (ts[d] == g0 || ts[d] == g1 || ts[d] == g2 || ts[d] == g3)) in = true;
                }
                cnt += in;
            }
            const int total = wave_sum(cnt);
            if (lane == src && total < 3) keep = false;   // self-atari of >= 7 stones: pruned
        }
        const unsigned long long kept = __ballot(keep);
        if (keep) L.cand[n + __popcll(kept & ((1ull << lane) - 1))] = (uint16_t)p;
        n += __popcll(kept);
    }
    if (lane == 0) L.cand[n] = 0;   // PASS
    wave_sync();
    return n + 1;
}

// e_0 + e_1 + ... + e_{n-1} in exactly that order (numpy's dirichlet), addend i held by lane i % 64 in v[i / 64].
// v_readlane moves the addends into scalar registers independently of the running sum, so only the n dependent
// float64 adds are on the critical path and nothing goes through LDS (staging the addends there and reading
// them back eight at a time cost 5.8 k cycles for 82 addends).  Blocks of eight; a block past n is skipped, the
// tail of the last block adds +0.0, which leaves a positive sum unchanged.
template <int R>
__device__ __forceinline__ double sequential_sum(const double (&v)[R], int n) {
    const int lane = threadIdx.x & 63;
    double z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) z[r] = lane + 64 * r < n ? v[r] : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int l0 = 0; l0 < 64; l0 += 8) {
            if (64 * r + l0 < n) {                                  // wave-uniform
                double x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) x[u] = read_lane_f64(z[r], l0 + u);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += x[u];
            }
        }
    }
    return acc;
}

// tree.py:247-270 expand_node + node.py:41-73: returns the new node index (or -1 on error).
template <int S, typename LT>
__device__ int expand_node(LT &L, const BoardScalars &b, int to_move, const SearchDev &D, int t,
                           int &num_nodes, int parent, int pedge, int lane) {
    using G = Geo<S>;
    constexpr int A = G::A;
    if (num_nodes >= D.N) {
        if (lane == 0) atomicOr(&D.err[t], kErrPoolFull);
        return -1;
    }
    const int node = num_nodes;
    // Dirichlet(1,..,1) prior from the host stream: p_i = e_i / (e_0 + e_1 + ... sequentially).
    // The stream values are requested BEFORE the candidate generation (n <= A is not known yet,
    // every lane takes its ceil(A/64) slots) so that their latency hides behind the LDS work.
    constexpr int R = (A + 63) / 64;
    const int64_t cur = D.rng_cursor[t];
    const double *e = D.rng + (size_t)t * D.rng_cap;
    double mine[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int64_t at = cur + lane + 64 * r;
        if (at >= D.rng_cap) at = D.rng_cap - 1;
        mine[r] = e[at];
    }
    const bool prof = D.prof && t == 0 && lane == 0;
    long long tp = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
    auto lap = [&](int slot) {
        if (prof) { const long long now = (long long)__builtin_amdgcn_s_memtime(); D.prof[slot] += now - tp; tp = now; }
    };
    const int n = gen_candidates<S>(L, b, to_move, D, lane);
    lap(8);
    if (cur + n > D.rng_cap) {
        if (lane == 0) atomicOr(&D.err[t], kErrRngEmpty);
        return -1;
    }
    // sequential sum e_0 + e_1 + ... exactly like numpy's dirichlet
    const double acc = sequential_sum<R>(mine, n);
    const double inv = 1.0 / acc;
    lap(9);
    const size_t base = ((size_t)t * D.N + node) * A;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        if (i < A) {
            D.ch_index[base + i] = kNotExpanded;
            D.ch_visits[base + i] = 0;
            D.ch_vl[base + i] = 0;
            D.ch_vsum[base + i] = 0.0;
            D.ch_value[base + i] = 0.0;
            D.ch_policy[base + i] = i < n ? mine[r] * inv : 0.0;
            D.action[base + i] = i < n ? (int16_t)L.cand[i] : (int16_t)0;
        }
    }
    if (lane == 0) {
        const size_t ns = (size_t)t * D.N + node;
        D.node[ns].children = n;
        D.node[ns].visits = 0;
        D.node[ns].vl = 0;
        D.node[ns].vsum = 0.f;
        D.node[ns].raw = 0.f;
        D.node[ns].parent = parent;
        D.node[ns].pedge = pedge;
        set_cursor(D, t, cur + n);
    }
    num_nodes += 1;
    wave_sync();
    lap(10);
    return node;
}

// The cell output point q (row-major) reads: its own, or the one a board symmetry (go_board.py:80-104; wave-uniform) maps it to.
struct NoSymmetry {};
template <int S>
__device__ __forceinline__ int plane_source(int q, NoSymmetry) { return (q / S + 1) * Geo<S>::W + (q % S) + 1; }
template <int S>
__device__ __forceinline__ int plane_source(int q, int sym) {
    constexpr int n = S - 1;
    const int y = q / S, x = q - y * S;
    int ry = y, rx = x;
    switch (sym) {
        case 1: rx = n - x; break;
        case 2: ry = n - y; break;
        case 3: ry = n - y; rx = n - x; break;
        case 4: ry = x; rx = y; break;
        case 5: ry = n - x; rx = y; break;
        case 6: ry = x; rx = n - y; break;
        case 7: ry = n - x; rx = n - y; break;
        default: break;
    }
    return (ry + 1) * Geo<S>::W + rx + 1;
}

// nn/feature.py:10-57 from the LDS board under `sym` (NoSymmetry, or 0..7: the bytes of featurize_kernel).  Lanes run over
// the output points: every plane store is one contiguous run.
template <int S, typename LT, typename Sym>
__device__ __forceinline__ void write_planes_under(const LT &L, const BoardScalars &b, int to_move, Sym sym, float *dst, int lane) {
    constexpr int P = Geo<S>::P;
    const bool pass_plane = b.moves > 1 && b.prev == 0;
    const float side = to_move == kWhite ? -1.f : 1.f;
    for (int q = lane; q < P; q += 64) {
        const int p = plane_source<S>(q, sym);
        int c = L.color[p];
        if (to_move == kWhite && c != 0) c = 3 - c;
        dst[q] = c == 0 ? 1.f : 0.f;
        dst[P + q] = c == 1 ? 1.f : 0.f;
        dst[2 * P + q] = c == 2 ? 1.f : 0.f;
        dst[3 * P + q] = (!pass_plane && p == b.prev) ? 1.f : 0.f;
        dst[4 * P + q] = pass_plane ? 1.f : 0.f;
        dst[5 * P + q] = side;
    }
}
// (the search kernels' call, as it was before the replayed samples took a symmetry: the same symbol, the same code)
template <int S, typename LT>
__device__ void write_planes(const LT &L, const BoardScalars &b, int to_move, float *dst, int lane) {
    write_planes_under<S>(L, b, to_move, NoSymmetry{}, dst, lane);
}

constexpr int kRcpN = 2048;

// a / b for an integer-valued b whose reciprocal y = RN(1 / b) is at hand: q0 = RN(a y) is within an ulp of the quotient, the
// remainder r = a - b q0 is exact in one FMA, and RN(q0 + r y) is the correctly rounded quotient (Markstein; b's significand
// is never all ones here: b < 2^31) - the bits of the IEEE division in four instructions instead of the ~25 of v_div_*.
// Checked against exact rational arithmetic for 300 000 (a, b <= 4096) on the CPU and by every tree digest of the GPU suite.
__device__ __forceinline__ double div_by_count(double a, double b, double y) {
    const double q0 = a * y;
    const double r = __builtin_fma(-q0, b, a);
    return __builtin_fma(r, y, q0);
}

// node.py:141-157 + pucb.py:8-29.  Everything the descent step needs from the node is loaded
// in ONE round trip (the loads are independent): the three node scalars and, per lane, the
// child arrays of its (up to ceil(A/64)) slots incl. action and child index; the winner's
// fields travel with the arg-max.
struct EdgePick {
    int edge, move, child, count, edge_vl, node_vl;   // count = visits + virtual loss of the edge
};

// pucb.py:8-29 on a node's statistics held in registers (lane i + 64 r: child i + 64 r); `total` = visits + virtual
// losses of the node.  The arithmetic of select_puct, shared with the kernels that load the statistics themselves.
// `rcp` (optional, LDS): rcp[n] = RN(1 / n) for n < kRcpN - both quotients then cost four instructions each instead of the
// ~25 of the division sequence (div_by_count: the same bits).
template <int S>
__device__ __forceinline__ EdgePick score_puct(const SearchDev &D, const int (&vis)[(Geo<S>::A + 63) / 64],
                                               const int (&vl)[(Geo<S>::A + 63) / 64], const int (&idx)[(Geo<S>::A + 63) / 64],
                                               const int (&act)[(Geo<S>::A + 63) / 64], const double (&vsum)[(Geo<S>::A + 63) / 64],
                                               const double (&pol)[(Geo<S>::A + 63) / 64], int nc, int total, int node_vl, int lane,
                                               const double *rcp = nullptr) {
    constexpr int R = (Geo<S>::A + 63) / 64;
    const double sq = __dsqrt_rn((double)(total + 1));
    double best = 0.0;
    int best_i = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        const int cnt = vis[r] + vl[r];
        // A group of 64 children none of which has been tried needs no division: q = 0 and u = (p sqrt) / 1, and
        // 0.0 + x / 1.0 is x bit for bit.  Most groups of most nodes are like that.
        if (__any(i < nc && cnt != 0)) {
            if (rcp && !__any(i < nc && cnt + 1 >= kRcpN)) {
                if (i < nc) {
                    const int c1 = cnt != 0 ? cnt : 1;
                    const double q = cnt != 0 ? div_by_count(vsum[r], (double)c1, rcp[c1]) : 0.0;
                    const double u = div_by_count(pol[r] * sq, (double)(cnt + 1), rcp[cnt + 1]);
                    double sc = q + u;
                    if (D.cgos && i == nc - 1) sc -= 0.1;
                    if (best_i < 0 || sc > best) { best = sc; best_i = i; }
                }
            } else if (i < nc) {
                const double q = cnt != 0 ? vsum[r] / (double)cnt : 0.0;
                const double u = (pol[r] * sq) / (double)(cnt + 1);
                double sc = q + u;
                if (D.cgos && i == nc - 1) sc -= 0.1;
                if (best_i < 0 || sc > best) { best = sc; best_i = i; }
            }
        } else if (i < nc) {
            double sc = pol[r] * sq;
            if (D.cgos && i == nc - 1) sc -= 0.1;
            if (best_i < 0 || sc > best) { best = sc; best_i = i; }
        }
    }
    best_i = wave_argmax_first(best, best_i);
    const int owner = best_i & 63, slot = best_i >> 6;
    int my_move = 0, my_child = 0, my_cnt = 0, my_vl = 0;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (r == slot) { my_move = act[r]; my_child = idx[r]; my_cnt = vis[r] + vl[r]; my_vl = vl[r]; }
    EdgePick pick;
    pick.edge = best_i;
    const int src = __builtin_amdgcn_readfirstlane(owner);        // wave-uniform after the arg-max
    pick.move = __builtin_amdgcn_readlane(my_move, src);
    pick.child = __builtin_amdgcn_readlane(my_child, src);
    pick.count = __builtin_amdgcn_readlane(my_cnt, src);
    pick.edge_vl = __builtin_amdgcn_readlane(my_vl, src);
    pick.node_vl = node_vl;
    return pick;
}

template <int S>
__device__ EdgePick select_puct(const SearchDev &D, int t, int node, int lane, const double *rcp = nullptr) {
    constexpr int A = Geo<S>::A;
    constexpr int R = (A + 63) / 64;
    const size_t ns = (size_t)t * D.N + node;
    const size_t base = ns * A;
    int vis[R], vl[R], idx[R], act[R];
    double vsum[R], pol[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        const int ii = i < A ? i : A - 1;          // the arrays always hold A slots
        vis[r] = D.ch_visits[base + ii];
        vl[r] = D.ch_vl[base + ii];
        vsum[r] = D.ch_vsum[base + ii];
        pol[r] = D.ch_policy[base + ii];
        idx[r] = D.ch_index[base + ii];
        act[r] = D.action[base + ii];
    }
    const int nc = D.node[ns].children;
    const int node_vl = D.node[ns].vl;
    const int total = D.node[ns].visits + node_vl;
    return score_puct<S>(D, vis, vl, idx, act, vsum, pol, nc, total, node_vl, lane, rcp);
}

template <int S, typename LT>
__device__ void load_root(LT &L, BoardScalars &b, int &to_move, const SearchDev &D, int t, int lane) {
    using G = Geo<S>;
    for (int p = lane; p < G::NC; p += 64) L.root_color[p] = D.root_cells[(size_t)t * G::NC + p];
    const RootMeta m = D.meta[t];
    for (int i = lane; i < m.hist_len; i += 64) L.hist[i] = D.root_hist[(size_t)t * G::HMAX + i];
    b = scalars_of(m);
    to_move = m.to_move;
    wave_sync();
    label_strings<S>(L.root_color, L.root_sid, lane);
}

// The empty board (GoBoard.clear), in LDS and in the scalars.
template <int S, typename LT>
__device__ __forceinline__ void empty_board(LT &L, BoardScalars &b, int lane) {
    using G = Geo<S>;
    for (int p = lane; p < G::NC; p += 64) {
        L.color[p] = (uint8_t)tg_root::empty_board_cell(p, G::W);
        L.sid[p] = 0;
    }
    if (lane == 0) L.hist[0] = 0;
    b = BoardScalars{/* hash */ 0, /* moves */ 1, 0, 0, 0, 0};
    wave_sync();
}

// The one writer of tree t's root from the LDS board (all lanes; num_nodes 0: the next root expansion resets the tree).
//   superko:       the board keeps its positions for superko - decides hist_len (tg_root::root_hist_len)
//   whole_history: the first hist_len words of L.hist go out (a replayed or new board); else the one word the last put_stone
//                  recorded, behind the history the tree has (a move played on the root)
//   clear_err:     the tree's sticky error word is cleared, as flush_roots does for a position set by the host
template <int S, typename LT>
__device__ __forceinline__ void store_root(const LT &L, const BoardScalars &b, int to_move, const SearchDev &D, int t, bool superko,
                                           bool whole_history, bool clear_err, int lane) {
    using G = Geo<S>;
    for (int p = lane; p < G::NC; p += 64) D.root_cells[(size_t)t * G::NC + p] = L.color[p];
    const int hl = tg_root::root_hist_len(b.moves, G::HMAX, superko);
    if (whole_history)
        for (int i = lane; i < hl; i += 64) D.root_hist[(size_t)t * G::HMAX + i] = L.hist[i];
    if (lane == 0) {
        if (!whole_history && b.moves - 1 < G::HMAX) D.root_hist[(size_t)t * G::HMAX + b.moves - 1] = b.hash;
        D.meta[t] = tg_root::root_meta(b, to_move, hl);
        if (clear_err) D.err[t] = 0;
    }
}

template <int S, typename LT>
__device__ void reset_work(LT &L, int lane) {
    for (int p = lane; p < Geo<S>::NC; p += 64) { L.color[p] = L.root_color[p]; L.sid[p] = L.root_sid[p]; }
    wave_sync();
}

// tree.py:49-54 / :330-336 (first half): reset the tree, expand the root, featurise it.
template <int S>
__global__ __launch_bounds__(64) void root_kernel(SearchDev D, float *planes) {   // planes [T][6][P]
    using G = Geo<S>;
    __shared__ Lds<S> L;
    const int t = blockIdx.x, lane = threadIdx.x;
    BoardScalars b;
    int to_move;
    load_root<S>(L, b, to_move, D, t, lane);
    reset_work<S>(L, lane);
    int num_nodes = 0;
    for (int i = lane; i < G::A; i += 64) D.noise[(size_t)t * G::A + i] = 0.0;
    const int root = expand_node<S>(L, b, to_move, D, t, num_nodes, -1, -1, lane);
    write_planes<S>(L, b, to_move, planes + (size_t)t * 6 * G::P, lane);
    if (lane == 0) {
        D.meta[t].num_nodes = num_nodes;
        write_queue_entry(D, TreeSlot{t, 0}, root, -1, -1, kNoRecordedPath);
        D.n_leaves[t] = root >= 0 ? 1 : 0;
    }
}

// root_kernel for the FRESH trees only (tg_search_root_planes_fresh): a tree without nodes is reset, expanded,
// featurised and queued as root_kernel does it - same draws, plane row t - and its halt word (and stopped_at entry, once the
// rule's buffers exist) cleared; a tree that has nodes keeps them: nothing of it is written but n_leaves[t] = 0, so that the
// backup behind the launch passes it by.
template <int S>
__global__ __launch_bounds__(64) void root_fresh_kernel(SearchDev D, float *planes, int32_t *stopped_at) {
    using G = Geo<S>;
    __shared__ Lds<S> L;
    const int t = blockIdx.x, lane = threadIdx.x;
    if (D.meta[t].num_nodes > 0) {                                     // (wave-uniform)
        if (lane == 0) D.n_leaves[t] = 0;
        return;
    }
    BoardScalars b;
    int to_move;
    load_root<S>(L, b, to_move, D, t, lane);
    reset_work<S>(L, lane);
    int num_nodes = 0;
    for (int i = lane; i < G::A; i += 64) D.noise[(size_t)t * G::A + i] = 0.0;
    const int root = expand_node<S>(L, b, to_move, D, t, num_nodes, -1, -1, lane);
    write_planes<S>(L, b, to_move, planes + (size_t)t * 6 * G::P, lane);
    if (lane == 0) {
        D.meta[t].num_nodes = num_nodes;
        write_queue_entry(D, TreeSlot{t, 0}, root, -1, -1, kNoRecordedPath);
        D.n_leaves[t] = root >= 0 ? 1 : 0;
        D.halt[t] = 0;
        if (stopped_at) stopped_at[t] = 0;
    }
}

// tree.py:199-244 search_mcts, `max_leaves` descents per tree.
template <int S>
__global__ __launch_bounds__(64) void select_puct_kernel(SearchDev D, int max_leaves, float *planes) {
    using G = Geo<S>;
    constexpr int A = G::A;
    __shared__ Lds<S> L;
    const int t = blockIdx.x, lane = threadIdx.x;
    planes = compact_planes(D, planes, t, max_leaves, 6 * G::P);
    BoardScalars rootb;
    int root_to_move;
    load_root<S>(L, rootb, root_to_move, D, t, lane);
    int num_nodes = D.meta[t].num_nodes;
    int queued = 0;
    const bool prof = D.prof && t == 0;
    long long pc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long tp = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
    auto lap = [&](int slot) {
        if (prof) { const long long now = (long long)__builtin_amdgcn_s_memtime(); pc[slot] += now - tp; tp = now; }
    };
    if (D.err[t] == 0 && D.halt[t] == 0 && num_nodes > 0) {
        const int n_desc = budget_descents(D, t, max_leaves);
        for (int k = 0; k < n_desc; ++k) {
            reset_work<S>(L, lane);
            BoardScalars b = rootb;
            int c = root_to_move;
            int node = 0;
            bool ok = true;
            lap(0);
            for (;;) {
                const size_t ns = (size_t)t * D.N + node;
                const size_t base = ns * A;
                const EdgePick pick = select_puct<S>(D, t, node, lane);
                const int e = pick.edge;
                const int mv = pick.move;
                lap(1);
                put_stone<S>(L, b, mv, c, D.zob, lane);
                lap(2);
                if (prof) pc[7] += 1;
                c = 3 - c;
                const int edge_cnt = pick.count + 1;                  // after the virtual loss
                int child = pick.child;
                if (lane == 0) {                                      // node.py:76-83
                    D.node[ns].vl = pick.node_vl + 1;
                    D.ch_vl[base + e] = pick.edge_vl + 1;
                }
                // two consecutive passes: never descend below (tree.py:224-229)
                const bool leaf = tg_queue::puct_descent_ends(edge_cnt, b.moves, b.prev, b.prevprev);
                lap(3);
                if (leaf) {
                    if (child == kNotExpanded) {
                        child = expand_node<S>(L, b, c, D, t, num_nodes, node, e, lane);
                        if (child < 0) { ok = false; break; }
                        if (lane == 0) D.ch_index[base + e] = child;
                    }
                    lap(4);
                    write_planes<S>(L, b, c, planes + ((size_t)t * max_leaves + k) * 6 * G::P, lane);
                    if (lane == 0) write_queue_entry(D, TreeSlot{t, k}, child, node, e, kNoRecordedPath);
                    wave_sync();
                    lap(5);
                    break;
                }
                node = child;
                wave_sync();
                lap(3);
            }
            if (!ok) break;
            ++queued;
        }
    }
    if (lane == 0) {
        D.meta[t].num_nodes = num_nodes;
        D.n_leaves[t] = queued;
        if (prof)
            for (int i = 0; i < 8; ++i) D.prof[i] += pc[i];
    }
}

// ---- PUCT selection, pipelined over three wavefronts per tree ------------------------------
// A descent is selection (PUCB walk: needs only the node pool) followed by board work (replay
// of the path on the LDS board, expansion, feature planes: needs no tree statistics).  With
// few trees per GPU the 256 descents of a mini-batch are a serial chain of ~12 us each in
// select_puct_kernel.  Here wave 0 (the selector) only walks the tree - it also assigns the
// node index of a new leaf, so numbering stays in descent order - and hands (path, parent,
// edge, node) to waves 1 and 2 (the workers, alternating), which replay the moves, generate
// candidates, draw the Dirichlet prior and write the planes.  The random draws are reserved in
// expansion order through a cursor chained between the workers; the selector waits for a
// worker only when it steps into a node whose expansion is still in flight.  Results are
// identical to the serial kernel (same tests).
constexpr int kPipeSlots = 4;           // job ring; even, so that a slot always belongs to one worker
constexpr int kPipeMaxDepth = 512;
constexpr int kPipeMaxK = 1024;
constexpr int kPipeSpinLimit = 1 << 24;

struct PipeJob {
    int k, parent, edge, child, expand, xseq, depth, src;
};

// Longest path a pipelined kernel follows (deeper: reported as an error, never silent).  A 9x9 game has at most
// 243 recorded moves (MAX_RECORDS = 3 P), so 256 covers every path there.
template <int S>
constexpr int kPathMax = S == 9 ? 256 : kPipeMaxDepth;

// The three-wave kernels are sized to sit NEXT TO a forward workgroup on a CU (the split-operand forward kernel
// leaves 19.6 KB of the 160 KB): boards without the softmax scratch, path buffers of kPathMax<S>, "job done"
// flags as a bit set.  Otherwise a selection launch of one board group waits for the forward pass of the other
// group to drain instead of overlapping it.
// (NW workers, 2 NW ring slots: with few trees per GPU the Gumbel kernel takes more workers per tree - the CUs are
// idle anyway and its jobs - expansions, leaves, ~100 plane copies per phase - are what a phase waits for.)
template <int S, int NW = 2>
struct PipeShared {
    static constexpr int kSlots = 2 * NW;
    Lds<S, false> board[NW];
    PipeJob job[kSlots];
    int16_t moves[kSlots][kPathMax<S>];
    int paths[kSlots][kPathMax<S>];       // Gumbel jobs: path_entry(node, edge) per level, for the worker's bookkeeping
    int job_seq[kSlots];              // k + 1 once job k sits in its slot
    int slot_done[kSlots];            // jobs finished in this slot so far
    unsigned done_bits[kPipeMaxK / 32];   // bit k: job k finished (node initialised, planes written)
    int16_t jobof[kPipeMaxK];         // node (n0 + i) is being created by job jobof[i]
    int cursor_seq;                   // expansions that have reserved their draws
    long long cursor_val;             // stream position after those reservations
    int final_count;                  // -1 while the selector is still queueing
    int err;
};

__device__ __forceinline__ int pipe_load(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void pipe_store(int *p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// job-done bits of PipeShared
template <typename Sh>
__device__ __forceinline__ void pipe_set_done(Sh &sh, int k) {
    __hip_atomic_fetch_or(&sh.done_bits[k >> 5], 1u << (k & 31), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <typename Sh>
__device__ __forceinline__ bool pipe_wait_done(const Sh &sh, int k);

// wave-uniform wait for *p >= want; false on a stall (reported, never a hang)
__device__ __forceinline__ bool pipe_wait_ge(const int *p, int want) {
    for (int spin = 0; spin < kPipeSpinLimit; ++spin) {
        if (pipe_load(p) >= want) return true;
        __builtin_amdgcn_s_sleep(1);
    }
    return false;
}

template <typename Sh>
__device__ __forceinline__ bool pipe_wait_done(const Sh &sh, int k) {
    const unsigned *p = &sh.done_bits[k >> 5];
    const unsigned bit = 1u << (k & 31);
    for (int spin = 0; spin < kPipeSpinLimit; ++spin) {
        if (__hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) & bit) return true;
        __builtin_amdgcn_s_sleep(1);
    }
    return false;
}

template <int S, typename LT>
__device__ void expand_fill(LT &L, const SearchDev &D, int t, int node, int parent, int pedge, int n, long long cur, int lane);

// expand_node for a worker: node index given by the selector, draws reserved through the chain
template <int S, typename LT, typename Sh>
__device__ bool expand_node_pipe(LT &L, const BoardScalars &b, int to_move, const SearchDev &D, int t,
                                 int node, int parent, int pedge, int xseq, Sh &sh, int lane) {
    const int n = gen_candidates<S>(L, b, to_move, D, lane);
    bool ok = pipe_wait_ge(&sh.cursor_seq, xseq);
    const long long cur = sh.cursor_val;
    if (!ok || cur + n > D.rng_cap) {
        if (lane == 0) {
            atomicOr(&D.err[t], ok ? kErrRngEmpty : kErrPipeline);
            pipe_store(&sh.err, 1);
            pipe_store(&sh.cursor_seq, xseq + 1);      // keep the chain moving
        }
        return false;
    }
    if (lane == 0) {
        sh.cursor_val = cur + n;
        pipe_store(&sh.cursor_seq, xseq + 1);
    }
    expand_fill<S>(L, D, t, node, parent, pedge, n, cur, lane);
    return true;
}

// the second half of an expansion: prior from the n draws at stream position `cur`, the node's arrays
template <int S, typename LT>
__device__ void expand_fill(LT &L, const SearchDev &D, int t, int node, int parent, int pedge, int n, long long cur, int lane) {
    using G = Geo<S>;
    constexpr int A = G::A;
    constexpr int R = (A + 63) / 64;
    const double *e = D.rng + (size_t)t * D.rng_cap;
    double mine[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        long long at = cur + lane + 64 * r;
        if (at >= D.rng_cap) at = D.rng_cap - 1;
        mine[r] = e[at];
    }
    // sequential sum e_0 + e_1 + ... exactly like numpy's dirichlet (see expand_node)
    const double acc = sequential_sum<R>(mine, n);
    const double inv = 1.0 / acc;
    const size_t base = ((size_t)t * D.N + node) * A;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        if (i < A) {
            D.ch_index[base + i] = kNotExpanded;
            D.ch_visits[base + i] = 0;
            D.ch_vl[base + i] = 0;
            D.ch_vsum[base + i] = 0.0;
            D.ch_value[base + i] = 0.0;
            D.ch_policy[base + i] = i < n ? mine[r] * inv : 0.0;
            D.action[base + i] = i < n ? (int16_t)L.cand[i] : (int16_t)0;
        }
    }
    if (lane == 0) {
        const size_t ns = (size_t)t * D.N + node;
        D.node[ns].children = n;
        D.node[ns].visits = 0;
        D.node[ns].vl = 0;
        D.node[ns].vsum = 0.f;
        D.node[ns].raw = 0.f;
        D.node[ns].parent = parent;
        D.node[ns].pedge = pedge;
    }
    wave_sync();
}

// Residency at 9x9: PipeShared<9> lets eight workgroups share a CU's LDS, but that takes 24 wavefronts per CU, six per SIMD,
// i.e. at most 80 VGPRs a wavefront.  Left to itself hipcc takes 97 (four waves per SIMD, FIVE workgroups per CU): 2 048
// trees on 256 CUs then run as a round of 1 280 and a round of 768.  The second launch bound holds the kernel to 80 registers
// (six of them spilled), so that every tree is resident from the start.  The larger boards are bounded by their LDS instead.
template <int S>
constexpr int kPipeWavesPerSimd = S == 9 ? 6 : 1;
static_assert(8 * sizeof(PipeShared<9>) <= 160 * 1024, "eight select_puct_pipe_kernel<9> workgroups per CU");

template <int S>
__global__ __launch_bounds__(192, kPipeWavesPerSimd<S>) void select_puct_pipe_kernel(SearchDev D, int max_leaves, float *planes) {
    using G = Geo<S>;
    constexpr int A = G::A;
    constexpr int R = (A + 63) / 64;
    __shared__ PipeShared<S> sh;
    const int t = blockIdx.x;
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    planes = compact_planes(D, planes, t, max_leaves, 6 * G::P);
    const RootMeta meta = D.meta[t];
    const int n0 = meta.num_nodes;
    if (threadIdx.x < kPipeSlots) {
        sh.job_seq[threadIdx.x] = 0;
        sh.slot_done[threadIdx.x] = 0;
    }
    for (int i = threadIdx.x; i < kPipeMaxK / 32; i += 192) sh.done_bits[i] = 0u;
    if (threadIdx.x == 0) {
        sh.cursor_seq = 0;
        sh.cursor_val = D.rng_cursor[t];
        sh.final_count = -1;
        sh.err = 0;
    }
    __syncthreads();
    const bool active = D.err[t] == 0 && D.halt[t] == 0 && n0 > 0;
    int num_nodes = n0;
    int queued = 0;

    if (wid == 0) {
        // ---- selector -------------------------------------------------------------------
        int nexp = 0;
        // The root's statistics, loaded once: every descent starts there, and within a launch only this wave changes the
        // root - its virtual losses and the child indices of fresh expansions - so it keeps the registers in step with
        // the stores below (which stay as they were: the workers, the backup and the next launch read the pool).
        int r_vis[R], r_vl[R], r_idx[R], r_act[R];
        double r_vsum[R], r_pol[R];
        int r_nc = 0, r_visits = 0, r_node_vl = 0;
        if (active) {
            const size_t root_ns = (size_t)t * D.N, root_base = root_ns * A;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = lane + 64 * r;
                const int ii = i < A ? i : A - 1;
                r_vis[r] = D.ch_visits[root_base + ii];
                r_vl[r] = D.ch_vl[root_base + ii];
                r_vsum[r] = D.ch_vsum[root_base + ii];
                r_pol[r] = D.ch_policy[root_base + ii];
                r_idx[r] = D.ch_index[root_base + ii];
                r_act[r] = D.action[root_base + ii];
            }
            r_nc = D.node[root_ns].children;
            r_visits = D.node[root_ns].visits;
            r_node_vl = D.node[root_ns].vl;
        }
        const int n_desc = budget_descents(D, t, max_leaves);
        for (int k = 0; active && k < n_desc; ++k) {
            if (pipe_load(&sh.err)) break;
            const int slot = k % kPipeSlots;
            bool ok = pipe_wait_ge(&sh.slot_done[slot], k / kPipeSlots);       // ring slot free again
            int node = 0, depth = 0;
            int moves = meta.moves, prev = meta.prev, prevprev = meta.prevprev;
            while (ok) {
                if (node >= n0) ok = pipe_wait_done(sh, sh.jobof[node - n0]);   // expansion still in flight?
                if (!ok) break;
                const size_t ns = (size_t)t * D.N + node;
                const size_t base = ns * A;
                const EdgePick pick = node == 0
                    ? score_puct<S>(D, r_vis, r_vl, r_idx, r_act, r_vsum, r_pol, r_nc, r_visits + r_node_vl, r_node_vl, lane)
                    : select_puct<S>(D, t, node, lane);
                const int e = pick.edge;
                const int mv = pick.move;
                if (depth >= kPathMax<S>) { ok = false; break; }
                if (lane == 0) {
                    sh.moves[slot][depth] = (int16_t)mv;
                    D.node[ns].vl = pick.node_vl + 1;                             // node.py:76-83
                    D.ch_vl[base + e] = pick.edge_vl + 1;
                    if (depth < kPathCap) D.q_path[((size_t)t * D.K + k) * kPathCap + depth] = path_entry(node, e);
                }
                if (node == 0) {                                                  // the same virtual loss on the registers
                    ++r_node_vl;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (lane + 64 * r == e) ++r_vl[r];
                }
                ++depth;
                prevprev = prev;
                prev = mv;
                ++moves;
                // two consecutive passes: never descend below (tree.py:224-229)
                if (tg_queue::puct_descent_ends(pick.count + 1, moves, prev, prevprev)) {
                    int child = pick.child;
                    const int expand = child == kNotExpanded;
                    int xseq = 0;
                    if (expand) {
                        if (num_nodes >= D.N || num_nodes - n0 >= kPipeMaxK) {
                            if (lane == 0) atomicOr(&D.err[t], kErrPoolFull);
                            ok = false;
                            break;
                        }
                        child = num_nodes++;
                        xseq = nexp++;
                        if (node == 0) {
#pragma unroll
                            for (int r = 0; r < R; ++r)
                                if (lane + 64 * r == e) r_idx[r] = child;
                        }
                    }
                    if (lane == 0) {
                        if (expand) {
                            D.ch_index[base + e] = child;
                            sh.jobof[child - n0] = (int16_t)k;
                        }
                        PipeJob &j = sh.job[slot];
                        j.k = k; j.parent = node; j.edge = e; j.child = child;
                        j.expand = expand; j.xseq = xseq; j.depth = depth;
                        write_queue_entry(D, TreeSlot{t, k}, child, node, e, depth);
                        pipe_store(&sh.job_seq[slot], k + 1);
                    }
                    wave_sync();
                    break;
                }
                node = pick.child;
            }
            if (!ok) {
                if (lane == 0) {
                    if (!(D.err[t] & kErrPoolFull)) atomicOr(&D.err[t], kErrPipeline);
                    pipe_store(&sh.err, 1);
                }
                break;
            }
            ++queued;
        }
        if (lane == 0) pipe_store(&sh.final_count, queued);
    } else {
        // ---- workers ---------------------------------------------------------------------
        Lds<S, false> &L = sh.board[wid - 1];
        BoardScalars rootb;
        int root_to_move;
        load_root<S>(L, rootb, root_to_move, D, t, lane);
        for (int k = wid - 1; active; k += 2) {
            const int slot = k % kPipeSlots;
            bool have = false, stalled = true;
            for (int spin = 0; spin < kPipeSpinLimit; ++spin) {
                if (pipe_load(&sh.job_seq[slot]) == k + 1) { have = true; stalled = false; break; }
                const int fc = pipe_load(&sh.final_count);
                if (fc >= 0 && k >= fc) { stalled = false; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            if (stalled && lane == 0) {
                atomicOr(&D.err[t], kErrPipeline);
                pipe_store(&sh.err, 1);
            }
            if (!have) break;
            const PipeJob j = sh.job[slot];
            reset_work<S>(L, lane);
            BoardScalars b = rootb;
            int c = root_to_move;
            for (int i = 0; i < j.depth; ++i) {
                put_stone<S>(L, b, sh.moves[slot][i], c, D.zob, lane);
                c = 3 - c;
            }
            if (j.expand) expand_node_pipe<S>(L, b, c, D, t, j.child, j.parent, j.edge, j.xseq, sh, lane);
            write_planes<S>(L, b, c, planes + ((size_t)t * max_leaves + k) * 6 * G::P, lane);
            wave_sync();
            if (lane == 0) {
                pipe_set_done(sh, k);                                          // releases the node arrays
                pipe_store(&sh.slot_done[slot], k / kPipeSlots + 1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        D.meta[t].num_nodes = num_nodes;
        D.n_leaves[t] = queued;
        set_cursor(D, t, sh.cursor_val);
    }
}

// ---- PUCT selection with the descents themselves pipelined ----------------------------------
// With few trees per GPU the selector wave above is the critical path: ~3.5 levels per descent, each an L2
// round trip plus ~2 k cycles of fp64 PUCB arithmetic, and descent k + 1 may not start before descent k has
// left its virtual loss behind.  But a descent only needs the virtual losses on the nodes it visits itself.
// So NSEL selector waves take the descents round-robin and a descent scores node n (at level L) once every
// earlier descent still in flight has either chosen a different level-L node or finished with n - a node is
// then always scored with exactly the statistics the serial order gives it:
//   * level_done[k] = levels descent k has left behind; lvl_node[k][L] = its level-L node, published with
//     level_done[k] = L.  Only the NSEL - 1 predecessors of k can still be in flight.
//   * the ROOT is visited by every descent, so its step is the chain that bounds the launch.  Its statistics
//     cannot change inside a launch (the backup runs between launches) except for the virtual losses, so every
//     selector keeps visits / value sums / priors of the root's children in registers and only the virtual
//     losses and child indices live in LDS.  sqrt(N + 1) and the prior products of descent k depend on k alone
//     and are computed BEFORE waiting for descent k - 1; after the wait only children whose virtual loss
//     changed since this wave's last visit get new quotients.  The root's virtual losses reach global memory
//     once, at the end of the launch.
//   * new node indices and the random draws stay in descent order: a descent allocates only after its
//     predecessor is completely done.  Board work goes to NWRK worker waves as before.
// Same trees bit for bit (tests/test_gpu_search.py).
constexpr int kMpDone = 1 << 30;        // level_done value of a finished descent
constexpr int kMpTrackDepth = 64;       // levels with a published node (deeper: wait for the predecessors outright)

template <int S, int NSEL, int NWRK>
struct MPipeShared {
    static constexpr int kMpSlots = 2 * NWRK;      // job ring; a multiple of the worker count
    static constexpr int kRing = 2 * NSEL;         // rows of lvl_node: a row is reused only after its reader is done
    Lds<S, false> board[NWRK];
    PipeJob job[kMpSlots];
    int16_t moves[kMpSlots][kPipeMaxDepth];
    int qpath[kMpSlots][kPathCap];    // path_entry(node, edge) of the first kPathCap levels: the worker writes the queue entry
    int job_seq[kMpSlots];            // k + 1 once job k sits in its slot
    int slot_done[kMpSlots];          // jobs finished in this slot so far
    int done[kPipeMaxK];              // job k finished (node initialised, planes written)
    int level_done[kPipeMaxK];        // levels descent k has left behind (kMpDone: leaf queued)
    int lvl_node[kRing][kMpTrackDepth];
    int16_t jobof[kPipeMaxK];         // node (n0 + i) is being created by job jobof[i]
    int root_vl[Geo<S>::A];           // virtual losses / child indices of the root's children
    int root_idx[Geo<S>::A];
    int num_nodes, nexp;              // owned by the descent whose predecessor is done
    int cursor_seq;
    long long cursor_val;
    int err;
};

// wave-uniform wait for *p >= want: the value read, or -1 on a stall or once another wave has reported an error
template <typename Sh>
__device__ __forceinline__ int mp_wait_val(const Sh &sh, const int *p, int want) {
    for (int spin = 0; spin < kPipeSpinLimit; ++spin) {
        const int v = pipe_load(p);
        if (v >= want) return v;
        if (spin >= 32) {
            if (pipe_load(&sh.err)) return -1;
            __builtin_amdgcn_s_sleep(1);
        }
    }
    return -1;
}
template <typename Sh>
__device__ __forceinline__ bool mp_wait_ge(const Sh &sh, const int *p, int want) {
    return mp_wait_val(sh, p, want) >= 0;
}
// ... and a word the writer stored BEFORE the flag, read in the same round trip: LDS operations of a wave are carried out in issue
// order on both sides (flag read first here, data written first there), so `data` is valid whenever the flag read says so
template <typename Sh>
__device__ __forceinline__ bool mp_wait_with(const Sh &sh, const int *flag, int want, const int *data, int &out) {
    for (int spin = 0; spin < kPipeSpinLimit; ++spin) {
        const int f = *reinterpret_cast<const volatile int *>(flag);
        const int d = *reinterpret_cast<const volatile int *>(data);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (f >= want) { out = d; return true; }
        if (spin >= 32) {
            if (pipe_load(&sh.err)) return false;
            __builtin_amdgcn_s_sleep(1);
        }
    }
    return false;
}

// flag store behind plain LDS stores of the same lane: LDS operations of a wave complete in order, the fence
// only keeps the compiler from reordering them
__device__ __forceinline__ void mp_publish(int *p, int v) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int S, int NSEL, int NWRK>
__global__ __launch_bounds__(64 * (NSEL + NWRK)) void select_puct_mpipe_kernel(SearchDev D, int max_leaves, float *planes) {
    using G = Geo<S>;
    using Shared = MPipeShared<S, NSEL, NWRK>;
    constexpr int A = G::A;
    constexpr int R = (A + 63) / 64;
    constexpr int NTHR = 64 * (NSEL + NWRK);
    constexpr int kMpSlots = Shared::kMpSlots, kRing = Shared::kRing;
    static_assert(kMpSlots % NWRK == 0 && kMpSlots >= NSEL, "job ring");
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    Shared &sh = *reinterpret_cast<Shared *>(mp_smem);
    const int t = blockIdx.x;
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long t_begin = (D.prof && t == 0) ? (long long)__builtin_amdgcn_s_memtime() : 0;
    planes = compact_planes(D, planes, t, max_leaves, 6 * G::P);
    const RootMeta meta = D.meta[t];
    const int n0 = meta.num_nodes;
    const size_t root_ns = (size_t)t * D.N, root_base = root_ns * A;
    const bool active = D.err[t] == 0 && D.halt[t] == 0 && n0 > 0;
    const int n_desc = budget_descents(D, t, max_leaves);              // (the same number in every wavefront: read before any descent)
    if (threadIdx.x < kMpSlots) {
        sh.job_seq[threadIdx.x] = 0;
        sh.slot_done[threadIdx.x] = 0;
    }
    for (int i = threadIdx.x; i < kPipeMaxK; i += NTHR) { sh.done[i] = 0; sh.level_done[i] = 0; }
    if (active)
        for (int i = threadIdx.x; i < A; i += NTHR) {
            sh.root_vl[i] = D.ch_vl[root_base + i];
            sh.root_idx[i] = D.ch_index[root_base + i];
        }
    if (threadIdx.x == 0) {
        sh.cursor_seq = 0;
        sh.cursor_val = D.rng_cursor[t];
        sh.num_nodes = n0;
        sh.nexp = 0;
        sh.err = 0;
    }
    __syncthreads();
    // per-phase s_memtime accumulators of tree 0 (tg_search_profile with TG_MPIPE_PROF=1; tools/profile_select.py)
    const bool prof = D.prof && t == 0;
    long long pc[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long tp = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
    auto lap = [&](int i) {
        if (prof) { const long long now = (long long)__builtin_amdgcn_s_memtime(); pc[i] += now - tp; tp = now; }
    };

    if (wid < NSEL) {
        // ---- selectors: descent k on wave k % NSEL ------------------------------------------
        __builtin_amdgcn_s_setprio(3);          // the critical path: ahead of the workers that share the SIMD
        // the root's children, constant for the launch; c_vl / c_q: virtual loss this wave last saw and its quotient
        int r_vis[R], r_act[R], c_vl[R];
        double r_vsum[R], r_pol[R], c_q[R];
        int root_nc = 0, root_total0 = 0;
        if (active) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = lane + 64 * r, ii = i < A ? i : A - 1;
                r_vis[r] = D.ch_visits[root_base + ii];
                r_act[r] = D.action[root_base + ii];
                r_vsum[r] = D.ch_vsum[root_base + ii];
                r_pol[r] = D.ch_policy[root_base + ii];
                c_vl[r] = D.ch_vl[root_base + ii];
                const int cnt = r_vis[r] + c_vl[r];
                c_q[r] = cnt != 0 ? r_vsum[r] / (double)cnt : 0.0;
            }
            root_nc = D.node[root_ns].children;
            root_total0 = D.node[root_ns].visits + D.node[root_ns].vl;
        }
        for (int k = wid; active && k < n_desc; k += NSEL) {
            if (pipe_load(&sh.err)) break;
            const int slot = k % kMpSlots;
            int *my_nodes = sh.lvl_node[k % kRing];
            lap(8);
            bool ok = mp_wait_ge(sh, &sh.slot_done[slot], k / kMpSlots);          // ring slot free again
            lap(0);
            int node = 0, depth = 0;
            int moves = meta.moves, prev = meta.prev;
            bool pool_full = false;
            while (ok) {
                EdgePick pick;
                size_t ns = root_ns, base = root_base;
                if (depth == 0) {
                    // every descent before this one has added one virtual loss to the root (node.py:76-83)
                    const double sq = __dsqrt_rn((double)(root_total0 + k + 1));
                    // scores for "virtual loss as this wave last saw it" and for "one more" (what one intervening
                    // descent leaves behind) - all the divisions happen before the wait
                    double psq[R], sc[R], sc1[R], q1[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int cnt = r_vis[r] + c_vl[r];
                        psq[r] = r_pol[r] * sq;
                        sc[r] = c_q[r] + psq[r] / (double)(cnt + 1);
                        q1[r] = r_vsum[r] / (double)(cnt + 1);
                        sc1[r] = q1[r] + psq[r] / (double)(cnt + 2);
                        // keep the arithmetic on this side of the wait (hipcc would sink it to its first use)
                        asm volatile("" : "+v"(sc[r]), "+v"(sc1[r]), "+v"(q1[r]), "+v"(psq[r]));
                    }
                    lap(1);
                    if (k > 0) ok = mp_wait_ge(sh, &sh.level_done[k - 1], 1);      // predecessor has left the root
                    lap(2);
                    if (!ok) break;
                    int idx[R];
                    bool slow = false;
                    int vl[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int i = lane + 64 * r, ii = i < A ? i : A - 1;
                        vl[r] = sh.root_vl[ii];
                        idx[r] = sh.root_idx[ii];
                        const int d = vl[r] - c_vl[r];
                        if (d == 1) { sc[r] = sc1[r]; c_q[r] = q1[r]; c_vl[r] = vl[r]; }
                        slow |= d != 0 && d != 1;
                    }
                    if (__any(slow)) {                                         // several descents through one child
#pragma unroll
                        for (int r = 0; r < R; ++r)
                            if (vl[r] != c_vl[r]) {
                                c_vl[r] = vl[r];
                                const int cnt = r_vis[r] + vl[r];
                                c_q[r] = cnt != 0 ? r_vsum[r] / (double)cnt : 0.0;
                                sc[r] = c_q[r] + psq[r] / (double)(cnt + 1);
                            }
                    }
                    double best = 0.0;
                    int best_i = -1;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int i = lane + 64 * r;
                        if (i < root_nc) {
                            double v = sc[r];
                            if (D.cgos && i == root_nc - 1) v -= 0.1;
                            if (best_i < 0 || v > best) { best = v; best_i = i; }
                        }
                    }
                    best_i = wave_argmax_first(best, best_i);
                    const int owner = best_i & 63, oslot = best_i >> 6;
                    int my_move = 0, my_child = 0, my_cnt = 0, my_vl = 0;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (r == oslot) { my_move = r_act[r]; my_child = idx[r]; my_cnt = r_vis[r] + vl[r]; my_vl = vl[r]; }
                    const int src = __builtin_amdgcn_readfirstlane(owner);
                    pick.edge = best_i;
                    pick.move = __builtin_amdgcn_readlane(my_move, src);
                    pick.child = __builtin_amdgcn_readlane(my_child, src);
                    pick.count = __builtin_amdgcn_readlane(my_cnt, src);
                    pick.edge_vl = __builtin_amdgcn_readlane(my_vl, src);
                    pick.node_vl = 0;
                    lap(3);
                } else {
                    lap(8);
                    // predecessors still in flight: wait until each has chosen its node of this level, and until
                    // it has left that node if it is this one
                    for (int j = k - 1; ok && j > k - NSEL && j >= 0; --j) {
                        const bool tracked = depth < kMpTrackDepth;
                        const int v = mp_wait_val(sh, &sh.level_done[j], tracked ? depth : depth + 1);
                        ok = v >= 0;
                        if (ok && v == depth && sh.lvl_node[j % kRing][depth] == node)
                            ok = mp_wait_ge(sh, &sh.level_done[j], depth + 1);
                    }
                    lap(4);
                    if (ok && node >= n0) ok = mp_wait_ge(sh, &sh.done[sh.jobof[node - n0]], 1);   // expansion in flight?
                    lap(5);
                    if (!ok) break;
                    ns = (size_t)t * D.N + node;
                    base = ns * A;
                    pick = select_puct<S>(D, t, node, lane);
                    lap(6);
                }
                const int e = pick.edge;
                const int mv = pick.move;
                if (depth >= kPipeMaxDepth) { ok = false; break; }
                // two consecutive passes: never descend below (tree.py:224-229)
                const bool leaf = tg_queue::puct_descent_ends(pick.count + 1, moves + 1, mv, prev);
                if (lane == 0) {
                    if (depth == 0) {
                        sh.root_vl[e] = pick.edge_vl + 1;
                    } else {
                        D.node[ns].vl = pick.node_vl + 1;                             // node.py:76-83
                        D.ch_vl[base + e] = pick.edge_vl + 1;
                    }
                    // the successors may have this node as soon as the virtual loss is in place (a descent that ends
                    // here publishes when its leaf is queued: the child index has to be there first)
                    if (!leaf) {
                        if (depth + 1 < kMpTrackDepth) my_nodes[depth + 1] = pick.child;
                        if (depth == 0) mp_publish(&sh.level_done[k], 1);         // only LDS was written at the root
                        else pipe_store(&sh.level_done[k], depth + 1);
                    }
                    sh.moves[slot][depth] = (int16_t)mv;
                    if (depth < kPathCap) sh.qpath[slot][depth] = path_entry(node, e);
                }
                ++depth;
                prev = mv;
                ++moves;
                if (prof) pc[13] += 1;
                if (leaf) {
                    lap(8);
                    if (k > 0) ok = mp_wait_ge(sh, &sh.level_done[k - 1], kMpDone); // node numbers in descent order
                    lap(7);
                    if (!ok) break;
                    int num_nodes = sh.num_nodes, nexp = sh.nexp;
                    int child = pick.child;
                    const int expand = child == kNotExpanded;
                    int xseq = 0;
                    if (expand) {
                        if (num_nodes >= D.N || num_nodes - n0 >= kPipeMaxK) { pool_full = true; ok = false; break; }
                        child = num_nodes++;
                        xseq = nexp++;
                    }
                    if (lane == 0) {
                        if (expand) {
                            D.ch_index[base + e] = child;
                            if (node == 0) sh.root_idx[e] = child;
                            sh.jobof[child - n0] = (int16_t)k;
                            sh.num_nodes = num_nodes;
                            sh.nexp = nexp;
                        }
                        PipeJob &j = sh.job[slot];
                        j.k = k; j.parent = node; j.edge = e; j.child = child;
                        j.expand = expand; j.xseq = xseq; j.depth = depth;
                        // (the leaf's queue entry - node, parent, edge, recorded path - is written by the worker)
                        pipe_store(&sh.job_seq[slot], k + 1);
                        pipe_store(&sh.level_done[k], kMpDone);
                    }
                    break;
                }
                node = pick.child;
            }
            if (!ok) {
                if (lane == 0 && !pipe_load(&sh.err)) {
                    atomicOr(&D.err[t], pool_full ? kErrPoolFull : kErrPipeline);
                    pipe_store(&sh.err, 1);
                }
                break;
            }
        }
    } else {
        // ---- workers: job k on wave k % NWRK --------------------------------------------------
        const int w = wid - NSEL;
        Lds<S, false> &L = sh.board[w];
        BoardScalars rootb;
        int root_to_move;
        load_root<S>(L, rootb, root_to_move, D, t, lane);
        lap(14);
        for (int k = w; active && k < n_desc; k += NWRK) {
            const int slot = k % kMpSlots;
            lap(12);
            const bool have = mp_wait_ge(sh, &sh.job_seq[slot], k + 1);
            lap(9);
            if (!have) {
                if (lane == 0 && !pipe_load(&sh.err)) {
                    atomicOr(&D.err[t], kErrPipeline);
                    pipe_store(&sh.err, 1);
                }
                break;
            }
            const PipeJob j = sh.job[slot];
            {
                // queue entry of leaf k (what the backup reads): off the selectors' critical path
                const size_t qs = (size_t)t * D.K + k;
                const int npath = j.depth < kPathCap ? j.depth : kPathCap;
                if (lane < npath) D.q_path[qs * kPathCap + lane] = sh.qpath[slot][lane];
                if (lane == 0) write_queue_entry(D, qs, j.child, j.parent, j.edge, j.depth);
            }
            reset_work<S>(L, lane);
            BoardScalars b = rootb;
            int c = root_to_move;
            for (int i = 0; i < j.depth; ++i) {
                put_stone<S>(L, b, sh.moves[slot][i], c, D.zob, lane);
                c = 3 - c;
            }
            lap(10);
            if (j.expand) expand_node_pipe<S>(L, b, c, D, t, j.child, j.parent, j.edge, j.xseq, sh, lane);
            lap(11);
            write_planes<S>(L, b, c, planes + ((size_t)t * max_leaves + k) * 6 * G::P, lane);
            wave_sync();
            if (lane == 0) {
                pipe_store(&sh.done[k], 1);                                        // releases the node arrays
                pipe_store(&sh.slot_done[slot], k / kMpSlots + 1);
            }
        }
    }
    if (prof && lane == 0)
        for (int i = 0; i < 15; ++i) atomicAdd(reinterpret_cast<unsigned long long *>(D.prof + i), (unsigned long long)pc[i]);
    __syncthreads();
    const bool good = active && !sh.err;
    if (good) {
        // the root's virtual losses (n_desc descents, one each) reach the pool here
        for (int i = threadIdx.x; i < A; i += NTHR) D.ch_vl[root_base + i] = sh.root_vl[i];
        if (threadIdx.x == 0) D.node[root_ns].vl += n_desc;
    }
    if (prof && threadIdx.x == 0) D.prof[15] += (long long)__builtin_amdgcn_s_memtime() - t_begin;
    if (threadIdx.x == 0) {
        D.meta[t].num_nodes = sh.num_nodes;
        D.n_leaves[t] = good ? n_desc : 0;
        set_cursor(D, t, sh.cursor_val);
    }
}

constexpr int kOwnNotYet = -3;        // alloc_child of a descent whose leaf the allocator has not taken yet

__device__ __forceinline__ int wave_min_i32(int v) {
    v = min(v, lane_partner_i32<0>(v));
    v = min(v, lane_partner_i32<1>(v));
    v = min(v, lane_partner_i32<2>(v));
    v = min(v, lane_partner_i32<3>(v));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// ---- PUCT selection of one tree on SEVERAL compute units -----------------------------------------------------------
// Both kernels above keep ~40 k wave-cycles of work per descent on the 16 waves a workgroup can have - on ONE CU -
// and 25 k of it is the workers' board work (path replay, candidates, priors, planes), which needs nothing from the
// selectors but the job.  Here a tree gets 1 + NWG workgroups: the first is the selecting half of the node-owner design (root
// owner, node owners, allocator, plus "shippers" and the draw cursor), the others are nothing but workers, on other
// CUs (consecutive workgroups go to different XCDs).  What crosses between them goes through memory with agent-coherent
// accesses (relaxed agent-scope atomics: sc1 loads and stores, served at the coherence point, no cache maintenance):
//   * shippers -> workers: the job (header, recorded path, moves) in a per-launch array of entries, one store
//     instruction per 64 words, `s_waitcnt vmcnt(0)`, then the entry's tag word.  Tags carry the launch number, so
//     nothing has to be cleared between launches.  All jobs of a launch have their own entry: the selecting half
//     never waits for the workers to free anything.  A store to the coherence point takes longer than the root takes for
//     a descent: NSHIP waves ship, job k on wave k % NSHIP;
//   * workers -> node owners: "node initialised" (only consulted when a descent steps into a node created in the same
//     launch): the node's arrays are ordinary stores, so the worker releases at agent scope (L2 write-back) before
//     it stores the tag, and the owner acquires (invalidate) before it loads the node;
//   * the random-draw cursor: inside ONE workgroup of workers a chain through LDS (NWG = 1); with more, counts in and
//     offsets out through a wave of the selecting half (see the kernel).
// Bounded spins everywhere (a stall is an error, never a hang).  Same trees bit for bit.
// -DTG_SPLIT_PROF (tools/experiments/split_prof.sh): s_memtime accumulators of tree 0 in D.prof - who waits for whom in a launch
// (0 root loop, 1 root's wait for a free slot, 2 allocator loop, 3 allocator's wait, 4 node owner 1 busy, 5 its steps, 6 shipper 0
// loop, 7-10 worker (1, 0): wait for a job / replay / expansion / planes, 12 start of the selecting half (absolute), 13 latest end
// of a worker (absolute), 15 selecting half start to end)
#ifdef TG_SPLIT_PROF
#define SP_NOW() ((long long)__builtin_amdgcn_s_memtime())
#define SP_ON(D, t) ((D).prof != nullptr && (t) == 0)
#else
#define SP_NOW() 0LL
#define SP_ON(D, t) false
#endif
constexpr int kXwHeader = 8;                                   // words: tag, parent, edge, child, expand, xseq, depth, k
template <int S>
constexpr int kXwEntryWords = kXwHeader + kPathCap + kPathMax<S> / 2;
constexpr int kXwMaxTrees = 16;

__device__ __forceinline__ int xw_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void xw_store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int S, int NNODE>
struct SplitSelShared {
    static constexpr int kSlots = 64;                 // descents inside the selecting half: one mail word per lane
    int16_t moves[kSlots][kPathMax<S>];
    int qpath[kSlots][kPathCap];
    int slot_free[kSlots];            // descents this slot has seen through (shipped to the workers)
    int mail[64];
    int st_node[kSlots], st_depth[kSlots], st_prev[kSlots], st_redge[kSlots];
    int lm_parent[kSlots], lm_edge[kSlots], lm_child[kSlots], lm_depth[kSlots];
    int leaf_ready[kSlots];
    int sp_child[kSlots], sp_expand[kSlots], sp_xseq[kSlots];   // the allocator's part of the job, for the shipper
    int ship_ready[kSlots];           // k + 1 once descent k's job can be shipped
    int alloc_child[kPipeMaxK];
    int exp_key[kPipeMaxK];
    int16_t jobof[kPipeMaxK];
    int num_nodes;
    int nexp_total;                   // expansions of the launch (once all_done)
    int all_done;
    int err;
    // the root owner's step is the chain a launch hangs on: sqrt(N + k + 1) of every descent and the correctly rounded
    // reciprocals of the counts a child can reach are made by the whole workgroup before the chain starts
    double sq[kPipeMaxK];
    double rcp[kRcpN];
    int choice[kPipeMaxK];            // root edge of descent k + 1 (0: not chosen yet): the chooser's only product, the clerk's input
};
template <int S, int NWRK>
struct SplitWrkShared {
    Lds<S, false> board[NWRK];
    int16_t moves[NWRK][kPathMax<S>];
    int cursor_seq;
    long long cursor_val;
    int err;
};

// NWG workgroups of workers.  With more than one, the draw cursor (expansion x takes the n_x draws behind those of
// expansions 0 .. x - 1) cannot be chained through one workgroup's LDS: a worker reports n_x once its candidates are
// counted, a wave of the selecting half adds the counts up in expansion order and hands out the offsets, and the worker
// - which has written its planes meanwhile - fills in the prior when its offset is there.
template <int S, int NNODE, int NWRK, int NSHIP, int NWG>
__global__ __launch_bounds__(1024) void select_puct_split_kernel(SearchDev D, int max_leaves, float *planes, int *xw_job,
                                                                   int *xw_done, int *xw_n, unsigned long long *xw_off,
                                                                   int tag_base, int cap, int test_mute) {
    using G = Geo<S>;
    constexpr int A = G::A;
    constexpr int R = (A + 63) / 64;
    constexpr int EW = kXwEntryWords<S>;
    extern __shared__ __attribute__((aligned(16))) unsigned char xw_smem[];
    const int t = blockIdx.x / (1 + NWG);
    const int role = blockIdx.x % (1 + NWG);          // 0: selecting half, 1 .. NWG: workers
    const bool selecting = role == 0;
    // test hook (TG_SPLIT_TEST_MUTE): the worker workgroups of a tree never show up - the selecting half must run into its
    // bounded waits and report a stalled pipeline (kErrPipeline), not hang (tests/test_gpu_search.py)
    if (test_mute && !selecting) return;
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    planes = compact_planes(D, planes, t, max_leaves, 6 * G::P);
    const RootMeta meta = D.meta[t];
    const int n0 = meta.num_nodes;
    const size_t root_ns = (size_t)t * D.N, root_base = root_ns * A;
    const bool active = D.err[t] == 0 && D.halt[t] == 0 && n0 > 0;
    const int n_desc = budget_descents(D, t, max_leaves);              // (the same number in every workgroup and wavefront of the tree)
    int *const jobs = xw_job + (size_t)t * cap * EW;
    int *const done = xw_done + (size_t)t * cap;
    int *const xn = xw_n + (size_t)t * cap;                                   // candidates of expansion x (tagged)
    unsigned long long *const xoff = xw_off + (size_t)t * (cap + 1);          // draws before expansion x (tagged)
    const long long cursor0 = D.rng_cursor[t];

    const bool sp = SP_ON(D, t) && lane == 0;
    const long long sp_t0 = SP_NOW();
    if (selecting) {
        using Shared = SplitSelShared<S, NNODE>;
        constexpr int kSlots = Shared::kSlots;
        Shared &sh = *reinterpret_cast<Shared *>(xw_smem);
        if (sp && threadIdx.x == 0) D.prof[12] = sp_t0;
        if (threadIdx.x < kSlots) {
            sh.slot_free[threadIdx.x] = 0; sh.leaf_ready[threadIdx.x] = 0; sh.ship_ready[threadIdx.x] = 0; sh.mail[threadIdx.x] = 0;
        }
        for (int i = threadIdx.x; i < kPipeMaxK; i += 1024) { sh.alloc_child[i] = kOwnNotYet; sh.exp_key[i] = -1; sh.choice[i] = 0; }
        if (threadIdx.x == 0) { sh.num_nodes = n0; sh.all_done = 0; sh.err = 0; }
        {
            const int total0 = D.node[root_ns].visits + D.node[root_ns].vl;
            for (int i = threadIdx.x; i < n_desc; i += 1024) sh.sq[i] = __dsqrt_rn((double)(total0 + i + 1));
            for (int i = threadIdx.x; i < kRcpN; i += 1024) sh.rcp[i] = 1.0 / (double)(i ? i : 1);
        }
        __syncthreads();
        auto fail = [&](int code, int site) {
            if (lane == 0 && !pipe_load(&sh.err)) {
                atomicOr(&D.err[t], code | (site << 8));
                pipe_store(&sh.err, 1);
            }
        };
        // ---- the root.  Every descent passes it, so its step is the chain a launch hangs on.  Two halves:
        //  * the CHOICE - scores of all children for sqrt(N + k + 1), arg-max, one more virtual loss on the winner - is all that is
        //    serial;
        //  * what a choice entails (move, child, leaf or step, the job for the owners / the allocator, slots) is clerical.
        // DUAL (9x9): wave 0 only chooses and leaves the edge in sh.choice[k]; the clerk (wave kClerk, on another SIMD) follows the
        // ring: one wave doing both took ~1 700 cycles per descent = 96 % of a launch, the chooser alone takes ~1 050.  At 19x19 the
        // sixteenth wave is worth more as a tenth node owner (deep trees: the launches hang on the owners): wave 0 does both there.
        constexpr bool DUAL = S == 9;
        constexpr int kClerk = DUAL ? NNODE + 2 + NSHIP + (NWG > 1 ? 1 : 0) : -1;
        int r_vis[R], r_act[R], r_idx[R], r_kref[R], c_vl[R], c_cnt[R], root_nc = 0;
        double r_vsum[R], r_pol[R], c_q[R], c_rcp[R], c_rcpn[R];
        auto chooser_init = [&]() {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = lane + 64 * r, ii = i < A ? i : A - 1;
                r_vsum[r] = D.ch_vsum[root_base + ii];
                r_pol[r] = D.ch_policy[root_base + ii];
                c_cnt[r] = D.ch_visits[root_base + ii] + D.ch_vl[root_base + ii];
                c_q[r] = c_cnt[r] != 0 ? r_vsum[r] / (double)c_cnt[r] : 0.0;
                // reciprocals of count + 1 (this step's denominator) and count + 2 (the next one, should this child be chosen:
                // requested a step ahead, so that no LDS round trip sits between two choices)
                if (__any(c_cnt[r] + 2 >= kRcpN)) { c_rcp[r] = 1.0 / (double)(c_cnt[r] + 1); c_rcpn[r] = 1.0 / (double)(c_cnt[r] + 2); }
                else { c_rcp[r] = sh.rcp[c_cnt[r] + 1]; c_rcpn[r] = sh.rcp[c_cnt[r] + 2]; }
            }
            root_nc = D.node[root_ns].children;
        };
        auto choose = [&](double sq) -> int {
            double best = 0.0;
            int best_i = -1;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = lane + 64 * r;
                if (i < root_nc) {
                    double v = c_q[r] + div_by_count(r_pol[r] * sq, (double)(c_cnt[r] + 1), c_rcp[r]);
                    if (D.cgos && i == root_nc - 1) v -= 0.1;
                    if (best_i < 0 || v > best) { best = v; best_i = i; }
                }
            }
            best_i = wave_argmax_first(best, best_i);
            if (best_i < 0) best_i = 0;                                      // (a diverged network: every score NaN)
            return best_i;
        };
        auto chosen = [&](int best_i) {                                      // one more virtual loss on the winner
            const int owner = best_i & 63, oslot = best_i >> 6;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r == oslot) {
                    // the winner's new count is its old denominator: q = value sum / count by the reciprocal it holds
                    const double q = div_by_count(r_vsum[r], (double)(c_cnt[r] + 1), c_rcp[r]);
                    double nn;
                    if (__any(lane == owner && c_cnt[r] + 3 >= kRcpN)) nn = 1.0 / (double)(c_cnt[r] + 3);
                    else nn = sh.rcp[c_cnt[r] + 3 < kRcpN ? c_cnt[r] + 3 : 0];
                    if (lane == owner) { c_q[r] = q; c_cnt[r] += 1; c_rcp[r] = c_rcpn[r]; c_rcpn[r] = nn; }
                }
        };
        auto clerk_init = [&]() {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = lane + 64 * r, ii = i < A ? i : A - 1;
                r_vis[r] = D.ch_visits[root_base + ii];
                r_act[r] = D.action[root_base + ii];
                r_idx[r] = D.ch_index[root_base + ii];
                c_vl[r] = D.ch_vl[root_base + ii];
                r_kref[r] = -1;
            }
        };
        auto clerk_step = [&](int k, int slot, int best_i) -> bool {
            const int owner = best_i & 63, oslot = best_i >> 6;
            int my_move = 0, my_child = 0, my_cnt = 0, my_kref = -1;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r == oslot) { my_move = r_act[r]; my_child = r_idx[r]; my_cnt = r_vis[r] + c_vl[r]; my_kref = r_kref[r]; }
            const int src = __builtin_amdgcn_readfirstlane(owner);
            const int e = best_i;
            const int mv = __builtin_amdgcn_readlane(my_move, src);
            int child = __builtin_amdgcn_readlane(my_child, src);
            const int count = __builtin_amdgcn_readlane(my_cnt, src);
            const int kref = __builtin_amdgcn_readlane(my_kref, src);
            const bool leaf = tg_queue::puct_descent_ends(count + 1, meta.moves + 1, mv, meta.prev);
            if (child == kNotExpanded && kref >= 0) child = -2 - kref;
            const bool expands = leaf && child == kNotExpanded;
            if (!leaf && child == kNotExpanded) return false;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r == oslot && lane == owner) {
                    c_vl[r] += 1;
                    if (expands) r_kref[r] = k;
                }
            if (lane == 0) {
                sh.moves[slot][0] = (int16_t)mv;
                sh.qpath[slot][0] = path_entry(0, e);
                if (leaf) {
                    sh.lm_parent[slot] = 0; sh.lm_edge[slot] = e; sh.lm_child[slot] = child; sh.lm_depth[slot] = 1;
                    mp_publish(&sh.leaf_ready[slot], k + 1);
                } else {
                    sh.st_node[slot] = child; sh.st_depth[slot] = 1; sh.st_prev[slot] = mv; sh.st_redge[slot] = e;
                    mp_publish(&sh.mail[slot], ((k + 1) << 8) | (1 + (1 + e) % NNODE));
                }
            }
            return true;
        };
        auto clerk_done = [&](bool ok) {
            if (!ok) fail(kErrPipeline, 1);
            if (ok) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int i = lane + 64 * r;
                    if (i < A) D.ch_vl[root_base + i] = c_vl[r];
                }
                if (lane == 0) D.node[root_ns].vl += n_desc;
            }
        };
        if (wid == 0) {
            __builtin_amdgcn_s_setprio(3);
            if (active) {
                chooser_init();
                if constexpr (!DUAL) clerk_init();
                double sq = sh.sq[0];
                bool ok = true;
                long long sp_acc = 0;
                for (int k = 0; k < n_desc; ++k) {
                    const double sqn = sh.sq[k + 1 < n_desc ? k + 1 : k];      // (used by the next step)
                    if constexpr (!DUAL) {
                        const long long sp_w = SP_NOW();
                        ok = mp_wait_ge(sh, &sh.slot_free[k % kSlots], k / kSlots);
                        sp_acc += SP_NOW() - sp_w;
                        if (!ok) break;
                    }
                    const int best_i = choose(sq);
                    if constexpr (DUAL) {
                        if (lane == 0) pipe_store(&sh.choice[k], best_i + 1);
                    } else {
                        ok = clerk_step(k, k % kSlots, best_i);
                        if (!ok) break;
                    }
                    chosen(best_i);
                    sq = sqn;
                }
                if (sp) D.prof[14] += SP_NOW() - sp_t0;
                if constexpr (!DUAL) {
                    if (sp) { D.prof[0] += SP_NOW() - sp_t0; D.prof[1] += sp_acc; }
                    clerk_done(ok);
                }
            }
        } else if (DUAL && wid == kClerk) {
            __builtin_amdgcn_s_setprio(3);
            if (active) {
                clerk_init();
                bool ok = true;
                long long sp_acc = 0;
                for (int k = 0; k < n_desc; ++k) {
                    const int slot = k % kSlots;
                    // the choice and the slot's release in one round trip
                    const long long sp_w = SP_NOW();
                    int ch = 0;
                    ok = false;
                    for (int spin = 0; spin < kPipeSpinLimit; ++spin) {
                        ch = *reinterpret_cast<const volatile int *>(&sh.choice[k]);
                        const int fr = *reinterpret_cast<const volatile int *>(&sh.slot_free[slot]);
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        if (ch >= 1 && fr >= k / kSlots) { ok = true; break; }
                        if (spin >= 32) {
                            if (pipe_load(&sh.err)) break;
                            __builtin_amdgcn_s_sleep(1);
                        }
                    }
                    sp_acc += SP_NOW() - sp_w;
                    if (!ok) break;
                    ok = clerk_step(k, slot, ch - 1);
                    if (!ok) break;
                }
                if (sp) { D.prof[0] += SP_NOW() - sp_t0; D.prof[1] += sp_acc; }
                clerk_done(ok);
            }
        } else if (wid <= NNODE) {
            // ---- owners of the nodes below the root ----------------------------------------------------
            __builtin_amdgcn_s_setprio(2);
            const int me = wid;
            int idle = 0;
            int unf0 = -1, unf1 = -1, unf2 = -1, unf3 = -1, n_unf = 0;
            long long sp_busy = 0, sp_steps = 0, sp_hits = 0;
            int sp_last = -1;
            while (active) {
                const int w = lane < kSlots ? pipe_load(&sh.mail[lane]) : 0;
                const bool mine = (w & 255) == me;
                int nd = mine ? sh.st_node[lane] : 0;
                bool ready = mine;
                bool fresh;
                {
                    const bool pending = mine && nd <= -2;
                    const int c = pipe_load(&sh.alloc_child[pending ? -2 - nd : 0]);
                    if (pending) {
                        if (c == kOwnNotYet) ready = false;
                        else nd = c;
                    }
                    fresh = ready && nd >= n0;                                    // created in this launch
                    if (__any(fresh)) {
                        // initialised by its worker?  (the other workgroup: an agent-coherent load)
                        const int jk = fresh ? (int)sh.jobof[nd - n0] : 0;
                        const int dn = xw_load(&done[jk]);
                        if (fresh && dn != (tag_base | (jk + 1))) ready = false;
                    }
                }
                const int kmin = wave_min_i32(ready ? (w >> 8) - 1 : 0x7fffffff);
                const int k = kmin == 0x7fffffff ? -1 : kmin;
                const int slot = k >= 0 ? k % kSlots : 0;
                const int node = __builtin_amdgcn_readlane(nd, slot);
                const bool was_fresh = __builtin_amdgcn_readlane((int)fresh, slot) != 0;
                if (k < 0) {
                    if (pipe_load(&sh.all_done) || pipe_load(&sh.err)) break;
                    if (++idle > kPipeSpinLimit / 16) { fail(kErrPipeline, 2); break; }
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                idle = 0;
                const long long sp_b = SP_NOW();
                const int depth = sh.st_depth[slot], prev = sh.st_prev[slot], redge = sh.st_redge[slot];
                if (depth >= kPathMax<S>) { fail(kErrPipeline, 3); break; }
                if (was_fresh) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");              // the worker's stores, not a stale line
                    unf0 = unf1 = unf2 = unf3 = -1;
                    n_unf = 0;
                } else if (node == unf0 || node == unf1 || node == unf2 || node == unf3 || n_unf >= 4) {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    unf0 = unf1 = unf2 = unf3 = -1;
                    n_unf = 0;
                } else {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                }
                if (n_unf == 0) unf0 = node;
                else if (n_unf == 1) unf1 = node;
                else if (n_unf == 2) unf2 = node;
                else unf3 = node;
                ++n_unf;
                const EdgePick pick = select_puct<S>(D, t, node, lane, sh.rcp);
                const int e = pick.edge, mv = pick.move;
                const size_t ns = (size_t)t * D.N + node, base = ns * A;
                const bool leaf = tg_queue::puct_descent_ends(pick.count + 1, meta.moves + depth + 1, mv, prev);
                int child = pick.child;
                const int key = path_entry(node, e);
                if (child == kNotExpanded && pick.count >= 1) {
                    int kref = -1;
                    for (int b0 = 0; b0 < k && kref < 0; b0 += 64) {
                        const unsigned long long hit = __ballot(b0 + lane < k && sh.exp_key[b0 + lane] == key);
                        if (hit) kref = b0 + __ffsll((long long)hit) - 1;
                    }
                    if (kref < 0) { fail(kErrPipeline, 4); break; }
                    child = -2 - kref;
                }
                if (lane == 0) {
                    D.node[ns].vl = pick.node_vl + 1;                                   // node.py:76-83
                    D.ch_vl[base + e] = pick.edge_vl + 1;
                    sh.moves[slot][depth] = (int16_t)mv;
                    if (depth < kPathCap) sh.qpath[slot][depth] = key;
                    if (leaf) {
                        if (child == kNotExpanded) sh.exp_key[k] = key;
                        sh.lm_parent[slot] = node; sh.lm_edge[slot] = e; sh.lm_child[slot] = child; sh.lm_depth[slot] = depth + 1;
                        sh.mail[slot] = 0;
                        mp_publish(&sh.leaf_ready[slot], k + 1);
                    } else {
                        sh.st_node[slot] = child; sh.st_depth[slot] = depth + 1; sh.st_prev[slot] = mv;
                        mp_publish(&sh.mail[slot], ((k + 1) << 8) | (1 + (depth + 1 + redge) % NNODE));
                    }
                }
                wave_sync();
                sp_busy += SP_NOW() - sp_b;
                sp_steps += 1;
                sp_hits += (node == sp_last && !was_fresh);
                sp_last = node;
            }
#ifndef TG_BACKUP_PROF
            if (sp && me == 1) { D.prof[4] += sp_busy; D.prof[5] += sp_steps; }
#ifdef TG_SPLIT_PROF_HITS      // all owners: steps in slot 11, steps on the node the owner handled last in slot 14
            if (sp) { atomicAdd(reinterpret_cast<unsigned long long *>(D.prof + 11), (unsigned long long)sp_steps); atomicAdd(reinterpret_cast<unsigned long long *>(D.prof + 14), (unsigned long long)sp_hits); }
#endif
#endif
        } else if (wid == NNODE + 1) {
            // ---- the allocator: leaves in descent order (LDS only: what later descents may be waiting for) ----
            int num_nodes = n0, nexp = 0;
            bool ok = active;
            long long sp_acc = 0;
            for (int k = 0; ok && k < n_desc; ++k) {
                const int slot = k % kSlots;
                const long long sp_w = SP_NOW();
                int child = 0;
                ok = mp_wait_with(sh, &sh.leaf_ready[slot], k + 1, &sh.lm_child[slot], child);
                sp_acc += SP_NOW() - sp_w;
                if (!ok) { fail(kErrPipeline, 5); break; }
                if (child <= -2) child = sh.alloc_child[-2 - child];
                const int expand = child == kNotExpanded;
                int xseq = 0;
                if (expand) {
                    if (num_nodes >= D.N || num_nodes - n0 >= kPipeMaxK) { fail(kErrPoolFull, 6); ok = false; break; }
                    child = num_nodes++;
                    xseq = nexp++;
                }
                // (the parent's child index in memory is the shipper's store: behind ship_ready, i.e. behind jobof)
                if (lane == 0) {
                    if (expand) sh.jobof[child - n0] = (int16_t)k;
                    sh.sp_child[slot] = child; sh.sp_expand[slot] = expand; sh.sp_xseq[slot] = xseq;
                    mp_publish(&sh.alloc_child[k], child);
                    mp_publish(&sh.ship_ready[slot], k + 1);
                }
            }
            if (lane == 0) {
                sh.num_nodes = num_nodes;
                sh.nexp_total = nexp;
                if (ok) mp_publish(&sh.all_done, 1);
            }
#ifndef TG_BACKUP_PROF
            if (sp) { D.prof[2] += SP_NOW() - sp_t0; D.prof[3] += sp_acc; }
#endif
        } else if (wid < NNODE + 2 + NSHIP) {
            // ---- shippers: job k to the workers' workgroup, on wave k % NSHIP (a store to the coherence point takes
            //      longer than the root takes for a descent: several jobs are under way at a time) ----
            const int j = wid - (NNODE + 2);
            for (int k = j; active && k < n_desc; k += NSHIP) {
                const int slot = k % kSlots;
                if (!mp_wait_ge(sh, &sh.ship_ready[slot], k + 1)) { fail(kErrPipeline, 8); break; }
                const int depth = sh.lm_depth[slot];
                int *const entry = jobs + (size_t)k * EW;
                {
                    // header (words 1..7), recorded path, moves (two per word): one store per 64 words
                    int word = 0;
                    if (lane == 1) word = sh.lm_parent[slot];
                    else if (lane == 2) word = sh.lm_edge[slot];
                    else if (lane == 3) word = sh.sp_child[slot];
                    else if (lane == 4) word = sh.sp_expand[slot];
                    else if (lane == 5) word = sh.sp_xseq[slot];
                    else if (lane == 6) word = depth;
                    else if (lane == 7) word = k;
                    else if (lane >= kXwHeader && lane < kXwHeader + kPathCap) word = sh.qpath[slot][lane - kXwHeader];
                    if (lane >= 1 && lane < kXwHeader + kPathCap) xw_store(&entry[lane], word);
                    // a new node becomes findable from its parent (jobof has been in LDS since before ship_ready)
                    if (lane == 4 && word) D.ch_index[((size_t)t * D.N + sh.lm_parent[slot]) * A + sh.lm_edge[slot]] = sh.sp_child[slot];
                    for (int jj = lane; 2 * jj < depth; jj += 64) {
                        const int lo = (unsigned short)sh.moves[slot][2 * jj];
                        const int hi = 2 * jj + 1 < depth ? (unsigned short)sh.moves[slot][2 * jj + 1] : 0;
                        xw_store(&entry[kXwHeader + kPathCap + jj], lo | (hi << 16));
                    }
                }
                __builtin_amdgcn_s_waitcnt(0x0F70);                                  // vmcnt(0): the entry is written ...
                if (lane == 0) {
                    xw_store(&entry[0], tag_base | (k + 1));                         // ... before its tag
                    mp_publish(&sh.slot_free[slot], k / kSlots + 1);
                }
            }
            if (sp && j == 0) D.prof[6] += SP_NOW() - sp_t0;
        }
        if (NWG > 1 && wid == NNODE + 2 + NSHIP && active) {
            // ---- the draw cursor: counts in, offsets out, in expansion order ----
            unsigned off = 0;
            bool ok = true;
            if (lane == 0) __hip_atomic_store(&xoff[0], ((unsigned long long)(unsigned)tag_base << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int x = 0; ok; ++x) {
                int v = 0;
                bool have = false;
                for (int spin = 0; spin < kPipeSpinLimit / 16; ++spin) {
                    if (x < cap) {
                        v = xw_load(&xn[x]);
                        if ((v & ~2047) == tag_base && (v & 2047) != 0) { have = true; break; }
                    }
                    if (pipe_load(&sh.all_done) && x >= sh.nexp_total) break;   // every expansion has been through
                    if (pipe_load(&sh.err)) { ok = false; break; }
                    if ((spin & 63) == 63 && xw_load(&D.err[t])) {
                        // a worker workgroup gave up (it has reported why): stop this workgroup's owners too, instead of
                        // letting them spin to their limits on nodes that will never be initialised
                        if (lane == 0) pipe_store(&sh.err, 1);
                        ok = false;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (!have) {
                    if (ok && !(pipe_load(&sh.all_done) && x >= sh.nexp_total)) { fail(kErrPipeline, 9); ok = false; }
                    break;
                }
                off += (unsigned)((v & 2047) - 1);
                if (lane == 0 && x + 1 <= cap)
                    __hip_atomic_store(&xoff[x + 1], ((unsigned long long)(unsigned)tag_base << 32) | off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (ok && lane == 0) set_cursor(D, t, cursor0 + (long long)off);
        }
        __syncthreads();
        const bool good = active && !sh.err;
        if (threadIdx.x == 0) {
            D.meta[t].num_nodes = sh.num_nodes;
            D.n_leaves[t] = good ? n_desc : 0;
            if (sp) D.prof[15] += SP_NOW() - sp_t0;
        }
    } else {
        // ---- the workers' workgroup: job k on wave k % NWRK ----------------------------------------------------
        using Shared = SplitWrkShared<S, NWRK>;
        Shared &sh = *reinterpret_cast<Shared *>(xw_smem);
        if (threadIdx.x == 0) { sh.cursor_seq = 0; sh.cursor_val = D.rng_cursor[t]; sh.err = 0; }
        __syncthreads();
        if (wid < NWRK) {
            const int w = wid;
            Lds<S, false> &L = sh.board[w];
            BoardScalars rootb;
            int root_to_move;
            load_root<S>(L, rootb, root_to_move, D, t, lane);
            long long sp_a[4] = {0, 0, 0, 0};
            for (int k = (role - 1) * NWRK + w; active && k < n_desc; k += NWG * NWRK) {
                const int *const entry = jobs + (size_t)k * EW;
                bool have = false;
                long long sp_x = SP_NOW();
                for (int spin = 0; spin < kPipeSpinLimit / 16; ++spin) {
                    if (xw_load(&entry[0]) == (tag_base | (k + 1))) { have = true; break; }
                    if ((spin & 63) == 63 && (xw_load(&D.err[t]) || pipe_load(&sh.err))) break;   // the other half gave up
                    __builtin_amdgcn_s_sleep(2);
                }
                if (!have) {
                    if (lane == 0 && !xw_load(&D.err[t])) atomicOr(&D.err[t], kErrPipeline | (7 << 8));
                    if (lane == 0) pipe_store(&sh.err, 1);
                    break;
                }
                { const long long n = SP_NOW(); sp_a[0] += n - sp_x; sp_x = n; }
                const int hw = lane < kXwHeader + kPathCap ? xw_load(&entry[lane]) : 0;
                const int parent = __builtin_amdgcn_readlane(hw, 1), edge = __builtin_amdgcn_readlane(hw, 2);
                const int child = __builtin_amdgcn_readlane(hw, 3), expand = __builtin_amdgcn_readlane(hw, 4);
                const int xseq = __builtin_amdgcn_readlane(hw, 5), depth = __builtin_amdgcn_readlane(hw, 6);
                for (int j = lane; 2 * j < depth; j += 64) {
                    const int mw = xw_load(&entry[kXwHeader + kPathCap + j]);
                    sh.moves[w][2 * j] = (int16_t)(mw & 0xffff);
                    if (2 * j + 1 < depth) sh.moves[w][2 * j + 1] = (int16_t)((unsigned)mw >> 16);
                }
                {
                    // queue entry of leaf k (what the backup reads)
                    const size_t qs = (size_t)t * D.K + k;
                    const int npath = depth < kPathCap ? depth : kPathCap;
                    if (lane >= kXwHeader && lane < kXwHeader + npath) D.q_path[qs * kPathCap + lane - kXwHeader] = hw;
                    if (lane == 0) write_queue_entry(D, qs, child, parent, edge, depth);
                }
                wave_sync();
                reset_work<S>(L, lane);
                BoardScalars b = rootb;
                int c = root_to_move;
                for (int i = 0; i < depth; ++i) {
                    put_stone<S>(L, b, sh.moves[w][i], c, D.zob, lane);
                    c = 3 - c;
                }
                { const long long n = SP_NOW(); sp_a[1] += n - sp_x; sp_x = n; }
                if constexpr (NWG == 1) {
                    if (expand) expand_node_pipe<S>(L, b, c, D, t, child, parent, edge, xseq, sh, lane);
                    write_planes<S>(L, b, c, planes + ((size_t)t * max_leaves + k) * 6 * G::P, lane);
                } else {
                    int n = 0;
                    if (expand) {
                        n = gen_candidates<S>(L, b, c, D, lane);
                        if (lane == 0) xw_store(&xn[xseq], tag_base | (n + 1));
                    }
                    { const long long n = SP_NOW(); sp_a[2] += n - sp_x; sp_x = n; }
                    write_planes<S>(L, b, c, planes + ((size_t)t * max_leaves + k) * 6 * G::P, lane);
                    { const long long n = SP_NOW(); sp_a[3] += n - sp_x; sp_x = n; }
                    if (expand) {
                        unsigned long long ov = 0;
                        bool got = false;
                        for (int spin = 0; spin < kPipeSpinLimit / 16; ++spin) {
                            ov = __hip_atomic_load(&xoff[xseq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if ((unsigned)(ov >> 32) == (unsigned)tag_base) { got = true; break; }
                            if ((spin & 63) == 63 && (xw_load(&D.err[t]) || pipe_load(&sh.err))) break;
                            __builtin_amdgcn_s_sleep(1);
                        }
                        const long long cur = cursor0 + (long long)(unsigned)ov;
                        if (!got || cur + n > D.rng_cap) {
                            if (lane == 0) {
                                if (!got) { if (!xw_load(&D.err[t])) atomicOr(&D.err[t], kErrPipeline | (10 << 8)); }
                                else atomicOr(&D.err[t], kErrRngEmpty);
                                pipe_store(&sh.err, 1);
                            }
                            break;
                        }
                        expand_fill<S>(L, D, t, child, parent, edge, n, cur, lane);
                    }
                }
                wave_sync();
                if (expand) {
                    // the node's arrays reach memory before its "initialised" tag does (a descent of this launch may enter it)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    if (lane == 0) xw_store(&done[k], tag_base | (k + 1));
                }
                { const long long n = SP_NOW(); sp_a[2] += n - sp_x; sp_x = n; }
            }
            if (sp && role == 1 && w == 0) { D.prof[7] += sp_a[0]; D.prof[8] += sp_a[1]; D.prof[9] += sp_a[2]; D.prof[10] += sp_a[3]; }
            if (sp) atomicMax(reinterpret_cast<unsigned long long *>(D.prof + 13), (unsigned long long)SP_NOW());
        }
        __syncthreads();
        if (NWG == 1 && threadIdx.x == 0) set_cursor(D, t, sh.cursor_val);
    }
}

// tree.py:273-315 process_mini_batch for the leaves queued by the preceding kernel.
// Policies (node.py:86-93 update_policy via the {pos: policy} map of tree.py:287-295) are independent per leaf: the
// eight waves of a tree take the leaves round-robin.  Values walk leaf -> root in leaf order, and the float32
// accumulation order is part of the contract - per NODE.  Leaves below different root children touch disjoint nodes,
// so when every leaf carries its recorded path (q_depth > 0: the pipelined selectors) the leaves are shared out by
// root edge: wave w backs up, in leaf order, the leaves whose root edge is w mod 8 - every (node, edge) still sees
// its additions in leaf order.  What all leaves share is the root NODE's float32 value sum: each wave leaves its
// leaves' root-level values in LDS and one lane adds them up in leaf order at the end.  (One wave doing all leaves one
// after the other was 0.12-0.19 ms per 256-leaf mini-batch of a single tree and 0.13 ms per Gumbel phase.)
// Leaves without a recorded path (serial selectors, paths deeper than kPathCap) keep the one-wave walk.
constexpr int kBackupCap = 1024;        // leaves per tree the partitioned walk has LDS for

// NWAVE waves per tree: 8 when the trees crowd the CUs, 16 for a few trees (the leaves per wave are what a launch takes)
// UNIQUE (tg_search_backup with slots_per_tree -1): `leaf_off` is the tree's plane range and leaf k's network outputs are those of
// plane q_src[k] of it - several leaves share one evaluation; leaf order and every accumulation are the same
template <int S, int NWAVE, bool UNIQUE = false>
__global__ __launch_bounds__(64 * NWAVE) void backup_kernel(SearchDev D, const float *policy, const float *value,
                                                     int stride, const int32_t *leaf_off, int use_logit) {
    using G = Geo<S>;
    constexpr int A = G::A, W = G::W, P = G::P;
    constexpr int NTHR = 64 * NWAVE;
    const int t = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    // COMPACT (D.rank): the tree's outputs lie at its rank's rows; a tree without a rank queued nothing, whatever n_leaves
    // holds, and its base is never formed
    const int row_t = D.rank ? D.rank[t] : t;
    const int n = row_t < 0 ? 0 : D.n_leaves[t];
    const size_t leaf_base = leaf_off ? (size_t)leaf_off[t] : (size_t)(row_t < 0 ? 0 : row_t) * stride;
    auto src_of = [&](int k) -> int {              // where leaf k's policy and value lie, from leaf_base
        if constexpr (UNIQUE) return D.q_src[(size_t)t * D.K + k];
        else return k;
    };
    // the root's statistics are touched by every leaf: they live in LDS for the whole launch
    // (256 dependent read-modify-writes through L2 otherwise) and are written back at the end
    __shared__ double r_vsum[A];
    __shared__ int r_vis[A], r_vl[A];
    __shared__ float r_nvsum;
    __shared__ int r_nvis, r_nvl;
    __shared__ uint16_t leaf_edge[kBackupCap];     // root edge of leaf k; | 0x8000 once backed up WITHOUT a parent (nothing for the root)
    __shared__ float rootv[kBackupCap];            // its value at the root's level
    __shared__ uint8_t leaf_neg[kBackupCap];       // leaf k names the reference's node[-1] (q_node < 0)
    const size_t rbase = (size_t)t * D.N * A;                     // root = node 0
#ifdef TG_BACKUP_PROF       // tools/experiments/split_prof.sh: D.prof 2 set-up, 3 policies (slowest wave), 4 values (slowest wave), 5 whole kernel
    const bool bp = D.prof != nullptr && t == 0 && lane == 0;
    const long long bp_t0 = (long long)__builtin_amdgcn_s_memtime();
    __shared__ unsigned long long bp_max[2];
    if (threadIdx.x < 2) bp_max[threadIdx.x] = 0;
#define BP_MARK(i) do { if (bp) atomicMax(&bp_max[i], (unsigned long long)__builtin_amdgcn_s_memtime()); } while (0)
#else
#define BP_MARK(i) do { } while (0)
#endif
    bool part = n > 0 && n <= kBackupCap;
    if (n > 0) {
        for (int i = threadIdx.x; i < A; i += NTHR) {
            r_vsum[i] = D.ch_vsum[rbase + i];
            r_vis[i] = D.ch_visits[rbase + i];
            r_vl[i] = D.ch_vl[rbase + i];
        }
        if (threadIdx.x == 0) {
            r_nvsum = D.node[(size_t)t * D.N].vsum;
            r_nvis = D.node[(size_t)t * D.N].visits;
            r_nvl = D.node[(size_t)t * D.N].vl;
        }
        if (part)
            for (int k = threadIdx.x; k < n; k += NTHR) {
                const size_t slot = (size_t)t * D.K + k;
                leaf_neg[k] = D.q_node[slot] < 0;
                if (D.q_depth[slot] > 0 && D.q_pnode[slot] >= 0) leaf_edge[k] = (uint16_t)path_edge(D.q_path[slot * kPathCap]);
                else part = false;
            }
    }
    part = __syncthreads_and(part) != 0;      // (also: every wave has read the leaf count before anybody resets it)
#ifdef TG_BACKUP_PROF
    const long long bp_t1 = (long long)__builtin_amdgcn_s_memtime();
#endif
    {
        // policies.  Each leaf is a chain of four dependent loads (queue entry, child count, actions, policy values).
        // (Gumbel leaves all name the reference's node[-1], tree.py:412-416: the last pool slot, which has no children
        // unless the pool is full - an error - so nothing is written for them and their order is immaterial.)
        // Four leaves of a wave at a time, every stage of the chain for all four before the next stage: the round
        // trips of the four overlap (one leaf after the other: 32 leaves x 4 round trips = 80 us of a 256-leaf launch).
        // Round 5: all leaves of a wave at once where the registers allow (16 at 9x9, 6 at 19x19 instead of four), and the
        // child count and the actions - both indexed by the node - in ONE stage: three round trips per pass, and a
        // 256-leaf launch of one tree is a single pass (25 -> 8 us).
        constexpr int RP = (A + 63) / 64, U = RP <= 2 ? 16 : 6;
        for (int k0 = wid; k0 < n; k0 += U * NWAVE) {
            int node[U], src[U];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * NWAVE;
                live[u] = k < n;
                node[u] = live[u] ? D.q_node[(size_t)t * D.K + k] : 0;
                src[u] = live[u] ? src_of(k) : 0;
            }
            int nc[U], pos[U][RP];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (node[u] < 0) node[u] = D.N - 1;
                nc[u] = live[u] ? D.node[(size_t)t * D.N + node[u]].children : 0;
#pragma unroll
                for (int r = 0; r < RP; ++r) {
                    const int i = lane + 64 * r;
                    pos[u][r] = live[u] && i < A ? (int)D.action[((size_t)t * D.N + node[u]) * A + i] : -1;
                }
            }
            float pv[U][RP];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float *pol = policy + (leaf_base + (UNIQUE ? src[u] : k0 + u * NWAVE)) * A;
#pragma unroll
                for (int r = 0; r < RP; ++r) {
                    if (lane + 64 * r >= nc[u]) pos[u][r] = -1;
                    const int ps = pos[u][r];
                    pv[u][r] = 0.f;
                    if (ps == 0) {
                        pv[u][r] = pol[P];
                        if (use_logit) pv[u][r] = pv[u][r] - 0.5f;
                    } else if (ps > 0) {
                        pv[u][r] = pol[(ps / W - 1) * S + (ps % W) - 1];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int r = 0; r < RP; ++r)
                    if (pos[u][r] >= 0) D.ch_policy[((size_t)t * D.N + node[u]) * A + lane + 64 * r] = (double)pv[u][r];
        }
    }
    BP_MARK(0);
    if (part) {
        // values, leaves shared out by root edge.  Lane i handles level i of a leaf's recorded path (all loads of all
        // levels are independent: one memory round trip per leaf); the value at level j above the leaf edge is the
        // reference's iterated float32 `value = 1.0 - value`.
        // A wave's leaves are a three-stage pipeline (round 5: one leaf after the other was two dependent round trips each -
        // 60-80 us per 256-leaf launch of one tree, most of whose leaves hang below one root child, i.e. on one wave):
        //   M  queue entry, path and network value of the leaf four places ahead are requested,
        //   S  the statistics of the leaf two places ahead (its metadata has arrived) are requested,
        //   U  the leaf in front is applied and stored.
        // The statistics of stage S were requested BEFORE the two leaves in front of it were applied: a lane that meets the
        // same edge (node) again takes the values it has just computed instead of the loaded ones - a node always sits at
        // the same level, i.e. in the same lane, so the lane's own last two updates are all that can be stale (its older
        // stores precede the loads in program order).  Same additions in the same order on every (node, edge).
        {
            struct Meta { int k, node, depth, entry; float v0, v1, v2; };
            struct Stats { double vs; int cv, cl; float ns; int nv, nl; };
            struct Fwd { long long ekey; int nkey; double vs; int cv, cl; float ns; int nv, nl; };
            int blk = 0;
            unsigned long long todo = 0;
            auto next_k = [&]() -> int {                 // this wave's leaves in leaf order, -1 when there are no more
                while (!todo) {
                    if (blk >= n) return -1;
                    const int kk = blk + lane;
                    todo = __ballot(kk < n && (int)(leaf_edge[kk < n ? kk : 0] % NWAVE) == wid);
                    blk += 64;
                }
                const int k = blk - 64 + __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                return k;
            };
            auto fetch = [&](int k) {
                Meta m;
                m.k = k;
                if (k >= 0) {
                    const size_t slot = (size_t)t * D.K + k;
                    m.node = D.q_node[slot];
                    m.depth = D.q_depth[slot];
                    m.entry = lane < kPathCap ? D.q_path[slot * kPathCap + lane] : 0;
                    const float *val = value + (leaf_base + src_of(k)) * 3;
                    m.v0 = val[0]; m.v1 = val[1]; m.v2 = val[2];
                } else {
                    m.node = 0; m.depth = 0; m.entry = 0; m.v0 = m.v1 = m.v2 = 0.f;
                }
                return m;
            };
            auto request = [&](const Meta &m) {
                Stats st{0.0, 0, 0, 0.f, 0, 0};
                if (m.k >= 0 && lane >= 1 && lane < m.depth) {
                    const size_t cs = (size_t)t * D.N + path_node(m.entry), ce = cs * A + path_edge(m.entry);
                    st.vs = D.ch_vsum[ce]; st.cv = D.ch_visits[ce]; st.cl = D.ch_vl[ce];
                    st.ns = D.node[cs].vsum; st.nv = D.node[cs].visits; st.nl = D.node[cs].vl;
                }
                return st;
            };
            Fwd f1{-1, -1, 0.0, 0, 0, 0.f, 0, 0}, f2 = f1;              // this lane's last and last-but-one update
            Meta m0 = fetch(next_k()), m1 = fetch(next_k()), m2 = fetch(next_k()), m3 = fetch(next_k());
            Stats s0 = request(m0), s1 = request(m1);
            while (m0.k >= 0) {
                const Meta m4 = fetch(next_k());                                    // M
                const Stats s2 = request(m2);                                       // S
                {                                                                   // U
                    const int k = m0.k, depth = m0.depth;
                    // (a Gumbel leaf with q_node < 0 is the reference's node[-1] quirk: every such leaf writes the LAST pool slot's
                    // raw value, the last one in leaf order wins - that one write is done below by wave 0, in leaf order, instead
                    // of by whichever wave comes last here)
                    if (lane == 0 && m0.node >= 0) D.node[(size_t)t * D.N + m0.node].raw = m0.v1 * 0.5f + m0.v2;   // tree.py:299
                    const float vleaf = m0.v0 + m0.v1 * 0.5f;   // tree.py:302
                    Fwd nf{-1, -1, 0.0, 0, 0, 0.f, 0, 0};
                    if (lane < depth) {
                        const int pn = path_node(m0.entry), pe = path_edge(m0.entry);
                        float v = vleaf;
                        for (int q = depth - 1 - lane; q > 0; --q) v = 1.0f - v;
                        const size_t cs = (size_t)t * D.N + pn;
                        const size_t ce = cs * A + pe;
                        if (lane == depth - 1) D.ch_value[ce] = (double)vleaf;   // set_leaf_value
                        if (lane == 0) {                                         // level 0 is the root: LDS copy
                            r_vsum[pe] = (double)((float)r_vsum[pe] + v);
                            r_vis[pe] += 1;
                            r_vl[pe] -= 1;
                            rootv[k] = v;
                        } else {
                            double vs = s0.vs;
                            int cv = s0.cv, cl = s0.cl;
                            float ns_ = s0.ns;
                            int nv = s0.nv, nl = s0.nl;
                            const long long ekey = (long long)ce;
                            if (f1.ekey == ekey) { vs = f1.vs; cv = f1.cv; cl = f1.cl; }
                            else if (f2.ekey == ekey) { vs = f2.vs; cv = f2.cv; cl = f2.cl; }
                            if (f1.nkey == pn) { ns_ = f1.ns; nv = f1.nv; nl = f1.nl; }
                            else if (f2.nkey == pn) { ns_ = f2.ns; nv = f2.nv; nl = f2.nl; }
                            nf.ekey = ekey; nf.nkey = pn;
                            nf.vs = (double)((float)vs + v);                     // float32 accumulation (file header)
                            nf.cv = cv + 1; nf.cl = cl - 1;
                            nf.ns = ns_ + v; nf.nv = nv + 1; nf.nl = nl - 1;
                            D.ch_vsum[ce] = nf.vs;
                            D.ch_visits[ce] = nf.cv;
                            D.ch_vl[ce] = nf.cl;
                            D.node[cs].vsum = nf.ns;
                            D.node[cs].visits = nf.nv;
                            D.node[cs].vl = nf.nl;
                        }
                    }
                    f2 = f1;
                    f1 = nf;
                }
                m0 = m1; m1 = m2; m2 = m3; m3 = m4;
                s0 = s1; s1 = s2;
                wave_sync();
            }
        }
        BP_MARK(1);
        __syncthreads();
        if (wid == 0) {
            // the root node's float32 value sum: every leaf's root-level value, in leaf order
            float acc = r_nvsum;
            for (int k0 = 0; k0 < n; k0 += 64) {
                const float mine = k0 + lane < n ? rootv[k0 + lane] : 0.f;
                const int cnt = min(64, n - k0);
                for (int j = 0; j < cnt; ++j)
                    acc += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), j));
            }
            if (lane == 0) {
                r_nvsum = acc;
                r_nvis += n;
                r_nvl -= n;
            }
            // node[-1]: the last leaf (in leaf order) without a node of its own decides the last slot's raw value
            int last = -1;
            for (int k0 = 0; k0 < n; k0 += 64) {
                const int kk = k0 + lane;
                const unsigned long long m = __ballot(kk < n && leaf_neg[kk < n ? kk : 0] != 0);      // (from the set-up pass: no round trip per 64 leaves here)
                if (m) last = k0 + 63 - __clzll((long long)m);
            }
            if (last >= 0 && lane == 0) {
                const float *val = value + (leaf_base + src_of(last)) * 3;
                D.node[(size_t)t * D.N + D.N - 1].raw = val[1] * 0.5f + val[2];
            }
        }
    } else if (wid == 0 && n > 0) {
        // one wave, all leaves in order.  A leaf whose root->leaf path was recorded by the selector (q_depth > 0) is
        // backed up with ONE memory round trip: lane i handles level i of the path; a node always sits at the same
        // level, i.e. in the same lane, so updates of a node shared by consecutive leaves stay in program order.
        // Other leaves follow the parent pointers in lane 0.  The next leaf's scalars are requested ahead.
        const size_t slot0 = (size_t)t * D.K;
        int node = D.q_node[slot0], cur = D.q_pnode[slot0], e = D.q_pedge[slot0], depth = D.q_depth[slot0];
        int entry = lane < kPathCap ? D.q_path[slot0 * kPathCap + lane] : 0;
        const float *val = value + (leaf_base + src_of(0)) * 3;
        float v0 = val[0], v1 = val[1], v2 = val[2];
        for (int k = 0; k < n; ++k) {
            // request the next leaf's scalars before backing this one up
            const int kn = k + 1 < n ? k + 1 : k;
            const size_t slot_n = (size_t)t * D.K + kn;
            const int node_n = D.q_node[slot_n], cur_n = D.q_pnode[slot_n], e_n = D.q_pedge[slot_n];
            const int depth_n = D.q_depth[slot_n];
            const int entry_n = lane < kPathCap ? D.q_path[slot_n * kPathCap + lane] : 0;
            const float *val_n = value + (leaf_base + src_of(kn)) * 3;
            const float v0_n = val_n[0], v1_n = val_n[1], v2_n = val_n[2];
            if (node < 0) node = D.N - 1;
            if (lane == 0) D.node[(size_t)t * D.N + node].raw = v1 * 0.5f + v2;   // tree.py:299
            if (cur >= 0) {
                const float vleaf = v0 + v1 * 0.5f;   // tree.py:302
                if (depth > 0) {
                    if (lane < depth) {
                        const int pn = path_node(entry), pe = path_edge(entry);
                        float v = vleaf;
                        for (int q = depth - 1 - lane; q > 0; --q) v = 1.0f - v;
                        const size_t cs = (size_t)t * D.N + pn;
                        const size_t ce = cs * A + pe;
                        if (lane == depth - 1) D.ch_value[ce] = (double)vleaf;   // set_leaf_value
                        if (pn == 0) {                                           // root: LDS copy
                            r_vsum[pe] = (double)((float)r_vsum[pe] + v);
                            r_vis[pe] += 1;
                            r_vl[pe] -= 1;
                            r_nvsum += v;
                            r_nvis += 1;
                            r_nvl -= 1;
                        } else {
                            const double vs = D.ch_vsum[ce];
                            const int cv = D.ch_visits[ce], cl = D.ch_vl[ce];
                            const float ns_ = D.node[cs].vsum;
                            const int nv = D.node[cs].visits, nl = D.node[cs].vl;
                            D.ch_vsum[ce] = (double)((float)vs + v);         // float32 accumulation (file header)
                            D.ch_visits[ce] = cv + 1;
                            D.ch_vl[ce] = cl - 1;
                            D.node[cs].vsum = ns_ + v;
                            D.node[cs].visits = nv + 1;
                            D.node[cs].vl = nl - 1;
                        }
                    }
                } else if (lane == 0) {
                    float v = vleaf;
                    D.ch_value[((size_t)t * D.N + cur) * A + e] = (double)v;   // set_leaf_value
                    while (cur > 0) {
                        const size_t cs = (size_t)t * D.N + cur;
                        const size_t ce = cs * A + e;
                        // all loads of a level first (independent, one round trip), then the stores
                        const double vs = D.ch_vsum[ce];
                        const int cv = D.ch_visits[ce], cl = D.ch_vl[ce];
                        const float ns_ = D.node[cs].vsum;
                        const int nv = D.node[cs].visits, nl = D.node[cs].vl;
                        const int pe = D.node[cs].pedge, pn = D.node[cs].parent;
                        D.ch_vsum[ce] = (double)((float)vs + v);
                        D.ch_visits[ce] = cv + 1;
                        D.ch_vl[ce] = cl - 1;
                        D.node[cs].vsum = ns_ + v;
                        D.node[cs].visits = nv + 1;
                        D.node[cs].vl = nl - 1;
                        v = 1.0f - v;
                        e = pe;
                        cur = pn;
                    }
                    if (cur == 0) {                                          // root: LDS copy
                        r_vsum[e] = (double)((float)r_vsum[e] + v);
                        r_vis[e] += 1;
                        r_vl[e] -= 1;
                        r_nvsum += v;
                        r_nvis += 1;
                        r_nvl -= 1;
                    }
                }
                wave_sync();
            }
            node = node_n; cur = cur_n; e = e_n; depth = depth_n; entry = entry_n;
            v0 = v0_n; v1 = v1_n; v2 = v2_n;
        }
    }
    __syncthreads();
    if (n > 0) {
        for (int i = threadIdx.x; i < A; i += NTHR) {
            D.ch_vsum[rbase + i] = r_vsum[i];
            D.ch_visits[rbase + i] = r_vis[i];
            D.ch_vl[rbase + i] = r_vl[i];
        }
        if (threadIdx.x == 0) {
            D.node[(size_t)t * D.N].vsum = r_nvsum;
            D.node[(size_t)t * D.N].visits = r_nvis;
            D.node[(size_t)t * D.N].vl = r_nvl;
        }
    }
    if (threadIdx.x == 0) D.n_leaves[t] = 0;
#ifdef TG_BACKUP_PROF
    if (bp && threadIdx.x == 0) {
        D.prof[2] += bp_t1 - bp_t0;
        D.prof[3] += (long long)bp_max[0] - bp_t1;
        D.prof[4] += (long long)bp_max[1] - (long long)bp_max[0];
        D.prof[5] += (long long)__builtin_amdgcn_s_memtime() - bp_t0;
    }
#endif
}


// numpy's float64 add.reduce order (pairwise_sum in numpy/core/src/umath/loops_utils.h.src):
// < 8 elements sequential; <= 128 elements eight interleaved accumulators combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) then the tail; larger arrays split in halves (multiple
// of 8).  The vector sits in LDS; the result is wave-uniform.  All 64 lanes call it with uniform arguments.
// Accumulator j only ever sees a[j], a[8 + j], a[16 + j], ... in that order, so lane j (< 8) owns it: its up to
// 15 LDS reads are independent and issued together, eight chains of dependent adds run side by side, the combine
// is three DPP steps (fp addition commutes exactly, so the mirrored partners give the same sums).
__device__ double np_sum_block(const double *a, int n) {
    if (n < 8) {
        double r = 0.;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    const int lane = threadIdx.x & 63;
    const int n8 = n - (n % 8);
    const int j = lane & 7;
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = 8 * k + j;
        v[k] = a[i < n8 ? i : j];                     // clamped: never past the vector
    }
    double r = v[0];
#pragma unroll
    for (int k = 1; k < 16; ++k)
        if (8 * k < n8) r += v[k];                    // wave-uniform
    r = r + lane_partner_f64<0>(r);                   // r0 + r1 | r2 + r3 | r4 + r5 | r6 + r7
    r = r + lane_partner_f64<1>(r);                   // (r0 + r1) + (r2 + r3) | (r4 + r5) + (r6 + r7)
    r = r + lane_partner_f64<2>(r);                   // lane i <-> 7 - i inside every group of eight
    double res = read_lane_f64(r, 0);
    for (int i = n8; i < n; ++i) res += a[i];
    return res;
}
__device__ double np_sum(const double *a, int n) {
    if (n <= 128) return np_sum_block(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    const int nr = n - n2;
    // one more level is enough for n <= 512 (A <= 362)
    double left, right;
    if (n2 <= 128) left = np_sum_block(a, n2);
    else { int m = n2 / 2; m -= m % 8; left = np_sum_block(a, m) + np_sum_block(a + m, n2 - m); }
    if (nr <= 128) right = np_sum_block(a + n2, nr);
    else { int m = nr / 2; m -= m % 8; right = np_sum_block(a + n2, m) + np_sum_block(a + n2 + m, nr - m); }
    return left + right;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double ov = __shfl_xor(v, o); v = ov > v ? ov : v; }
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int ov = __shfl_xor(v, o); v = ov > v ? ov : v; }
    return v;
}

// node.py:324-346 select_move_by_sequential_halving_for_root
template <int S>
__device__ int select_root_halving(const SearchDev &D, int t, int node, int count_threshold, int lane) {
    constexpr int A = Geo<S>::A;
    constexpr int R = (A + 63) / 64;
    const size_t ns = (size_t)t * D.N + node;
    const size_t base = ns * A;
    // one memory round trip: every lane requests its slots of all five arrays up front
    int vis[R], vl[R];
    double vsum[R], logit[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        const int ii = i < A ? i : A - 1;
        vis[r] = D.ch_visits[base + ii];
        vl[r] = D.ch_vl[base + ii];
        vsum[r] = D.ch_vsum[base + ii];
        logit[r] = D.ch_policy[base + ii] + D.noise[(size_t)t * A + ii];
    }
    const int nc = D.node[ns].children;
    int mx = 0;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (lane + 64 * r < nc) mx = max(mx, vis[r]);
    mx = wave_max_i32(mx);
    const double sigma = (double)(50 + mx) * 1.0;                   // (C_VISIT + max) * C_SCALE
    double best = 0.0;
    int best_i = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        if (i < nc) {
            const int v = vis[r];
            const int cnt = v + vl[r];
            const double q = v > 0 ? vsum[r] / (double)v : 0.0;
            const double sc = cnt >= count_threshold ? -10000.0 : logit[r] + sigma * q;
            if (best_i < 0 || sc > best) { best = sc; best_i = i; }
        }
    }
    best_i = wave_argmax_first(best, best_i);
    return best_i;
}

// node.py:281-321 calculate_completed_q_value(use_mixed_value=True) + calculate_improved_policy of one node, short of the last
// division: afterwards L.w1[i] = exp(logit_i + sigma * completed_q_i - max) for the node's children and the return value is
// their np.sum, so child i's improved policy is L.w1[i] / sum.  vis[r] = children_visits of child lane + 64 r; nc / nv = the
// node's num_children / node_visits.  One wave; uses L.w1, L.w2.  (The one copy of this arithmetic: select_node_halving
// scores with it, improved_policy_kernel writes it out.)
template <int S, typename Scratch>
__device__ __forceinline__ double improved_policy_weights(Scratch &L, const SearchDev &D, int t, int node, int lane,
                                                          int (&vis)[(Geo<S>::A + 63) / 64], int &nc_out, int &nv_out) {
    constexpr int A = Geo<S>::A;
    constexpr int R = (A + 63) / 64;
    const size_t ns = (size_t)t * D.N + node;
    const size_t base = ns * A;
    const int nc = D.node[ns].children;
    const int nv = D.node[ns].visits;
    const double raw = (double)D.node[ns].raw;
    double logit[R], q[R];
    double mx = -INFINITY;
    int maxv = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        logit[r] = 0.0; q[r] = 0.0; vis[r] = 0;
        if (i < nc) {
            logit[r] = D.ch_policy[base + i];
            vis[r] = D.ch_visits[base + i];
            q[r] = vis[r] > 0 ? D.ch_vsum[base + i] / (double)vis[r] : 0.0;
            mx = logit[r] > mx ? logit[r] : mx;
            maxv = max(maxv, vis[r]);
        }
    }
    maxv = wave_max_i32(maxv);
    double mixed;
    if (nv == 0 && maxv == 0) {
        // A node nobody has been below (every node a phase creates, when its first descent arrives): all q are 0, so
        // v_pi is a sum of zeros and mixed = (raw + (0 * 0) / sum_prob) / (0 + 1) = raw bit for bit - the prior's softmax
        // (an exp pass, three pairwise sums, a division pass) is not needed to know that.
        mixed = raw;
    } else {
        mx = wave_max_f64(mx);
        wave_sync();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            if (i < nc) L.w1[i] = exp(logit[r] - mx);
        }
        wave_sync();
        const double s1 = np_sum(L.w1, nc);
        wave_sync();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            if (i < nc) {
                const double pi = L.w1[i] / s1;
                L.w1[i] = pi;
                L.w2[i] = pi * q[r];
            }
        }
        wave_sync();
        const double sum_prob = np_sum(L.w1, nc);
        const double v_pi = np_sum(L.w2, nc);
        mixed = (raw + ((double)nv * v_pi) / sum_prob) / ((double)nv + 1.0);
    }
    const double sigma = (double)(50 + maxv) * 1.0;
    double il[R];
    double mx2 = -INFINITY;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        il[r] = 0.0;
        if (i < nc) {
            il[r] = logit[r] + sigma * (vis[r] > 0 ? q[r] : mixed);
            mx2 = il[r] > mx2 ? il[r] : mx2;
        }
    }
    mx2 = wave_max_f64(mx2);
    wave_sync();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        if (i < nc) L.w1[i] = exp(il[r] - mx2);
    }
    wave_sync();
    nc_out = nc;
    nv_out = nv;
    return np_sum(L.w1, nc);
}

// node.py:349-361 select_move_by_sequential_halving_for_node
template <int S, typename Scratch>
__device__ int select_node_halving(Scratch &L, const SearchDev &D, int t, int node, int lane) {   // uses L.w1, L.w2
    constexpr int R = (Geo<S>::A + 63) / 64;
    int vis[R], nc, nv;
    const double s2 = improved_policy_weights<S>(L, D, t, node, lane, vis, nc, nv);
    double best = 0.0;
    int best_i = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        if (i < nc) {
            const double sc = L.w1[i] / s2 - ((double)vis[r] / (1.0 + (double)nv));
            if (best_i < 0 || sc > best) { best = sc; best_i = i; }
        }
    }
    wave_sync();
    best_i = wave_argmax_first(best, best_i);
    return best_i;
}

// ---- Gumbel / sequential-halving selection: one workgroup per tree, a selector wave + NW workers -----------
// (root: node.py:324-346, below: :349-361).  Two modes inside one kernel:
//  * the usual one (round 6; `la_*` below): the selector ranks the root and works out which root children the phase enters
//    ("entries") and which descents repeat them; every wave walks its share of the entries; the selector numbers the new nodes;
//    a worker takes whole entries - expansion, the step into the new node, the leaf - off one board replay; the repeats of all
//    entries are shared out over the workers;
//  * one by one, through the job ring of select_puct_pipe_kernel (any path longer than the per-entry buffers, or the test hook
//    SearchDev::gumbel_one_by_one): the selector walks and queues LEAF (replay the path, write the planes of leaf `plane_slot`)
//    and EXPAND jobs (replay, expand the child it is about to enter - it then waits for exactly that job, because it continues
//    INTO the new node), the workers share the repeats out afterwards as plane copies.
// 9x9 (2 / 6 / 10 workers), 13x13 (2 / 6) and 19x19 (2 / 4: a worker's board is 19 KB there).
// UNIQUE (tg_search_select_gumbel with slots_per_tree -1): the network evaluates each distinct leaf once.  `leaf_off[t]` is the
// start of tree t's plane range of min(width * levels, kUniqueE) slots; entry f's planes go to slot f of it, repeats write no
// planes at all, the slots behind the last entry get a copy of entry 0's planes (the forward pass covers the whole range), and
// every leaf slot q - queue entry, path and virtual losses as ever - also gets q_src[q] = the entry whose plane holds its
// position.  More entries than the range holds: the tree's error flag, nothing written past the range.
template <int S>
struct HalvingScratch {
    double w1[Geo<S>::A + 7];
    double w2[Geo<S>::A + 7];
};

template <int S, int NW, bool UNIQUE = false>
__global__ __launch_bounds__(64 * (1 + NW)) void select_gumbel_pipe_kernel(SearchDev D, const int32_t *num_considered,
                                                                 const int32_t *max_count, int stride,
                                                                 const int32_t *leaf_off, float *planes) {
    using G = Geo<S>;
    constexpr int A = G::A;
    constexpr int kPipeSlots = PipeShared<S, NW>::kSlots;      // (shadows the three-wave kernels' ring size)
    constexpr int NTHR = 64 * (1 + NW);
    __shared__ PipeShared<S, NW> sh;
    __shared__ HalvingScratch<S> hs;
    __shared__ int16_t sel_moves[kPathMax<S>];
    __shared__ int sel_path[kPathMax<S>];
    // Leaves by root child.  ~100 descents of a phase go to 2..16 root children and all descents through one root
    // child end on the same leaf (nothing moves within a phase).  The root choices of the whole phase are simulated up
    // front (ballots on a copy of the counters): a root child's FIRST descent gets an entry f (rm_pos = its root child,
    // rm_slot = its leaf slot), every later descent only `sched[leaf slot] = f`.  Only the first descents are walked
    // (rm_* completed: leaf, path); the scheduled leaves are shared out among the workers - queue entry, path, planes written
    // from the entry's position code in LDS (one-by-one mode: when the ring has drained, virtual losses per leaf, planes copied
    // from the first leaf's slot) - no per-leaf work of the selector, which was the slowest wave of a phase (2.2 k cycles per
    // repeated descent, 87 of 100).
    constexpr int kRootMemo = 24, kRootPath = 32;        // (a phase enters at most 16 + 1 root children)
    __shared__ int rm_pos[kRootMemo], rm_parent[kRootMemo], rm_edge[kRootMemo], rm_child[kRootMemo], rm_job[kRootMemo],
        rm_slot[kRootMemo], rm_depth[kRootMemo];
    __shared__ int rm_path[kRootMemo][kRootPath];
    __shared__ int8_t sched[kPipeMaxK / 2];
    __shared__ int bulk_n;
    // The look-ahead walks (below: "Expansions first") of a phase's root children are independent of each other - disjoint
    // subtrees, statistics that do not move - and the workers have nothing to do until the first job is queued: every wave of
    // the workgroup walks its share (entry f on wave f mod (1 + NW), its own softmax scratch), the selector then hands out node
    // numbers, draws and jobs in entry order as before.  (The walks were 112 k of the selector's 194 k cycles per phase.)
    __shared__ HalvingScratch<S> hsw[NW];
    __shared__ int la_ready, la_done, la_n;
    __shared__ int la_mv[kRootMemo], la_vis[kRootMemo], la_child[kRootMemo], la_e[kRootMemo];       // entry f at the root
    __shared__ int la_res[kRootMemo], la_node[kRootMemo], la_edge[kRootMemo], la_chd[kRootMemo], la_depth[kRootMemo];   // where its walk ended
    __shared__ int16_t la_moves[kRootMemo][kRootPath];
    // ... and the first descents themselves are the workers' too: entry f - its expansion (node number and place in the draw
    // order given by the selector), the step into the node just made, the leaf's queue entry, virtual losses and planes - is one
    // piece of work on one board replay, entry f on worker f mod NW; the selector queues nothing.  (One by one through the job
    // ring - EXPAND job, wait, step, LEAF job - the first descents were 60 k of the selector's 123 k cycles per phase.)
    __shared__ int la_go, la_fast, la_ndesc, la_xseq[kRootMemo];
    // an entry's leaf position for its repeats, one byte per point (colour as the side to move sees it | 4: the previous move) +
    // (pass plane, side): the repeats are shared out over ALL workers once their entry's leaf stands (the best root child's ~50
    // repeats of a late phase were one worker's: 25 k of its 46 k cycles)
    __shared__ uint8_t ent_code[kRootMemo][(G::P + 3) & ~3];
    __shared__ int ent_meta[kRootMemo], ent_done[kRootMemo];
    constexpr int kWalkLeaf = 1, kWalkExpand = 2, kWalkDeep = 3, kWalkPoolFull = 4;
    const int t = blockIdx.x;
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const RootMeta meta = D.meta[t];
    const int n0 = meta.num_nodes;
    if (threadIdx.x < kPipeSlots) {
        sh.job_seq[threadIdx.x] = 0;
        sh.slot_done[threadIdx.x] = 0;
    }
    for (int i = threadIdx.x; i < kPipeMaxK / 32; i += NTHR) sh.done_bits[i] = 0u;
    if (threadIdx.x < kRootMemo) ent_done[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        la_ready = 0; la_done = 0; la_n = 0; la_go = 0; la_fast = 0;
        sh.cursor_seq = 0;
        sh.cursor_val = D.rng_cursor[t];
        sh.final_count = -1;
        sh.err = 0;
    }
    __syncthreads();
    const int width = num_considered[t], levels = max_count[t];
    const size_t leaf_base = leaf_off ? (size_t)leaf_off[t] : (size_t)t * stride;
    const bool active = D.err[t] == 0 && n0 > 0 && width * levels <= stride;
    const int ucap = min(width * levels, kUniqueE);      // (UNIQUE: this tree's plane slots)
    int num_nodes = n0;
    int queued = 0;

    // s_memtime accumulators of tree 0's selector (tg_search_profile; tools/profile_gumbel.py): 0 set-up (root into
    // registers, ranking), 1 the phase's root choices, 8 nodes and EXPAND jobs handed out, 7 this wave's share of the entries'
    // walks, 3 waiting for the other waves' shares, 2 first descents, 4 waiting for a free job slot (inside 1..2), 5 write-back,
    // 6 first descents (count)
    const bool prof = D.prof && t == 0;
    const long long t_begin = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
    long long tp = t_begin, pc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto lap = [&](int i) {
        if (prof) { const long long now = (long long)__builtin_amdgcn_s_memtime(); pc[i] += now - tp; tp = now; }
    };
    // entry f's walk from its root child down to where the first descent will end - a leaf, or the point of expansion - without
    // side effects; paths longer than the per-entry buffers are left to the selector's one-by-one code (kWalkDeep)
    auto walk = [&](int f, HalvingScratch<S> &scratch) {
        int node = 0, depth = 0, res = kWalkDeep;
        int mv = la_mv[f], visits = la_vis[f], child = la_child[f], e = la_e[f];
        while (depth < (D.gumbel_one_by_one ? 0 : kRootPath - 2)) {
            if (lane == 0) { la_moves[f][depth] = (int16_t)mv; rm_path[f][depth] = path_entry(node, e); }
            ++depth;
            if (visits < 1) { res = kWalkLeaf; break; }
            if (child == kNotExpanded) { res = kWalkExpand; break; }
            if (child >= n0) break;                                       // (created in this launch: cannot happen, subtrees are disjoint)
            node = child;
            e = select_node_halving<S>(scratch, D, t, node, lane);
            const size_t nb = ((size_t)t * D.N + node) * A;
            mv = D.action[nb + e];
            visits = D.ch_visits[nb + e];
            child = D.ch_index[nb + e];
        }
        if (lane == 0) { la_res[f] = res; la_node[f] = node; la_edge[f] = e; la_chd[f] = child; la_depth[f] = depth; }
    };
    if (wid == 0) {
        // ---- selector -------------------------------------------------------------------
        // Within a phase nothing backs values up, so (a) the root's score "logit + noise + sigma q" of every child
        // is a constant - only "visits + virtual loss >= threshold" moves, and the virtual loss is added by this
        // wave: the root lives in registers for the whole launch (loaded once, written back once); (b) below the
        // root the choice (node.py:349-361: completed Q, two softmaxes - the costly part) is a pure function of
        // statistics that do not change: it is computed at a node's first visit and remembered (LDS, by node).
        // Virtual losses below the root are fire-and-forget atomics (nobody reads them before the backup).
        constexpr int R = (A + 63) / 64;
        int jid = 0, nexp = 0;
        bool ok = active;
        double r_score[R];
        int r_cnt[R], r_vis[R], r_idx[R], r_act[R], r_vl0[R];
        int r_nc = 0, r_added = 0;
        if (active) {
            const size_t base = (size_t)t * D.N * A;
            double vsum[R];
            r_nc = D.node[(size_t)t * D.N].children;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = lane + 64 * r, ii = i < A ? i : A - 1;
                r_vis[r] = D.ch_visits[base + ii];
                r_vl0[r] = D.ch_vl[base + ii];
                vsum[r] = D.ch_vsum[base + ii];
                r_score[r] = D.ch_policy[base + ii] + D.noise[(size_t)t * A + ii];
                r_idx[r] = D.ch_index[base + ii];
                r_act[r] = D.action[base + ii];
            }
            int mx = 0;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (lane + 64 * r < r_nc) mx = max(mx, r_vis[r]);
            mx = wave_max_i32(mx);
            const double sigma = (double)(50 + mx) * 1.0;                   // (C_VISIT + max) * C_SCALE
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double q = r_vis[r] > 0 ? vsum[r] / (double)r_vis[r] : 0.0;
                r_score[r] = r_score[r] + sigma * q;
                r_cnt[r] = r_vis[r] + r_vl0[r];
            }
        }
        // The scores are constants of the launch, so "arg-max over the children still under the threshold" is "the
        // first such child in score order": the children are ranked once (score descending, index ascending - the
        // order np.argmax resolves ties in) and every per-child register array is permuted into rank order.  A root
        // choice is then a compare, a ballot and a find-first-bit instead of a float64 arg-max over the wave
        // (1.4 k cycles of the 6.6 k a descent cost the selector).  When no child is under the threshold every
        // score is -10000 and np.argmax returns child 0: pos0 is where that child sits.
        int r_edge[R];
        int pos0 = 0;
        if (active) {
            wave_sync();
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (lane + 64 * r < A) hs.w1[lane + 64 * r] = r_score[r];
            wave_sync();
            int rank[R];
#pragma unroll
            for (int r = 0; r < R; ++r) rank[r] = 0;
            for (int j = 0; j < r_nc; ++j) {
                const double sj = hs.w1[j];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int i = lane + 64 * r;
                    rank[r] += (sj > r_score[r] || (sj == r_score[r] && j < i)) ? 1 : 0;
                }
            }
            __shared__ int ptmp[A + 1];
            auto permute = [&](int (&v)[R]) {
                wave_sync();
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (lane + 64 * r < r_nc) ptmp[rank[r]] = v[r];
                wave_sync();
#pragma unroll
                for (int r = 0; r < R; ++r) v[r] = lane + 64 * r < r_nc ? ptmp[lane + 64 * r] : 0;
            };
#pragma unroll
            for (int r = 0; r < R; ++r) r_edge[r] = lane + 64 * r;
            permute(r_edge);
            permute(r_cnt);
            permute(r_vis);
            permute(r_idx);
            permute(r_act);
            // rank of child 0
            wave_sync();
            if (lane == 0) ptmp[A] = rank[0];
            wave_sync();
            pos0 = ptmp[A];
        }
        // remembered choices below the root: tag = node, value = (edge, move, visits of the edge, child)
        constexpr int kMemo = 64;
        __shared__ int memo_tag[kMemo], memo_edge[kMemo], memo_move[kMemo], memo_vis[kMemo], memo_child[kMemo];
        for (int i = lane; i < kMemo; i += 64) memo_tag[i] = -1;
        // (leaves by root child: rm_* / sched above.  The network still evaluates every queued leaf.)
        int n_first = 0, n_desc = 0, n_iter = 0;             // entries so far; descents so far; threshold levels walked one by one
        wave_sync();
        auto publish = [&](int plane_slot, int parent, int edge, int child, int expand, int xseq, int depth, int src,
                           const int *path_src = nullptr, const int16_t *moves_src = nullptr) -> bool {
            if (jid >= kPipeMaxK) return false;
            const int slot = jid % kPipeSlots;
            const long long w0 = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
            if (!pipe_wait_ge(&sh.slot_done[slot], jid / kPipeSlots)) return false;
            if (prof) pc[4] += (long long)__builtin_amdgcn_s_memtime() - w0;
            if (path_src && moves_src) {                         // an entry's recorded walk
                for (int i = lane; i < depth; i += 64) { sh.moves[slot][i] = moves_src[i]; sh.paths[slot][i] = path_src[i]; }
            } else if (path_src) {                               // COPY job: the worker needs the path only
                for (int i = lane; i < depth; i += 64) sh.paths[slot][i] = path_src[i];
            } else {
                for (int i = lane; i < depth; i += 64) { sh.moves[slot][i] = sel_moves[i]; sh.paths[slot][i] = sel_path[i]; }
            }
            wave_sync();
            if (lane == 0) {
                PipeJob &j = sh.job[slot];
                j.k = plane_slot; j.parent = parent; j.edge = edge; j.child = child;
                j.expand = expand; j.xseq = xseq; j.depth = depth; j.src = src;
                pipe_store(&sh.job_seq[slot], jid + 1);
            }
            wave_sync();
            ++jid;
            return true;
        };
        // Expansions first.  Every root child is entered several times in a phase, and only its FIRST descent can meet
        // a node that has to be expanded (the later ones find it there; the new node's children are unvisited, so
        // the descent ends right below it).  Waiting for each of those expansions in turn (replay + candidates +
        // prior: ~5 us) was a third of a launch.  So the root choices of the phase are simulated on a copy of the
        // counters (ballots: cheap), and each root child, at its first appearance, is walked down WITHOUT side
        // effects to the point of expansion: the node is allocated and its EXPAND job queued - node numbers and
        // draws in descent order, exactly as before - and nobody waits.  The descents proper then find the children
        // allocated and wait, if at all, for a job that is about to finish.  Subtrees of different root children are
        // disjoint and statistics are constant within a phase, so every choice is what the one-by-one order makes.
        lap(0);
        // ---- the root choices of the phase, simulated on a copy of the counters: entries (first appearances) and the schedule ----
        // A choice is "the first child in rank order whose count is under the threshold, child 0 if there is none" and adds one to
        // that child's count: a threshold level hands its `width` descents out greedily in rank order - child i takes
        // min(th - count_i, what is left), whatever remains goes to child 0 - so a level is a prefix sum over the wave, not
        // `width` ballots in a row (one by one: 58 k of the selector's 156 k cycles per phase).
        if (ok) {
            int s_cnt[R], f_of[R];
#pragma unroll
            for (int r = 0; r < R; ++r) { s_cnt[r] = r_cnt[r]; f_of[r] = -1; }
            const int owner0 = pos0 & 63, rr0 = pos0 >> 6;
            for (int th = 1; ok && th <= levels; ++th) {
                const int qbase = n_desc;
                ++n_iter;
                int need[R], pre[R], take[R];
                int running = 0;
                bool multi = false;                                       // a child more than one descent under the threshold
                const unsigned long long below = (1ull << lane) - 1ull;
                int under_before = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    need[r] = (lane + 64 * r < r_nc && s_cnt[r] < th) ? th - s_cnt[r] : 0;
                    // (every child under the threshold takes at least one descent: only the first `width` of them can take any -
                    // the never-visited children further down the ranking, `th` under it, stay out of the sums)
                    const unsigned long long under = __ballot(need[r] > 0);
                    if (under_before + __popcll(under & below) >= width) need[r] = 0;
                    under_before += __popcll(under);
                    multi = multi || __ballot(need[r] > 1) != 0ull;
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (!multi) {                                         // (the usual level: the prefix sum is a bit count)
                        const unsigned long long m = __ballot(need[r] == 1);
                        pre[r] = running + __popcll(m & below);
                        running += __popcll(m);
                    } else {
                        const int incl = wave_scan_add_i32(need[r]);
                        pre[r] = running + incl - need[r];
                        running += __builtin_amdgcn_readlane(incl, 63);
                    }
                }
                const int given = running < width ? running : width;
                const int leftover = width - given;                       // descents that find no child under the threshold: child 0
                int max_take = 0;
                unsigned long long fresh[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int room = width - pre[r];
                    take[r] = room <= 0 ? 0 : (need[r] < room ? need[r] : room);
                    s_cnt[r] += take[r];
                    max_take = max(max_take, take[r]);
                    fresh[r] = __ballot(take[r] > 0 && f_of[r] < 0);
                }
                max_take = multi ? wave_max_i32(max_take) : (given > 0 ? 1 : 0);
                // entries: the children that appear for the first time, in the order of their first descents
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const bool mine = take[r] > 0 && f_of[r] < 0;
                    if (mine) f_of[r] = n_first + __popcll(fresh[r] & below);
                    n_first += __popcll(fresh[r]);
                    if (mine && f_of[r] < kRootMemo) {
                        const int f = f_of[r];
                        rm_pos[f] = lane + 64 * r; rm_slot[f] = qbase + pre[r];
                        la_mv[f] = r_act[r]; la_vis[f] = r_vis[r]; la_child[f] = r_idx[r]; la_e[f] = r_edge[r];
                    }
                }
                if (leftover > 0) {
                    int f0 = -1;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (r == rr0) f0 = __builtin_amdgcn_readlane(f_of[r], owner0);
                    const bool fresh0 = f0 < 0;
                    if (fresh0) f0 = n_first++;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (r == rr0 && lane == owner0) {
                            s_cnt[r] += leftover;
                            f_of[r] = f0;
                            if (fresh0 && f0 < kRootMemo) {
                                rm_pos[f0] = pos0; rm_slot[f0] = qbase + given;
                                la_mv[f0] = r_act[r]; la_vis[f0] = r_vis[r]; la_child[f0] = r_idx[r]; la_e[f0] = r_edge[r];
                            }
                        }
                    for (int k = lane; k < leftover; k += 64) sched[qbase + given + k] = (int8_t)((fresh0 && k == 0) ? -1 : f0);
                }
                if (n_first > (UNIQUE ? kUniqueE : kRootMemo)) { ok = false; break; }   // (never: <= 17 root children per phase)
                // the schedule: descent q repeats the leaf of entry sched[q] (-1: it IS the entry's first descent)
                for (int k = 0; k < max_take; ++k)
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (k < take[r]) sched[qbase + pre[r] + k] = (int8_t)((k == 0 && ((fresh[r] >> lane) & 1ull)) ? -1 : f_of[r]);
                n_desc += width;
                // Steady state: `width` children stand exactly at the threshold and nothing ranked before the last of them can
                // come under a later one - every remaining level gives each of them one descent, in the same order.
                if (leftover == 0 && th < levels) {
                    unsigned long long tk[R];
                    int last = -1, ntk = 0;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        tk[r] = __ballot(take[r] > 0);
                        if (tk[r]) last = 64 * r + 63 - __clzll((long long)tk[r]);
                        ntk += __popcll(tk[r]);
                    }
                    bool steady = ntk == width;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int i = lane + 64 * r;
                        const bool fine = i > last || i >= r_nc || (take[r] > 0 ? s_cnt[r] == th : s_cnt[r] >= levels);
                        steady = steady && __ballot(!fine) == 0ull;
                    }
                    if (steady) {
                        const int rem = levels - th;
                        int before = 0;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            if (take[r] > 0) {
                                const int ord = before + __popcll(tk[r] & below);
                                for (int l = 0; l < rem; ++l) sched[n_desc + l * width + ord] = (int8_t)f_of[r];
                                s_cnt[r] += rem;
                            }
                            before += __popcll(tk[r]);
                        }
                        n_desc += rem * width;
                        break;
                    }
                }
            }
            // every descent adds one virtual loss to its root child (node.py:76-83): the simulated counters are the final ones
#pragma unroll
            for (int r = 0; r < R; ++r) r_cnt[r] = s_cnt[r];
            r_added = n_desc;
        }
        wave_sync();
        lap(1);
        // ---- the entries' walks, shared out over the workgroup's waves (this one takes its share) ----
        if (active) {
            const int n_walk = ok ? n_first : 0;
            if (lane == 0) { la_n = n_walk; pipe_store(&la_ready, 1); }
            for (int f = 0; f < n_walk; f += 1 + NW) walk(f, hs);
            wave_sync();
            if (lane == 0) __hip_atomic_fetch_add(&la_done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            lap(7);
            if (!pipe_wait_ge(&la_done, 1 + NW)) ok = false;
        }
        lap(3);
        // (a path longer than the per-entry buffers anywhere in the phase: every entry goes the one-by-one way through the job
        // ring - expansions of both kinds in one phase would wait for each other's place in the draw order across the two queues)
        bool fast = ok;
        if (ok) {
            if (__ballot(lane < n_first && la_res[lane] == kWalkDeep)) {
                fast = false;
                if (lane < n_first) la_res[lane] = kWalkDeep;
                wave_sync();
            }
        }
        // One entry, one by one (paths longer than the per-entry buffers): walked down WITHOUT side effects to the point of
        // expansion, the node allocated and its EXPAND job queued.
        auto lookahead_serial = [&](int f) {
            const int pos = rm_pos[f];
            const int owner = pos & 63, rr = pos >> 6;
            int node = 0, depth = 0;
            int mv = la_mv[f], visits = la_vis[f], child = la_child[f], e = la_e[f];
            while (ok) {
                if (depth >= kPathMax<S>) break;                  // the descent proper reports it
                if (lane == 0) { sel_moves[depth] = (int16_t)mv; sel_path[depth] = path_entry(node, e); }
                ++depth;
                wave_sync();
                if (visits < 1) break;                            // ends on a leaf: nothing to expand
                if (child == kNotExpanded) {
                    if (num_nodes >= D.N || num_nodes - n0 >= kPipeMaxK) break;   // reported by the descent proper
                    child = num_nodes++;
                    if (node == 0) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
                            if (r == rr && lane == owner) r_idx[r] = child;
                    } else if (lane == 0) {
                        memo_child[node & (kMemo - 1)] = child;
                    }
                    if (lane == 0) {
                        D.ch_index[((size_t)t * D.N + node) * A + e] = child;
                        sh.jobof[child - n0] = (int16_t)jid;
                    }
                    wave_sync();
                    ok = publish(-1, node, e, child, 1, nexp++, depth, -1);
                    break;                                        // its children are unvisited: a leaf follows
                }
                node = child;
                if (node >= n0) break;                            // (created in this launch: cannot happen, subtrees are disjoint)
                const int slot = node & (kMemo - 1);
                if (memo_tag[slot] != node) {
                    e = select_node_halving<S>(hs, D, t, node, lane);
                    const size_t nb = ((size_t)t * D.N + node) * A;
                    mv = D.action[nb + e];
                    visits = D.ch_visits[nb + e];
                    child = D.ch_index[nb + e];
                    wave_sync();
                    if (lane == 0) {
                        memo_tag[slot] = node; memo_edge[slot] = e; memo_move[slot] = mv;
                        memo_vis[slot] = visits; memo_child[slot] = child;
                    }
                    wave_sync();
                } else {
                    e = memo_edge[slot]; mv = memo_move[slot]; visits = memo_vis[slot]; child = memo_child[slot];
                }
            }
        };
        // Expansions first.  Every root child is entered several times in a phase, and only its FIRST descent can meet
        // a node that has to be expanded (the later ones find it there; the new node's children are unvisited, so
        // the descent ends right below it).  Waiting for each of those expansions in turn (replay + candidates +
        // prior: ~5 us) was a third of a launch.  So every entry has been walked down to its point of expansion (above):
        // here the nodes are allocated and the EXPAND jobs queued - node numbers and draws in descent order, exactly as the
        // one-by-one order makes them - and nobody waits.  The descents proper then find the children allocated and wait, if
        // at all, for a job that is about to finish.  Subtrees of different root children are disjoint and statistics are
        // constant within a phase, so every choice is what the one-by-one order makes.
        if (active && !fast && lane == 0) { la_fast = 0; pipe_store(&la_go, 1); }      // (the workers: straight to the job ring)
        if (!fast) {
            for (int f = 0; ok && f < n_first; ++f) lookahead_serial(f);
        } else {
            // lane f: entry f.  Node numbers and places in the draw order go to the entries that expand, in entry order; when
            // the pool runs out the rest are marked (reported where the one-by-one order reports them).
            const int res = lane < n_first ? la_res[lane] : 0;
            const unsigned long long xm = __ballot(res == kWalkExpand);
            const int ord = __popcll(xm & ((1ull << lane) - 1ull));
            const int room_pool = D.N - num_nodes, room_launch = kPipeMaxK - (num_nodes - n0);
            const int room = max(0, min(room_pool, room_launch));
            if (res == kWalkExpand) {
                if (ord >= room) {
                    la_res[lane] = kWalkPoolFull;
                } else {
                    const int child = num_nodes + ord;
                    la_chd[lane] = child;
                    la_xseq[lane] = nexp + ord;
                    D.ch_index[((size_t)t * D.N + la_node[lane]) * A + la_edge[lane]] = child;
                }
            }
            const int granted = min(__popcll(xm), room);
            num_nodes += granted;
            nexp += granted;
        }
        wave_sync();
        if (active && fast && lane == 0) { la_fast = ok ? 1 : 0; la_ndesc = n_desc; pipe_store(&la_go, 1); }
        lap(8);
        // One entry's first descent, one by one (see lookahead_serial).
        auto descend_serial = [&](int f) {
            {
                const int my_q = rm_slot[f];
                int node = 0, depth = 0, root_pos = 0;
                while (ok) {
                    const size_t ns = (size_t)t * D.N + node;
                    const size_t base = ns * A;
                    int e, mv, visits, child;
                    if (node == 0) {
                        // node.py:324-346: the root child this entry was made for (rank-ordered register copy)
                        const int pos = rm_pos[f];
                        const int owner = pos & 63, rr = pos >> 6;
                        int m_mv = 0, m_vis = 0, m_idx = 0, m_e = 0;
#pragma unroll
                        for (int r = 0; r < R; ++r)
                            if (r == rr) { m_mv = r_act[r]; m_vis = r_vis[r]; m_idx = r_idx[r]; m_e = r_edge[r]; }
                        mv = __builtin_amdgcn_readlane(m_mv, owner);
                        visits = __builtin_amdgcn_readlane(m_vis, owner);
                        child = __builtin_amdgcn_readlane(m_idx, owner);
                        e = __builtin_amdgcn_readlane(m_e, owner);
                        root_pos = pos;
                    } else {
                        const int slot = node & (kMemo - 1);
                        if (memo_tag[slot] == node) {
                            e = memo_edge[slot]; mv = memo_move[slot]; visits = memo_vis[slot]; child = memo_child[slot];
                        } else {
                            if (node >= n0) ok = pipe_wait_done(sh, sh.jobof[node - n0]);   // expansion in flight?
                            if (!ok) break;
                            e = select_node_halving<S>(hs, D, t, node, lane);
                            mv = D.action[base + e];
                            visits = D.ch_visits[base + e];
                            child = D.ch_index[base + e];
                            wave_sync();
                            if (lane == 0) {
                                memo_tag[slot] = node; memo_edge[slot] = e; memo_move[slot] = mv;
                                memo_vis[slot] = visits; memo_child[slot] = child;
                            }
                            wave_sync();
                        }
                        // (node.py:76-83: the virtual losses below the root are added by the worker that takes the leaf
                        // job - nobody reads them before the backup)
                    }
                    if (depth >= kPathMax<S>) { ok = false; break; }
                    if (lane == 0) {
                        sel_moves[depth] = (int16_t)mv;
                        sel_path[depth] = path_entry(node, e);
                    }
                    ++depth;
                    wave_sync();
                    if (visits < 1) {                                     // tree.py:412-416
                        // the queue entry of this leaf (node to evaluate - still NOT_EXPANDED: node[-1] -, parent, edge,
                        // path) is written by the worker that takes the job
                        const int leaf_jid = jid;
                        if (depth <= kRootPath) {
                            // the later descents through this root child: left to the workers (sched)
                            if (lane == 0) { rm_parent[f] = node; rm_edge[f] = e; rm_child[f] = child; rm_job[f] = leaf_jid; rm_depth[f] = depth; }
                            if (lane < depth) rm_path[f][lane] = sel_path[lane];
                            wave_sync();
                            ok = publish(my_q, node, e, child, 0, 0, depth, UNIQUE ? f : -1);
                        } else {
                            // a path too long for rm_path: the later descents become COPY jobs here (planes of this leaf's slot;
                            // UNIQUE: no planes, the job names the entry)
                            if (UNIQUE && lane == 0) rm_job[f] = leaf_jid;
                            ok = publish(my_q, node, e, child, 0, 0, depth, UNIQUE ? f : -1);
                            for (int qq = 0; ok && qq < n_desc; ++qq)
                                if (sched[qq] == f) {
                                    ok = publish(qq, node, e, child, 2, leaf_jid, depth, UNIQUE ? f : my_q);
                                    if (lane == 0) sched[qq] = (int8_t)-1;
                                }
                            wave_sync();
                        }
                        lap(2);
                        if (prof) pc[6] += 1;
                        break;
                    }
                    if (child == kNotExpanded) {                          // tree.py:418-420
                        if (num_nodes >= D.N || num_nodes - n0 >= kPipeMaxK) {
                            if (lane == 0) atomicOr(&D.err[t], kErrPoolFull);
                            ok = false;
                            break;
                        }
                        child = num_nodes++;
                        if (node == 0) {
                            const int owner = root_pos & 63, rr = root_pos >> 6;
#pragma unroll
                            for (int r = 0; r < R; ++r)
                                if (r == rr && lane == owner) r_idx[r] = child;
                        } else if (lane == 0) {
                            memo_child[node & (kMemo - 1)] = child;
                        }
                        if (lane == 0) {
                            D.ch_index[base + e] = child;
                            sh.jobof[child - n0] = (int16_t)jid;
                        }
                        wave_sync();
                        ok = publish(-1, node, e, child, 1, nexp++, depth, -1);
                        if (!ok) break;
                    }
                    node = child;
                }
            }
        };
        // the first descents: the workers' (see la_go) - here only what the one-by-one order reports at this point, and the
        // one-by-one descents of a phase with a long path
        for (int f = 0; ok && f < n_first; ++f) {
            if (pipe_load(&sh.err)) { ok = false; break; }
            const int res = la_res[f];
            if (res == kWalkDeep) { descend_serial(f); continue; }
            if (res == kWalkPoolFull) {                                   // tree.py:418-420
                if (lane == 0) atomicOr(&D.err[t], kErrPoolFull);
                ok = false;
                break;
            }
            if (prof) pc[6] += 1;
        }
        lap(2);
        if (active) {
            // the root's virtual losses back to the pool
            const size_t base = (size_t)t * D.N * A;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = lane + 64 * r;
                if (i < r_nc) D.ch_vl[base + r_edge[r]] = r_cnt[r] - r_vis[r];       // rank order -> child index
            }
            if (lane == 0) D.node[(size_t)t * D.N].vl += r_added;
        }
        if (active && !ok && lane == 0) {
            if (!(D.err[t] & (kErrPoolFull | kErrRngEmpty))) atomicOr(&D.err[t], kErrPipeline);
            pipe_store(&sh.err, 1);
        }
        if (ok) queued = n_desc;                           // every descent has queued one leaf
        if (lane == 0) {
            bulk_n = ok ? queued : 0;
            pipe_store(&sh.final_count, jid);
        }
        lap(5);
        if (prof && lane == 0) {
            for (int i = 0; i < 9; ++i) D.prof[i] += pc[i];
            D.prof[12] += 1; D.prof[14] += n_iter;
            D.prof[15] += (long long)__builtin_amdgcn_s_memtime() - t_begin;
        }
    } else {
        // ---- workers ---------------------------------------------------------------------
        Lds<S, false> &L = sh.board[wid - 1];
        BoardScalars rootb;
        int root_to_move;
        load_root<S>(L, rootb, root_to_move, D, t, lane);
        // (s_memtime accumulators of tree 0's first worker: 9 waiting for the selector's go, 10 its entries, 11 the scheduled copies,
        // 13 start of the kernel to its end)
        const bool wprof = prof && wid == 1 && lane == 0;
        long long wt1 = 0, wt2 = 0, wt3 = 0, wt4 = 0;
        if (active) {
            // this wave's share of the entries' walks (see `walk`): nothing else to do until the first job is queued
            if (pipe_wait_ge(&la_ready, 1)) {
                const int n_walk = la_n;
                for (int f = wid; f < n_walk; f += 1 + NW) walk(f, hsw[wid - 1]);
            } else if (lane == 0) {
                atomicOr(&D.err[t], kErrPipeline);
                pipe_store(&sh.err, 1);
            }
            wave_sync();
            if (lane == 0) __hip_atomic_fetch_add(&la_done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (wprof) wt1 = (long long)__builtin_amdgcn_s_memtime();
            // this wave's share of the first descents (see la_go): expansions reserve their draws in entry order (xseq), an
            // entry waits only for entries before it - each on a worker that takes its entries in ascending order
            if (!pipe_wait_ge(&la_go, 1)) {
                if (lane == 0) { atomicOr(&D.err[t], kErrPipeline); pipe_store(&sh.err, 1); }
            } else if (la_fast) {
                if (wprof) wt2 = (long long)__builtin_amdgcn_s_memtime();
                const int n_ent = la_n;
                for (int f = wid - 1; f < n_ent; f += NW) {
                    const int res = la_res[f];
                    if (res != kWalkLeaf && res != kWalkExpand) continue;      // (pool full: reported by the selector)
                    if (pipe_load(&sh.err)) break;
                    int depth = la_depth[f], parent = la_node[f], edge = la_edge[f], child = la_chd[f];
                    reset_work<S>(L, lane);
                    BoardScalars b = rootb;
                    int c = root_to_move;
                    for (int i = 0; i < depth; ++i) {
                        put_stone<S>(L, b, la_moves[f][i], c, D.zob, lane);
                        c = 3 - c;
                    }
                    if (res == kWalkExpand) {
                        if (!expand_node_pipe<S>(L, b, c, D, t, child, parent, edge, la_xseq[f], sh, lane)) break;
                        // node.py:349-361 at the node just made (its arrays were written by this wave's lanes)
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                        const int node = child;
                        const size_t nb = ((size_t)t * D.N + node) * A;
                        const int e2 = select_node_halving<S>(hsw[wid - 1], D, t, node, lane);
                        const int mv2 = D.action[nb + e2];
                        const int visits2 = D.ch_visits[nb + e2];
                        child = D.ch_index[nb + e2];
                        if (visits2 >= 1) {                                    // (a node made in this launch has no visited child)
                            if (lane == 0) { atomicOr(&D.err[t], kErrPipeline); pipe_store(&sh.err, 1); }
                            break;
                        }
                        if (lane == 0) { la_moves[f][depth] = (int16_t)mv2; rm_path[f][depth] = path_entry(node, e2); }
                        put_stone<S>(L, b, mv2, c, D.zob, lane);
                        c = 3 - c;
                        parent = node; edge = e2; depth += 1;
                        wave_sync();
                    }
                    // tree.py:412-416: the leaf's queue entry (node to evaluate - still NOT_EXPANDED: node[-1] -, parent, edge,
                    // path), the virtual losses of its path below the root (node.py:76-83), its planes
                    const int q = rm_slot[f];
                    const size_t qs = (size_t)t * D.K + q;
                    if (lane == 0) write_queue_entry<UNIQUE>(D, qs, child, parent, edge, depth, f);
                    const int my_entry = lane < depth ? rm_path[f][lane] : 0;
                    if (lane < depth && lane < kPathCap) D.q_path[qs * kPathCap + lane] = my_entry;
                    write_planes<S>(L, b, c, planes + (leaf_base + (UNIQUE ? f : q)) * 6 * G::P, lane);
                    // the later descents through this root child end on the same leaf (see `sched`): how many, for the virtual
                    // losses (node.py:76-83 below the root: one per descent on every node and edge of the path - added once); the
                    // position for whoever writes their queue entries and planes (below)
                    const int n_all = la_ndesc;
                    int n_through = 1;
                    for (int q0 = 0; q0 < n_all; q0 += 64)
                        n_through += __popcll(__ballot(q0 + lane < n_all && sched[q0 + lane] == f));
                    if (lane >= 1 && lane < depth) {
                        const size_t ns = (size_t)t * D.N + path_node(my_entry);
                        atomicAdd(&D.node[ns].vl, n_through);
                        atomicAdd(&D.ch_vl[ns * A + path_edge(my_entry)], n_through);
                    }
                    {
                        const bool pass_plane = b.moves > 1 && b.prev == 0;
                        for (int pt = lane; pt < G::P; pt += 64) {
                            const int p = (pt / S + 1) * G::W + (pt % S) + 1;
                            int col = L.color[p];
                            if (c == kWhite && col != 0) col = 3 - col;
                            ent_code[f][pt] = (uint8_t)(col | ((!pass_plane && p == b.prev) ? 4 : 0));
                        }
                        if (lane == 0) {
                            ent_meta[f] = (pass_plane ? 1 : 0) | (c == kWhite ? 2 : 0);
                            rm_parent[f] = parent; rm_edge[f] = edge; rm_child[f] = child; rm_job[f] = -1; rm_depth[f] = depth;
                        }
                    }
                    wave_sync();
                    if (lane == 0) pipe_store(&ent_done[f], 1);
                }
                // the repeats, shared out over the workers: queue entry, path and planes of leaf slot q = those of its entry
                auto entry_stands = [&](int f) -> bool {                   // entry f's leaf: queue data and position code in LDS
                    for (int spin = 0; spin < kPipeSpinLimit; ++spin) {
                        if (pipe_load(&ent_done[f])) return true;
                        if (pipe_load(&sh.err)) break;
                        __builtin_amdgcn_s_sleep(1);
                    }
                    if (lane == 0) { atomicOr(&D.err[t], kErrPipeline); pipe_store(&sh.err, 1); }
                    return false;
                };
                auto planes_of_entry = [&](int f, float *dst) {
                    const int meta_f = ent_meta[f];
                    const float pass_f = (meta_f & 1) ? 1.f : 0.f, side_f = (meta_f & 2) ? -1.f : 1.f;
                    for (int pt = lane; pt < G::P; pt += 64) {
                        const int code = ent_code[f][pt], col = code & 3;
                        dst[pt] = col == 0 ? 1.f : 0.f;
                        dst[G::P + pt] = col == 1 ? 1.f : 0.f;
                        dst[2 * G::P + pt] = col == 2 ? 1.f : 0.f;
                        dst[3 * G::P + pt] = (code & 4) ? 1.f : 0.f;
                        dst[4 * G::P + pt] = pass_f;
                        dst[5 * G::P + pt] = side_f;
                    }
                };
                const int n_rep = la_ndesc;
                for (int q = wid - 1; q < n_rep; q += NW) {
                    const int f = sched[q];
                    if (f < 0) continue;
                    if (la_res[f] != kWalkLeaf && la_res[f] != kWalkExpand) continue;
                    if (!entry_stands(f)) break;
                    const int depth = rm_depth[f];
                    const size_t qs = (size_t)t * D.K + q;
                    if (lane == 0) write_queue_entry<UNIQUE>(D, qs, rm_child[f], rm_parent[f], rm_edge[f], depth, f);
                    if (lane < depth && lane < kPathCap) D.q_path[qs * kPathCap + lane] = rm_path[f][lane];
                    if constexpr (!UNIQUE) planes_of_entry(f, planes + (leaf_base + q) * 6 * G::P);
                }
                if constexpr (UNIQUE) {
                    // the slots of the range behind the last entry: entry 0's position once more (never read by the backup)
                    if (n_ent > 0 && (la_res[0] == kWalkLeaf || la_res[0] == kWalkExpand))
                        for (int p = n_ent + wid - 1; p < ucap; p += NW) {
                            if (!entry_stands(0)) break;
                            planes_of_entry(0, planes + (leaf_base + p) * 6 * G::P);
                        }
                }
                if (wprof) wt3 = (long long)__builtin_amdgcn_s_memtime();
            }
        }
        for (int k = wid - 1; active; k += NW) {
            const int slot = k % kPipeSlots;
            bool have = false, stalled = true;
            for (int spin = 0; spin < kPipeSpinLimit; ++spin) {
                if (pipe_load(&sh.job_seq[slot]) == k + 1) { have = true; stalled = false; break; }
                const int fc = pipe_load(&sh.final_count);
                if (fc >= 0 && k >= fc) { stalled = false; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            if (stalled && lane == 0) {
                atomicOr(&D.err[t], kErrPipeline);
                pipe_store(&sh.err, 1);
            }
            if (!have) break;
            const PipeJob j = sh.job[slot];
            if (j.k >= 0) {
                // the leaf's queue entry and the virtual losses of its path below the root (node.py:76-83) - what the
                // selector would otherwise spend ~2 k cycles per descent on (64-bit addressing of seven arrays)
                const size_t qs = (size_t)t * D.K + j.k;
                if (lane == 0) write_queue_entry<UNIQUE>(D, qs, j.child, j.parent, j.edge, j.depth, j.src);
                for (int i = lane; i < j.depth; i += 64) {
                    const int entry = sh.paths[slot][i];
                    if (i < kPathCap) D.q_path[qs * kPathCap + i] = entry;
                    if (i >= 1) {
                        const size_t ns = (size_t)t * D.N + path_node(entry);
                        atomicAdd(&D.node[ns].vl, 1);
                        atomicAdd(&D.ch_vl[ns * A + path_edge(entry)], 1);
                    }
                }
            }
            if (UNIQUE && j.expand == 2) {
                // a repeat of entry j.src: no planes of its own
            } else if (j.expand == 2) {
                // COPY: the planes of leaf slot j.src (written by job j.xseq) are this leaf's planes
                if (!pipe_wait_done(sh, j.xseq)) {
                    if (lane == 0) { atomicOr(&D.err[t], kErrPipeline); pipe_store(&sh.err, 1); }
                    break;
                }
                static_assert((6 * G::P) % 2 == 0, "8-byte copies");
                const float2 *src = reinterpret_cast<const float2 *>(planes + (leaf_base + j.src) * 6 * G::P);
                float2 *dst = reinterpret_cast<float2 *>(planes + (leaf_base + j.k) * 6 * G::P);
                for (int i = lane; i < 3 * G::P; i += 64) dst[i] = src[i];
            } else {
                reset_work<S>(L, lane);
                BoardScalars b = rootb;
                int c = root_to_move;
                for (int i = 0; i < j.depth; ++i) {
                    put_stone<S>(L, b, sh.moves[slot][i], c, D.zob, lane);
                    c = 3 - c;
                }
                if (j.expand) expand_node_pipe<S>(L, b, c, D, t, j.child, j.parent, j.edge, j.xseq, sh, lane);
                if (j.k >= 0) write_planes<S>(L, b, c, planes + (leaf_base + (UNIQUE ? j.src : j.k)) * 6 * G::P, lane);
            }
            wave_sync();
            if (lane == 0) {
                pipe_set_done(sh, k);
                pipe_store(&sh.slot_done[slot], k / kPipeSlots + 1);
            }
        }
        // the scheduled leaves (see `sched`): leaf slot q of this tree repeats the leaf of root-child entry f
        if (wprof) wt4 = (long long)__builtin_amdgcn_s_memtime();
        const int nq = (active && !la_fast && pipe_load(&sh.final_count) >= 0 && !pipe_load(&sh.err)) ? bulk_n : 0;
        for (int q = wid - 1; q < nq; q += NW) {
            const int f = sched[q];
            if (f < 0) continue;
            const int depth = rm_depth[f];
            const size_t qs = (size_t)t * D.K + q;
            if (lane == 0) write_queue_entry<UNIQUE>(D, qs, rm_child[f], rm_parent[f], rm_edge[f], depth, f);
            if (lane < depth) {
                const int entry = rm_path[f][lane];
                if (lane < kPathCap) D.q_path[qs * kPathCap + lane] = entry;
                if (lane >= 1) {                                                   // node.py:76-83 below the root
                    const size_t ns = (size_t)t * D.N + path_node(entry);
                    atomicAdd(&D.node[ns].vl, 1);
                    atomicAdd(&D.ch_vl[ns * A + path_edge(entry)], 1);
                }
            }
            if constexpr (UNIQUE) continue;                                        // (a repeat has no planes of its own)
            if (!pipe_wait_done(sh, rm_job[f])) {                                  // the first leaf's planes are there
                if (lane == 0) { atomicOr(&D.err[t], kErrPipeline); pipe_store(&sh.err, 1); }
                break;
            }
            const float2 *src = reinterpret_cast<const float2 *>(planes + (leaf_base + rm_slot[f]) * 6 * G::P);
            float2 *dst = reinterpret_cast<float2 *>(planes + (leaf_base + q) * 6 * G::P);
            for (int i = lane; i < 3 * G::P; i += 64) dst[i] = src[i];
        }
        if constexpr (UNIQUE) {
            // the slots of the range behind the last entry: a copy of entry 0's planes (slot 0 of the range, LEAF job rm_job[0])
            if (nq > 0)
                for (int p = la_n + wid - 1; p < ucap; p += NW) {
                    if (!pipe_wait_done(sh, rm_job[0])) {
                        if (lane == 0) { atomicOr(&D.err[t], kErrPipeline); pipe_store(&sh.err, 1); }
                        break;
                    }
                    const float2 *src = reinterpret_cast<const float2 *>(planes + leaf_base * 6 * G::P);
                    float2 *dst = reinterpret_cast<float2 *>(planes + (leaf_base + p) * 6 * G::P);
                    for (int i = lane; i < 3 * G::P; i += 64) dst[i] = src[i];
                }
        }
        if (wprof) {
            const long long wt5 = (long long)__builtin_amdgcn_s_memtime();
            D.prof[9] += wt2 - wt1; D.prof[10] += wt3 - wt2; D.prof[11] += wt5 - wt4; D.prof[13] += wt5 - t_begin;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        D.meta[t].num_nodes = num_nodes;
        D.n_leaves[t] = queued;
        set_cursor(D, t, sh.cursor_val);
    }
}

// tree.py:359-422: one sequential-halving phase per launch: for threshold 1..max_count,
// num_considered descents each; every descent ends in a queued leaf.
// UNIQUE: nothing is saved here - every leaf has planes of its own in the packed order (`leaf_off`), q_src is the identity.
template <int S, bool UNIQUE = false>
__global__ __launch_bounds__(64) void select_gumbel_kernel(SearchDev D, const int32_t *num_considered,
                                                           const int32_t *max_count, int stride,
                                                           const int32_t *leaf_off, float *planes) {
    using G = Geo<S>;
    constexpr int A = G::A;
    __shared__ Lds<S> L;
    const int t = blockIdx.x, lane = threadIdx.x;
    BoardScalars rootb;
    int root_to_move;
    load_root<S>(L, rootb, root_to_move, D, t, lane);
    int num_nodes = D.meta[t].num_nodes;
    int queued = 0;
    const int width = num_considered[t], levels = max_count[t];
    // packed layout (leaf_off != null): this tree's leaves follow those of the trees before it
    const size_t leaf_base = leaf_off ? (size_t)leaf_off[t] : (size_t)t * stride;
    bool ok = D.err[t] == 0 && num_nodes > 0 && width * levels <= stride;
    for (int th = 1; ok && th <= levels; ++th) {
        for (int j = 0; ok && j < width; ++j) {
            reset_work<S>(L, lane);
            BoardScalars b = rootb;
            int c = root_to_move;
            int node = 0;
            for (;;) {
                const size_t ns = (size_t)t * D.N + node;
                const size_t base = ns * A;
                const int e = node == 0 ? select_root_halving<S>(D, t, node, th, lane)
                                        : select_node_halving<S>(L, D, t, node, lane);
                const int mv = D.action[base + e];
                put_stone<S>(L, b, mv, c, D.zob, lane);
                c = 3 - c;
                const int visits = D.ch_visits[base + e];
                int child = D.ch_index[base + e];
                wave_sync();
                if (lane == 0) {
                    D.node[ns].vl += 1;
                    D.ch_vl[base + e] += 1;
                }
                if (visits < 1) {                                     // tree.py:412-416
                    write_planes<S>(L, b, c, planes + (leaf_base + queued) * 6 * G::P, lane);
                    // (the child is still NOT_EXPANDED: node[-1])
                    if (lane == 0) write_queue_entry<UNIQUE>(D, TreeSlot{t, queued}, child, node, e, kNoRecordedPath, queued);
                    wave_sync();
                    break;
                }
                if (child == kNotExpanded) {                          // tree.py:418-420
                    child = expand_node<S>(L, b, c, D, t, num_nodes, node, e, lane);
                    if (child < 0) { ok = false; break; }
                    if (lane == 0) D.ch_index[base + e] = child;
                }
                node = child;
                wave_sync();
            }
            if (ok) ++queued;
        }
    }
    if (lane == 0) {
        D.meta[t].num_nodes = num_nodes;
        D.n_leaves[t] = queued;
    }
}


// Apply one move per tree to its ROOT position on the device (GoBoard.put_stone on the game
// board, go_board.py:131-185) so that self-play boards never leave the GPU.
template <int S>
__global__ __launch_bounds__(64) void play_kernel(SearchDev D, const int32_t *moves) {
    using G = Geo<S>;
    __shared__ Lds<S> L;
    const int t = blockIdx.x, lane = threadIdx.x;
    int mv = moves[t];
    if (mv == -2) {
        // the move of the most visited root child (node.py:167-175 get_best_move_index: np.argmax, first index on ties),
        // chosen here so that a driver that only advances its positions needs no read-back between two searches
        constexpr int R = (G::A + 63) / 64;
        const size_t rbase = (size_t)t * D.N * G::A;
        const int nc = D.meta[t].num_nodes > 0 ? D.node[(size_t)t * D.N].children : 0;
        double best = 0.0;
        int best_i = -1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            if (i < nc) {
                const double v = (double)D.ch_visits[rbase + i];
                if (best_i < 0 || v > best) { best = v; best_i = i; }
            }
        }
        best_i = wave_argmax_first(best, best_i);
        mv = best_i >= 0 ? (int)D.action[rbase + best_i] : -1;
    }
    if (mv < 0) return;                                 // RESIGN / idle tree
    BoardScalars b;
    int to_move;
    load_root<S>(L, b, to_move, D, t, lane);
    reset_work<S>(L, lane);
    put_stone<S>(L, b, mv, to_move, D.zob, lane);
    store_root<S>(L, b, 3 - to_move, D, t, D.superko != 0, false, false, lane);
}

// ---- policy-only play (nn/policy_player.py:13-46, gtp/client.py:206-211): one move per board from one forward pass ----
// What the kernels of a tg_policy handle get besides the engine's SearchDev.  Per board the generator of Python's `random`
// module (MT19937; random.getstate()[1] is the 624 words + position), one random() per move.  Games mode: slot t plays the
// games t, t + T, t + 2T, ...; a slot whose game is over is parked and takes its next game at an EVEN global ply only, so
// that every live board has the same side to move.
struct PolicyDev {
    uint32_t *mt;               // [T][625] generator state per board (lazy convention: position 624 = twist first)
    int32_t *moves;             // [T] the move chosen by the last launch (-1: parked slot)
    const uint32_t *game_mt;    // [games][625] generator state every game starts from
    int32_t *slot;              // [T][4] game in progress (-1: parked), consecutive passes, next game, games finished
    int32_t *fin_pub;           // [T] host-mapped copy of "games finished"
    int32_t *log;               // [games][max_moves] the moves of every game
    int32_t *len, *reason;      // [games] moves played; 0 = running, 1 = two passes, 2 = max_moves reached
    uint8_t *final_cells;       // [games][NC] the board a game ended on
    const uint8_t *no_superko;  // [T] != 0: this board is a GoBoard(check_superko=False) on a handle that checks (null: none)
    int32_t games, max_moves, ply, flags;
};
enum : int32_t { kPolPlay = 1, kPolAnswerPass = 2, kPolGames = 4 };

// GoBoard.is_legal (go_board.py:260-304) for every on-board point: occupied, suicide, ko, positional superko (with the
// opponent-key quirk of :292-296) - the legality half of gen_candidates, WITHOUT its self-atari and eye filters.  Lane l
// gets bit r of the result for point q = 64 r + l (row-major).
template <int S, typename LT>
__device__ unsigned legal_points(LT &L, const BoardScalars &b, int me, const SearchDev &D, bool superko, int lane) {
    using G = Geo<S>;
    constexpr int W = G::W, NC = G::NC, P = G::P;
    const int opp = 3 - me;
    for (int p = lane; p < NC; p += 64) { L.libcnt[p] = 0; L.strhash[p] = 0; }
    wave_sync();
    for (int p = lane; p < NC; p += 64) {
        const int c = L.color[p];
        if (c == kBlack || c == kWhite) {
            if (superko) atomicXor((unsigned long long *)&L.strhash[L.sid[p]], (unsigned long long)D.zob[opp * NC + p]);
        } else if (c == kEmpty) {
            const int s0 = L.sid[p - W], s1 = L.sid[p - 1], s2 = L.sid[p + 1], s3 = L.sid[p + W];
            if (s0) atomicAdd(&L.libcnt[s0], 1u);
            if (s1 && s1 != s0) atomicAdd(&L.libcnt[s1], 1u);
            if (s2 && s2 != s0 && s2 != s1) atomicAdd(&L.libcnt[s2], 1u);
            if (s3 && s3 != s0 && s3 != s1 && s3 != s2) atomicAdd(&L.libcnt[s3], 1u);
        }
    }
    wave_sync();
    unsigned mask = 0;
    const int hl = b.moves < G::HMAX ? b.moves : G::HMAX;
#pragma unroll
    for (int r = 0; r < (P + 63) / 64; ++r) {
        const int q = 64 * r + lane;
        const int p = (q < P) ? (q / S + 1) * W + (q % S) + 1 : 0;
        bool legal = false;
        uint64_t h = 0;
        if (q < P && L.color[p] == kEmpty) {
            const int nn[4] = {p - W, p - 1, p + 1, p + W};
            int col[4], sid[4], lib[4], ne = 0;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                col[d] = L.color[nn[d]];
                sid[d] = L.sid[nn[d]];
                lib[d] = sid[d] ? (int)L.libcnt[sid[d]] : 0;
                ne += col[d] == kEmpty;
            }
            bool suicide = true;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                if (col[d] == opp && lib[d] == 1) suicide = false;
                if (col[d] == me && lib[d] > 1) suicide = false;
            }
            legal = !(ne == 0 && suicide);
            if (b.ko_pos == p && b.ko_move == b.moves - 1) legal = false;
            if (legal && superko) {
                h = b.hash ^ D.zob[me * NC + p];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    bool dup = false;
#pragma unroll
                    for (int e = 0; e < d; ++e) dup |= sid[e] == sid[d];
                    if (sid[d] && !dup && lib[d] == 1) h ^= L.strhash[sid[d]];
                }
            }
        }
        if (superko) {                                  // wave-uniform scan of the history, as in gen_candidates
            bool seen = false;
            for (int i = 0; i < hl; i += 4) {
                const uint64_t a0 = L.hist[i];
                const uint64_t a1 = L.hist[i + 1 < G::HMAX ? i + 1 : i];
                const uint64_t a2 = L.hist[i + 2 < G::HMAX ? i + 2 : i];
                const uint64_t a3 = L.hist[i + 3 < G::HMAX ? i + 3 : i];
                seen |= a0 == h;
                seen |= i + 1 < hl && a1 == h;
                seen |= i + 2 < hl && a2 == h;
                seen |= i + 3 < hl && a3 == h;
            }
            if (seen) legal = false;
        }
        if (legal) mask |= 1u << r;
    }
    return mask;
}

// word i (wave-uniform) of a generator state held in registers
__device__ __forceinline__ uint32_t mt_word(const tg_rng::MtRegs &m, int i) {
    uint32_t v = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r)
        if ((i >> 6) == r) v = m.k[r];
    return (uint32_t)__shfl((int)v, i & 63);
}

// One random.random() of board t's generator (CPython _randommodule.c: a = genrand >> 5, b = genrand >> 6,
// (a * 67108864.0 + b) / 9007199254740992.0).  Both words inside the current block: two loads and the new position.  A
// draw that needs the next block - position 624, or 623 with its second word behind the twist - takes the state through
// registers and writes the new block back.
__device__ double policy_draw(uint32_t *st, int lane) {
    using namespace tg_rng;
    const int pos = (int)st[kMtN];
    uint32_t w0, w1;
    if (pos + 2 <= kMtN) {
        w0 = st[pos];
        w1 = st[pos + 1];
        wave_sync();                                      // (every lane has read the position before lane 0 moves it)
        if (lane == 0) st[kMtN] = (uint32_t)(pos + 2);
    } else {
        MtRegs m;
        mt_load(m, st, lane);
        w0 = pos < kMtN ? mt_word(m, pos) : 0u;           // position 623: the last word of the old block
        mt_twist(m, lane);
        int at = 0;
        if (pos >= kMtN) w0 = mt_word(m, at++);
        w1 = mt_word(m, at++);
        wave_sync();
        mt_store(m, st, lane);
        if (lane == 0) st[kMtN] = (uint32_t)at;
    }
    w0 = mt_temper(w0);
    w1 = mt_temper(w1);
    const unsigned long long bits = ((unsigned long long)(w0 >> 5) << 26) | (unsigned long long)(w1 >> 6);
    return (double)bits * 0x1p-53;                        // exact: the same value as the quotient above
}

// The empty board of a new game on slot t, in LDS and as the slot's root position, and game g's generator state.
template <int S, typename LT>
__device__ void policy_start_game(LT &L, BoardScalars &b, int &to_move, const SearchDev &D, const PolicyDev &Pd, int t, int g,
                                  int lane) {
    empty_board<S>(L, b, lane);
    to_move = kBlack;
    store_root<S>(L, b, to_move, D, t, D.superko != 0, true, false, lane);     // (one word of history either way)
    if (g >= 0)
        for (int i = lane; i < tg_rng::kStateWords; i += 64)
            Pd.mt[(size_t)t * tg_rng::kStateWords + i] = Pd.game_mt[(size_t)g * tg_rng::kStateWords + i];
    wave_sync();
}

// Planes [T][6][P] of the current root position of every board, symmetry 0 (nn/feature.py:10-57 as policy_player.py:25
// calls it).  No tree is reset, no root expanded, no draw consumed, the leaf queue is left alone.  init != 0 (games mode,
// before the first ply): every slot gets an empty board first and slot t < games starts game t.
template <int S>
__global__ __launch_bounds__(64) void policy_planes_kernel(SearchDev D, PolicyDev Pd, float *planes, int init) {
    using G = Geo<S>;
    __shared__ Lds<S, false> L;
    const int t = blockIdx.x, lane = threadIdx.x;
    BoardScalars b;
    int to_move;
    if (init) {
        const int g = t < Pd.games ? t : -1;
        policy_start_game<S>(L, b, to_move, D, Pd, t, g, lane);
        if (lane == 0) {
            int32_t *sl = Pd.slot + (size_t)t * 4;
            sl[0] = g;
            sl[1] = 0;
            sl[2] = t + D.T;
            sl[3] = 0;
            Pd.fin_pub[t] = 0;
        }
    } else {
        for (int p = lane; p < G::NC; p += 64) L.color[p] = D.root_cells[(size_t)t * G::NC + p];
        const RootMeta m = D.meta[t];
        b = scalars_of(m);
        to_move = m.to_move;
        wave_sync();
    }
    write_planes<S>(L, b, to_move, planes + (size_t)t * 6 * G::P, lane);
}

// One move per board from policy [T][A] (softmax output, index P = PASS), one wavefront per board:
//   candidates = legal on-board points in row-major order, then PASS               (policy_player.py:32-36)
//   kept       = candidates with double(p) > max_p * 0.1, in fp64                  (:38-41)
//   move       = random.choices(kept, weights)                                     (:46; CPython 3.10 Lib/random.py:
//                cum = sequential fp64 running sum, x = random() * cum[-1], kept[bisect_right(cum, x, 0, n - 1)])
//   kPolAnswerPass: PASS when the previous move was a pass (gtp/client.py:209-211) - the draw is consumed all the same.
// kPolPlay: the move is played on the root position as play_kernel does.  kPolGames: move log, two-pass / max_moves end,
// parked slots and their refill at even plies (PolicyDev).  next_planes != null (with kPolPlay): the planes of the position
// AFTER the move go there, so that a ply of a game is this launch and the forward pass.  Parked slots do nothing.
template <int S>
__global__ __launch_bounds__(64) void policy_move_kernel(SearchDev D, PolicyDev Pd, const float *policy, float *next_planes) {
    using G = Geo<S>;
    constexpr int W = G::W, NC = G::NC, P = G::P, A = G::A, R = (P + 63) / 64;
    __shared__ Lds<S> L;
    const int t = blockIdx.x, lane = threadIdx.x;
    const bool games = (Pd.flags & kPolGames) != 0;
    int32_t *sl = Pd.slot + (size_t)t * 4;
    // the slot's record in registers (every lane), written back by lane 0 at the end
    int game = games ? sl[0] : 0, passes = games ? sl[1] : 0, next_game = games ? sl[2] : 0, finished = games ? sl[3] : 0;
    BoardScalars b;
    int to_move = kBlack;
    bool have_board = false;
    if (game >= 0) {
        load_root<S>(L, b, to_move, D, t, lane);
        reset_work<S>(L, lane);
        const bool superko = D.superko && !(Pd.no_superko && Pd.no_superko[t]);
        const unsigned legal = legal_points<S>(L, b, to_move, D, superko, lane);
        const float *pol = policy + (size_t)t * A;
        double w[R];
        double mx = (double)pol[P];                       // PASS is always a candidate
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int q = 64 * r + lane;
            w[r] = ((legal >> r) & 1u) ? (double)pol[q] : 0.0;
            if (((legal >> r) & 1u) && w[r] > mx) mx = w[r];
        }
        mx = wave_max_f64(mx);
        const double cut = mx * 0.1;
        // kept candidates, compacted in order: coordinates in L.cand, weights in L.w1
        int n = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int q = 64 * r + lane;
            const bool keep = ((legal >> r) & 1u) && w[r] > cut;
            const unsigned long long kept = __ballot(keep);
            if (keep) {
                const int at = n + __popcll(kept & ((1ull << lane) - 1));
                L.cand[at] = (uint16_t)((q / S + 1) * W + (q % S) + 1);
                L.w1[at] = w[r];
            }
            n += __popcll(kept);
        }
        if ((double)pol[P] > cut) {
            if (lane == 0) { L.cand[n] = 0; L.w1[n] = (double)pol[P]; }
            ++n;
        }
        wave_sync();
        // the running sum, in order, on one lane (n dependent fp64 adds; n >= 1: the maximum itself is always kept)
        if (lane == 0) {
            double c = L.w1[0];
            L.w2[0] = c;
            for (int i = 1; i < n; ++i) { c += L.w1[i]; L.w2[i] = c; }
        }
        wave_sync();
        const double u = policy_draw(Pd.mt + (size_t)t * tg_rng::kStateWords, lane);
        // bisect_right(cum, x, 0, n - 1): cum is non-decreasing, so it is the number of entries <= x among the first n - 1
        // (n == 0 - a policy of NaNs, where the reference raises - plays PASS)
        const double x = n > 0 ? u * (L.w2[n - 1] + 0.0) : 0.0;
        int cnt = 0;
        for (int i = lane; i < n - 1; i += 64) cnt += L.w2[i] <= x;
        cnt = wave_sum(cnt);
        int mv = n > 0 ? (int)L.cand[cnt] : 0;
        if ((Pd.flags & kPolAnswerPass) && b.moves > 1 && b.prev == 0) mv = 0;
        if (lane == 0) Pd.moves[t] = mv;
        if (Pd.flags & kPolPlay) {
            put_stone<S>(L, b, mv, to_move, D.zob, lane);
            to_move = 3 - to_move;
            store_root<S>(L, b, to_move, D, t, superko, false, false, lane);
            have_board = true;
            if (games) {
                const int len = b.moves - 1;              // moves of this game so far (a game starts at moves == 1)
                passes = mv == 0 ? passes + 1 : 0;
                const int why = passes == 2 ? 1 : len >= Pd.max_moves ? 2 : 0;
                if (why) {
                    for (int p = lane; p < NC; p += 64) Pd.final_cells[(size_t)game * NC + p] = L.color[p];
                    have_board = false;
                }
                if (lane == 0) {
                    if (len <= Pd.max_moves) Pd.log[(size_t)game * Pd.max_moves + len - 1] = mv;
                    if (why) {
                        Pd.len[game] = len;
                        Pd.reason[game] = why;
                        Pd.fin_pub[t] = finished + 1;
                    }
                }
                if (why) {                                // park the slot
                    next_game = game + D.T;
                    finished += 1;
                    game = -1;
                }
                wave_sync();
            }
        }
    } else if (lane == 0) {
        Pd.moves[t] = -1;
    }
    if (games && game < 0 && ((Pd.ply + 1) & 1) == 0 && next_game < Pd.games) {     // the next ply is even: take the next game
        game = next_game;
        passes = 0;
        policy_start_game<S>(L, b, to_move, D, Pd, t, game, lane);
        have_board = true;
    }
    if (games && lane == 0) { sl[0] = game; sl[1] = passes; sl[2] = next_game; sl[3] = finished; }
    if (next_planes && have_board) write_planes<S>(L, b, to_move, next_planes + (size_t)t * 6 * P, lane);
}

// ---- training samples from game records (nn/data_generator.py:37-149): replay a record, featurise the sampled plies ----
// What replay_samples_kernel reads and writes.  Game g's moves are moves[offsets[g] .. offsets[g + 1]) (padded coordinates,
// 0 = PASS); its samples are the rows s_off[g] .. s_off[g + 1) of (s_ply, s_sym), sorted by ply, and sample row r owns
// planes[r].  flags[g]: 0 = every sample of the game written; 1 = a move outside what put_stone is specified for (not a
// coordinate of this board, or a point that is not empty) - the game stops there and the host redoes it.
struct ReplayDev {
    const int32_t *moves;
    const int64_t *offsets;
    const int32_t *s_ply;
    const int8_t *s_sym;
    const int64_t *s_off;
    float *planes;              // [samples][6][P]
    int32_t *flags;             // [games]
    const uint64_t *zob;        // [4][NC] of zeros: no caller of the planes reads a hash
    int32_t games;
};

// The one replay of a game record: from the empty board, in front of each ply `visit(ply, to_move)` sees the LDS board and
// `b` and says whether to go on; then the move is checked and played with put_stone under `zob`.  colors: one per move, or
// null - alternating from black.  visit_final: the position behind the last move (ply == n_moves) is visited too, while its
// ply is one the host board records (< HMAX: go_board.py _save - prev_move and get_to_move have nothing to read beyond).
// Returns false where the replay stopped by rule - a record longer than the host board's move record (nothing is visited), a
// move put_stone is not specified for - and true where the visitor or the record ended it.  All lanes, wave-uniform arguments.
template <int S, typename LT, typename Visit>
__device__ __forceinline__ bool replay_record(LT &L, BoardScalars &b, const int32_t *moves, const int8_t *colors, int64_t n_moves,
                                              bool visit_final, const uint64_t *zob, int lane, Visit visit) {
    using G = Geo<S>;
    empty_board<S>(L, b, lane);
    if (tg_root::record_too_long(n_moves, G::HMAX)) return false;
    const int end = visit_final && n_moves < G::HMAX ? (int)n_moves + 1 : (int)n_moves;
    for (int ply = 0; ply < end; ++ply) {
        const int to_move = tg_root::record_to_move(colors, n_moves, ply);
        if (!visit(ply, to_move)) return true;
        if (ply == n_moves) break;
        const int mv = moves[ply];
        if (!tg_root::record_move_playable(mv, G::NC, L.color)) return false;
        put_stone<S>(L, b, mv, to_move, zob, lane);
    }
    return true;
}

// One wavefront per game record, grid-stride over the games: the record is replayed (replay_record) with colours
// alternating from black (data_generator.py:55-63 / :122-134 ignore the SGF colour tags), and before the move of every
// sampled ply the planes of the side to move go out, once per (ply, symmetry) row.  A game is left as soon as its last
// sample is written; the final position is never sampled.  The GAME is flagged where the replay stopped by rule.  No
// workgroup reads what another wrote.
template <int S>
__global__ __launch_bounds__(64) void replay_samples_kernel(ReplayDev R) {
    constexpr int P = Geo<S>::P;
    __shared__ Lds<S, false> L;
    const int lane = threadIdx.x;
    for (int g = blockIdx.x; g < R.games; g += gridDim.x) {
        const int64_t m0 = R.offsets[g];
        int64_t si = R.s_off[g];
        const int64_t se = R.s_off[g + 1];
        BoardScalars b;
        const bool done = replay_record<S>(L, b, R.moves + m0, nullptr, R.offsets[g + 1] - m0, false, R.zob, lane, [&](int ply, int to_move) {
            for (; si < se && R.s_ply[si] == ply; ++si)
                write_planes_under<S>(L, b, to_move, (int)R.s_sym[si], R.planes + (size_t)si * 6 * P, lane);
            return si < se;
        });
        if (lane == 0) R.flags[g] = done ? 0 : 1;
        wave_sync();                                      // (the next game's board is written over this one)
    }
}

// replay_samples_kernel's walk with the candidate list of every sampled ply (tg_replay_run_cand): in front of the move of a sampled
// ply the planes go out as there (no planes: R.planes null), then gen_candidates - expand_node's filter for the side to move,
// under `superko` with the history put_stone recorded under R.zob - and its bit image: bit a of word a / 32 for the row-major
// board point a of every candidate, PASS = P always, the tail bits zero; the same words for every row of the ply, whatever its
// symmetry.  The image is put together in L.libcnt, which nothing reads between two gen_candidates.  No workgroup reads what
// another wrote.
template <int S>
__global__ __launch_bounds__(64) void replay_cand_kernel(ReplayDev R, uint32_t *cand, int superko) {
    using G = Geo<S>;
    constexpr int P = G::P, W = G::W, MW = (G::A + 31) / 32;
    __shared__ Lds<S, false> L;
    const int lane = threadIdx.x;
    SearchDev D{};                                        // (gen_candidates reads the keys and the superko switch, nothing else)
    D.zob = R.zob;
    D.superko = superko;
    for (int g = blockIdx.x; g < R.games; g += gridDim.x) {
        const int64_t m0 = R.offsets[g];
        int64_t si = R.s_off[g];
        const int64_t se = R.s_off[g + 1];
        BoardScalars b;
        const bool done = replay_record<S>(L, b, R.moves + m0, nullptr, R.offsets[g + 1] - m0, false, R.zob, lane, [&](int ply, int to_move) {
            const int64_t first = si;
            for (; si < se && R.s_ply[si] == ply; ++si)
                if (R.planes) write_planes_under<S>(L, b, to_move, (int)R.s_sym[si], R.planes + (size_t)si * 6 * P, lane);
            if (si > first) {
                const int n = gen_candidates<S>(L, b, to_move, D, lane);
                uint32_t *words = L.libcnt;
                for (int w = lane; w < MW; w += 64) words[w] = 0u;
                wave_sync();
                for (int i = lane; i < n - 1; i += 64) {
                    const int p = L.cand[i];
                    const int a = (p / W - 1) * S + p % W - 1;
                    atomicOr(&words[a >> 5], 1u << (a & 31));
                }
                if (lane == 0) atomicOr(&words[P >> 5], 1u << (P & 31));
                wave_sync();
                for (int64_t r = first; r < si; ++r)
                    for (int w = lane; w < MW; w += 64) cand[(size_t)r * MW + w] = words[w];
                wave_sync();
            }
            return si < se;
        });
        if (lane == 0) R.flags[g] = done ? 0 : 1;
        wave_sync();                                      // (the next game's board is written over this one)
    }
}

// ---- search roots from game records (mcts/analysis.py game_positions, nn/data_generator.py _sampled_positions + ---------
// SearchEngine.set_root per position): replay a record once, write the root of every tree that sits on one of its plies ----
// What record_roots_kernel reads and writes.  Game g's moves are moves[offsets[g] .. offsets[g + 1]) with colours colors[..]
// (NULL: alternating from black).  rec[r] is the r-th record that has trees in this launch; its trees are the rows
// m_off[r] .. m_off[r + 1) of (m_ply, m_tree), sorted by ply - several rows may share a ply.  flags[t]: 0 = tree t's root
// written; 1 = not reached (tg_search_set_roots_from_records in include/tamago_hip.h states the rule), the tree's root is
// as it was.
struct RecordRootsDev {
    const int32_t *moves;
    const int8_t *colors;
    const int64_t *offsets;
    const int32_t *rec;         // [n_rec]
    const int32_t *m_off;       // [n_rec + 1]
    const int32_t *m_ply;
    const int32_t *m_tree;
    int32_t *flags;             // [T]
    int32_t n_rec;
};

// One wavefront per record, grid-stride over the records: the record is replayed (replay_record, final position included)
// under the handle's Zobrist keys, and in front of the move of ply p every tree whose position is "before move p" gets the
// LDS board as its root (store_root: what flush_roots uploads for a position staged by tg_search_set_root - the whole
// history, the sticky error word cleared).  A record is left behind its last tree.  The TREES the replay did not reach are
// flagged and keep their roots.  Every tree is in one row, so no two wavefronts write the same root, and no workgroup reads
// what another wrote.
template <int S>
__global__ __launch_bounds__(64) void record_roots_kernel(SearchDev D, RecordRootsDev R) {
    __shared__ Lds<S, false> L;
    const int lane = threadIdx.x;
    for (int r = blockIdx.x; r < R.n_rec; r += gridDim.x) {
        const int g = R.rec[r];
        const int64_t m0 = R.offsets[g];
        int si = R.m_off[r];
        const int se = R.m_off[r + 1];
        BoardScalars b;
        replay_record<S>(L, b, R.moves + m0, R.colors ? R.colors + m0 : nullptr, R.offsets[g + 1] - m0, true, D.zob, lane,
                         [&](int ply, int to_move) {
            for (; si < se && R.m_ply[si] == ply; ++si) {
                const int t = R.m_tree[si];
                store_root<S>(L, b, to_move, D, t, D.superko != 0, true, true, lane);
                if (lane == 0) R.flags[t] = 0;
            }
            return si < se;
        });
        for (int i = si + lane; i < se; i += 64) R.flags[R.m_tree[i]] = 1;
        wave_sync();                                      // (the next record's board is written over this one)
    }
}

// ---- tree reuse: the subtree under a new root becomes the whole tree, in place (tg_search_reroot) ----------------------
// No reference counterpart (the reference rebuilds its tree every move, mcts/tree.py:49-54).  Four launches in stream order,
// for every tree whose roots[t] >= 0 (the others return at once):
//   mark:   flag[i] = node i lies in the subtree of r = roots[t].  A child is always created after its parent (every
//           expansion takes the next index of the tree's counter while its parent already has one), so climbing the parent
//           pointers from i ends at r or below it after at most the tree's depth; a count per chunk of kRerootChunk nodes.
//   scan:   exclusive scan of the chunk counts (one wave per tree); the new num_nodes and, if a position was staged for the
//           tree, its new RootMeta; the leaf queue is emptied and the root noise cleared.
//   assign: map[i] = rank of i among the flagged nodes (the new index, creation order kept), -1 for the others.
//   move:   every flagged node i is moved to map[i] <= i with its child indices and parent pointer remapped.
// The move is in place: a destination can be a slot whose own node has not been moved yet.  One workgroup per tree walks
// the sources in increasing order, a window of them at a time, field by field: the window's values are read into LDS, a
// barrier, then written to their destinations.  A destination d = map[i] <= i is either a source of an earlier window
// (already read) or one of this window (read before the barrier); reads of later windows never touch a slot written
// earlier, because every destination of a window lies below the window's last source.  Extra device memory: map [T][N]
// and the chunk counts [T][N / kRerootChunk] (int32).
constexpr int kRerootChunk = 4096;           // nodes per mark / assign workgroup (256 threads x 16)
constexpr int kRerootLds = 48 * 1024;        // bytes of LDS for one window of one field

__device__ __forceinline__ int block_excl_scan_256(int v, int *wave_tot, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = wave_scan_add_i32(v);
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    int off = 0;
    total = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < w) off += wave_tot[k];
        total += wave_tot[k];
    }
    return off + inc - v;
}

__global__ __launch_bounds__(256) void reroot_mark_kernel(SearchDev D, const int32_t *roots, int32_t *map, int32_t *blk,
                                                           int32_t *old_n, int nblk) {
    __shared__ int wave_tot[4];
    const int t = blockIdx.x, r = roots[t];
    if (r < 0) return;
    const int n = D.meta[t].num_nodes;
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        old_n[t] = r < n ? n : -1;
        if (r >= n) atomicOr(&D.err[t], kErrReroot);
    }
    const NodeRec *rec = D.node + (size_t)t * D.N;
    int32_t *mp = map + (size_t)t * D.N;
    const int first = blockIdx.y * kRerootChunk + threadIdx.x * 16;
    int cnt = 0;
    for (int k = 0; k < 16; ++k) {
        const int i = first + k;
        if (i >= n || r >= n) break;
        int j = i;
        while (j > r) {
            const int p = rec[j].parent;
            j = p < j ? p : -1;              // (a parent at or above its child would be a corrupt pool: not in the subtree)
        }
        const int f = j == r ? 1 : 0;
        mp[i] = f;
        cnt += f;
    }
    int total;
    (void)block_excl_scan_256(cnt, wave_tot, total);
    if (threadIdx.x == 0) blk[(size_t)t * nblk + blockIdx.y] = total;
}

__global__ __launch_bounds__(64) void reroot_scan_kernel(SearchDev D, int A, const int32_t *roots, const int32_t *has_pos,
                                                          int32_t *blk, int nblk, const int32_t *old_n, int32_t *ident,
                                                          const RootMeta *stage) {
    const int t = blockIdx.x, lane = threadIdx.x;
    if (roots[t] < 0 || old_n[t] < 0) return;
    const int used = (old_n[t] + kRerootChunk - 1) / kRerootChunk;
    int run = 0;
    for (int base = 0; base < used; base += 64) {
        const int b = base + lane;
        const int v = b < used ? blk[(size_t)t * nblk + b] : 0;
        const int inc = wave_scan_add_i32(v);
        if (b < used) blk[(size_t)t * nblk + b] = run + inc - v;
        run += __shfl(inc, 63);
    }
    for (int i = lane; i < A; i += 64) D.noise[(size_t)t * A + i] = 0.0;
    if (lane == 0) {
        RootMeta m = has_pos[t] ? stage[t] : D.meta[t];
        m.num_nodes = run;
        D.meta[t] = m;
        ident[t] = run == old_n[t] ? 1 : 0;      // every node kept: the order-preserving map is the identity, nothing moves
        D.n_leaves[t] = 0;
        D.err[t] = 0;
    }
}

__global__ __launch_bounds__(256) void reroot_assign_kernel(SearchDev D, const int32_t *roots, int32_t *map, const int32_t *blk,
                                                             const int32_t *old_n, int nblk) {
    __shared__ int wave_tot[4];
    const int t = blockIdx.x;
    if (roots[t] < 0 || old_n[t] < 0) return;
    const int n = old_n[t];
    if ((int)blockIdx.y * kRerootChunk >= n) return;     // (uniform per workgroup: the scan below has every thread)
    int32_t *mp = map + (size_t)t * D.N;
    const int first = blockIdx.y * kRerootChunk + threadIdx.x * 16;
    uint32_t bits = 0;
    int cnt = 0;
    for (int k = 0; k < 16; ++k) {
        const int i = first + k;
        if (i < n && mp[i]) { bits |= 1u << k; ++cnt; }
    }
    int total;
    int next = blk[(size_t)t * nblk + blockIdx.y] + block_excl_scan_256(cnt, wave_tot, total);
    for (int k = 0; k < 16; ++k) {
        const int i = first + k;
        if (i < n) mp[i] = (bits >> k) & 1u ? next++ : -1;
    }
}

// one field of one window: rows [lo, lo + cnt) of `arr` (A elements per node) to their destinations (see above)
template <typename E, bool REMAP>
__device__ __forceinline__ void reroot_move_rows(E *arr, int per, int lo, int cnt, int n, const int32_t *mp, E *buf) {
    const int total = cnt * per;
    for (int e = threadIdx.x; e < total; e += blockDim.x) {
        const int i = lo + e / per;
        if (mp[i] >= 0) buf[e] = arr[(size_t)i * per + e % per];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < total; e += blockDim.x) {
        const int i = lo + e / per, d = mp[i];
        if (d >= 0) {
            E v = buf[e];
            if constexpr (REMAP) v = v >= 0 && v < n ? (E)mp[v] : (E)kNotExpanded;
            arr[(size_t)d * per + e % per] = v;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(1024) void reroot_move_kernel(SearchDev D, int A, const int32_t *roots, const int32_t *map,
                                                           const int32_t *old_n, const int32_t *ident) {
    __shared__ double lds[kRerootLds / sizeof(double)];
    const int t = blockIdx.x, r = roots[t];
    if (r < 0 || old_n[t] < 0 || ident[t]) return;
    const int n = old_n[t];
    const int32_t *mp = map + (size_t)t * D.N;
    const size_t pool = (size_t)t * D.N * A;
    const int W = (int)(kRerootLds / sizeof(double)) / A;    // nodes per window (A doubles each)
    for (int lo = r; lo < n; lo += W) {
        const int cnt = n - lo < W ? n - lo : W;
#define MOVE(field, E, per_child, remap) reroot_move_rows<E, remap>(D.field + pool, A, lo, cnt, n, mp, reinterpret_cast<E *>(lds));
        TG_NODE_POOL_CHILD_ARRAYS(MOVE)
#undef MOVE
        // the node records: 8 words each, parent remapped (the new root's parent and edge are -1)
        int32_t *buf = reinterpret_cast<int32_t *>(lds);
        int32_t *recs = reinterpret_cast<int32_t *>(D.node + (size_t)t * D.N);
        for (int e = threadIdx.x; e < cnt * 8; e += blockDim.x) {
            const int i = lo + e / 8;
            if (mp[i] >= 0) buf[e] = recs[(size_t)i * 8 + e % 8];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * 8; e += blockDim.x) {
            const int i = lo + e / 8, d = mp[i], w = e % 8;
            if (d < 0) continue;
            int32_t v = buf[e];
            if (w == 5) v = i == r || v < 0 || v >= n ? -1 : mp[v];   // NodeRec::parent
            else if (w == 6 && i == r) v = -1;                   // NodeRec::pedge
            recs[(size_t)d * 8 + w] = v;
        }
        __syncthreads();
    }
}

}  // namespace

// ======================================================================================
// host side
// ======================================================================================
// the row of a read-out record (readout.h) that starts `offset` bytes into it
template <class E>
__device__ __forceinline__ E *record_row(unsigned char *rec, size_t offset) { return reinterpret_cast<E *>(rec + offset); }

// One node of one tree packed into one record (tg_search_read_node: one launch + one copy instead of thirteen
// copies): [num_children, node_visits, node_virtual_loss, node_value_sum bits, raw_value bits, error flags, num_nodes, 0]
// (tg_pool::NodeHead), children_index[A], children_visits[A], children_virtual_loss[A], action[A] (int32), then
// value_sum[A], policy[A], value[A] (float64, 8-byte aligned).
__global__ __launch_bounds__(64) void gather_node_kernel(SearchDev D, int A, int tree, int node, unsigned char *out) {
    const int lane = threadIdx.x;
    const size_t ns = (size_t)tree * D.N + node, base = ns * A;
    int32_t *head = reinterpret_cast<int32_t *>(out);
    if (lane == 0) {
        head[tg_pool::kHeadChildren] = D.node[ns].children;
        head[tg_pool::kHeadVisits] = D.node[ns].visits;
        head[tg_pool::kHeadVl] = D.node[ns].vl;
        head[tg_pool::kHeadVsumBits] = __float_as_int(D.node[ns].vsum);
        head[tg_pool::kHeadRawBits] = __float_as_int(D.node[ns].raw);
        head[tg_pool::kHeadErr] = D.err[tree];
        head[tg_pool::kHeadNumNodes] = D.meta[tree].num_nodes;   // (tg_search_node_record_num_nodes: no second read after a search)
        head[tg_pool::kHeadPad] = 0;
    }
    // every child array at its place of the record (tg_pool::node_record_offset: up to four bytes widened to int32, eight as they are)
    for (int i = lane; i < A; i += 64) {
#define PUT(field, E, per_child, remap) \
        record_row<std::conditional_t<sizeof(E) == 8, E, int32_t>>(out, tg_pool::node_record_offset(tg_pool::k_##field, A))[i] = D.field[base + i];
        TG_NODE_POOL_CHILD_ARRAYS(PUT)
#undef PUT
    }
}

// Analysis read-out (tg_search_read_analysis, no reference counterpart): the root of every tree and the principal variation
// of each visited root child, mcts/tree.py:432-473 get_pv_lists / get_best_move_sequence, in one launch.  One wave per
// (tree, root child), kAnaWaves per workgroup.  Record of one tree (readout.h, TG_ANALYSIS_RECORD_ROWS):
//   [num_children, node_visits, node_value_sum bits, error flags], then action[A], children_visits[A], pv_len[A], resume[A]
//   (int32), then children_value_sum[A], children_policy[A] (float64, 8-byte aligned), then pv[A][max_depth] (int16).
// The walk of child i starts at root.children_index[i] (-1 looked up as node N - 1, the host's node[-1]) with the PV
// [action[i]].  At each node: no visits -> stop; else append action[best], best = np.argmax(children_visits[:num_children])
// (wave_argmax_first: first index on ties, child 0 of an all-zero row); children_index[best] == -1 -> stop; else go on
// there.  pv_len = moves written.  A walk that is not over after max_depth moves stores the node it would visit next in
// resume (-1 otherwise): the host continues there with tg_search_read_node, so the PV is exact at any max_depth.
using tg_readout::kAnaWaves, tg_readout::kAnaMaxDepth;

__global__ __launch_bounds__(64 * kAnaWaves) void read_analysis_kernel(SearchDev D, int A, int max_depth, unsigned char *out) {
    using namespace tg_readout;
    const int t = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * kAnaWaves + (threadIdx.x >> 6);             // root child of this wave (wave-uniform)
    const size_t root = (size_t)t * D.N, rbase = root * A;
    unsigned char *rec = out + (size_t)t * analysis_record_bytes(A, max_depth);
    int32_t *head = reinterpret_cast<int32_t *>(rec);
    int32_t *act = record_row<int32_t>(rec, analysis_record_offset(kAna_action, A));
    int32_t *vis = record_row<int32_t>(rec, analysis_record_offset(kAna_visits, A));
    int32_t *pv_len = record_row<int32_t>(rec, analysis_record_offset(kAna_pv_len, A));
    int32_t *resume = record_row<int32_t>(rec, analysis_record_offset(kAna_resume, A));
    double *vsum = record_row<double>(rec, analysis_record_offset(kAna_value_sum, A));
    double *pol = record_row<double>(rec, analysis_record_offset(kAna_policy, A));
    int16_t *pv = record_row<int16_t>(rec, analysis_pv_offset(A)) + (size_t)i * max_depth;
    if (i == 0 && lane == 0) {
        head[kAnaChildren] = D.node[root].children;
        head[kAnaVisits] = D.node[root].visits;
        head[kAnaVsumBits] = __float_as_int(D.node[root].vsum);
        head[kAnaErr] = D.err[t];
    }
    if (i >= A) return;
    const int nc = D.node[root].children;
    const int v0 = D.ch_visits[rbase + i];
    if (lane == 0) {
        act[i] = D.action[rbase + i];
        vis[i] = v0;
        vsum[i] = D.ch_vsum[rbase + i];
        pol[i] = D.ch_policy[rbase + i];
    }
    int len = 0, next = -1;
    if (i < nc && v0 > 0) {
        if (lane == 0) pv[0] = D.action[rbase + i];
        len = 1;
        int node = D.ch_index[rbase + i];
        if (node == kNotExpanded) node = D.N - 1;                       // tree.node[-1] (_NodeList: the pool's last slot)
        while (node >= 0 && node < D.N) {
            if (len == max_depth) { next = node; break; }
            const size_t ns = root + node, base = ns * A;
            if (D.node[ns].visits == 0) break;
            const int n = D.node[ns].children;
            double best = 0.0;
            int best_i = -1;
            for (int j = lane; j < n; j += 64) {
                const double v = (double)D.ch_visits[base + j];
                if (best_i < 0 || v > best) { best = v; best_i = j; }
            }
            best_i = wave_argmax_first(best, best_i);
            if (best_i < 0) best_i = 0;
            if (lane == 0) pv[len] = D.action[base + best_i];
            ++len;
            node = D.ch_index[base + best_i];
        }
    }
    if (lane == 0) {
        pv_len[i] = len;
        resume[i] = next;
    }
}

// Improved-policy read-out (tg_search_read_improved_policy): node.py:281-321 at the root of every tree, as a dense float32
// row in the network's output order (board points row-major, PASS last) - what sgf/selfplay_record.py:56 writes into a
// game record as "%.3e" text and nn/feature.py:80-102 reads back as a training target, without the text.  One wave per
// tree: improved_policy_weights (the arithmetic the selection kernels score with), the row assembled in LDS - 1e-18
// everywhere (feature.py's value for a move that was no candidate), child i's value at the slot of action[i] - and stored
// with plain vector stores.  bad[t]: the root has no children (not expanded) or an action that is no point of the board.
template <int S>
__global__ __launch_bounds__(64) void improved_policy_kernel(SearchDev D, float *rows, int32_t *bad) {
    using G = Geo<S>;
    constexpr int A = G::A, R = (A + 63) / 64;
    __shared__ HalvingScratch<S> hs;
    __shared__ float row[A];
    const int t = blockIdx.x, lane = threadIdx.x;
    const size_t ns = (size_t)t * D.N, base = ns * A;
    const int children = D.node[ns].children;
    const bool expanded = D.meta[t].num_nodes > 0 && children >= 1 && children <= A;      // (wave-uniform)
    for (int i = lane; i < A; i += 64) row[i] = 1e-18f;
    bool stray = false;
    if (expanded) {
        int vis[R], nc, nv;
        const double sum = improved_policy_weights<S>(hs, D, t, 0, lane, vis, nc, nv);
        wave_sync();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            if (i < nc) {
                const int pos = D.action[base + i];
                const int y = pos / G::W - 1, x = pos % G::W - 1;
                const bool on_board = pos > 0 && y >= 0 && y < S && x >= 0 && x < S;
                if (pos == 0 || on_board) row[pos == 0 ? G::P : y * S + x] = (float)(hs.w1[i] / sum);
                else stray = true;
            }
        }
    }
    const bool any_stray = __ballot(stray) != 0ull;
    wave_sync();
    for (int i = lane; i < A; i += 64) rows[(size_t)t * A + i] = row[i];
    if (lane == 0) bad[t] = (!expanded || any_stray) ? 1 : 0;
}

// Root statistics of every tree packed into one record per tree (one launch + ONE device-to-host copy instead of
// nine strided copies, each a host round trip): [num_children, node_visits, raw_value bits, error flags] then
// visits[A], virtual_loss[A], action[A] (int32), value_sum[A], policy[A] (float64) - readout.h, TG_ROOT_RECORD_ROWS.
__device__ __forceinline__ void write_root_record(const SearchDev &D, int A, int t, int lane, unsigned char *rec) {
    using namespace tg_readout;
    const size_t ns = (size_t)t * D.N, base = ns * A;
    int32_t *head = reinterpret_cast<int32_t *>(rec);
    if (lane == 0) {
        head[kRootChildren] = D.node[ns].children;
        head[kRootVisits] = D.node[ns].visits;
        head[kRootRawBits] = __float_as_int(D.node[ns].raw);
        head[kRootErr] = D.err[t];
    }
    for (int i = lane; i < A; i += 64) {
#define PUT(row, E, member) record_row<E>(rec, root_record_offset(kRoot_##row, A))[i] = D.member[base + i];
        TG_ROOT_RECORD_ROWS(PUT)
#undef PUT
    }
}
__global__ __launch_bounds__(64) void gather_roots_kernel(SearchDev D, int A, unsigned char *out, size_t rec_bytes) {
    write_root_record(D, A, blockIdx.x, threadIdx.x, out + (size_t)blockIdx.x * rec_bytes);
}

// Self-play, the end of a move WITHOUT the host (tg_selfplay_play_move): the root records as above, then the move itself -
// final root choice (tree.py:344, node.py:324-346: argmax of logit + noise + sigma(q) with the visit threshold), resign rule
// (worker.py:59-62), two-pass / move-limit end (worker.py:44, :80) - in the arithmetic the host used to do it in
// (float64, IEEE operations, first maximum wins), so that play_kernel and the next root expansion can follow at once.
// state [T][kStateWords], tail [T] (RootTail, its kind a MoveKind): readout.h.  moves_out[t]: the point played (0 = pass)
// or -1 (nothing to play: resigned, game over, idle slot).
__global__ __launch_bounds__(64) void finish_roots_kernel(SearchDev D, int A, unsigned char *out, size_t rec_bytes,
                                                          const int32_t *state, int max_moves, int32_t *moves_out, RootTail *tail) {
    using namespace tg_readout;
    const int t = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)t * D.N * A;
    write_root_record(D, A, t, lane, out + (size_t)t * rec_bytes);
    const int n = D.node[(size_t)t * D.N].children;
    const int32_t *st = state + (size_t)kStateWords * t;
    const int flags = st[kStateFlags], passes = st[kStatePasses], played = st[kStatePlayed];
    int best = -1, kind = kIdle, pos = -1, mv = -1;
    if (!(flags & kStateIdle) && n > 0) {
        int mc = 0;
        for (int i = lane; i < n; i += 64) {
            const int v = D.ch_visits[base + i];
            mc = v > mc ? v : mc;
        }
        mc = wave_max_i32(mc);
        const double sigma_sel = (double)(50 + mc) * 1.0;
        double bv = 0.0;
        int bi = -1;
        for (int i = lane; i < n; i += 64) {
            const int v = D.ch_visits[base + i];
            const double qi = v > 0 ? D.ch_vsum[base + i] / (double)v : 0.0;
            const double ev = (v + D.ch_vl[base + i] >= 100) ? -10000.0
                                                              : (D.ch_policy[base + i] + D.noise[(size_t)t * A + i]) + sigma_sel * qi;
            if (bi < 0 || ev > bv) { bv = ev; bi = i; }
        }
        best = wave_argmax_first(bv, bi);
        if (best < 0) best = 0;                            // every evaluation NaN (a diverged network): the host's rule "i == 0 || ev > best" keeps child 0
        const int bvis = D.ch_visits[base + best];
        const double value = bvis == 0 ? 0.5 : D.ch_vsum[base + best] / (double)bvis;
        pos = D.action[base + best];
        if (!(flags & kStateNeverResign) && value < 0.05) {
            kind = kResign;
        } else {
            const int p2 = pos == 0 ? passes + 1 : 0;
            if (p2 == 2) kind = kSecondPass;
            else if (played + 1 >= max_moves) kind = kMoveLimit;
            else { kind = kMove; mv = pos; }
        }
    }
    if (lane == 0) {
        moves_out[t] = mv;
        RootTail r{};
        r.best = best; r.kind = kind; r.pos = pos; r.cursor = D.rng_cursor[t];
        tail[t] = r;
    }
}

// PUCT match move (tg_search_best_moves): the end of search_best_move (mcts/tree.py:76-77, :87-105) for every tree, one
// wave each - a one-child root answers PASS; otherwise the first maximum of the root's child visits (node.py:169-177), its
// value children_value_sum / children_visits (node.py:364-369: float64 IEEE division, 0.5 without visits) and RESIGN when
// that is < resign_threshold.  play != 0: the move is played on the root position as play_kernel plays it (RESIGN plays
// nothing).  sit_out[t] != 0 (sit_out may be null): the tree is not read and not played, its record says so.
template <int S>
__global__ __launch_bounds__(64) void best_moves_kernel(SearchDev D, double resign_threshold, int play, const uint8_t *sit_out,
                                                        BestMove *out) {
    using G = Geo<S>;
    using namespace tg_readout;
    constexpr int A = G::A, R = (A + 63) / 64;
    __shared__ Lds<S> L;
    const int t = blockIdx.x, lane = threadIdx.x;
    const size_t ns = (size_t)t * D.N, base = ns * A;
    BestMove rec{};
    const bool sat = sit_out && sit_out[t] != 0;                       // (wave-uniform, like everything that branches below)
    const int n = (!sat && D.meta[t].num_nodes > 0) ? D.node[ns].children : 0;
    if (sat) rec.status = kBestSatOut;
    else if (n < 1 || n > A) rec.status = kBestNoRoot;
    if (!sat && D.err[t]) rec.status |= kBestTreeError;
    int mv = -1;
    if (rec.status == 0) {
        int best_i = 0;
        if (n > 1) {
            double best = 0.0;
            best_i = -1;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = lane + 64 * r;
                if (i < n) {
                    const double v = (double)D.ch_visits[base + i];
                    if (best_i < 0 || v > best) { best = v; best_i = i; }
                }
            }
            best_i = wave_argmax_first(best, best_i);
            if (best_i < 0 || best_i >= n) best_i = 0;                 // (visit counts are never NaN: an index stays inside the root's children whatever happens)
        }
        const int bvis = D.ch_visits[base + best_i];
        const double vsum = D.ch_vsum[base + best_i];
        const double value = bvis == 0 ? 0.5 : vsum / (double)bvis;
        mv = n == 1 ? 0 : (value < resign_threshold ? -1 : (int)D.action[base + best_i]);
        rec.num_children = n;
        rec.move = mv;
        rec.best = best_i;
        rec.visits = bvis;
        rec.value_sum = vsum;
        rec.node_visits = D.node[ns].visits;
    }
    if (lane == 0) out[t] = rec;
    if (!play || mv < 0) return;
    BoardScalars b;
    int to_move;
    load_root<S>(L, b, to_move, D, t, lane);
    reset_work<S>(L, lane);
    put_stone<S>(L, b, mv, to_move, D.zob, lane);
    store_root<S>(L, b, 3 - to_move, D, t, D.superko != 0, false, false, lane);
}

// ---- tree reuse in lock-step matches: every root advanced by a move on the device (tg_search_advance) ----
// One wavefront per tree.  moves[t] < 0: the tree and its position are left alone (roots[t] = -1).  Otherwise the root edge
// whose action is the move is looked for (lanes striding over the root's children, as best_moves_kernel reads a root; a root's
// actions are distinct), the move is played on the root position as play_kernel plays it, and
//   - the edge has an expanded child: roots[t] = that node - the reroot kernels queued behind this one make its subtree the
//     tree (num_nodes is put back for them: store_root writes the record of a position without a tree);
//   - else (no such edge, an unexpanded one, a tree without a root or with its error word set): the tree is FRESH - num_nodes
//     0, the leaf queue emptied, roots[t] = -1.
// A move onto a point that is not empty (a stone, the border) is not played: the tree's sticky error word gets kErrOccupied and
// nothing else of the tree changes.  out[t]: tg_readout::AdvanceRec but for kept_nodes, which advance_nodes_kernel fills in
// behind the reroot.
template <int S>
__global__ __launch_bounds__(64) void advance_kernel(SearchDev D, const int32_t *moves, int32_t *roots, AdvanceRec *out) {
    using G = Geo<S>;
    using namespace tg_readout;
    constexpr int A = G::A, R = (A + 63) / 64;
    __shared__ Lds<S> L;
    const int t = blockIdx.x, lane = threadIdx.x;
    const int mv = moves[t];
    AdvanceRec rec{-1, 0, 0, 0};
    if (mv < 0 || mv >= G::NC) {                                       // (wave-uniform, like everything that branches below)
        rec.status = kAdvanceLeftAlone;
        if (lane == 0) { roots[t] = -1; out[t] = rec; }
        return;
    }
    if (mv > 0 && D.root_cells[(size_t)t * G::NC + mv] != kEmpty) {
        rec.status = kAdvanceOccupied;
        if (lane == 0) { atomicOr(&D.err[t], kErrOccupied); roots[t] = -1; out[t] = rec; }
        return;
    }
    const size_t ns = (size_t)t * D.N, base = ns * A;
    const int n_nodes = D.meta[t].num_nodes;
    int nc = (n_nodes > 0 && D.err[t] == 0) ? D.node[ns].children : 0;
    if (nc < 0 || nc > A) nc = 0;
    int edge = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        if (i < nc && (int)D.action[base + i] == mv) edge = i;
    }
    edge = max(edge, lane_partner_i32<0>(edge));
    edge = max(edge, lane_partner_i32<1>(edge));
    edge = max(edge, lane_partner_i32<2>(edge));
    edge = max(edge, lane_partner_i32<3>(edge));
    edge = max(edge, lane_partner_i32<4>(edge));
    edge = max(edge, lane_partner_i32<5>(edge));
    int child = edge >= 0 ? D.ch_index[base + edge] : kNotExpanded;
    const bool kept = child > 0 && child < n_nodes;                    // (node 0 is the root: never a child)
    if (kept) {
        rec.kept_visits = D.node[ns + child].visits;
        rec.num_children = D.node[ns + child].children;
    }
    BoardScalars b;
    int to_move;
    load_root<S>(L, b, to_move, D, t, lane);
    reset_work<S>(L, lane);
    put_stone<S>(L, b, mv, to_move, D.zob, lane);
    store_root<S>(L, b, 3 - to_move, D, t, D.superko != 0, false, false, lane);
    if (lane == 0) {
        if (kept) D.meta[t].num_nodes = n_nodes;
        D.n_leaves[t] = 0;
        roots[t] = kept ? child : -1;
        out[t] = rec;
    }
}

// ... and behind the reroot: what each kept tree holds now
__global__ void advance_nodes_kernel(SearchDev D, const int32_t *roots, AdvanceRec *out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < D.T && roots[t] >= 0) out[t].kept_nodes = D.meta[t].num_nodes;
}

// The trees whose visit budget is spent are halted (tg_search_budget_rule; the rule itself: visit_budget.h), so that
// compaction drops them: stop_rule_kernel's conventions - a tree that is halted, in error or without a root is
// left alone and is not live; one that halts records the root's visits in stopped_at; one that goes on counts into *live.
__global__ void budget_rule_kernel(SearchDev D, const int32_t *total, int32_t *stopped_at, int32_t *live) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= D.T || D.halt[t] != 0 || D.err[t] != 0 || D.meta[t].num_nodes <= 0) return;
    const int32_t visits = D.node[(size_t)t * D.N].visits;
    if (tg_budget::spent(total[t], visits)) {
        D.halt[t] = 1;
        stopped_at[t] = visits;
    } else {
        atomicAdd(live, 1);
    }
}

// the draw cursors into pinned host memory (self-play: read by the host a root evaluation later - no copy, no copy stream)
__global__ void publish_cursors_kernel(const int64_t *cursor, int64_t *out, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < T) out[t] = cursor[t];
}

// ---- halt words and the early stop of a CONSTANT_PLAYOUT search on the device (the rule itself: stop_rule.h) ----
// host-set words: mask[t] != 0 halts tree t, a zero entry leaves its word alone
// (a word that was clear gets stopped_at 0: the host halted the tree, not the rule)
__global__ void set_halt_kernel(SearchDev D, const uint8_t *mask, int32_t *stopped_at) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < D.T && mask[t] && D.halt[t] == 0) {
        D.halt[t] = 1;
        stopped_at[t] = 0;
    }
}

template <int STEP>
__device__ __forceinline__ tg_stop::Top2 top2_step(tg_stop::Top2 a) {
    const tg_stop::Top2 b{lane_partner_i32<STEP>(a.first), lane_partner_i32<STEP>(a.second)};
    return tg_stop::merge(a, b);
}

// is_move_decided (time_manager.py:146-163) for the root of every tree, one wavefront per tree: the two largest child visit
// counts over all A slots (unused slots hold 0; a lane takes ceil(A / 64) of them, the last pass tail-masked; then a butterfly
// over (first, second) pairs), halt[t] = 1 iff total[t] - root visits < first - second.  A tree that halts records the root's
// visits in stopped_at; one that goes on adds itself to *live.  Trees already halted, in error or without a root are left
// alone and are not live.  total: host-mapped, constant while launches that read it are queued.
template <int S>
__global__ __launch_bounds__(64) void stop_rule_kernel(SearchDev D, const int32_t *total, int32_t *stopped_at, int32_t *live) {
    constexpr int A = Geo<S>::A, R = tg_stop::passes(A);
    const int t = blockIdx.x, lane = threadIdx.x;
    if (D.halt[t] != 0 || D.err[t] != 0 || D.meta[t].num_nodes <= 0) return;      // (wave-uniform)
    const size_t root_ns = (size_t)t * D.N, root_base = root_ns * A;
    tg_stop::Top2 top{0, 0};
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + tg_stop::kLanes * r;
        if (i < A) top = tg_stop::push(top, D.ch_visits[root_base + i]);
    }
    top = top2_step<0>(top);
    top = top2_step<1>(top);
    top = top2_step<2>(top);
    top = top2_step<3>(top);
    top = top2_step<4>(top);
    top = top2_step<5>(top);
    if (lane == 0) {
        const int32_t visits = D.node[root_ns].visits;
        if (tg_stop::decided(total[t], visits, top)) {
            D.halt[t] = 1;
            stopped_at[t] = visits;
        } else {
            atomicAdd(live, 1);
        }
    }
}

// Live ranks (the rule itself: live_rank.h): rank[t] = the live trees before tree t, -1 for a tree the PUCT
// selectors pass by; *count = the live trees.  ONE workgroup of kChunk threads takes the trees a chunk at a time: a wavefront
// scans its 64 flags, the wave totals go through LDS and every thread adds up those of the wavefronts before its own, the
// chunk's total carries into the next chunk.  One launch, plain vector stores.
__global__ __launch_bounds__(tg_live::kChunk) void live_rank_kernel(SearchDev D, int32_t *rank, int32_t *count) {
    using tg_live::Rule;
    __shared__ int32_t wave_total[tg_live::kWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int32_t carry = 0;
    for (int c0 = 0; c0 < D.T; c0 += tg_live::kChunk) {
        const int t = c0 + (int)threadIdx.x;
        const int32_t own = t < D.T && tg_live::live(D.err[t], D.halt[t], D.meta[t].num_nodes) ? 1 : 0;
        const int32_t inclusive = wave_scan_add_i32(own);
        if (lane == 63) wave_total[wid] = inclusive;
        __syncthreads();
        int32_t waves_before = 0, chunk_total = 0;
#pragma unroll
        for (int w = 0; w < tg_live::kWaves; ++w) {
            const int32_t n = wave_total[w];
            if (w < wid) waves_before += n;
            chunk_total += n;
        }
        if (t < D.T) rank[t] = Rule::rank(own, carry, waves_before, Rule::before(inclusive, own));
        carry = Rule::next_carry(carry, chunk_total);
        __syncthreads();                                   // (wave_total is written again for the next chunk)
    }
    if (threadIdx.x == 0) *count = carry;
}

// Grouped ranks (the rule itself: group_rank.h): the live trees sorted by group[t] in [0, G) - a stable counting
// sort.  rank[t] = offset[group[t]] + the live trees of its group before tree t, -1 for a tree the PUCT selectors pass by;
// count[g] = the live trees of group g.  ONE workgroup of kChunk threads, live_rank_kernel's form, the trees taken twice: a
// counting pass, the offsets, an assigning pass.  A wavefront takes one ballot per distinct group among its 64 trees: the
// lanes below a tree give its position within the group, the whole ballot the wave's total for it.  Plain vector stores.
__device__ __forceinline__ int32_t group_ballots(bool own, int g, int lane, int32_t *wave_row) {
    int32_t upto = 0, total = 0;                           // (total: lane l keeps the wave's total of group l)
    unsigned long long todo = __ballot(own);
    while (todo) {                                         // (wave-uniform)
        const int leader = __ffsll((long long)todo) - 1;
        const int gl = __shfl(g, leader);
        const unsigned long long same = __ballot(own && g == gl);
        if (own && g == gl) upto = __popcll(same & ((2ull << lane) - 1ull));
        if (lane == gl) total = __popcll(same);
        todo &= ~same;
    }
    wave_row[lane] = total;
    return upto;
}

__global__ __launch_bounds__(tg_group::kChunk) void group_rank_kernel(SearchDev D, const int32_t *group, int G, int32_t *rank,
                                                                       int32_t *count) {
    using tg_group::Rule;
    constexpr int kG = tg_group::kMaxGroups;
    __shared__ int32_t wave_total[tg_group::kWaves][kG];
    __shared__ int32_t chunk_total[kG], carry[kG], placed[kG];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    auto flags = [&](int t, int *g) {
        *g = t < D.T ? group[t] : -1;
        return t < D.T && tg_group::ranked(tg_live::live(D.err[t], D.halt[t], D.meta[t].num_nodes), *g, G);
    };
    if (tid < kG) carry[tid] = placed[tid] = 0;
    // ---- counting pass
    for (int c0 = 0; c0 < D.T; c0 += tg_group::kChunk) {
        int g;
        const bool own = flags(c0 + tid, &g);
        (void)group_ballots(own, g, lane, wave_total[wid]);
        __syncthreads();
        if (tid < kG) {
            int32_t n = 0;
#pragma unroll
            for (int w = 0; w < tg_group::kWaves; ++w) n += wave_total[w][tid];
            carry[tid] += n;
        }
        __syncthreads();                                   // (wave_total is written again for the next chunk)
    }
    // ---- offsets: the counts scanned in place order by the first wavefront
    if (tid < G) {
        count[tid] = carry[tid];
        placed[Rule::place(tid, G)] = carry[tid];
    }
    __syncthreads();
    if (wid == 0) {
        const int32_t n = placed[lane];
        chunk_total[lane] = Rule::offset(wave_scan_add_i32(n), n);      // (chunk_total: scratch for the segment starts)
    }
    __syncthreads();
    if (tid < G) carry[tid] = chunk_total[Rule::place(tid, G)];
    __syncthreads();
    // ---- assigning pass
    for (int c0 = 0; c0 < D.T; c0 += tg_group::kChunk) {
        const int t = c0 + tid;
        int g;
        const bool own = flags(t, &g);
        const int32_t upto = group_ballots(own, g, lane, wave_total[wid]);
        __syncthreads();
        if (own) {
            int32_t waves_before = 0;
#pragma unroll
            for (int w = 0; w < tg_group::kWaves; ++w)
                if (w < wid) waves_before += wave_total[w][g];
            rank[t] = Rule::rank(carry[g], waves_before, Rule::within(upto));
        } else if (t < D.T) {
            rank[t] = tg_group::kNotLive;
        }
        if (tid < kG) {
            int32_t n = 0;
#pragma unroll
            for (int w = 0; w < tg_group::kWaves; ++w) n += wave_total[w][tid];
            chunk_total[tid] = n;
        }
        __syncthreads();                                   // (every rank of the chunk has read its carry)
        if (tid < G) carry[tid] = Rule::next_carry(carry[tid], chunk_total, tid, G);
        __syncthreads();                                   // (wave_total and chunk_total are written again for the next chunk)
    }
}

// Rows by rank: the root evaluation writes tree t's planes to row t, a grouped forward pass wants them at row
// rank[t], and its outputs back at row t.  GATHER: dst[rank[t]] = src[t]; else dst[t] = src[rank[t]]; a tree without a rank is
// skipped either way.  One wavefront per tree, 16 bytes a lane where the rows allow, declared with the alignment ALIGN that
// really holds for a row's start (rows of 6 P, P + 1 or 3 floats are no multiple of 16 bytes), a tail of up to three floats.
template <int ALIGN>
struct RowVec;
template <>
struct RowVec<16> {
    typedef float type __attribute__((ext_vector_type(4), aligned(16)));
};
template <>
struct RowVec<8> {
    typedef float type __attribute__((ext_vector_type(4), aligned(8)));
};
template <>
struct RowVec<4> {
    typedef float type __attribute__((ext_vector_type(4), aligned(4)));
};
constexpr int kRowWaves = 4;
template <bool GATHER, int ALIGN>
__global__ __launch_bounds__(64 * kRowWaves) void rows_by_rank_kernel(const float *src, float *dst, const int32_t *rank, int T,
                                                                       int row_floats) {
    using V = typename RowVec<ALIGN>::type;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kRowWaves + (threadIdx.x >> 6), n_waves = gridDim.x * kRowWaves;
    const int n16 = row_floats / 4, tail = row_floats - 4 * n16;
    for (int t = wave; t < T; t += n_waves) {
        const int32_t r = rank[t];
        if (r < 0 || r >= T) continue;                     // (a rank is below the live count, which is at most T)
        const float *from = src + (size_t)(GATHER ? t : r) * row_floats;
        float *to = dst + (size_t)(GATHER ? r : t) * row_floats;
        for (int i = lane; i < n16; i += 64) reinterpret_cast<V *>(to)[i] = reinterpret_cast<const V *>(from)[i];
        if (lane < tail) to[4 * n16 + lane] = from[4 * n16 + lane];
    }
}

// ---- whole-tree read-out (the layout, the scan rule and the digest rule: tree_dump.h) ----
// The trees of a call: `trees` lists n tree indices (any subset in any order, no duplicates: the host checked), null: tree j
// is list entry j.  The current root of a device tree is node 0 (a reroot compacts the kept subtree to the front).
constexpr int kDumpCurrentRoot = 0;
__device__ __forceinline__ int dump_tree(const int32_t *trees, int j) { return trees ? trees[j] : j; }

// first[j][i] = the children of the nodes before node i of listed tree j (exclusive scan), sizes[j] = {num_nodes, total}.  ONE
// workgroup of kChunk threads per listed tree takes the nodes a chunk at a time (live_rank_kernel's form): a wavefront scans
// its 64 counts, the wave totals go through LDS, the chunk's total carries into the next chunk.  Plain vector stores.
__global__ __launch_bounds__(tg_dump::kChunk) void dump_scan_kernel(SearchDev D, int A, const int32_t *trees, int64_t *first,
                                                                    int64_t *sizes) {
    using tg_dump::ScanRule;
    __shared__ int32_t wave_total[tg_dump::kWaves];
    const int j = blockIdx.x, t = dump_tree(trees, j);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = tg_dump::clamp_nodes(D.meta[t].num_nodes, D.N);
    const NodeRec *node = D.node + (size_t)t * D.N;
    int64_t *out = first + (size_t)j * D.N;
    int64_t carry = 0;
    for (int c0 = 0; c0 < n; c0 += tg_dump::kChunk) {
        const int i = c0 + (int)threadIdx.x;
        const int32_t own = i < n ? tg_dump::clamp_children(node[i].children, A) : 0;
        const int32_t inclusive = wave_scan_add_i32(own);
        if (lane == 63) wave_total[wid] = inclusive;
        __syncthreads();
        int32_t waves_before = 0, chunk_total = 0;
#pragma unroll
        for (int w = 0; w < tg_dump::kWaves; ++w) {
            const int32_t s = wave_total[w];
            if (w < wid) waves_before += s;
            chunk_total += s;
        }
        if (i < n) out[i] = ScanRule::first(carry, waves_before, ScanRule::before(inclusive, own));
        carry = ScanRule::next_carry(carry, chunk_total);
        __syncthreads();                                   // (wave_total is written again for the next chunk)
    }
    if (threadIdx.x == 0) {
        sizes[2 * j] = n;
        sizes[2 * j + 1] = carry;
    }
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, step);
    return v;
}

// The walk over the nodes of the listed trees, one wavefront per node, grid-stride (blockIdx.y over the list, blockIdx.x and
// the workgroup's wavefronts over a tree's nodes).  PACK: the wavefront writes the node's DumpNode and, for each child array,
// copies the node's `children` entries to the packed row, a lane per child, as many passes as `children` takes - only the used
// part of the [A]-strided pool row is read; plain vector loads and stores.  DIGEST: it sums the terms of its nodes in
// registers and adds them to the tree's two words once at its end (64-bit adds on device memory, the only atomics; the host
// zeroed the words in front of the launch and applies the finaliser behind it).
constexpr int kDumpWaves = 4;
template <bool PACK, bool DIGEST>
__global__ __launch_bounds__(64 * kDumpWaves) void dump_walk_kernel(SearchDev D, int A, const int32_t *trees, int n_list,
                                                                     const int64_t *first, const int64_t *sizes, const int64_t *rec_at,
                                                                     unsigned char *out, unsigned long long *sums) {
    using tg_dump::DigestRule;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const bool tree_wave = blockIdx.x == 0 && wid == 0;       // the wavefront that speaks for the tree as a whole
    for (int j = blockIdx.y; j < n_list; j += gridDim.y) {
        const int t = dump_tree(trees, j);
        // (PACK: the node count the scan saw - the record's layout was computed from it)
        const int n = PACK ? (int)sizes[2 * j] : tg_dump::clamp_nodes(D.meta[t].num_nodes, D.N);
        const size_t total = PACK ? (size_t)sizes[2 * j + 1] : 0;
        unsigned char *rec = PACK ? out + rec_at[j] : nullptr;
        tg_dump::Sums acc;
        if (tree_wave && lane == 0) {
            if constexpr (PACK) {
                int32_t *head = reinterpret_cast<int32_t *>(rec);
                head[tg_dump::kHeadNumNodes] = n;
                head[tg_dump::kHeadCurrentRoot] = kDumpCurrentRoot;
                head[tg_dump::kHeadErr] = D.err[t];
                head[tg_dump::kHeadToMove] = D.meta[t].to_move;
                head[tg_dump::kHeadTotalLo] = (int32_t)(uint32_t)total;
                head[tg_dump::kHeadTotalHi] = (int32_t)(uint32_t)((uint64_t)total >> 32);
                head[tg_dump::kHeadPad0] = 0;
                head[tg_dump::kHeadPad1] = 0;
            }
            if constexpr (DIGEST) tg_dump::add_tree_terms<DigestRule>(acc, n, kDumpCurrentRoot);
        }
        for (int i = blockIdx.x * kDumpWaves + wid; i < n; i += gridDim.x * kDumpWaves) {
            const size_t ns = (size_t)t * D.N + i, base = ns * A;
            const NodeRec r = D.node[ns];
            const int32_t c = tg_dump::clamp_children(r.children, A);
            int64_t at = 0;
            if constexpr (PACK) at = first[(size_t)j * D.N + i];
            if (lane == 0) {
                if constexpr (PACK) {
                    tg_dump::DumpNode d;
                    d.visits = r.visits, d.vl = r.vl, d.vsum_bits = __float_as_uint(r.vsum), d.raw_bits = __float_as_uint(r.raw);
                    d.children = c, d.parent = r.parent, d.pedge = r.pedge, d.pad = 0, d.first_child = at;
                    *reinterpret_cast<tg_dump::DumpNode *>(rec + tg_dump::node_offset(i)) = d;
                }
                if constexpr (DIGEST) tg_dump::add_node_terms<DigestRule>(acc, i, r, c);
            }
            const int32_t used = DigestRule::used(c, A);
            for (int k = lane; k < used; k += 64) {
#define WALK(field, E, per_child, remap)                                                                                         \
                {                                                                                                                \
                    const E v = D.field[base + k];                                                                               \
                    if constexpr (PACK)                                                                                          \
                        if ((uint64_t)(at + k) < total)          /* (always: the scan counted these children) */               \
                            record_row<std::conditional_t<sizeof(E) == 8, E, int32_t>>(rec, tg_dump::row_offset(tg_pool::k_##field, n, total))[at + k] = v; \
                    if constexpr (DIGEST) acc.add<DigestRule>(tg_dump::kFieldArrays + tg_pool::k_##field, i, k, tg_dump::bits_of(v)); \
                }
                TG_NODE_POOL_CHILD_ARRAYS(WALK)
#undef WALK
            }
        }
        if constexpr (DIGEST) {
            const uint64_t s0 = wave_sum_u64(acc.s[0]), s1 = wave_sum_u64(acc.s[1]);
            if (lane == 0 && (s0 | s1)) {
                atomicAdd(&sums[2 * j], (unsigned long long)s0);
                atomicAdd(&sums[2 * j + 1], (unsigned long long)s1);
            }
        }
    }
}

// ---- whole-tree write-in (which records may enter: tree_load.h check_record, applied on the host) ----
// The inverse of the walk: one wavefront per node of every listed tree (dump_walk_kernel's grid shape).  The wavefront reads
// the node's DumpNode out of the record, writes the NodeRec and, for each child array, scatters the node's entries into the
// [A]-strided pool row, a lane per entry, as many passes as A takes: below `children` from the packed row (action narrowed to
// int16), at and beyond it the canonical tail - what expand_node leaves in a fresh row.  Whatever the host said, node counts
// and child counts are clamped to the pool (clamp_nodes / clamp_children) and a packed row is read within `total` only.  The
// wavefront that speaks for the tree sets num_nodes, empties the leaf queue and clears the noise row, the error word and the
// halt word.  A record whose side to move is not the tree's root position's (meta[t].to_move, which the load never writes) is
// refused by every wavefront alike: flags[j] = 1, nothing of the tree written.  Plain vector loads and stores.
__global__ __launch_bounds__(64 * kDumpWaves) void load_walk_kernel(SearchDev D, int A, const int32_t *trees, int n_list,
                                                                     const int64_t *rec_at, const unsigned char *in, int32_t *flags,
                                                                     int32_t *stopped_at) {
    using tg_load::FillRule;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const bool tree_wave = blockIdx.x == 0 && wid == 0;
    for (int j = blockIdx.y; j < n_list; j += gridDim.y) {
        const int t = dump_tree(trees, j);
        const unsigned char *rec = in + rec_at[j];
        const int32_t *head = reinterpret_cast<const int32_t *>(rec);
        const int n = tg_dump::clamp_nodes(head[tg_dump::kHeadNumNodes], D.N);
        const bool refused = n > 0 && head[tg_dump::kHeadToMove] != D.meta[t].to_move;      // (wave-uniform)
        if (tree_wave && lane == 0) flags[j] = refused ? 1 : 0;
        if (refused) continue;
        const size_t total = (size_t)((uint64_t)(uint32_t)head[tg_dump::kHeadTotalLo] | ((uint64_t)(uint32_t)head[tg_dump::kHeadTotalHi] << 32));
        if (tree_wave) {
            for (int i = lane; i < A; i += 64) D.noise[(size_t)t * A + i] = 0.0;
            if (lane == 0) {
                D.meta[t].num_nodes = n;
                D.n_leaves[t] = 0;
                D.err[t] = 0;
                D.halt[t] = 0;
                if (stopped_at) stopped_at[t] = 0;
            }
        }
        for (int i = blockIdx.x * kDumpWaves + wid; i < n; i += gridDim.x * kDumpWaves) {
            const size_t ns = (size_t)t * D.N + i, base = ns * A;
            const tg_dump::DumpNode d = *reinterpret_cast<const tg_dump::DumpNode *>(rec + tg_dump::node_offset(i));
            const int32_t c = tg_dump::clamp_children(d.children, A);
            if (lane == 0) {
                NodeRec r;
                r.visits = d.visits, r.vl = d.vl, r.vsum = __uint_as_float(d.vsum_bits), r.raw = __uint_as_float(d.raw_bits);
                r.children = c, r.parent = d.parent, r.pedge = d.pedge, r.pad = 0;
                D.node[ns] = r;
            }
            const int64_t at = d.first_child;
            for (int k = lane; k < A; k += 64) {
#define FILL(field, E, per_child, remap)                                                                                         \
                {                                                                                                                \
                    using Wd = std::conditional_t<sizeof(E) == 8, E, int32_t>;                                                   \
                    E v = tg_load::tail_value<E>(tg_pool::k_##field);                                                            \
                    if (FillRule::from_record(k, c) && (uint64_t)(at + k) < total)   /* (always: the host checked the scan) */   \
                        v = (E) reinterpret_cast<const Wd *>(rec + tg_dump::row_offset(tg_pool::k_##field, n, total))[at + k];   \
                    D.field[base + k] = v;                                                                                       \
                }
                TG_NODE_POOL_CHILD_ARRAYS(FILL)
#undef FILL
            }
        }
    }
}

// the owners of the handles' buffers, events and streams (host only: included behind the kernels)
#include <memory>

#include "host_resources.h"
#include "search_plan.h"
#include "stream_windows.h"

static_assert(tg_plan::kPipeMaxLeaves == kPipeMaxK && tg_plan::kGumbelPipeMaxN == kPipeMaxK / 2 && tg_plan::kSplitMaxTrees == kXwMaxTrees,
              "search_plan.h restates the kernels' limits");

// Where a phase's leaves go (the public slots_per_tree, decoded once at the C entry points: leaf_layout): tree t's at
// t * slots_per_tree; packed behind each other (0); or each tree's DISTINCT leaves in a plane range of its own (-1).
// Compact has no slots_per_tree code: the compact PUCT entry points ask for it - live tree t's leaves at
// rank[t] * slots_per_tree, the trees the selectors pass by compacted away
enum class LeafLayout { Strided, Packed, Unique, Compact };

struct tg_search {
    tg_search_config cfg{};
    SearchDev dev{};                       // what the kernels get, by value: borrows from `allocs` and the owners below
    int num_cus = 256;
    int S = 0, W = 0, NC = 0, P = 0, A = 0, HMAX = 0;
    std::vector<tg::DevBuf<unsigned char>> allocs;       // SearchDev's arrays (dev_alloc; tg_search_grow swaps the pool's)
    hipStream_t last_stream = nullptr;
    bool stream_known = false;             // a launch has named its stream (which may be the null stream: last_stream == nullptr)

    // ---- staged roots: a position set by the host (tg_search_set_root) waits here until a launch needs the roots (flush_roots:
    // all of them) or a reroot takes its tree's; a root written on the device meanwhile (records, policy games) drops it.
    // Uploads go out of a pinned mirror (a copy out of pageable memory makes the host wait for the stream: self-play queues this
    // behind a whole move's kernels) of one slot, [cells | history, 8-byte aligned | RootMeta]: begin() waits for its last upload.
    class StagedRoots {
    public:
        void create(int T, int NC, int HMAX);
        // tree's position becomes this one: m, NC cells, m.hist_len words of history (null: one word, 0)
        void stage(int tree, const RootMeta &m, const uint8_t *cells, const uint64_t *history);
        bool any() const { return n_dirty_ > 0; }
        bool staged(int tree) const { return dirty_[tree] != 0; }
        void drop(int tree) { n_dirty_ -= dirty_[tree]; dirty_[tree] = 0; }
        void drop_all() { std::fill(dirty_.begin(), dirty_.end(), 0); n_dirty_ = 0; }
        // Uploads on `st`, between begin() and end(st).  upload, the only per-tree one: tree's staged position - cells and
        // (superko) history to D's root arrays, the RootMeta to meta_dst; take: and it is staged no longer.  upload_all: every
        // staged position to D's roots (three copies when every tree has one), begin and end included; none is staged after.
        int begin();
        int upload(int tree, const SearchDev &D, RootMeta *meta_dst, hipStream_t st);
        int take(int tree, const SearchDev &D, RootMeta *meta_dst, hipStream_t st) {
            const int rc = upload(tree, D, meta_dst, st);
            if (rc == TG_OK) drop(tree);
            return rc;
        }
        int end(hipStream_t st) { return pin_.commit(0, st); }
        int upload_all(const SearchDev &D, hipStream_t st);

    private:
        std::vector<uint8_t> cells_, dirty_;      // [T][NC]; [T] 1: staged
        std::vector<uint64_t> hist_;              // [T][HMAX]
        std::vector<RootMeta> meta_;              // [T]
        int n_dirty_ = 0;
        size_t NC_ = 0, HMAX_ = 0, hist_at_ = 0, meta_at_ = 0;     // a tree's strides; where the mirror's history and metas start
        tg::StagingRing<uint8_t, 1> pin_;
        uint8_t *m_cells_ = nullptr;              // the mirror, from begin()
        uint64_t *m_hist_ = nullptr;
        RootMeta *m_meta_ = nullptr;
    } roots;
    // roots written from game records (tg_search_set_roots_from_records): one call's inputs, pinned and on the device, and the
    // per-tree flags on their way back; the call returns with its stream idle, so the next one finds them free
    tg::PinBuf<uint8_t> rec_stage;
    tg::DevBuf<uint8_t> rec_in;
    size_t rec_cap = 0;
    tg::DevBuf<int32_t> rec_flags;                // [T]
    tg::PinBuf<int32_t> rec_flags_back;           // pinned [T]

    // ---- halt words (SearchDev::halt) and the stop rule's buffers, allocated when halting is first used
    struct Halting {
        bool armed = false;                       // a word may be non-zero: the next root reset clears them (clear_halt)
        tg::PinBuf<uint8_t> mask;                 // host-mapped [T]: tg_search_set_halt's argument, read by set_halt_kernel
        tg::PinBuf<int32_t> total;                // host-mapped [T]: the visit totals the rule launches read
        tg::Event inputs_read;                    // behind the last launch that reads mask / total
        tg::DevBuf<int32_t> stopped_at;           // [T] root visits when the rule halted the tree
        tg::DevBuf<int32_t> live;                 // one counter per rule launch of a call
        tg::PinBuf<int32_t> live_back;            // pinned [1]: a counter on its way to the host
    } halting;
    // ---- live ranks (SearchDev::rank in the compact launches), allocated when compaction is first used.
    // Fresh: no call has written a halt word or reset a root since live_rank_kernel was queued.  Shrunk: halt words were SET
    // since (tg_search_set_halt, the stop rule) - the live set only lost trees, so every tree the selectors take still has
    // its rank, and a halted one an idle slot.  Stale: a root was reset since, a tree may be live without a rank.
    struct LiveRanks {
        enum class State { Stale, Shrunk, Fresh } state = State::Stale;
        tg::DevBuf<int32_t> rank;                 // [T] + the live count behind it
        size_t T = 0;
        int32_t *count() { return rank.get() + T; }
        void mark_shrunk() { if (state == State::Fresh) state = State::Shrunk; }
        void mark_stale() { state = State::Stale; }
        bool usable(bool shrunk_ok) const { return state == State::Fresh || (shrunk_ok && state == State::Shrunk); }
        // GROUPED: the table in force is group_rank_kernel's - the live trees sorted by group; count / offset
        // are the segments as the host read them.  live_rank_kernel replaces it with plain live ranks (launch_live_rank).
        bool grouped = false;
        int n_groups = 0;
        int32_t group_count[tg_group::kMaxGroups] = {}, group_offset[tg_group::kMaxGroups] = {};
        tg::PinBuf<int32_t> group_in;             // host-mapped [T]: tg_search_group_live's argument, read by group_rank_kernel
        tg::DevBuf<int32_t> group_count_dev;      // [kMaxGroups]
        tg::PinBuf<int32_t> group_count_back;     // pinned [kMaxGroups]: the counts on their way to the host
    } ranks;
    // A best-effort guard of tg_search_puct_chain_early, kept by the host calls alone: set when tg_search_root_planes is QUEUED
    // (the expansion itself ends with the backup behind it, which the host does not see), dropped by the calls of this API
    // that replace or move roots (staged roots, roots from records, tg_search_play, tg_search_best_moves(play)).  The self-play
    // handle's own moves (launch_finish_roots + launch_play) do not drop it: they are followed by a root launch before any
    // search, and the early chain is not offered on that path.
    bool roots_expanded = false;

    // ---- random windows: double-buffered, filled on a private copy stream so that the host can
    // prepare mini-batch j+1 while the forward pass of mini-batch j runs ----
    tg::Stream copy_stream;
    tg::Event ev_sel;                             // behind the last selection launch (tg_search_rng_consumed)
    tg::PinBuf<int64_t> consumed_pin;             // host-mapped [T]: the kernels' mirror of the cursors (SearchDev::cursor_pub)

    // The streams' owner: per tree the MT19937 state at the stream's logical position (`base_`) and behind the last generated
    // piece of a window (`cont_`), [T][625] words each, device-resident (csrc/legacy_rng_device.h); windows and Gumbel noise
    // are GENERATED on `copy_stream`, by generate() alone.  The host keeps, per tree, only what it was seeded with until that
    // is uploaded and the stream book (csrc/stream_windows.h): the draws consumed since the device state was last brought up
    // to date go to the next generation launch from the base state through a ring of host-mapped arrays.
    class Windows;
    class Streams {
    public:
        // what the noise draw is ordered behind - every reader of the previous noise: `after`, an event the caller knows to lie
        // behind them; null: everything queued on the launch stream so far (known: a launch has named it), else the device
        struct NoiseOrder {
            hipEvent_t after;
            bool launch_known;
            hipStream_t launch;
        };
        void create(int T, int A, double *noise_dev, hipStream_t copy_stream, const Windows *win) {
            T_ = T, A_ = A, noise_dev_ = noise_dev, cs_ = copy_stream, win_ = win;
        }
        int seed(int tree, const uint32_t *mt_key, int mt_pos);       // (numpy's get_state() layout)
        int seed_all(const uint32_t *seeds);                          // tree t: numpy's RandomState(seeds[t])
        int trees() const { return T_; }
        hipStream_t stream() const { return cs_; }                    // the generation stream
        bool has_stream(int tree) const { return book_.seeded(tree); }
        bool unused(int tree) const { return book_.unused(tree); }    // state() needs no launch
        // tree's state behind everything it consumed.  Precondition: unused(tree), or Windows::complete_rest()
        int state(int tree, uint32_t *mt_key_out, int *mt_pos_out);
        void add_consumed(int tree, int64_t draws, bool skip) { book_.add_consumed(tree, draws, skip); }      // skip: not this stream's draws
        int check_seeded(const char *entry, const uint8_t *skip) const;          // TG_OK: every tree (skip[t] != 0: not looked at) has a stream
        // THE generation launch: dirty seeds go up, a request from the base state takes a lag slot (skip[t] != 0: tree t takes
        // no part) and is refused while a window has columns to come, rng_words_kernel + rng_draws_kernel, the slot committed.
        int generate(const tg_streams::Piece &p, const uint8_t *skip, const NoiseOrder *order);
        // A draws of each tree's stream as root Gumbel noise, into the device's noise rows and on their way to the host's.
        // Precondition: the windows are settled and abandoned - the launch moves the base state
        int draw_noise(const uint8_t *skip, const NoiseOrder &order);
        int host_noise(const double **noise, size_t *count);          // the last root noise [T][A], device-drawn or set
        int clear_host_noise(int tree);                               // a tree's row of the mirror zeroed, as a root reset leaves the device's
        void set_host_noise(const double *noise) { noise_host_.assign(noise, noise + (size_t)T_ * A_); noise_back_pending_ = false; }   // (a device-drawn one on its way back is superseded)

    private:
        int alloc();
        int sync_seeds();
        int order_noise(const NoiseOrder &o);
        int T_ = 0, A_ = 0;
        hipStream_t cs_ = nullptr;
        const Windows *win_ = nullptr;                // asked only: may a base launch go out, where a window's buffer is
        double *noise_dev_ = nullptr;                 // SearchDev::noise [T][A]
        tg_streams::StreamBook book_;
        std::vector<uint32_t> seeds_;                 // [T][625]: what each tree was seeded with (key + pos)
        tg::DevBuf<uint32_t> base_, cont_;
        tg::DevBuf<uint32_t> words_;                  // scratch: the tempered words of the piece being generated (rng_words_kernel)
        tg::DevBuf<int> pos0_;
        tg::DevBuf<uint32_t> snap_;                   // [T][snapshots][624]: state snapshots behind base_ (T <= 64)
        tg::DevBuf<int> snap_n_;
        tg::DevBuf<long long> cont_blk_;
        tg::StagingRing<uint32_t, 1> seed_pin_;       // pinned [T][625]: seeds on their way up, one state on its way down
        tg::StagingRing<long long, 8> lag_ring_;      // host-mapped, per slot [T] lag (int64) then [T] skip (bytes)
        tg::PinBuf<double> noise_back_;               // pinned [T][A]: the device-drawn root noise on its way to noise_host_
        tg::Event noise_back_ev_, noise_order_ev_;
        bool noise_back_pending_ = false;
        std::vector<double> noise_host_;
    } rng;

    // The windows: two buffers and the events behind their last fills, and the window book (csrc/stream_windows.h: the state,
    // its transitions, THE INVARIANT).  Each method carries out what the book's transition of that name returns.
    class Windows {
    public:
        int create(SearchDev *D, size_t draws);
        int start(Streams &gen, int64_t pitch, int64_t cols, int64_t eager) { return carry_out(book_.start(pitch, cols, eager), gen, nullptr, nullptr); }
        int extend(Streams &gen, size_t upto, hipStream_t st) { return carry_out(book_.extend((int64_t)upto), gen, nullptr, st); }
        int complete_rest(Streams &gen) { return carry_out(book_.complete_rest(), gen, nullptr, nullptr); }
        int settle(Streams &gen) { return carry_out(book_.settle(), gen, nullptr, nullptr); }
        int install(Streams &gen, SearchDev *D, hipStream_t st) { return carry_out(book_.install(), gen, D, st); }
        int accept(Streams &gen, const double *host, size_t stride, size_t count);     // (tg_search_set_rng: the host buffer holds a row of `stride` per tree)
        // (the book changes through the transitions above and these two only)
        void abandon() { book_.abandon(); }
        int record(const int64_t *cursor, const uint8_t *skip, int T, int64_t *delta) { return book_.record(cursor, skip, T, delta); }
        const tg_streams::WindowBook &book() const { return book_; }
        double *buffer(int b) const { return buf_[b].get(); }
        hipEvent_t rest_event() const { return ev_[book_.active()].get(); }     // the event the active window's second part is behind

    private:
        int carry_out(const tg_streams::Actions &acts, Streams &gen, SearchDev *D, hipStream_t st);
        tg::DevBuf<double> buf_[2];               // [T][draws per tree] each
        tg::Event ev_[2];                         // behind the last fill of each
        tg_streams::WindowBook book_;
    } win;

    tg::Stream own_stream;                        // tg_search_own_stream: a launch stream of the handle's own (self-play lanes)

    // ---- phase upload (tg_search_select_gumbel) ----
    tg::DevBuf<int32_t> phase_dev;                // [num_considered | max_count | packed leaf offsets], T each
    // pinned staging ring for the phase description: the host never waits for the copy of the current call, only
    // (practically never) for the one kPhaseRing calls ago
    static constexpr int kPhaseRing = 8;
    tg::StagingRing<int32_t, kPhaseRing> phase_pin;
    // the layout of the last selection, which tg_search_backup and tg_search_unique_planes check: of the whole engine or of
    // a self-play move's sub-groups (whose ranges are theirs alone), and for a UNIQUE one the planes its forward pass must
    // cover and each tree's share (host arithmetic)
    struct LastSelection {
        bool subgroups = false;
        LeafLayout layout = LeafLayout::Strided;
        int64_t planes = 0;
        std::vector<int32_t> caps;
        bool whole(LeafLayout l) const { return !subgroups && layout == l; }
    } last;

    // ---- per-move uploads ----
    // pinned staging rings for the small per-move uploads (root noise, chosen moves): queued on the launch stream behind
    // the kernels that still read the old contents - the host does not wait for the stream (it used to: a pipeline drain
    // per upload, twice per self-play move)
    static constexpr int kPinRing = 4;
    tg::StagingRing<double, kPinRing> noise_pin;
    tg::StagingRing<int32_t, kPinRing> moves_pin;
    tg::DevBuf<int32_t> moves_dev;
    // finish_roots_kernel (self-play: the move decided on the device): per-tree state uploads, the event behind its records
    tg::PinBuf<int64_t> cur_pin;                  // publish_cursors_kernel's target (pinned, mapped) + its event
    tg::Event cur_ev;
    tg::DevBuf<int32_t> state_dev;
    tg::StagingRing<int32_t, kPinRing> state_pin;
    tg::Event fin_ev;

    // ---- tg_search_reroot: index map [T][N] and chunk counts [T][chunks] (sized by the pool: released by tg_search_grow), per tree
    // [new root | position staged | old num_nodes | identity] and the staged RootMeta; pinned ring for the per-call upload ----
    tg::DevBuf<int32_t> rr_map, rr_blk, rr_small;
    tg::DevBuf<RootMeta> rr_stage;
    tg::StagingRing<int32_t, kPinRing> rr_pin;

    // ---- tree reuse in lock-step matches ----
    // tg_search_advance: the records [T], device and pinned host (the moves go up through moves_pin into moves_dev, the roots
    // the advance kernel finds into rr_small for the reroot kernels)
    tg::DevBuf<AdvanceRec> adv_dev;
    tg::PinBuf<AdvanceRec> adv_host;
    // visit budgets (tg_search_set_budget): the totals [T] on the device; `on`: in force - the PUCT selection launches get the
    // pointer (SearchDev::budget), every other launch and every launch while off a null one
    struct Budgets {
        bool on = false;
        tg::DevBuf<int32_t> total;
        tg::StagingRing<int32_t, kPinRing> pin;
    } budgets;

    // ---- read-outs: one record per launch, device and pinned host ----
    tg::DevBuf<unsigned char> roots_dev, node_dev, ana_dev;      // gather_roots_kernel / gather_node_kernel / read_analysis_kernel records
    tg::PinBuf<unsigned char> roots_host, node_host, ana_host;
    tg::DevBuf<int32_t> ip_bad_dev;                              // improved_policy_kernel: per tree, "no row" [T]
    tg::PinBuf<int32_t> ip_bad_host;
    tg::DevBuf<BestMove> best_dev;                               // best_moves_kernel: records [T], the caller's sit_out flags [T]
    tg::PinBuf<BestMove> best_host;
    tg::DevBuf<uint8_t> sit_dev;
    tg::StagingRing<uint8_t, kPinRing> sit_pin;
    // ---- whole-tree read-out: the list of trees, the scan's offsets [n][N] and sizes [n][2], where each record
    // starts [n], the digest sums [n][2]; pinned mirrors of the small ones.  Every call ends with its stream idle, so the next
    // one finds them free; all grown on demand (the offsets are sized by the pool: a grown pool asks for more)
    struct TreeDump {
        tg::DevBuf<int32_t> list_dev;
        tg::DevBuf<int64_t> first_dev, small_dev;             // small: sizes [n][2] | rec_at [n] | sums [n][2]
        tg::PinBuf<int32_t> list_pin;
        tg::PinBuf<int64_t> small_pin;
        tg::DevBuf<unsigned char> out_dev;
        size_t pin_cap = 0;                                   // list entries the pinned mirrors hold
    } dump;
    // ---- whole-tree write-in: one call's records, pinned and on the device, and the per-tree flags on their way
    // back (the list and where each record starts go through `dump`'s buffers).  Every call ends with its stream idle
    struct TreeLoad {
        tg::PinBuf<unsigned char> in_pin;
        tg::DevBuf<unsigned char> in_dev;
        size_t in_cap = 0;
        tg::DevBuf<int32_t> flags_dev;
        tg::PinBuf<int32_t> flags_pin;
        size_t flags_cap = 0;
    } load;

    // ---- split-kernel mailboxes ----
    // select_puct_split_kernel: job entries and "node initialised" tags that cross between a tree's workgroups.  The tags
    // carry the launch number (20 bits), so nothing is cleared between launches - only where that number wraps.
    struct SplitMailboxes {
        tg::DevBuf<int> job, done, n;
        tg::DevBuf<unsigned long long> off;
        size_t trees = 0, words = 0;           // words of a job entry (kXwEntryWords<S>)
        int cap = 0;                           // entries per tree
        unsigned seq = 0;
        int per_cu = -1;                       // resident select_puct_split_kernel workgroups per CU (queried once per handle)
        int ensure(int T, int K, int entry_words) {
            if (off.get()) return TG_OK;       // (the last of the four: a failure half-way is made up for by the next call)
            trees = (size_t)T, words = (size_t)entry_words, cap = K < kPipeMaxK ? K : kPipeMaxK;
            int rc;
            if ((rc = job.alloc_zeroed(trees * cap * words)) || (rc = done.alloc_zeroed(trees * cap)) ||
                (rc = n.alloc_zeroed(trees * cap)) || (rc = off.alloc_zeroed(trees * (cap + 1))))
                return rc;
            return TG_OK;
        }
        // the next launch's tag; where the launch number wraps: start from clean buffers, on the launch's stream
        int next_tag(hipStream_t st) {
            if ((++seq & 0xFFFFFu) != 0) return TG_OK;
            TG_HIP(hipMemsetAsync(job.get(), 0, trees * cap * words * sizeof(int), st));
            TG_HIP(hipMemsetAsync(done.get(), 0, trees * cap * sizeof(int), st));
            TG_HIP(hipMemsetAsync(n.get(), 0, trees * cap * sizeof(int), st));
            TG_HIP(hipMemsetAsync(off.get(), 0, trees * (cap + 1) * sizeof(unsigned long long), st));
            seq = 1;
            return TG_OK;
        }
        int tag() const { return (int)((seq & 0xFFFFFu) << 11); }
    } split;
};

namespace {

// one of SearchDev's arrays, zero-filled: owned by s->allocs, borrowed by the device view
template <typename T>
int dev_alloc(tg_search *s, T **out, size_t count) {
    tg::DevBuf<unsigned char> buf;
    if (int rc = buf.alloc_zeroed(count * sizeof(T))) return rc;
    *out = reinterpret_cast<T *>(buf.get());
    s->allocs.push_back(std::move(buf));
    return TG_OK;
}

// the stream a call launches on becomes the handle's launch stream
hipStream_t use_stream(tg_search *s, void *stream) {
    s->last_stream = static_cast<hipStream_t>(stream);
    s->stream_known = true;
    return s->last_stream;
}

// the host waits for the launch stream (no stream named yet, or the null stream: for the device)
int sync_launch_stream(tg_search *s) {
    if (s->last_stream) TG_HIP(hipStreamSynchronize(s->last_stream));
    else TG_HIP(hipDeviceSynchronize());
    return TG_OK;
}

// f(std::integral_constant<int, S>) for the board size the handle was created with (9, 13 or 19: tg_search_create) - for
// the launches of ONE kernel template at the three sizes
template <typename F>
auto with_board_size(int S, F &&f) {
    if (S == 9) return f(std::integral_constant<int, 9>{});
    if (S == 13) return f(std::integral_constant<int, 13>{});
    return f(std::integral_constant<int, 19>{});
}

// Host threads for the per-tree host work of a call (random windows, Gumbel noise, move bookkeeping): a small
// persistent pool (threads created once per process; a job is a [0, n) index range handed out through an atomic
// counter, the caller works along).  Spawning std::threads per call cost 20-30 us each - more than the work of a
// 16-board shard (0.28 ms of serial bookkeeping per lock-step move, TG_SP_TIMING).  One job at a time: a second caller
// (another lock-step group's host thread) finding the pool busy runs its trees itself.
class TreePool {
public:
    static TreePool &get() {
        static TreePool pool;
        return pool;
    }
    int size() const { return (int)workers_.size(); }
    template <typename F>
    bool run(int n, int max_threads, F &fn) {
        std::unique_lock<std::mutex> job(job_mu_, std::try_to_lock);
        if (!job.owns_lock()) return false;
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = [&fn](int t) { fn(t); };
            n_ = n;
            next_.store(0);
            active_ = std::min(max_threads - 1, (int)workers_.size());
            pending_ = active_;
            ++epoch_;
        }
        cv_.notify_all();
        for (int t; (t = next_.fetch_add(1)) < n;) fn(t);
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [&] { return pending_ == 0; });
        fn_ = nullptr;
        return true;
    }

private:
    TreePool() {
        unsigned hw = std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) {
            const int n = CPU_COUNT(&set);
            if (n > 0) hw = (unsigned)n;
        }
        int n = (int)std::min<unsigned>(hw ? hw : 1u, 16u);
        if (const char *env = getenv("TG_HOST_THREADS")) {
            const int cap = atoi(env);
            if (cap >= 1 && cap < n) n = cap;
        }
        for (int w = 0; w + 1 < n; ++w) workers_.emplace_back([this, w] { loop(w); });
    }
    ~TreePool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &th : workers_) th.join();
    }
    void loop(int w) {
        long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return stop_ || epoch_ != seen; });
            if (stop_) return;
            seen = epoch_;
            if (w >= active_) continue;
            lk.unlock();
            for (int t; (t = next_.fetch_add(1)) < n_;) fn_(t);
            lk.lock();
            if (--pending_ == 0) done_cv_.notify_one();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_, job_mu_;
    std::condition_variable cv_, done_cv_;
    std::function<void(int)> fn_;
    std::atomic<int> next_{0};
    int n_ = 0, active_ = 0, pending_ = 0;
    long epoch_ = 0;
    bool stop_ = false;
};

template <typename F>
void parallel_trees(int n, F &&fn) {
    TreePool &pool = TreePool::get();
    // threads worth waking: one per eight trees, from 32 trees on (waking sleeping threads costs ~0.1 ms: at 16 boards
    // the pool made the per-move bookkeeping slower, 0.44 vs 0.28 ms; at 64 boards the shard gained 8 %)
    const int want = n >= 32 ? std::min(pool.size() + 1, n / 8) : 1;
    if (want >= 2 && pool.run(n, want, fn)) return;
    for (int t = 0; t < n; ++t) fn(t);
}

// One pool array [T][n_old * per_node] to be re-allocated as [T][n_new * per_node], keeping every tree's rows.  The
// growth is transactional: every new array is allocated and filled FIRST; only when all of that has
// succeeded are the pointers swapped and the old arrays freed - a failing hipMalloc (old and new pools are resident
// together: up to 2 x 13 GB at the 4 M-node cap) leaves the handle exactly as it was.
struct GrowItem {
    void **field;          // address of the SearchDev pointer
    size_t elem;           // bytes per element
    size_t per_node;       // elements per node
    tg::DevBuf<unsigned char> fresh;
};

int grow_fill(const GrowItem &g, size_t trees, size_t n_old, size_t n_new) {
    const size_t row_old = n_old * g.per_node * g.elem, row_new = n_new * g.per_node * g.elem;
    TG_HIP(hipMemset(g.fresh.get(), 0, trees * row_new));
    if (row_old < ((size_t)1 << 30)) {
        TG_HIP(hipMemcpy2D(g.fresh.get(), row_new, *g.field, row_old, row_old, trees, hipMemcpyDeviceToDevice));
    } else {
        // rows beyond 1 GB (millions of nodes per tree): one linear copy per tree, no 2D pitch limits involved
        for (size_t t = 0; t < trees; ++t)
            TG_HIP(hipMemcpy(g.fresh.get() + t * row_new, static_cast<const unsigned char *>(*g.field) + t * row_old,
                             row_old, hipMemcpyDeviceToDevice));
    }
    return TG_OK;
}

// ---- search launches: search_plan.h chooses, ONE table holds the instantiations -----------------------

// What the plan functions are asked with: the handle's shape, the launch's, and every selection knob - read HERE and
// nowhere else.  TG_SELECT_SPLIT, TG_SPLIT_TEST_MUTE and TG_GUMBEL_ONE_BY_ONE per call (tests toggle them inside one
// process), the others once per process; all through tg::knob but TG_SHARED_DEVICE, which a deployment sets.
// launch_trees: the engine's or a slice's (sub_dev); most: max_leaves (PUCT) / the most descents a tree of the launch makes
struct LaunchContext { tg_plan::PlanInputs in; tg_plan::SearchKnobs knobs; };

LaunchContext launch_context(const tg_search *s, int launch_trees, int most, bool unique) {
    static const tg_plan::SearchKnobs once = [] {
        const auto number = [](const char *name, int unset) { const char *v = tg::knob(name); return v ? atoi(v) : unset; };
        tg_plan::SearchKnobs k;
        k.serial = tg::knob("TG_SELECT_SERIAL") != nullptr;
        k.mpipe_prof = tg::knob("TG_MPIPE_PROF") != nullptr;
        k.mpipe_max_trees = number("TG_SELECT_MPIPE_TREES", 256);
        k.split_cfg = number("TG_SPLIT_CFG", 0);
        k.mpipe_cfg = number("TG_MPIPE_CFG", 0);
        k.gumbel_workers = number("TG_GUMBEL_WORKERS", 0);
        return k;
    }();
    static const bool shared_device = getenv("TG_SHARED_DEVICE") && atoi(getenv("TG_SHARED_DEVICE")) != 0;
    LaunchContext c;
    c.knobs = once;
    const char *split = tg::knob("TG_SELECT_SPLIT");
    c.knobs.split = !split || atoi(split) != 0;
    c.knobs.split_test_mute = tg::knob("TG_SPLIT_TEST_MUTE") != nullptr;
    c.knobs.gumbel_one_by_one = tg::knob("TG_GUMBEL_ONE_BY_ONE") != nullptr;
    c.in.S = s->S;
    c.in.T = s->dev.T;
    c.in.launch_trees = launch_trees;
    c.in.N = s->dev.N;
    c.in.most = most;
    c.in.unique = unique;
    c.in.prof = s->dev.prof != nullptr;
    c.in.shared_device = shared_device;
    c.in.num_cus = s->num_cus;
#ifdef TG_SPLIT_PROF
    c.in.split_prof_build = true;
#endif
    return c;
}

// A launch's arguments beyond its plan.  D: the engine's device view or a slice of it (sub_dev)
struct LaunchArgs {
    const SearchDev &D;
    hipStream_t st;
    float *planes = nullptr;                                       // selections: the leaves' planes
    int max_leaves = 0, mute = 0;                                  // PUCT
    // Gumbel: `limit` leaf slots per tree (the stride of the strided layout); off: the trees' leaf offsets or (UNIQUE) plane
    // ranges, nullptr in the strided layout (the backup's, too)
    const int32_t *nc = nullptr, *mc = nullptr, *off = nullptr;
    int limit = 0;
    const float *policy = nullptr, *value = nullptr;               // backup (slots_per_tree: the strided layout's, else 0)
    int slots_per_tree = 0, use_logit = 0;
};
using LaunchFn = int (*)(tg_search *, const tg_plan::LaunchPlan &, const LaunchArgs &);

template <int S, int NNODE, int NWRK>
constexpr size_t kSplitLds = sizeof(SplitSelShared<S, NNODE>) > sizeof(SplitWrkShared<S, NWRK>) ? sizeof(SplitSelShared<S, NNODE>)
                                                                                                 : sizeof(SplitWrkShared<S, NWRK>);
// The split kernel made ready on the handle's device and asked how many of its workgroups a CU holds: the attribute once per
// kernel and device, the query once per handle (neither is free).  A tree's workgroups wait for each other through memory:
// all (1 + NWG) T of them must be resident at once, which an ordinary launch does not promise.  They are one per CU (1024
// threads, > 80 KB of LDS); a device with fewer CUs than that (partitioned devices) gets the one-workgroup kernels.
template <int S, int NNODE, int NWRK, int NSHIP, int NWG>
int split_room(tg_search *s) {
    constexpr size_t lds = kSplitLds<S, NNODE, NWRK>;
    static_assert(lds <= 160 * 1024, "LDS");
    // (16 waves: chooser + clerk + owners + allocator + shippers + the draw cursor when there are several worker workgroups)
    static_assert(NNODE + 2 + NSHIP + (NWG > 1 ? 1 : 0) + (S == 9 ? 1 : 0) <= 16 && NWRK <= 16, "wavefronts per workgroup");
    static std::atomic<uint64_t> configured{0};          // per device, thread-safe (a process-wide bool was neither)
    if (tg::first_on_device(configured, s->cfg.device))
        TG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&select_puct_split_kernel<S, NNODE, NWRK, NSHIP, NWG>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (s->split.per_cu < 0) {
        int per_cu = 0;
        TG_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, select_puct_split_kernel<S, NNODE, NWRK, NSHIP, NWG>, 1024, lds));
        s->split.per_cu = per_cu;
    }
    return TG_OK;
}
template <int S, int NNODE, int NWRK, int NSHIP, int NWG>
int split_launch(tg_search *s, const tg_plan::LaunchPlan &p, const LaunchArgs &a) {
    hipLaunchKernelGGL((select_puct_split_kernel<S, NNODE, NWRK, NSHIP, NWG>), dim3(p.grid), dim3(p.block), (kSplitLds<S, NNODE, NWRK>),
                       a.st, a.D, a.max_leaves, a.planes, s->split.job.get(), s->split.done.get(), s->split.n.get(),
                       s->split.off.get(), s->split.tag(), s->split.cap, a.mute);
    return TG_OK;
}
template <int S, int NSEL, int NWRK>
int mpipe_launch(tg_search *s, const tg_plan::LaunchPlan &p, const LaunchArgs &a) {
    constexpr size_t lds = sizeof(MPipeShared<S, NSEL, NWRK>);     // 9x9: 16 wavefronts; 19x19: a worker's board is 25 KB of LDS
    static_assert(lds <= 160 * 1024, "LDS");
    static std::atomic<uint64_t> configured{0};
    if (tg::first_on_device(configured, s->cfg.device))
        TG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&select_puct_mpipe_kernel<S, NSEL, NWRK>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((select_puct_mpipe_kernel<S, NSEL, NWRK>), dim3(p.grid), dim3(p.block), lds, a.st, a.D, a.max_leaves, a.planes);
    return TG_OK;
}
template <int S, bool PIPE>
int puct_launch(tg_search *, const tg_plan::LaunchPlan &p, const LaunchArgs &a) {
    if constexpr (PIPE) hipLaunchKernelGGL(select_puct_pipe_kernel<S>, dim3(p.grid), dim3(p.block), 0, a.st, a.D, a.max_leaves, a.planes);
    else hipLaunchKernelGGL(select_puct_kernel<S>, dim3(p.grid), dim3(p.block), 0, a.st, a.D, a.max_leaves, a.planes);
    return TG_OK;
}
template <int S, int NW, bool UNIQUE>       // NW 0: the one-wavefront kernel
int gumbel_launch(tg_search *, const tg_plan::LaunchPlan &p, const LaunchArgs &a) {
    if constexpr (NW == 0)
        hipLaunchKernelGGL((select_gumbel_kernel<S, UNIQUE>), dim3(p.grid), dim3(p.block), 0, a.st, a.D, a.nc, a.mc, a.limit, a.off, a.planes);
    else
        hipLaunchKernelGGL((select_gumbel_pipe_kernel<S, NW, UNIQUE>), dim3(p.grid), dim3(p.block), 0, a.st, a.D, a.nc, a.mc, a.limit, a.off, a.planes);
    return TG_OK;
}
template <int S, int NWAVE, bool UNIQUE>
int backup_launch(tg_search *, const tg_plan::LaunchPlan &p, const LaunchArgs &a) {
    hipLaunchKernelGGL((backup_kernel<S, NWAVE, UNIQUE>), dim3(p.grid), dim3(p.block), 0, a.st, a.D, a.policy, a.value, a.slots_per_tree,
                       a.off, a.use_logit);
    return TG_OK;
}

// Every selection and backup kernel that is built: what a plan can name
struct KernelRow {
    tg_plan::Kernel kernel;
    int S, p[4];
    bool unique;
    LaunchFn launch;
    int (*room)(tg_search *);                  // PuctSplit only
};
using K = tg_plan::Kernel;
#define TG_SPLIT_ROW(S, ...) {K::PuctSplit, S, {__VA_ARGS__}, false, &split_launch<S, __VA_ARGS__>, &split_room<S, __VA_ARGS__>}
#define TG_MPIPE_ROW(S, ...) {K::PuctMPipe, S, {__VA_ARGS__}, false, &mpipe_launch<S, __VA_ARGS__>}
#define TG_PUCT_ROWS(S) {K::PuctPipe, S, {}, false, &puct_launch<S, true>}, {K::Puct, S, {}, false, &puct_launch<S, false>}
#define TG_GUMBEL_ROWS(S, NW) \
    {NW ? K::GumbelPipe : K::Gumbel, S, {NW}, false, &gumbel_launch<S, NW, false>}, {NW ? K::GumbelPipe : K::Gumbel, S, {NW}, true, &gumbel_launch<S, NW, true>}
#define TG_BACKUP_ROWS(S, NWAVE) {K::Backup, S, {NWAVE}, false, &backup_launch<S, NWAVE, false>}, {K::Backup, S, {NWAVE}, true, &backup_launch<S, NWAVE, true>}
constexpr KernelRow kKernelRows[] = {
    TG_SPLIT_ROW(9, 6, 16, 3, 1),   TG_SPLIT_ROW(9, 8, 16, 3, 1),  TG_SPLIT_ROW(9, 10, 16, 2, 1),  TG_SPLIT_ROW(9, 9, 12, 3, 1),
    TG_SPLIT_ROW(9, 10, 16, 3, 1),  TG_SPLIT_ROW(9, 9, 16, 3, 3),  TG_SPLIT_ROW(9, 9, 16, 3, 2),
    TG_SPLIT_ROW(19, 6, 7, 3, 1),   TG_SPLIT_ROW(19, 12, 7, 2, 1), TG_SPLIT_ROW(19, 10, 7, 3, 1),  TG_SPLIT_ROW(19, 10, 7, 3, 3),
    TG_SPLIT_ROW(19, 10, 7, 3, 2),
    TG_MPIPE_ROW(9, 4, 4),  TG_MPIPE_ROW(9, 4, 8),  TG_MPIPE_ROW(9, 4, 12), TG_MPIPE_ROW(9, 8, 8), TG_MPIPE_ROW(9, 6, 10),
    TG_MPIPE_ROW(13, 4, 4), TG_MPIPE_ROW(13, 6, 5), TG_MPIPE_ROW(13, 8, 6), TG_MPIPE_ROW(13, 6, 6),
    TG_MPIPE_ROW(19, 4, 4), TG_MPIPE_ROW(19, 6, 5), TG_MPIPE_ROW(19, 8, 6), TG_MPIPE_ROW(19, 6, 6),
    TG_PUCT_ROWS(9), TG_PUCT_ROWS(13), TG_PUCT_ROWS(19),
    TG_GUMBEL_ROWS(9, 15), TG_GUMBEL_ROWS(9, 10), TG_GUMBEL_ROWS(9, 6), TG_GUMBEL_ROWS(9, 4), TG_GUMBEL_ROWS(9, 2), TG_GUMBEL_ROWS(9, 0),
    TG_GUMBEL_ROWS(13, 6), TG_GUMBEL_ROWS(13, 2), TG_GUMBEL_ROWS(13, 0),
    TG_GUMBEL_ROWS(19, 4), TG_GUMBEL_ROWS(19, 2), TG_GUMBEL_ROWS(19, 0),
    TG_BACKUP_ROWS(9, 16), TG_BACKUP_ROWS(9, 8), TG_BACKUP_ROWS(13, 8), TG_BACKUP_ROWS(19, 16), TG_BACKUP_ROWS(19, 8),
};

// the instantiation a plan names (none: a rule and the table disagree)
constexpr const KernelRow *kernel_row(K kernel, int S, const int (&p)[4], bool unique) {
    for (const KernelRow &r : kKernelRows)
        if (r.kernel == kernel && r.S == S && r.p[0] == p[0] && r.p[1] == p[1] && r.p[2] == p[2] && r.p[3] == p[3] && r.unique == unique)
            return &r;
    return nullptr;
}
template <size_t R>
constexpr bool all_built(K kernel, const tg_plan::CfgRow (&rows)[R]) {
    for (const tg_plan::CfgRow &r : rows)
        if (!kernel_row(kernel, r.S, r.p, false)) return false;
    return true;
}
static_assert(all_built(K::PuctSplit, tg_plan::kSplitRows) && all_built(K::PuctMPipe, tg_plan::kMPipeRows),
              "every kernel TG_SPLIT_CFG / TG_MPIPE_CFG can choose has its row");
int no_row(const char *who) { return tg::fail(TG_ERR_STATE, "%s: the launch plan names a kernel that is not built", who); }

// THE launcher of the selection and backup kernels
int launch_plan(tg_search *s, const char *who, const tg_plan::LaunchPlan &plan, const LaunchArgs &a) {
    const KernelRow *row = kernel_row(plan.kernel, plan.S, plan.p, plan.unique);
    if (!row) return no_row(who);
    if (int rc = row->launch(s, plan, a)) return rc;
    TG_HIP(hipGetLastError());
    return TG_OK;
}

// The PUCT plan of a launch of the whole engine.  Where all that is open is the room for the split kernel's workgroups
// (split_wanted), the kernel that would take the launch is asked (split_room) - and a launch (`st`) first gets the
// mailboxes and its tag: the order of effects of an attempted split launch is allocate, advance the tag, set the
// attribute, query, check the room, launch.  The name query (st == nullptr) asks only.
int plan_puct(tg_search *s, int max_leaves, const hipStream_t *st, LaunchContext *c, tg_plan::LaunchPlan *out) {
    *c = launch_context(s, s->dev.T, max_leaves, false);
    if (tg_plan::split_wanted(c->in, c->knobs)) {
        int p[4], rc;
        tg_plan::cfg_params(tg_plan::kSplitRows, s->S, c->knobs.split_cfg, p);
        const KernelRow *row = kernel_row(K::PuctSplit, s->S, p, false);
        if (!row) return no_row("tg_search_select_puct");
        if (st && ((rc = s->split.ensure(s->dev.T, s->dev.K, s->S == 9 ? kXwEntryWords<9> : kXwEntryWords<19>)) ||
                   (rc = s->split.next_tag(*st))))
            return rc;
        if ((rc = row->room(s))) return rc;
        c->in.split_per_cu = s->split.per_cu;
    }
    *out = tg_plan::plan_select_puct(c->in, c->knobs);
    return TG_OK;
}

// max_n: the most descents any tree of this launch makes - what the pipelined kernel's per-phase tables are sized against
int launch_gumbel_select(tg_search *s, const SearchDev &D, const int32_t *nc_dev, const int32_t *mc_dev, const int32_t *off,
                         int limit, int max_n, float *planes_dev, hipStream_t st, bool unique) {
    const LaunchContext c = launch_context(s, D.T, max_n, unique);
    SearchDev Dk = D;
    Dk.gumbel_one_by_one = c.knobs.gumbel_one_by_one ? 1 : 0;
    LaunchArgs a{Dk, st, planes_dev};
    a.nc = nc_dev, a.mc = mc_dev, a.off = off, a.limit = limit;
    return launch_plan(s, "tg_search_select_gumbel", tg_plan::plan_select_gumbel(c.in, c.knobs), a);
}

int launch_backup(tg_search *s, const SearchDev &D, const float *policy_dev, const float *value_dev, int slots_per_tree,
                  const int32_t *off, int use_logit, hipStream_t st, bool unique) {
    LaunchArgs a{D, st};
    a.policy = policy_dev, a.value = value_dev, a.slots_per_tree = slots_per_tree, a.off = off, a.use_logit = use_logit;
    return launch_plan(s, "tg_search_backup", tg_plan::plan_backup(launch_context(s, D.T, 0, unique).in), a);
}

// -- one Gumbel phase's layout --
bool leaf_layout(int slots_per_tree, int K, LeafLayout *out) {
    *out = slots_per_tree == 0 ? LeafLayout::Packed : (slots_per_tree == -1 ? LeafLayout::Unique : LeafLayout::Strided);
    return *out != LeafLayout::Strided || (slots_per_tree >= 1 && slots_per_tree <= K);
}

// One phase of trees [t0, t1), laid out in the rows [num_considered | max_count | leaf offsets or plane ranges] of the
// engine's T trees (nc, mc and rows are indexed by the engine's tree), the first tree's range at `base`.  A tree's range
// is its nc * mc leaves (<= limit); UNIQUE: its plane slots (mcts/sequential_halving.py unique_plane_caps; caps[t], where
// asked for) - min(leaves, kUniqueE) where the launch takes the pipelined kernel, which the plan of exactly this launch
// says before the launch (no read-back).
struct PhaseLayout {
    int64_t queued = 0, positions = 0;      // leaves the launch queues; positions its forward pass covers
    int32_t max_n = 0;                      // the most descents a tree makes
};
int layout_phase(const tg_search *s, const char *who, const int32_t *nc, const int32_t *mc, int t0, int t1, int limit,
                 LeafLayout layout, int64_t base, int32_t *rows, int32_t *caps, PhaseLayout *out) {
    const size_t T = (size_t)s->dev.T;
    *out = PhaseLayout{};
    for (int t = t0; t < t1; ++t) {
        const int64_t n = (int64_t)nc[t] * mc[t];
        if (nc[t] < 0 || mc[t] < 0 || n > limit) return tg::fail(TG_ERR_ARG, "%s: tree %d phase does not fit %d slots", who, t, limit);
        if (n > out->max_n) out->max_n = (int32_t)n;
    }
    const bool unique = layout == LeafLayout::Unique;
    const LaunchContext c = launch_context(s, t1 - t0, out->max_n, unique);
    const bool capped = unique && tg_plan::plan_select_gumbel(c.in, c.knobs).kernel == K::GumbelPipe;
    int64_t at = base;
    for (int t = t0; t < t1; ++t) {
        const int64_t n = (int64_t)nc[t] * mc[t], range = capped && n > kUniqueE ? kUniqueE : n;
        rows[t] = nc[t];
        rows[T + t] = mc[t];
        rows[2 * T + t] = (int32_t)at;
        if (caps) caps[t] = (int32_t)range;
        at += range;
        out->queued += n;
    }
    out->positions = at - base;
    return TG_OK;
}
}  // namespace

extern "C" {

int tg_search_create(const tg_search_config *cfg, tg_search **out) {
    if (!cfg || !out) return tg::fail(TG_ERR_ARG, "tg_search_create: null argument");
    // 9 and 19 have the tuned kernels; 13 (the third size TamaGo is played at: board/constant.py:4 BOARD_SIZE is a free
    // constant, main.py --size) runs on the board-size-generic ones (one wavefront per tree for selection, the 19x19 backup) -
    // same trees, no pipelining.  Other sizes: instantiate them below (kGenericSize) and rebuild.
    if (cfg->board_size != 9 && cfg->board_size != 19 && cfg->board_size != 13)
        return tg::fail(TG_ERR_ARG, "tg_search_create: board size %d not built (9, 13 and 19 are)", cfg->board_size);
    if (cfg->num_trees < 1 || cfg->tree_size < 2 || cfg->batch_size < 1)
        return tg::fail(TG_ERR_ARG, "tg_search_create: num_trees/tree_size/batch_size out of range");
    TG_HIP(hipSetDevice(cfg->device));
    std::unique_ptr<tg_search> handle(new tg_search);     // (nothing is queued before it is handed out: released as it stands)
    tg_search *s = handle.get();
    s->cfg = *cfg;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0) s->num_cus = cus;
    }
    s->S = cfg->board_size;
    s->W = s->S + 2;
    s->NC = s->W * s->W;
    s->P = s->S * s->S;
    s->A = s->P + 1;
    s->HMAX = 3 * s->P;
    SearchDev &D = s->dev;
    D.T = cfg->num_trees;
    D.N = cfg->tree_size;
    D.K = cfg->batch_size;
    D.cgos = cfg->cgos_mode;
    D.superko = cfg->check_superko;
    const size_t T = D.T, N = D.N, A = s->A, K = D.K;
    int rc = TG_OK;
#define ALLOC(field, count) if ((rc = dev_alloc(s, &D.field, (count)))) return rc;
#define POOL(field, E, per_child, remap) ALLOC(field, T * N * tg_pool::per_node(per_child, A))
    TG_NODE_POOL_ARRAYS(POOL)
#undef POOL
    ALLOC(noise, T * A)
    ALLOC(root_cells, T * s->NC) ALLOC(root_hist, T * s->HMAX) ALLOC(meta, T)
#define QUEUE(field, E, per_slot) ALLOC(field, T * K * (per_slot))
    TG_LEAF_QUEUE_ARRAYS(QUEUE)
#undef QUEUE
    ALLOC(n_leaves, T)
    ALLOC(rng_cursor, T) ALLOC(err, T) ALLOC(halt, T)
#undef ALLOC
    // random windows: one mini-batch worth of expansions each (grown on demand)
    if ((rc = s->win.create(&D, T * K * A))) return rc;
    // the cursors' host-mapped mirror (tg_search_rng_consumed)
    if (s->consumed_pin.alloc(T, hipHostMallocMapped)) return tg::fail(TG_ERR_HIP, "tg_search_create: cursor mirror");
    std::memset(s->consumed_pin.get(), 0, T * sizeof(int64_t));
    D.cursor_pub = s->consumed_pin.dev();
    if (s->copy_stream.create() || s->ev_sel.create())
        return tg::fail(TG_ERR_HIP, "tg_search_create: stream/event creation failed");
    s->rng.create((int)T, (int)A, D.noise, s->copy_stream.get(), &s->win);
    uint64_t *zob = nullptr;
    if ((rc = dev_alloc(s, &zob, (size_t)4 * s->NC))) return rc;
    D.zob = zob;
    s->roots.create((int)T, s->NC, s->HMAX);
    *out = handle.release();
    return TG_OK;
}

int tg_search_destroy(tg_search *s) {
    if (!s) return TG_OK;
    (void)hipSetDevice(s->cfg.device);
    // the launch stream is idle BEFORE any member is released (the owners do not wait for it themselves)
    if (s->stream_known) (void)hipStreamSynchronize(s->last_stream);      // (nullptr: the null stream)
    delete s;
    return TG_OK;
}

int tg_search_grow(tg_search *s, int new_tree_size) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_grow: null argument");
    SearchDev &D = s->dev;
    if (new_tree_size <= D.N) return TG_OK;
    TG_HIP(hipSetDevice(s->cfg.device));
    TG_HIP(hipDeviceSynchronize());           // nothing may still be running on the old arrays
    const size_t T = D.T, n0 = D.N, n1 = (size_t)new_tree_size, A = s->A;
    std::vector<GrowItem> items;
#define GROW(field, E, per_child, remap) \
    items.push_back(GrowItem{reinterpret_cast<void **>(&D.field), sizeof(E), tg_pool::per_node(per_child, A)});
    TG_NODE_POOL_ARRAYS(GROW)
#undef GROW
    // phase 1: every new array allocated and filled; on any failure the new arrays are released (with `items`) and nothing changed
    int rc = TG_OK;
    for (GrowItem &g : items) {
        const size_t bytes = T * n1 * g.per_node * g.elem;
        if (g.fresh.reserve(bytes)) {
            rc = tg::fail(TG_ERR_HIP, "tg_search_grow: %s allocating %zu bytes - the pool keeps its %zu nodes per tree",
                          tg_last_error(), bytes, n0);
            break;
        }
        if ((rc = grow_fill(g, T, n0, n1))) break;
    }
    if (rc == TG_OK && hipDeviceSynchronize() != hipSuccess) rc = tg::fail(TG_ERR_HIP, "tg_search_grow: copy failed");
    if (rc != TG_OK) {
        (void)hipGetLastError();
        return rc;
    }
    // phase 2: swap (cannot fail); the old arrays go with `items`
    for (GrowItem &g : items)
        for (tg::DevBuf<unsigned char> &a : s->allocs)
            if (a.get() == *g.field) {
                std::swap(a, g.fresh);
                *g.field = a.get();
                break;
            }
    D.N = new_tree_size;
    s->cfg.tree_size = new_tree_size;
    // tg_search_reroot's index map is sized by the pool: the next reroot allocates it again (the device is idle here)
    s->rr_map.reset();
    s->rr_blk.reset();
    return TG_OK;
}

int tg_search_set_zobrist(tg_search *s, const uint64_t *keys, size_t n) {
    if (!s || !keys) return tg::fail(TG_ERR_ARG, "tg_search_set_zobrist: null argument");
    if (n != (size_t)4 * s->NC) return tg::fail(TG_ERR_ARG, "tg_search_set_zobrist: expected %d keys", 4 * s->NC);
    TG_HIP(hipMemcpy(const_cast<uint64_t *>(s->dev.zob), keys, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    return TG_OK;
}

int tg_search_set_root(tg_search *s, int tree, const tg_root_position *pos) {
    if (!s || !pos || !pos->cells) return tg::fail(TG_ERR_ARG, "tg_search_set_root: null argument");
    if (tree < 0 || tree >= s->dev.T) return tg::fail(TG_ERR_ARG, "tg_search_set_root: tree %d out of range", tree);
    if (pos->moves < 1) return tg::fail(TG_ERR_ARG, "tg_search_set_root: moves must be >= 1");
    if (pos->to_move != kBlack && pos->to_move != kWhite)
        return tg::fail(TG_ERR_ARG, "tg_search_set_root: to_move must be 1 or 2");
    if (s->dev.superko && !pos->hash_history && pos->moves > 1)
        return tg::fail(TG_ERR_ARG, "tg_search_set_root: hash_history required with check_superko");
    const BoardScalars b{pos->hash, pos->moves, pos->ko_pos, pos->ko_move, pos->prev_move, pos->prev_prev_move};
    const int hist_len = tg_root::root_hist_len(pos->moves, s->HMAX, s->dev.superko != 0);   // (the handle's flag, as on the device)
    s->roots.stage(tree, tg_root::root_meta(b, pos->to_move, hist_len), pos->cells, pos->hash_history);
    return TG_OK;
}

// ---- the staged roots' transitions (tg_search::StagedRoots) ----
void tg_search::StagedRoots::create(int T, int NC, int HMAX) {
    NC_ = NC, HMAX_ = HMAX;
    cells_.assign((size_t)T * NC, 0);
    hist_.assign((size_t)T * HMAX, 0);
    meta_.assign(T, RootMeta{});
    dirty_.assign(T, 0);
    hist_at_ = (cells_.size() + 7) & ~(size_t)7;
    meta_at_ = hist_at_ + hist_.size() * sizeof(uint64_t);
}

void tg_search::StagedRoots::stage(int tree, const RootMeta &m, const uint8_t *cells, const uint64_t *history) {
    std::memcpy(&cells_[tree * NC_], cells, NC_);
    uint64_t *hist = &hist_[tree * HMAX_];
    hist[0] = 0;
    if (history) std::memcpy(hist, history, (size_t)m.hist_len * sizeof(uint64_t));
    meta_[tree] = m;
    n_dirty_ += 1 - dirty_[tree];
    dirty_[tree] = 1;
}

int tg_search::StagedRoots::begin() {
    int slot;
    if (int rc = pin_.acquire(meta_at_ + meta_.size() * sizeof(RootMeta), &m_cells_, &slot)) return rc;
    m_hist_ = reinterpret_cast<uint64_t *>(m_cells_ + hist_at_);
    m_meta_ = reinterpret_cast<RootMeta *>(m_cells_ + meta_at_);
    return TG_OK;
}

int tg_search::StagedRoots::upload(int t, const SearchDev &D, RootMeta *meta_dst, hipStream_t st) {
    std::memcpy(m_cells_ + t * NC_, &cells_[t * NC_], NC_);
    TG_HIP(hipMemcpyAsync(D.root_cells + t * NC_, m_cells_ + t * NC_, NC_, hipMemcpyHostToDevice, st));
    if (D.superko) {
        const size_t hb = (size_t)meta_[t].hist_len * sizeof(uint64_t);
        std::memcpy(m_hist_ + t * HMAX_, &hist_[t * HMAX_], hb);
        TG_HIP(hipMemcpyAsync(D.root_hist + t * HMAX_, m_hist_ + t * HMAX_, hb, hipMemcpyHostToDevice, st));
    }
    m_meta_[t] = meta_[t];
    TG_HIP(hipMemcpyAsync(meta_dst, m_meta_ + t, sizeof(RootMeta), hipMemcpyHostToDevice, st));
    return TG_OK;
}

int tg_search::StagedRoots::upload_all(const SearchDev &D, hipStream_t st) {
    if (int rc = begin()) return rc;
    if (n_dirty_ == D.T) {
        std::memcpy(m_cells_, cells_.data(), cells_.size());
        std::memcpy(m_meta_, meta_.data(), meta_.size() * sizeof(RootMeta));
        TG_HIP(hipMemcpyAsync(D.root_cells, m_cells_, cells_.size(), hipMemcpyHostToDevice, st));
        if (D.superko) {
            std::memcpy(m_hist_, hist_.data(), hist_.size() * sizeof(uint64_t));
            TG_HIP(hipMemcpyAsync(D.root_hist, m_hist_, hist_.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        }
        TG_HIP(hipMemcpyAsync(D.meta, m_meta_, meta_.size() * sizeof(RootMeta), hipMemcpyHostToDevice, st));
    } else {
        for (int t = 0; t < D.T; ++t)
            if (int rc = staged(t) ? upload(t, D, D.meta + t, st) : TG_OK) return rc;
    }
    if (int rc = end(st)) return rc;
    drop_all();
    return TG_OK;
}

// The halt words and stopped_at entries of trees [t0, t0 + n) cleared on st (stopped_at: once the rule's buffers exist).
static int clear_halt_range(tg_search *s, int t0, int n, hipStream_t st) {
    TG_HIP(hipMemsetAsync(s->dev.halt + t0, 0, (size_t)n * sizeof(int32_t), st));
    if (s->halting.stopped_at.get()) TG_HIP(hipMemsetAsync(s->halting.stopped_at.get() + t0, 0, (size_t)n * sizeof(int32_t), st));
    return TG_OK;
}

// Whatever resets a tree clears its halt word and its stopped_at: the root expansion every tree's (clear_halt), a staged root
// going up, a root from a record and a reroot those of the trees they touch (clear_halt_of: pick(t) says which; one memset per
// run of neighbouring trees).  Nothing is queued unless a word may be set.  The live ranks are stale either way: a reset
// tree has another root, and may be live again.
static int clear_halt(tg_search *s, hipStream_t st) {
    s->ranks.mark_stale();
    if (!s->halting.armed) return TG_OK;
    s->halting.armed = false;
    return clear_halt_range(s, 0, s->dev.T, st);
}

static int clear_halt_of(tg_search *s, hipStream_t st, const std::function<bool(int)> &pick) {
    s->ranks.mark_stale();
    if (!s->halting.armed) return TG_OK;
    const int T = s->dev.T;
    for (int t = 0; t < T;) {
        if (!pick(t)) { ++t; continue; }
        int end = t + 1;
        while (end < T && pick(end)) ++end;
        if (end - t == T) return clear_halt(s, st);
        if (int rc = clear_halt_range(s, t, end - t, st)) return rc;
        t = end;
    }
    return TG_OK;
}

static int flush_roots(tg_search *s, hipStream_t st) {
    if (!s->roots.any()) return TG_OK;
    if (int rc = clear_halt_of(s, st, [&](int t) { return s->roots.staged(t); })) return rc;
    s->roots_expanded = false;
    if (int rc = s->roots.upload_all(s->dev, st)) return rc;
    TG_HIP(hipMemsetAsync(s->dev.err, 0, (size_t)s->dev.T * sizeof(int32_t), st));
    return TG_OK;
}

// ---- the random windows (tg_search::Windows; the streams that fill them: tg_search::Streams below) ----
int tg_search::Windows::create(SearchDev *D, size_t draws) {
    // one mini-batch worth of expansions each (grown on demand)
    for (int b = 0; b < 2; ++b)
        if (buf_[b].reserve(draws)) return tg::fail(TG_ERR_HIP, "rng window: %s", tg_last_error());
    if (ev_[0].create() || ev_[1].create()) return tg::fail(TG_ERR_HIP, "tg_search_create: stream/event creation failed");
    book_.create(D->T);
    D->rng = buf_[0].get();
    D->rng_cap = 0;             // nothing installed yet
    return TG_OK;
}

// what a transition of the book returned.  D, st: the device view and launch stream of install (st alone: extend)
int tg_search::Windows::carry_out(const tg_streams::Actions &acts, Streams &gen, SearchDev *D, hipStream_t st) {
    using tg_streams::Action;
    int rc;
    for (const Action &a : acts) {
        switch (a.what) {
        case Action::Generate:
            // (growing frees the old window first: implicit device synchronisation, rare)
            if ((rc = buf_[a.buf].reserve((size_t)gen.trees() * (size_t)a.piece.pitch)) || (rc = gen.generate(a.piece, nullptr, nullptr)) ||
                (rc = ev_[a.buf].record(gen.stream())))
                return rc;
            book_.generated(a.piece);
            break;
        case Action::Wait:
            TG_HIP(hipStreamWaitEvent(st, ev_[a.buf].get(), 0));
            break;
        case Action::Publish:
            D->rng = buf_[a.buf].get();
            D->rng_cap = a.pitch;
            break;
        case Action::ResetCursors:
            TG_HIP(hipMemsetAsync(D->rng_cursor, 0, (size_t)D->T * sizeof(int64_t), st));
            if (D->cursor_pub) TG_HIP(hipMemsetAsync(D->cursor_pub, 0, (size_t)D->T * sizeof(int64_t), st));
            break;
        }
    }
    return TG_OK;
}

int tg_search::Windows::accept(Streams &gen, const double *host, size_t stride, size_t count) {
    const int idx = book_.free_buffer(), T = gen.trees();
    // (growing frees the old window first: implicit device synchronisation, rare)
    if (int rc = buf_[idx].reserve((size_t)T * count)) return rc;
    // rows are packed with pitch `count`; the kernels index with rng_cap = count
    TG_HIP(hipMemcpy2DAsync(buf_[idx].get(), count * sizeof(double), host, stride * sizeof(double), count * sizeof(double), T,
                            hipMemcpyHostToDevice, gen.stream()));
    if (int rc = ev_[idx].record(gen.stream())) return rc;
    TG_HIP(hipStreamSynchronize(gen.stream()));   // the host buffer may be released on return
    book_.accept((int64_t)count);
    return TG_OK;
}

static int after_select(tg_search *s, hipStream_t st) { return s->ev_sel.record(st); }

int tg_search_set_rng(tg_search *s, const double *exp_stream_host, size_t stride, size_t count) {
    if (!s || !exp_stream_host) return tg::fail(TG_ERR_ARG, "tg_search_set_rng: null argument");
    if (count > stride) return tg::fail(TG_ERR_ARG, "tg_search_set_rng: count > stride");
    return s->win.accept(s->rng, exp_stream_host, stride, count);
}

int tg_search_rng_consumed(tg_search *s, int64_t *consumed_host) {
    if (!s || !consumed_host) return tg::fail(TG_ERR_ARG, "tg_search_rng_consumed: null argument");
    // The kernels that move a cursor mirror it into host-mapped memory (SearchDev::cursor_pub); the host waits for the last
    // selection launch's event only - the forward pass / backup behind it keep running - and reads the mirror.  (Until round 6
    // a copy on the side stream: for a few trees that copy is a one-workgroup kernel, and it queued for a CU behind the forward
    // pass's 256 workgroups - the cursors, and with them the generation of the next random window, arrived ~57 us late.)
    if (!s->ev_sel.recorded()) {
        TG_HIP(hipDeviceSynchronize());
    } else if (s->dev.T >= 256) {
        // Many trees: the selection launch takes milliseconds - sleep instead of spinning (a rank's driver thread burnt a whole
        // core doing nothing; eight ranks share the host; hipEventSynchronize spins whatever the event's flags say here).
        for (;;) {
            const hipError_t q = hipEventQuery(s->ev_sel.get());
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return tg::fail(TG_ERR_HIP, "tg_search_rng_consumed: hipEventQuery: %s", hipGetErrorString(q));
            std::this_thread::sleep_for(std::chrono::microseconds(s->dev.T >= 1024 ? 200 : 50));
        }
    } else {
        TG_HIP(hipEventSynchronize(s->ev_sel.get()));
    }
    std::memcpy(consumed_host, s->consumed_pin.get(), (size_t)s->dev.T * sizeof(int64_t));
    return TG_OK;
}

// a tree's sticky error flags, as every call that meets them reports them
static int fail_tree(int tree, int32_t err) { return tg::fail(TG_ERR_OVERFLOW, "%s", tg_readout::error_text(tree, err).c_str()); }

static int check_errors(tg_search *s) {
    std::vector<int32_t> err(s->dev.T);
    TG_HIP(hipMemcpy(err.data(), s->dev.err, err.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int t = 0; t < s->dev.T; ++t)
        if (err[t]) return fail_tree(t, err[t]);
    return TG_OK;
}

int tg_search_root_planes(tg_search *s, float *planes_dev, void *stream) {
    if (!s || !planes_dev) return tg::fail(TG_ERR_ARG, "tg_search_root_planes: null argument");
    hipStream_t st = use_stream(s, stream);
    {
        int rc = flush_roots(s, st);
        if (rc) return rc;
        if ((rc = clear_halt(s, st))) return rc;
        if ((rc = s->win.install(s->rng, &s->dev, st))) return rc;
    }
    s->roots_expanded = true;
    if (s->last.layout == LeafLayout::Compact) s->last.layout = LeafLayout::Strided;      // (tree t's root planes: row t)
    with_board_size(s->S, [&](auto size) {
        hipLaunchKernelGGL(root_kernel<decltype(size)::value>, dim3(s->dev.T), dim3(64), 0, st, s->dev, planes_dev);
    });
    TG_HIP(hipGetLastError());
    return after_select(s, st);
}

// The engine's device view of a COMPACT launch: the live ranks in force
static SearchDev compact_dev(const tg_search *s) {
    SearchDev D = s->dev;
    D.rank = s->ranks.rank.get();
    return D;
}

// One PUCT selection of the whole engine.  compact: tree t's leaves at row rank[t] * max_leaves, by the ranks in the handle's
// table - the caller has seen to it that every tree the selectors take has one (fresh ranks; within a chain, ranks taken at a
// poll of a set of live trees that only shrinks).  The layout is recorded for the backup.
static int select_puct_impl(tg_search *s, const char *who, int max_leaves, float *planes_dev, int32_t *n_leaves_dev, void *stream,
                            bool compact) {
    if (!s || !planes_dev) return tg::fail(TG_ERR_ARG, "%s: null argument", who);
    if (max_leaves < 0 || max_leaves > s->dev.K)
        return tg::fail(TG_ERR_ARG, "%s: max_leaves %d outside [0, batch_size]", who, max_leaves);
    hipStream_t st = use_stream(s, stream);
    {
        int rc = s->win.install(s->rng, &s->dev, st);
        if (rc) return rc;
    }
    LaunchContext c;
    tg_plan::LaunchPlan plan;
    if (int rc = plan_puct(s, max_leaves, &st, &c, &plan)) return rc;
    SearchDev D = compact ? compact_dev(s) : s->dev;
    if (s->budgets.on) D.budget = s->budgets.total.get();          // (per-tree descents; the plan is max_leaves' as ever)
    LaunchArgs a{D, st, planes_dev, max_leaves, c.knobs.split_test_mute ? 1 : 0};
    if (int rc = launch_plan(s, who, plan, a)) return rc;
    if (compact) {
        s->last.subgroups = false;
        s->last.layout = LeafLayout::Compact;
    } else if (s->last.layout == LeafLayout::Compact) {
        s->last.layout = LeafLayout::Strided;      // (what the record held before compaction existed stays as it was)
    }
    if (n_leaves_dev)
        TG_HIP(hipMemcpyAsync(n_leaves_dev, s->dev.n_leaves, (size_t)s->dev.T * sizeof(int32_t),
                              hipMemcpyDeviceToDevice, st));
    return after_select(s, st);
}

int tg_search_select_puct(tg_search *s, int max_leaves, float *planes_dev, int32_t *n_leaves_dev, void *stream) {
    return select_puct_impl(s, "tg_search_select_puct", max_leaves, planes_dev, n_leaves_dev, stream, false);
}

int tg_search_select_puct_compact(tg_search *s, int max_leaves, int shrunk_ok, float *planes_dev, int32_t *n_leaves_dev, void *stream) {
    if (s && !s->ranks.usable(shrunk_ok != 0))
        return tg::fail(TG_ERR_STATE, "tg_search_select_puct_compact: no fresh live ranks (tg_search_compact_live behind the last call that %s)",
                        shrunk_ok ? "reset a root" : "wrote halt words or reset a root");
    return select_puct_impl(s, "tg_search_select_puct_compact", max_leaves, planes_dev, n_leaves_dev, stream, true);
}

int tg_search_launch_name(tg_search *s, int family, int max_n, int unique, char *out, size_t cap) {
    if (!s || !out || !cap) return tg::fail(TG_ERR_ARG, "tg_search_launch_name: null argument");
    LaunchContext c = launch_context(s, s->dev.T, max_n, unique != 0);
    if (family == 0) {
        tg_plan::LaunchPlan plan;
        if (int rc = plan_puct(s, max_n, nullptr, &c, &plan)) return rc;
        plan.name(out, cap);
    } else if (family == 1) {
        tg_plan::plan_select_gumbel(c.in, c.knobs).name(out, cap);
    } else if (family == 2) {
        tg_plan::plan_backup(c.in).name(out, cap);
    } else {
        return tg::fail(TG_ERR_ARG, "tg_search_launch_name: family %d (0 PUCT, 1 Gumbel, 2 backup)", family);
    }
    return TG_OK;
}

int tg_search_profile(tg_search *s, int enable, long long *cycles_host) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_profile: null argument");
    if (int rc = sync_launch_stream(s)) return rc;
    if (enable && !s->dev.prof) {
        int rc = dev_alloc(s, &s->dev.prof, (size_t)16);
        if (rc) return rc;
    }
    if (cycles_host && s->dev.prof)
        TG_HIP(hipMemcpy(cycles_host, s->dev.prof, 16 * sizeof(long long), hipMemcpyDeviceToHost));
    if (s->dev.prof) TG_HIP(hipMemset(s->dev.prof, 0, 16 * sizeof(long long)));
    if (!enable) s->dev.prof = nullptr;       // buffer stays allocated until destroy
    return TG_OK;
}

// play_kernel on the moves in moves_dev (the host's: tg_search_play; the device's own: finish_roots_kernel)
static int launch_play(tg_search *s, hipStream_t st) {
    with_board_size(s->S, [&](auto size) {
        hipLaunchKernelGGL(play_kernel<decltype(size)::value>, dim3(s->dev.T), dim3(64), 0, st, s->dev, s->moves_dev.get());
    });
    TG_HIP(hipGetLastError());
    return TG_OK;
}

int tg_search_play(tg_search *s, const int32_t *moves_host, void *stream) {
    if (!s || !moves_host) return tg::fail(TG_ERR_ARG, "tg_search_play: null argument");
    hipStream_t st = use_stream(s, stream);
    int rc = flush_roots(s, st);
    if (rc) return rc;
    s->roots_expanded = false;
    const size_t n = (size_t)s->dev.T;
    if (!s->moves_dev.get() && (rc = s->moves_dev.alloc_zeroed(n))) return rc;
    int32_t *pin;
    int slot;
    if ((rc = s->moves_pin.acquire(n, &pin, &slot))) return rc;
    std::memcpy(pin, moves_host, n * sizeof(int32_t));
    TG_HIP(hipMemcpyAsync(s->moves_dev.get(), pin, n * sizeof(int32_t), hipMemcpyHostToDevice, st));   // (the caller's buffer is free)
    if ((rc = s->moves_pin.commit(slot, st))) return rc;
    return launch_play(s, st);
}

static int launch_reroot(tg_search *s, hipStream_t st);
int tg_search_reroot(tg_search *s, const int32_t *new_root_host, void *stream) {
    if (!s || !new_root_host) return tg::fail(TG_ERR_ARG, "tg_search_reroot: null argument");
    SearchDev &D = s->dev;
    const int T = D.T;
    bool any = false;
    for (int t = 0; t < T; ++t) {
        const int r = new_root_host[t];
        if (r < -1 || r >= D.N) return tg::fail(TG_ERR_ARG, "tg_search_reroot: tree %d: new root %d outside [-1, %d)", t, r, D.N);
        any |= r >= 0;
    }
    if (!any) return TG_OK;
    hipStream_t st = use_stream(s, stream);
    int rc;
    if ((rc = clear_halt_of(s, st, [&](int t) { return new_root_host[t] >= 0; }))) return rc;
    const int nblk = (D.N + kRerootChunk - 1) / kRerootChunk;
    // (hipMalloc: no synchronisation, nothing zeroed; grow releases the two that are sized by the pool)
    if ((rc = s->rr_small.reserve((size_t)4 * T)) || (rc = s->rr_stage.reserve((size_t)T)) ||
        (rc = s->rr_map.reserve((size_t)T * D.N)) || (rc = s->rr_blk.reserve((size_t)T * nblk)))
        return rc;
    if ((rc = s->roots.begin())) return rc;
    // the positions staged by tg_search_set_root for the trees that get a new root: cells and history straight to the device,
    // the RootMeta to rr_stage (the scan kernel installs it with the new num_nodes); other trees' staged positions stay staged
    int32_t *pin;
    int slot;
    if ((rc = s->rr_pin.acquire((size_t)2 * T, &pin, &slot))) return rc;
    bool staged = false;
    for (int t = 0; t < T; ++t) {
        pin[t] = new_root_host[t];
        pin[T + t] = new_root_host[t] >= 0 && s->roots.staged(t) ? 1 : 0;
        if (!pin[T + t]) continue;
        staged = true;
        if ((rc = s->roots.take(t, D, s->rr_stage.get() + t, st))) return rc;
    }
    if (staged && (rc = s->roots.end(st))) return rc;
    TG_HIP(hipMemcpyAsync(s->rr_small.get(), pin, (size_t)2 * T * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = s->rr_pin.commit(slot, st))) return rc;
    return launch_reroot(s, st);
}

// the four reroot kernels on rr_small's [new root | position staged | old num_nodes | identity], rr_stage and the maps
static int launch_reroot(tg_search *s, hipStream_t st) {
    SearchDev &D = s->dev;
    const int T = D.T, nblk = (D.N + kRerootChunk - 1) / kRerootChunk;
    int32_t *small = s->rr_small.get(), *map = s->rr_map.get(), *blk = s->rr_blk.get();
    const int32_t *roots = small, *has_pos = small + T;
    int32_t *old_n = small + 2 * T, *ident = small + 3 * T;
    hipLaunchKernelGGL(reroot_mark_kernel, dim3(T, nblk), dim3(256), 0, st, D, roots, map, blk, old_n, nblk);
    TG_HIP(hipGetLastError());
    hipLaunchKernelGGL(reroot_scan_kernel, dim3(T), dim3(64), 0, st, D, s->A, roots, has_pos, blk, nblk, old_n, ident,
                       s->rr_stage.get());
    TG_HIP(hipGetLastError());
    hipLaunchKernelGGL(reroot_assign_kernel, dim3(T, nblk), dim3(256), 0, st, D, roots, map, blk, old_n, nblk);
    TG_HIP(hipGetLastError());
    hipLaunchKernelGGL(reroot_move_kernel, dim3(T), dim3(1024), 0, st, D, s->A, roots, map, old_n, ident);
    TG_HIP(hipGetLastError());
    return TG_OK;
}

// ---- tree reuse in lock-step matches: roots advanced on the device, root expansion of the fresh trees only ----
static_assert(sizeof(tg_advance_record) == sizeof(AdvanceRec) && offsetof(tg_advance_record, kept_nodes) == offsetof(AdvanceRec, kept_nodes) &&
                  offsetof(tg_advance_record, status) == offsetof(AdvanceRec, status),
              "include/tamago_hip.h restates csrc/readout.h's AdvanceRec");

int tg_search_advance(tg_search *s, const int32_t *moves_host, tg_advance_record *records_host, void *stream) {
    if (!s || !moves_host) return tg::fail(TG_ERR_ARG, "tg_search_advance: null argument");
    SearchDev &D = s->dev;
    const int T = D.T;
    bool any = false;
    for (int t = 0; t < T; ++t) {
        const int mv = moves_host[t];
        if (mv < -1 || mv >= s->NC)
            return tg::fail(TG_ERR_ARG, "tg_search_advance: tree %d: move %d is neither -1, PASS (0) nor a cell below %d", t, mv, s->NC);
        any |= mv >= 0;
    }
    TG_HIP(hipSetDevice(s->cfg.device));
    hipStream_t st = use_stream(s, stream);
    const size_t n = (size_t)T;
    int rc;
    if (!s->adv_host.get() && ((rc = s->adv_dev.reserve(n)) || (rc = s->adv_host.alloc(n)))) return rc;
    if (any) {
        if ((rc = flush_roots(s, st))) return rc;                      // (a staged position is played on, as tg_search_play does)
        if ((rc = clear_halt_of(s, st, [&](int t) { return moves_host[t] >= 0; }))) return rc;
        s->roots_expanded = false;
        const int nblk = (D.N + kRerootChunk - 1) / kRerootChunk;
        if ((rc = s->rr_small.reserve((size_t)4 * T)) || (rc = s->rr_stage.reserve(n)) || (rc = s->rr_map.reserve(n * D.N)) ||
            (rc = s->rr_blk.reserve(n * nblk)))
            return rc;
        if (!s->moves_dev.get() && (rc = s->moves_dev.alloc_zeroed(n))) return rc;
        int32_t *pin;
        int slot;
        if ((rc = s->moves_pin.acquire(n, &pin, &slot))) return rc;
        std::memcpy(pin, moves_host, n * sizeof(int32_t));
        TG_HIP(hipMemcpyAsync(s->moves_dev.get(), pin, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if ((rc = s->moves_pin.commit(slot, st))) return rc;
        int32_t *roots = s->rr_small.get();
        TG_HIP(hipMemsetAsync(roots + T, 0, n * sizeof(int32_t), st));   // (no position is staged for a tree: flushed above)
        with_board_size(s->S, [&](auto size) {
            hipLaunchKernelGGL(advance_kernel<decltype(size)::value>, dim3(T), dim3(64), 0, st, D, s->moves_dev.get(), roots, s->adv_dev.get());
        });
        TG_HIP(hipGetLastError());
        if ((rc = launch_reroot(s, st))) return rc;
        hipLaunchKernelGGL(advance_nodes_kernel, dim3((T + 255) / 256), dim3(256), 0, st, D, roots, s->adv_dev.get());
        TG_HIP(hipGetLastError());
    }
    if (!records_host) return TG_OK;
    if (!any) {
        for (int t = 0; t < T; ++t) records_host[t] = tg_advance_record{-1, 0, 0, TG_ADVANCE_LEFT_ALONE};
        return TG_OK;
    }
    TG_HIP(hipMemcpyAsync(s->adv_host.get(), s->adv_dev.get(), n * sizeof(AdvanceRec), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    std::memcpy(records_host, s->adv_host.get(), n * sizeof(AdvanceRec));
    for (int t = 0; t < T; ++t)
        if (records_host[t].status & TG_ADVANCE_OCCUPIED) return check_errors(s);
    return TG_OK;
}

int tg_search_root_planes_fresh(tg_search *s, float *planes_dev, void *stream) {
    if (!s || !planes_dev) return tg::fail(TG_ERR_ARG, "tg_search_root_planes_fresh: null argument");
    hipStream_t st = use_stream(s, stream);
    {
        int rc = flush_roots(s, st);
        if (rc) return rc;
        if ((rc = s->win.install(s->rng, &s->dev, st))) return rc;
    }
    s->ranks.mark_stale();                                             // (a fresh tree's halt word is cleared: it may be live again)
    s->roots_expanded = true;
    if (s->last.layout == LeafLayout::Compact) s->last.layout = LeafLayout::Strided;      // (tree t's root planes: row t)
    with_board_size(s->S, [&](auto size) {
        hipLaunchKernelGGL(root_fresh_kernel<decltype(size)::value>, dim3(s->dev.T), dim3(64), 0, st, s->dev, planes_dev,
                           s->halting.stopped_at.get());
    });
    TG_HIP(hipGetLastError());
    return after_select(s, st);
}

int tg_search_set_budget(tg_search *s, const int32_t *total_host, void *stream) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_set_budget: null argument");
    if (!total_host) {
        s->budgets.on = false;
        return TG_OK;
    }
    const size_t n = (size_t)s->dev.T;
    for (size_t t = 0; t < n; ++t)
        if (total_host[t] < 1) return tg::fail(TG_ERR_ARG, "tg_search_set_budget: tree %zu: a total of %d visits (at least 1)", t, total_host[t]);
    TG_HIP(hipSetDevice(s->cfg.device));
    hipStream_t st = use_stream(s, stream);
    int rc;
    if ((rc = s->budgets.total.reserve(n))) return rc;
    int32_t *pin;
    int slot;
    if ((rc = s->budgets.pin.acquire(n, &pin, &slot))) return rc;
    std::memcpy(pin, total_host, n * sizeof(int32_t));
    TG_HIP(hipMemcpyAsync(s->budgets.total.get(), pin, n * sizeof(int32_t), hipMemcpyHostToDevice, st));   // (behind the launches that read the old totals)
    if ((rc = s->budgets.pin.commit(slot, st))) return rc;
    s->budgets.on = true;
    return TG_OK;
}

int tg_search_read_positions(tg_search *s, uint8_t *cells_host, int32_t *moves_host, int32_t *to_move_host) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_read_positions: null argument");
    int rc;
    if ((rc = sync_launch_stream(s)) || (rc = flush_roots(s, s->last_stream)) || (rc = sync_launch_stream(s))) return rc;
    if (cells_host)
        TG_HIP(hipMemcpy(cells_host, s->dev.root_cells, (size_t)s->dev.T * s->NC, hipMemcpyDeviceToHost));
    if (moves_host || to_move_host) {
        std::vector<RootMeta> meta(s->dev.T);
        TG_HIP(hipMemcpy(meta.data(), s->dev.meta, meta.size() * sizeof(RootMeta), hipMemcpyDeviceToHost));
        for (int t = 0; t < s->dev.T; ++t) {
            if (moves_host) moves_host[t] = meta[t].moves;
            if (to_move_host) to_move_host[t] = meta[t].to_move;
        }
    }
    return TG_OK;
}

int tg_search_read_root_state(tg_search *s, int tree, uint64_t *hash, int32_t *meta8, uint64_t *hist_host, int hist_cap) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_read_root_state: null argument");
    if (tree < 0 || tree >= s->dev.T) return tg::fail(TG_ERR_ARG, "tg_search_read_root_state: tree %d out of range", tree);
    if (hist_cap < 0 || (hist_cap > 0 && !hist_host)) return tg::fail(TG_ERR_ARG, "tg_search_read_root_state: history buffer");
    int rc;
    if ((rc = sync_launch_stream(s)) || (rc = flush_roots(s, s->last_stream)) || (rc = sync_launch_stream(s))) return rc;
    RootMeta m;
    TG_HIP(hipMemcpy(&m, s->dev.meta + tree, sizeof(RootMeta), hipMemcpyDeviceToHost));
    if (hash) *hash = m.hash;
    if (meta8) {
        const int32_t v[8] = {m.moves, m.ko_pos, m.ko_move, m.prev, m.prevprev, m.to_move, m.num_nodes, m.hist_len};
        std::memcpy(meta8, v, sizeof(v));
    }
    const int n = std::min(std::min(m.hist_len, s->HMAX), hist_cap);
    if (n > 0)
        TG_HIP(hipMemcpy(hist_host, s->dev.root_hist + (size_t)tree * s->HMAX, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return TG_OK;
}

int tg_search_set_roots_from_records(tg_search *s, const int32_t *moves_host, const int8_t *colors_host, const int64_t *offsets_host,
                                     int games, const int32_t *root_game_host, const int32_t *root_ply_host, int32_t *flags_host,
                                     void *stream) {
    if (!s || !offsets_host || !root_game_host || !root_ply_host || !flags_host)
        return tg::fail(TG_ERR_ARG, "tg_search_set_roots_from_records: null argument");
    if (s->S != 9 && s->S != 13 && s->S != 19)
        return tg::fail(TG_ERR_ARG, "tg_search_set_roots_from_records: board size %d not built (9, 13 and 19 are)", s->S);
    if (games < 0) return tg::fail(TG_ERR_ARG, "tg_search_set_roots_from_records: negative number of games");
    if (offsets_host[0] != 0) return tg::fail(TG_ERR_ARG, "tg_search_set_roots_from_records: offsets start at 0");
    for (int g = 0; g < games; ++g)
        if (offsets_host[g + 1] < offsets_host[g])
            return tg::fail(TG_ERR_ARG, "tg_search_set_roots_from_records: game %d: offsets decrease", g);
    const size_t M = (size_t)offsets_host[games];
    if (M && !moves_host) return tg::fail(TG_ERR_ARG, "tg_search_set_roots_from_records: null argument");
    if (colors_host)
        for (size_t i = 0; i < M; ++i)
            if (colors_host[i] != kBlack && colors_host[i] != kWhite)
                return tg::fail(TG_ERR_ARG, "tg_search_set_roots_from_records: move %zu: colour %d is neither 1 nor 2", i, (int)colors_host[i]);
    const int T = s->dev.T;
    // the per-record lists of (ply, tree), sorted by ply; the records without a tree take no part
    struct Member { int32_t game, ply, tree; };
    std::vector<Member> members;
    members.reserve(T);
    for (int t = 0; t < T; ++t) {
        const int g = root_game_host[t];
        if (g < 0) continue;
        if (g >= games) return tg::fail(TG_ERR_ARG, "tg_search_set_roots_from_records: tree %d: game %d of %d", t, g, games);
        const int64_t n = offsets_host[g + 1] - offsets_host[g];
        if (root_ply_host[t] < 0 || root_ply_host[t] > n)
            return tg::fail(TG_ERR_ARG, "tg_search_set_roots_from_records: tree %d: ply %d outside [0, %lld]", t, root_ply_host[t], (long long)n);
        members.push_back({g, root_ply_host[t], t});
    }
    std::fill(flags_host, flags_host + T, 0);
    if (members.empty()) return TG_OK;
    std::sort(members.begin(), members.end(), [](const Member &a, const Member &b) {
        return a.game != b.game ? a.game < b.game : a.ply != b.ply ? a.ply < b.ply : a.tree < b.tree;
    });
    const size_t K = members.size();
    size_t R = 0;
    for (size_t i = 0; i < K; ++i) R += i == 0 || members[i].game != members[i - 1].game;
    TG_HIP(hipSetDevice(s->cfg.device));
    hipStream_t st = use_stream(s, stream);
    if (int rc = clear_halt_of(s, st, [&](int t) { return root_game_host[t] >= 0; })) return rc;
    s->roots_expanded = false;
    // one pinned image, one copy: [offsets | moves | records | row offsets | row plies | row trees | colours]
    const size_t G1 = (size_t)games + 1;
    const size_t o_off = 0, o_moves = o_off + G1 * 8, o_rec = o_moves + M * 4, o_moff = o_rec + R * 4, o_ply = o_moff + (R + 1) * 4,
                 o_tree = o_ply + K * 4, o_col = o_tree + K * 4;
    const size_t bytes = o_col + (colors_host ? M : 0);
    int rc;
    if (bytes > s->rec_cap) {
        const size_t cap = bytes + bytes / 2;
        if ((rc = s->rec_stage.alloc(cap)) || (rc = s->rec_in.reserve(cap))) { s->rec_cap = 0; return rc; }
        s->rec_cap = cap;
    }
    if (!s->rec_flags.get() && ((rc = s->rec_flags_back.alloc(T)) || (rc = s->rec_flags.reserve(T)))) { s->rec_flags.reset(); return rc; }
    uint8_t *pin = s->rec_stage.get();
    std::memcpy(pin + o_off, offsets_host, G1 * 8);
    if (M) std::memcpy(pin + o_moves, moves_host, M * 4);
    if (M && colors_host) std::memcpy(pin + o_col, colors_host, M);
    {
        int32_t *rec = reinterpret_cast<int32_t *>(pin + o_rec), *moff = reinterpret_cast<int32_t *>(pin + o_moff);
        int32_t *ply = reinterpret_cast<int32_t *>(pin + o_ply), *tree = reinterpret_cast<int32_t *>(pin + o_tree);
        size_t r = 0;
        for (size_t i = 0; i < K; ++i) {
            if (i == 0 || members[i].game != members[i - 1].game) { rec[r] = members[i].game; moff[r] = (int32_t)i; ++r; }
            ply[i] = members[i].ply;
            tree[i] = members[i].tree;
        }
        moff[R] = (int32_t)K;
    }
    TG_HIP(hipMemcpyAsync(s->rec_in.get(), pin, bytes, hipMemcpyHostToDevice, st));
    RecordRootsDev Rd{};
    const uint8_t *base = s->rec_in.get();
    Rd.offsets = reinterpret_cast<const int64_t *>(base + o_off);
    Rd.moves = reinterpret_cast<const int32_t *>(base + o_moves);
    Rd.colors = colors_host ? reinterpret_cast<const int8_t *>(base + o_col) : nullptr;
    Rd.rec = reinterpret_cast<const int32_t *>(base + o_rec);
    Rd.m_off = reinterpret_cast<const int32_t *>(base + o_moff);
    Rd.m_ply = reinterpret_cast<const int32_t *>(base + o_ply);
    Rd.m_tree = reinterpret_cast<const int32_t *>(base + o_tree);
    Rd.flags = s->rec_flags.get();
    Rd.n_rec = (int)R;
    const size_t grid_cap = (size_t)s->num_cus * 32;      // one-wave workgroups: the waves a CU holds (tg_replay_create)
    const int grid = (int)(R < grid_cap ? R : grid_cap);
    with_board_size(s->S, [&](auto size) {
        hipLaunchKernelGGL(record_roots_kernel<decltype(size)::value>, dim3(grid), dim3(64), 0, st, s->dev, Rd);
    });
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(s->rec_flags_back.get(), s->rec_flags.get(), (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    // later call wins per tree: a position staged earlier for a tree written here is dropped; a flagged tree keeps what it had
    for (const Member &m : members) {
        flags_host[m.tree] = s->rec_flags_back.get()[m.tree] ? 1 : 0;
        if (!flags_host[m.tree]) s->roots.drop(m.tree);
    }
    return TG_OK;
}

int tg_search_set_noise(tg_search *s, const double *noise_host) {
    if (!s || !noise_host) return tg::fail(TG_ERR_ARG, "tg_search_set_noise: null argument");
    const size_t n = (size_t)s->dev.T * s->A;
    s->rng.set_host_noise(noise_host);
    if (!s->stream_known) {                        // no launch stream yet: the null stream, synchronously
        TG_HIP(hipDeviceSynchronize());
        TG_HIP(hipMemcpy(s->dev.noise, noise_host, n * sizeof(double), hipMemcpyHostToDevice));
        return TG_OK;
    }
    double *pin;
    int slot;
    if (int rc = s->noise_pin.acquire(n, &pin, &slot)) return rc;                  // (waits for four uploads ago: long done)
    std::memcpy(pin, noise_host, n * sizeof(double));
    // in stream order: behind the kernels that read the previous noise (the last search), ahead of the next selection
    TG_HIP(hipMemcpyAsync(s->dev.noise, pin, n * sizeof(double), hipMemcpyHostToDevice, s->last_stream));
    return s->noise_pin.commit(slot, s->last_stream);
}

// ---- library-owned legacy streams, device-resident (csrc/legacy_rng_device.h): tg_search::Streams ---------------

static_assert(tg_streams::kMtN == tg_rng::kMtN && tg_streams::kSnapEvery == tg_rng::kSnapEvery, "stream_windows.h restates the generator's constants");

// TG_RNG_OVERGEN (windows' worth a few-tree window is over-generated to; read once), TG_RNG_NO_SNAP (no state snapshots; read per launch)
static int knob_overgen() {
    static const int overgen = tg::knob("TG_RNG_OVERGEN") ? std::max(1, atoi(tg::knob("TG_RNG_OVERGEN"))) : tg_streams::kOvergenDefault;
    return overgen;
}
static bool knob_no_snap() { return tg::knob("TG_RNG_NO_SNAP") != nullptr; }

// on the first seed (the seed staging rows and the lag ring are pinned at their first use: sync_seeds, generate)
int tg_search::Streams::alloc() {
    if (noise_back_.get()) return TG_OK;                 // (the last of the set: a failure half-way is made up for by the next call)
    const size_t T = (size_t)T_, words = T * tg_rng::kStateWords;
    int rc;
    if ((rc = base_.reserve(words)) || (rc = cont_.reserve(words)) || (rc = pos0_.reserve(T)) || (rc = snap_n_.reserve(T)) ||
        (rc = cont_blk_.reserve(T)))
        return rc;
    TG_HIP(hipMemset(snap_n_.get(), 0, T * sizeof(int)));
    TG_HIP(hipMemset(cont_blk_.get(), 0, T * sizeof(long long)));
    TG_HIP(hipMemset(base_.get(), 0, words * sizeof(uint32_t)));
    TG_HIP(hipMemset(cont_.get(), 0, words * sizeof(uint32_t)));
    TG_HIP(hipStreamSynchronize(nullptr));               // (the fills above: not ordered before a non-blocking stream otherwise)
    seeds_.resize(words);
    book_.create(T_);
    return noise_back_.alloc(T * (size_t)A_);
}

int tg_search::Streams::seed(int tree, const uint32_t *mt_key, int mt_pos) {
    if (int rc = alloc()) return rc;
    uint32_t *row = &seeds_[(size_t)tree * tg_rng::kStateWords];
    std::memcpy(row, mt_key, tg_rng::kMtN * sizeof(uint32_t));
    row[tg_rng::kMtN] = (uint32_t)mt_pos;
    book_.seed(tree);
    return TG_OK;
}

// MT19937's init_genrand: the 624 words from one 32-bit seed.  numpy's RandomState(seed) for an integer below 2^32 IS this
// state at position 624 (_legacy_seeding -> mt19937_seed); CPython's random.seed mixes a key into the one for 19650218
// (tg_policy_seed_states).
static void mt_init_genrand(uint32_t seed, uint32_t *mt) {
    mt[0] = seed;
    for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
}

int tg_search::Streams::seed_all(const uint32_t *seeds) {
    if (int rc = alloc()) return rc;
    parallel_trees(T_, [&](int t) {
        uint32_t *row = &seeds_[(size_t)t * tg_rng::kStateWords];
        mt_init_genrand(seeds[t], row);
        row[tg_rng::kMtN] = tg_rng::kMtN;
        book_.seed(t);
    });
    return TG_OK;                                  // (every row dirty: sync_seeds sends them up in one copy)
}

int tg_search::Streams::check_seeded(const char *entry, const uint8_t *skip) const {
    const int bad = book_.first_unseeded(T_, skip);
    if (bad == tg_streams::StreamBook::kNoneSeeded) return tg::fail(TG_ERR_ARG, "%s: streams are not seeded", entry);
    return bad < 0 ? TG_OK : tg::fail(TG_ERR_ARG, "%s: tree %d has no stream", entry, bad);
}

// seeds that have not gone up yet: staged in pinned memory, copied on the generation stream ahead of the launch that needs them
int tg_search::Streams::sync_seeds() {
    int t0, t1 = 0;
    if (!book_.next_dirty_run(0, &t0, &t1)) return TG_OK;
    uint32_t *pin;
    int slot;
    if (int rc = seed_pin_.acquire(seeds_.size(), &pin, &slot)) return rc;   // (waits for the previous use of the staging rows)
    do {
        const size_t o = (size_t)t0 * tg_rng::kStateWords, n = (size_t)(t1 - t0) * tg_rng::kStateWords;
        std::memcpy(pin + o, &seeds_[o], n * sizeof(uint32_t));
        TG_HIP(hipMemcpyAsync(base_.get() + o, pin + o, n * sizeof(uint32_t), hipMemcpyHostToDevice, cs_));
        TG_HIP(hipMemsetAsync(snap_n_.get() + t0, 0, (size_t)(t1 - t0) * sizeof(int), cs_));   // (snapshots of the old stream; defensive: stream_windows.h)
    } while (book_.next_dirty_run(t1, &t0, &t1));
    return seed_pin_.commit(slot, cs_);
}

int tg_search::Streams::generate(const tg_streams::Piece &p, const uint8_t *skip, const NoiseOrder *order) {
    using tg_streams::Kind;
    const int T = T_;
    int rc, slot = -1;
    tg_rng::FillArgs a{};
    if ((rc = sync_seeds())) return rc;
    if (!p.from_cont) {
        // The draws consumed since the device states were brought up to date: a slot of the host-mapped ring (the launch reads
        // it over the bus: T x 8 bytes), [T] lag (int64) | [T] skip (bytes); committed behind the launch
        long long *lag;
        if ((rc = lag_ring_.acquire((size_t)T + ((size_t)T + 7) / 8, &lag, &slot, hipHostMallocMapped))) return rc;   // (waits for eight launches ago: long done)
        unsigned char *sk = reinterpret_cast<unsigned char *>(lag + T);
        for (int t = 0; t < T; ++t) {
            sk[t] = skip && skip[t] ? 1 : 0;
            lag[t] = (long long)book_.take_lag(t, sk[t] != 0);
        }
        a.lag = lag_ring_.dev(slot);
    }
    if (p.kind == Kind::Noise) {
        if ((rc = order_noise(*order))) return rc;
        a.skip = reinterpret_cast<const unsigned char *>(a.lag + T);
        a.noise = noise_dev_;
    }
    if (win_->book().refuses(p))                   // (stream_windows.h: the continuation state is that window's)
        return tg::fail(TG_ERR_STATE, "random streams: a generation launch from the base state while a window has columns to come");
    // (growing frees the old scratch first: implicit device synchronisation, rare - the largest piece so far)
    const long long pitch = tg_streams::scratch_pitch(p.count);
    if ((rc = words_.reserve((size_t)T * (size_t)pitch))) return rc;
    a.base = base_.get(); a.cont = cont_.get(); a.from_cont = p.from_cont ? 1 : 0;
    if (p.kind == Kind::Window) a.out = win_->buffer(p.buf);
    a.pitch = p.pitch; a.first = p.first; a.count = p.count;
    a.words = words_.get(); a.words_pitch = pitch; a.pos0 = pos0_.get();
    const size_t per_snap = (size_t)T * tg_rng::kMtN;
    const tg_streams::SnapPlan snaps = tg_streams::snap_plan(T, knob_no_snap(), p, (int64_t)(snap_.capacity() / per_snap));
    if (snaps.on) {
        if (snaps.grow) {
            // (frees the old snapshots first: implicit device synchronisation, rare - the largest window so far)
            if ((rc = snap_.reserve((size_t)snaps.want * per_snap))) return rc;
            TG_HIP(hipMemsetAsync(snap_n_.get(), 0, (size_t)T * sizeof(int), cs_));
        }
        a.snap = snap_.get(); a.snap_cap = (int)(snap_.capacity() / per_snap); a.snap_n = snap_n_.get();
    }
    a.cont_blk = cont_blk_.get();
    hipLaunchKernelGGL(tg_rng::rng_words_kernel, dim3(T), dim3(64), 0, cs_, a);
    TG_HIP(hipGetLastError());
    if (a.count > 0) {
        hipLaunchKernelGGL(tg_rng::rng_draws_kernel, dim3((unsigned)((a.count + 255) / 256), T), dim3(256), 0, cs_, a);
        TG_HIP(hipGetLastError());
    }
    return slot >= 0 ? lag_ring_.commit(slot, cs_) : TG_OK;
}

int tg_search::Streams::state(int tree, uint32_t *mt_key_out, int *mt_pos_out) {
    const uint32_t *row = &seeds_[(size_t)tree * tg_rng::kStateWords];
    if (!book_.unused(tree)) {
        // bring the device states up to date (a generation launch of zero draws commits the consumed ones), then read this tree's
        int rc, seed_slot;                          // (not committed: the copy below is waited for here)
        uint32_t *pin;
        if ((rc = generate(tg_streams::Piece{}, nullptr, nullptr)) || (rc = seed_pin_.acquire(seeds_.size(), &pin, &seed_slot))) return rc;
        pin += (size_t)tree * tg_rng::kStateWords;
        TG_HIP(hipMemcpyAsync(pin, base_.get() + (size_t)tree * tg_rng::kStateWords, tg_rng::kStateWords * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, cs_));
        TG_HIP(hipStreamSynchronize(cs_));
        row = pin;
    }
    std::memcpy(mt_key_out, row, tg_rng::kMtN * sizeof(uint32_t));
    *mt_pos_out = (int)row[tg_rng::kMtN];
    return TG_OK;
}

int tg_search_seed_stream(tg_search *s, int tree, const uint32_t *mt_key, int mt_pos) {
    if (!s || !mt_key) return tg::fail(TG_ERR_ARG, "tg_search_seed_stream: null argument");
    if (tree < 0 || tree >= s->dev.T) return tg::fail(TG_ERR_ARG, "tg_search_seed_stream: tree %d out of range", tree);
    if (mt_pos < 0 || mt_pos > 624) return tg::fail(TG_ERR_ARG, "tg_search_seed_stream: MT19937 position %d outside [0, 624]", mt_pos);
    TG_HIP(hipSetDevice(s->cfg.device));
    if (int rc = s->rng.seed(tree, mt_key, mt_pos)) return rc;
    s->win.abandon();                              // the generated window belongs to the old stream
    return TG_OK;
}

int tg_search_seed_streams(tg_search *s, const uint32_t *seeds_host) {
    if (!s || !seeds_host) return tg::fail(TG_ERR_ARG, "tg_search_seed_streams: null argument");
    TG_HIP(hipSetDevice(s->cfg.device));
    if (int rc = s->rng.seed_all(seeds_host)) return rc;
    s->win.abandon();                              // the generated window belongs to the old streams
    return TG_OK;
}

int tg_search_stream_state(tg_search *s, int tree, uint32_t *mt_key_out, int *mt_pos_out) {
    if (!s || !mt_key_out || !mt_pos_out) return tg::fail(TG_ERR_ARG, "tg_search_stream_state: null argument");
    if (!s->rng.has_stream(tree)) return tg::fail(TG_ERR_ARG, "tg_search_stream_state: tree %d has no stream", tree);
    // An observer - the search may go on from the window in place: the commit starts from the base state, so a rest still to
    // come (deferred or not) is completed first, and the next selection launch waits for it as it would have
    if (!s->rng.unused(tree))
        if (int rc = s->win.complete_rest(s->rng)) return rc;
    return s->rng.state(tree, mt_key_out, mt_pos_out);
}

// The next window of `need` draws per tree, unless the one in place still covers the request (and `force` is off).  first > 0:
// in parts - the first `first` draws of every tree's row now, enough for the first launch, the rest by Windows::extend /
// complete_rest while that launch runs (tg_streams::feed_rule).
static int feed_streams_impl(tg_search *s, size_t need, int force, size_t first) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_feed_streams: null argument");
    int rc;
    if ((rc = s->win.settle(s->rng))) return rc;   // (an earlier window in parts was never completed: complete it first)
    if ((rc = s->rng.check_seeded("tg_search_feed_streams", nullptr))) return rc;
    const tg_streams::Feed f = tg_streams::feed_rule(s->dev.T, (int64_t)need, force != 0, (int64_t)first, s->win.book().left(), knob_overgen());
    return f.start ? s->win.start(s->rng, f.pitch, f.cols, f.eager) : TG_OK;
}

int tg_search_feed_streams(tg_search *s, size_t need, int force) { return feed_streams_impl(s, need, force, 0); }

// skip[t] != 0: tree t's stream was replaced since the window was generated - what the device consumed there is not its (a
// self-play slot whose game ended while the device had already gone on to the next root)
// used_in: the device cursors, if the caller has them already (publish_cursors_kernel)
static int advance_streams_impl(tg_search *s, int64_t *consumed_host, const uint8_t *skip, const int64_t *used_in = nullptr) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_advance_streams: null argument");
    const int T = s->dev.T;
    if (int rc = s->rng.check_seeded("tg_search_advance_streams", skip)) return rc;
    std::vector<int64_t> used(T);
    if (used_in) {
        std::memcpy(used.data(), used_in, (size_t)T * sizeof(int64_t));
    } else {
        int rc = tg_search_rng_consumed(s, used.data());
        if (rc) return rc;
    }
    std::vector<int64_t> delta(T);
    const int bad = s->win.record(used.data(), skip, T, delta.data());
    if (bad >= 0)
        return tg::fail(TG_ERR_ARG, "tg_search_advance_streams: tree %d consumed %lld draws, cursor %lld of a window of %lld", bad,
                        (long long)delta[bad], (long long)used[bad], (long long)s->win.book().capacity());
    for (int t = 0; t < T; ++t) {
        const bool skipped = skip && skip[t];
        s->rng.add_consumed(t, delta[t], skipped);
        if (consumed_host) consumed_host[t] = skipped ? 0 : delta[t];
    }
    // Few trees: the next window is generated NOW - the consumed draws committed, two windows' worth generated - instead of in
    // front of the next selection launch (one 19x19 tree: five regenerations per move, ~90 us each).  Nothing is consumed
    // between here and that launch, so its tg_search_feed_streams finds the window in place.
    if (const int64_t need = s->win.book().eager_due(skip != nullptr)) return feed_streams_impl(s, (size_t)need, 0, 0);
    return TG_OK;
}

int tg_search_advance_streams(tg_search *s, int64_t *consumed_host) { return advance_streams_impl(s, consumed_host, nullptr); }

// the last root noise on the host (finish_move's own arithmetic, callers that ask for it): a device-drawn one is waited for
int tg_search::Streams::host_noise(const double **noise, size_t *count) {
    if (noise_back_pending_) {
        TG_HIP(hipEventSynchronize(noise_back_ev_.get()));
        noise_host_.assign(noise_back_.get(), noise_back_.get() + (size_t)T_ * A_);
        noise_back_pending_ = false;
    }
    *noise = noise_host_.data();
    *count = noise_host_.size();
    return TG_OK;
}

int tg_search::Streams::clear_host_noise(int tree) {
    const double *rows;
    size_t count;
    if (int rc = host_noise(&rows, &count)) return rc;         // (a device-drawn one on its way back lands first)
    if (count >= (size_t)(tree + 1) * A_) std::fill(noise_host_.begin() + (size_t)tree * A_, noise_host_.begin() + (size_t)(tree + 1) * A_, 0.0);
    return TG_OK;
}

// the generation stream behind the readers of the previous noise
int tg_search::Streams::order_noise(const NoiseOrder &o) {
    if (o.after) {
        TG_HIP(hipStreamWaitEvent(cs_, o.after, 0));
    } else if (o.launch_known) {
        if (int rc = noise_order_ev_.record(o.launch)) return rc;
        TG_HIP(hipStreamWaitEvent(cs_, noise_order_ev_.get(), 0));
    } else {
        TG_HIP(hipDeviceSynchronize());
    }
    return TG_OK;
}

// node.py:275-278 for every root: A draws of each tree's stream as Gumbel(0, 1) = -log(-log(1 - u)), generated on the device
// straight into the root noise rows, in stream order behind the kernels that read the previous noise and ahead of the next
// selection.  skip[t] != 0: tree t draws nothing (zero noise) - its stream must not move yet.
int tg_search::Streams::draw_noise(const uint8_t *skip, const NoiseOrder &order) {
    int rc;
    const double *rows;
    size_t n;
    tg_streams::Piece p;
    p.kind = tg_streams::Kind::Noise;
    p.count = A_;
    if ((rc = host_noise(&rows, &n)) || (rc = generate(p, skip, &order))) return rc;      // (the staging rows are about to be rewritten: a noise still on its way is taken in first)
    TG_HIP(hipMemcpyAsync(noise_back_.get(), noise_dev_, (size_t)T_ * A_ * sizeof(double), hipMemcpyDeviceToHost, cs_));
    if ((rc = noise_back_ev_.record(cs_))) return rc;
    noise_back_pending_ = true;
    if (order.launch_known) TG_HIP(hipStreamWaitEvent(order.launch, noise_back_ev_.get(), 0));
    else TG_HIP(hipStreamSynchronize(cs_));
    return TG_OK;
}

// order_after: an event the caller knows to lie behind every reader of the previous noise (self-play's chained moves: the
// cursor event, recorded right behind the root expansion - the noise is then generated UNDER the root's forward pass and
// backup instead of behind them); null: behind everything queued on the launch stream so far.
static int draw_noise_impl(tg_search *s, double *noise_host, const uint8_t *skip, hipEvent_t order_after = nullptr) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_draw_noise: null argument");
    int rc;
    if ((rc = s->rng.check_seeded("tg_search_draw_noise", skip))) return rc;
    // The noise sits between two windows, and its launch moves the base state.  A window in parts: a rest that launches may be
    // waiting for is completed (no driver leaves one open here), a deferred one is dropped with its never-installed window -
    // abandoned, so every request that follows starts a new window, and nothing reads columns from behind the noise.
    if ((rc = s->win.settle(s->rng))) return rc;
    s->win.abandon();
    if ((rc = s->rng.draw_noise(skip, {order_after, s->stream_known, s->last_stream}))) return rc;
    if (noise_host) {
        const double *rows;
        size_t n;
        if ((rc = s->rng.host_noise(&rows, &n))) return rc;
        std::memcpy(noise_host, rows, n * sizeof(double));
    }
    return TG_OK;
}

int tg_search_draw_noise(tg_search *s, double *noise_host) { return draw_noise_impl(s, noise_host, nullptr); }

// A launch stream that belongs to the handle (non-blocking, created on first request): self-play lanes run each engine on one of
// these instead of streams out of the host framework's pool - the hardware queue a stream lands on goes by creation order, and
// a pool of 32 streams created in one go leaves the library's own streams sharing queues with them (measured: two lanes on pool
// streams 2.99-3.10 M leaf-evals/s, on streams created here 3.65 M).
int tg_search_own_stream(tg_search *s, void **stream_out) {
    if (!s || !stream_out) return tg::fail(TG_ERR_ARG, "tg_search_own_stream: null argument");
    TG_HIP(hipSetDevice(s->cfg.device));
    if (int rc = s->own_stream.create()) return rc;
    *stream_out = s->own_stream.get();
    return TG_OK;
}

// ---- test hooks of the device streams (tests/test_gpu_rng.py) ----
// columns [first, first + count) of tree `tree`'s row of the most recently generated window
int tg_search_debug_read_window(tg_search *s, int tree, size_t first, size_t count, double *out_host) {
    if (!s || (!out_host && count)) return tg::fail(TG_ERR_ARG, "tg_search_debug_read_window: null argument");
    int64_t pitch;
    const double *win = s->win.buffer(s->win.book().newest(&pitch));
    if (tree < 0 || tree >= s->dev.T || !win || (int64_t)(first + count) > pitch)
        return tg::fail(TG_ERR_ARG, "tg_search_debug_read_window: outside the window (%lld draws per tree)", (long long)pitch);
    TG_HIP(hipStreamSynchronize(s->copy_stream.get()));
    TG_HIP(hipMemcpy(out_host, win + (size_t)tree * pitch + first, count * sizeof(double), hipMemcpyDeviceToHost));
    return TG_OK;
}

// What a search does to the streams, without a search: per step a window of steps[i] + slack draws is generated - whole
// (part == 0) or in parts of `part` draws (first part, continued pieces, the rest: Windows::start / extend / complete_rest) - and
// steps[i] draws of every tree count as consumed.
int tg_search_debug_stream_walk(tg_search *s, const int64_t *steps, int n_steps, int64_t slack, int64_t part) {
    if (!s || !steps || n_steps < 0 || slack < 0 || part < 0) return tg::fail(TG_ERR_ARG, "tg_search_debug_stream_walk: bad argument");
    int rc;
    for (int i = 0; i < n_steps; ++i) {
        if (steps[i] < 0) return tg::fail(TG_ERR_ARG, "tg_search_debug_stream_walk: negative step");
        const size_t need = (size_t)(steps[i] + slack);
        if (need == 0) continue;
        if ((rc = feed_streams_impl(s, need, 1, part > 0 ? (size_t)part : 0))) return rc;
        if (part > 0) {
            for (size_t upto = (size_t)(2 * part); upto + (size_t)part < need; upto += (size_t)part)
                if ((rc = s->win.extend(s->rng, upto, s->copy_stream.get()))) return rc;
            if ((rc = s->win.complete_rest(s->rng))) return rc;
        }
        for (int t = 0; t < s->dev.T; ++t) s->rng.add_consumed(t, steps[i], false);
        s->win.abandon();
    }
    return TG_OK;
}

// trees [t0, t0 + n) of the engine as a device view of their own (every per-tree array moved on; same kernels)
static SearchDev sub_dev(const tg_search *s, int t0, int n) {
    SearchDev D = s->dev;
    const size_t o = (size_t)t0, N = (size_t)D.N, A = (size_t)s->A, K = (size_t)D.K;
#define SUB(field, E, per_child, remap) D.field += o * N * tg_pool::per_node(per_child, A);
    TG_NODE_POOL_ARRAYS(SUB)
#undef SUB
    D.noise += o * A;
    D.root_cells += o * s->NC; D.root_hist += o * s->HMAX; D.meta += o;
#define SUB(field, E, per_slot) D.field += o * K * (per_slot);
    TG_LEAF_QUEUE_ARRAYS(SUB)
#undef SUB
    D.n_leaves += o;
    D.rng += o * (size_t)D.rng_cap; D.rng_cursor += o; D.err += o; D.halt += o;
    if (D.cursor_pub) D.cursor_pub += o;
    D.T = n;
    return D;
}

int tg_search_select_gumbel(tg_search *s, const int32_t *num_considered_host, const int32_t *max_count_host,
                            int slots_per_tree, float *planes_dev, void *stream) {
    if (!s || !num_considered_host || !max_count_host || !planes_dev)
        return tg::fail(TG_ERR_ARG, "tg_search_select_gumbel: null argument");
    LeafLayout layout;
    if (!leaf_layout(slots_per_tree, s->dev.K, &layout))
        return tg::fail(TG_ERR_ARG, "tg_search_select_gumbel: slots_per_tree %d outside [1, batch_size]", slots_per_tree);
    const int T = s->dev.T;
    const bool strided = layout == LeafLayout::Strided, unique = layout == LeafLayout::Unique;
    const int limit = strided ? slots_per_tree : s->dev.K;
    // staging: [num_considered | max_count | leaf offsets] in a ring of pinned buffers (a pageable staging vector
    // needed a stream synchronisation per phase: the host then waited for the previous phase's forward and backup)
    // (a slot whose phase is refused below is simply never committed)
    int32_t *phase_host;
    int ring, rc;
    if ((rc = s->phase_pin.acquire((size_t)3 * T, &phase_host, &ring))) return rc;
    if (unique) s->last.caps.resize(T);
    PhaseLayout ph;
    if ((rc = layout_phase(s, "tg_search_select_gumbel", num_considered_host, max_count_host, 0, T, limit, layout, 0, phase_host,
                           unique ? s->last.caps.data() : nullptr, &ph)))
        return rc;
    hipStream_t st = use_stream(s, stream);
    if (!s->phase_dev.get() && (rc = s->phase_dev.alloc_zeroed((size_t)3 * T))) return rc;
    const int32_t *phase_dev = s->phase_dev.get();
    TG_HIP(hipMemcpyAsync(s->phase_dev.get(), phase_host, (size_t)3 * T * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = s->phase_pin.commit(ring, st)) || (rc = s->win.install(s->rng, &s->dev, st))) return rc;
    s->last.subgroups = false;
    s->last.layout = layout;
    s->last.planes = ph.positions;
    const int32_t *off = strided ? nullptr : phase_dev + 2 * (size_t)T;
    if ((rc = launch_gumbel_select(s, s->dev, phase_dev, phase_dev + T, off, limit, ph.max_n, planes_dev, st, unique))) return rc;
    return after_select(s, st);
}

// The planes the forward pass must cover after the last UNIQUE selection (slots_per_tree -1), and each tree's share: tree t's
// distinct leaves lie at the start of its range of cap[t] slots, in the order of their first descents (tree.py:375-384 queues
// one leaf per descent; a phase's descents through one root child, node.py:324-346, end on the same leaf).  Host arithmetic,
// no synchronisation.
int tg_search_unique_planes(tg_search *s, int64_t *total_host, int32_t *cap_host) {
    if (!s || !total_host) return tg::fail(TG_ERR_ARG, "tg_search_unique_planes: null argument");
    if (!s->last.whole(LeafLayout::Unique)) return tg::fail(TG_ERR_STATE, "tg_search_unique_planes: the last selection was not a unique one");
    *total_host = s->last.planes;
    if (cap_host) std::memcpy(cap_host, s->last.caps.data(), s->last.caps.size() * sizeof(int32_t));
    return TG_OK;
}

int tg_search_backup(tg_search *s, const float *policy_dev, const float *value_dev, int slots_per_tree,
                     int use_logit, void *stream) {
    if (!s || !policy_dev || !value_dev) return tg::fail(TG_ERR_ARG, "tg_search_backup: null argument");
    LeafLayout layout;
    const bool in_range = leaf_layout(slots_per_tree, s->dev.K, &layout);
    const bool strided = layout == LeafLayout::Strided, unique = layout == LeafLayout::Unique;
    if (layout == LeafLayout::Packed && s->last.layout != LeafLayout::Packed)      // (a move's packed sub-groups count)
        return tg::fail(TG_ERR_ARG, "tg_search_backup: packed layout (slots_per_tree 0) needs a preceding packed tg_search_select_gumbel");
    if (unique && !s->last.whole(LeafLayout::Unique))
        return tg::fail(TG_ERR_ARG, "tg_search_backup: unique layout (slots_per_tree -1) needs a preceding unique tg_search_select_gumbel");
    if (!in_range) return tg::fail(TG_ERR_ARG, "tg_search_backup: slots_per_tree %d outside [1, batch_size]", slots_per_tree);
    if (strided && s->last.layout == LeafLayout::Compact)
        return tg::fail(TG_ERR_ARG, "tg_search_backup: the last selection was a compact one (tg_search_backup_compact reads its rows)");
    hipStream_t st = use_stream(s, stream);
    const int32_t *off = strided ? nullptr : s->phase_dev.get() + 2 * (size_t)s->dev.T;
    return launch_backup(s, s->dev, policy_dev, value_dev, strided ? slots_per_tree : 0, off, use_logit, st, unique);
}

int tg_search_backup_compact(tg_search *s, const float *policy_dev, const float *value_dev, int slots_per_tree,
                             int use_logit, void *stream) {
    if (!s || !policy_dev || !value_dev) return tg::fail(TG_ERR_ARG, "tg_search_backup_compact: null argument");
    if (slots_per_tree < 1 || slots_per_tree > s->dev.K)
        return tg::fail(TG_ERR_ARG, "tg_search_backup_compact: slots_per_tree %d outside [1, batch_size] (the compact layout has no packed or unique form)",
                        slots_per_tree);
    if (!s->last.whole(LeafLayout::Compact))
        return tg::fail(TG_ERR_ARG, "tg_search_backup_compact: needs a preceding compact PUCT selection of the whole engine");
    hipStream_t st = use_stream(s, stream);
    return launch_backup(s, compact_dev(s), policy_dev, value_dev, slots_per_tree, nullptr, use_logit, st, false);
}

}  // extern "C"

// root records of all trees -> s->roots_host (pinned); also surfaces the sticky error flags
using tg_readout::root_record_bytes, tg_readout::root_record_offset;
static int alloc_root_records(tg_search *s) {                   // [T] records, then [T] RootTail
    if (s->roots_host.get()) return TG_OK;
    const size_t bytes = tg_readout::root_records_bytes(s->dev.T, s->A);
    if (int rc = s->roots_dev.reserve(bytes)) return rc;
    return s->roots_host.alloc(bytes);
}
static void parse_root_records(const tg_search *s, int32_t *num_children_host, int32_t *node_visits_host, float *raw_value_host,
                               int32_t *action_host, int32_t *visits_host, int32_t *virtual_loss_host, double *value_sum_host,
                               double *policy_host) {
    const size_t A = s->A, T = s->dev.T, rec = root_record_bytes(A);
    for (size_t t = 0; t < T; ++t) {
        const unsigned char *r = s->roots_host.get() + rec * t;
        const int32_t *head = reinterpret_cast<const int32_t *>(r);
        if (num_children_host) num_children_host[t] = head[tg_readout::kRootChildren];
        if (node_visits_host) node_visits_host[t] = head[tg_readout::kRootVisits];
        if (raw_value_host) std::memcpy(&raw_value_host[t], &head[tg_readout::kRootRawBits], 4);
        // every row to the caller's <row>_host: a row added to the list without a destination here does not compile
#define GET(row, E, member) \
        if (row##_host) std::memcpy(row##_host + t * A, r + root_record_offset(tg_readout::kRoot_##row, A), A * sizeof(E));
        TG_ROOT_RECORD_ROWS(GET)
#undef GET
    }
}
static int root_record_errors(const tg_search *s) {
    const size_t rec = root_record_bytes(s->A);
    for (int t = 0; t < s->dev.T; ++t) {
        const int32_t err = reinterpret_cast<const int32_t *>(s->roots_host.get() + rec * t)[tg_readout::kRootErr];
        if (err) return fail_tree(t, err);
    }
    return TG_OK;
}
// the records + the device's own decision (finish_roots_kernel), queued on `st`; the host waits for fin_ev, not for the stream
static int launch_finish_roots(tg_search *s, const int32_t *state_host, int max_moves, hipStream_t st) {
    const int T = s->dev.T, A = s->A;
    const size_t rec = root_record_bytes(A), n = (size_t)tg_readout::kStateWords * T;
    int rc;
    if ((rc = alloc_root_records(s))) return rc;
    if (!s->moves_dev.get() && (rc = s->moves_dev.alloc_zeroed((size_t)T))) return rc;
    if (!s->state_dev.get() && (rc = s->state_dev.alloc_zeroed(n))) return rc;
    int32_t *pin;
    int slot;
    if ((rc = s->state_pin.acquire(n, &pin, &slot))) return rc;
    std::memcpy(pin, state_host, n * sizeof(int32_t));
    TG_HIP(hipMemcpyAsync(s->state_dev.get(), pin, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = s->state_pin.commit(slot, st))) return rc;
    unsigned char *roots_dev = s->roots_dev.get();
    RootTail *tail_dev = reinterpret_cast<RootTail *>(roots_dev + tg_readout::root_tail_offset(T, A));
    hipLaunchKernelGGL(finish_roots_kernel, dim3(T), dim3(64), 0, st, s->dev, A, roots_dev, rec, s->state_dev.get(), max_moves,
                       s->moves_dev.get(), tail_dev);
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(s->roots_host.get(), roots_dev, tg_readout::root_records_bytes(T, A), hipMemcpyDeviceToHost, st));
    return s->fin_ev.record(st);
}
static int gather_roots(tg_search *s) {
    const int T = s->dev.T, A = s->A;
    const size_t rec = root_record_bytes(A);
    if (int rc = alloc_root_records(s)) return rc;
    hipStream_t st = s->last_stream;
    hipLaunchKernelGGL(gather_roots_kernel, dim3(T), dim3(64), 0, st, s->dev, A, s->roots_dev.get(), rec);
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(s->roots_host.get(), s->roots_dev.get(), rec * T, hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    return root_record_errors(s);
}

extern "C" {

int tg_search_read_roots(tg_search *s, int32_t *num_children_host, int32_t *action_host,
                         int32_t *visits_host) {
    if (!s || !num_children_host || !action_host || !visits_host)
        return tg::fail(TG_ERR_ARG, "tg_search_read_roots: null argument");
    return tg_search_read_root_stats(s, num_children_host, nullptr, nullptr, action_host, visits_host, nullptr, nullptr, nullptr);
}

int tg_search_read_root_stats(tg_search *s, int32_t *num_children_host, int32_t *node_visits_host,
                              float *raw_value_host, int32_t *action_host, int32_t *visits_host,
                              int32_t *virtual_loss_host, double *value_sum_host, double *policy_host) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_read_root_stats: null argument");
    int rc = gather_roots(s);
    if (rc) return rc;
    parse_root_records(s, num_children_host, node_visits_host, raw_value_host, action_host, visits_host, virtual_loss_host,
                       value_sum_host, policy_host);
    return TG_OK;
}

static_assert(sizeof(tg_best_move) == sizeof(BestMove) && offsetof(tg_best_move, value_sum) == offsetof(BestMove, value_sum) &&
                  offsetof(tg_best_move, status) == offsetof(BestMove, status),
              "include/tamago_hip.h restates csrc/readout.h's BestMove");

int tg_search_best_moves(tg_search *s, double resign_threshold, int play, const uint8_t *sit_out_host, tg_best_move *records_host,
                         void *stream) {
    if (!s || !records_host) return tg::fail(TG_ERR_ARG, "tg_search_best_moves: null argument");
    if (play != 0 && play != 1) return tg::fail(TG_ERR_ARG, "tg_search_best_moves: play %d is neither 0 nor 1", play);
    if (resign_threshold != resign_threshold) return tg::fail(TG_ERR_ARG, "tg_search_best_moves: resign_threshold is not a number");
    hipStream_t st = use_stream(s, stream);
    const size_t T = (size_t)s->dev.T;
    int rc;
    if (play && (rc = flush_roots(s, st))) return rc;            // (a staged position is played on, as tg_search_play does)
    if (play) s->roots_expanded = false;
    if (!s->best_host.get() && ((rc = s->best_dev.reserve(T)) || (rc = s->best_host.alloc(T)))) return rc;
    const uint8_t *sit_dev = nullptr;
    if (sit_out_host) {
        if (!s->sit_dev.get() && (rc = s->sit_dev.alloc_zeroed(T))) return rc;
        uint8_t *pin;
        int slot;
        if ((rc = s->sit_pin.acquire(T, &pin, &slot))) return rc;
        std::memcpy(pin, sit_out_host, T);
        TG_HIP(hipMemcpyAsync(s->sit_dev.get(), pin, T, hipMemcpyHostToDevice, st));
        if ((rc = s->sit_pin.commit(slot, st))) return rc;
        sit_dev = s->sit_dev.get();
    }
    with_board_size(s->S, [&](auto size) {
        hipLaunchKernelGGL(best_moves_kernel<decltype(size)::value>, dim3(s->dev.T), dim3(64), 0, st, s->dev, resign_threshold, play,
                           sit_dev, s->best_dev.get());
    });
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(s->best_host.get(), s->best_dev.get(), T * sizeof(BestMove), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    std::memcpy(records_host, s->best_host.get(), T * sizeof(BestMove));
    for (size_t t = 0; t < T; ++t) {
        const int32_t status = s->best_host.get()[t].status;
        if (status & tg_readout::kBestTreeError) return check_errors(s);
        if (status & tg_readout::kBestNoRoot) return tg::fail(TG_ERR_STATE, "tg_search_best_moves: tree %zu has no expanded root", t);
    }
    return TG_OK;
}

int tg_search_read_path(tg_search *s, int tree, int slot, int32_t *nodes_host, int32_t *edges_host, int capacity,
                        int32_t *length_host) {
    if (!s || !nodes_host || !edges_host || !length_host)
        return tg::fail(TG_ERR_ARG, "tg_search_read_path: null argument");
    if (tree < 0 || tree >= s->dev.T || slot < 0 || slot >= s->dev.K)
        return tg::fail(TG_ERR_ARG, "tg_search_read_path: tree %d / slot %d out of range", tree, slot);
    if (int rc = sync_launch_stream(s)) return rc;
    const SearchDev &D = s->dev;
    // (the queue entries stay valid until the next selection launch, also after tg_search_backup)
    // leaf -> root over the parent pointers, then reversed into the reference's root -> leaf order
    std::vector<int32_t> nodes, edges;
    int32_t cur = -1, e = -1;
    const size_t q = (size_t)tree * D.K + slot;
    TG_HIP(hipMemcpy(&cur, D.q_pnode + q, sizeof(int32_t), hipMemcpyDeviceToHost));
    TG_HIP(hipMemcpy(&e, D.q_pedge + q, sizeof(int32_t), hipMemcpyDeviceToHost));
    while (cur >= 0) {
        nodes.push_back(cur);
        edges.push_back(e);
        const size_t cs = (size_t)tree * D.N + cur;
        NodeRec rec;
        TG_HIP(hipMemcpy(&rec, D.node + cs, sizeof(NodeRec), hipMemcpyDeviceToHost));
        e = rec.pedge;
        cur = rec.parent;
        if ((int)nodes.size() > D.N) return tg::fail(TG_ERR_HIP, "tg_search_read_path: parent chain does not end");
    }
    *length_host = (int32_t)nodes.size();
    if ((int)nodes.size() > capacity)
        return tg::fail(TG_ERR_ARG, "tg_search_read_path: path of %zu steps exceeds capacity %d", nodes.size(), capacity);
    for (size_t i = 0; i < nodes.size(); ++i) {
        nodes_host[i] = nodes[nodes.size() - 1 - i];
        edges_host[i] = edges[nodes.size() - 1 - i];
    }
    return TG_OK;
}

int tg_search_read_queue(tg_search *s, int tree, int32_t *node_index_host, int capacity, int32_t *count_host) {
    if (!s || !node_index_host || !count_host) return tg::fail(TG_ERR_ARG, "tg_search_read_queue: null argument");
    if (tree < 0 || tree >= s->dev.T) return tg::fail(TG_ERR_ARG, "tg_search_read_queue: tree %d out of range", tree);
    if (int rc = sync_launch_stream(s)) return rc;
    const SearchDev &D = s->dev;
    int32_t n = 0;
    TG_HIP(hipMemcpy(&n, D.n_leaves + tree, sizeof(int32_t), hipMemcpyDeviceToHost));
    *count_host = n;
    if (n > capacity) return tg::fail(TG_ERR_ARG, "tg_search_read_queue: %d leaves exceed capacity %d", n, capacity);
    if (n > 0)
        TG_HIP(hipMemcpy(node_index_host, D.q_node + (size_t)tree * D.K, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return TG_OK;
}

int tg_search_num_nodes(tg_search *s, int32_t *num_nodes_host) {
    if (!s || !num_nodes_host) return tg::fail(TG_ERR_ARG, "tg_search_num_nodes: null argument");
    int rc;
    if ((rc = sync_launch_stream(s)) || (rc = check_errors(s))) return rc;
    std::vector<RootMeta> meta(s->dev.T);
    TG_HIP(hipMemcpy(meta.data(), s->dev.meta, meta.size() * sizeof(RootMeta), hipMemcpyDeviceToHost));
    for (int t = 0; t < s->dev.T; ++t) num_nodes_host[t] = meta[t].num_nodes;
    return TG_OK;
}

int tg_search_read_node(tg_search *s, int tree, int node, int32_t *num_children, int32_t *node_visits,
                        int32_t *node_virtual_loss, int32_t *action, int32_t *children_index, int32_t *children_visits,
                        int32_t *children_virtual_loss, double *children_value_sum, double *children_policy,
                        double *children_value, float *node_value_sum, float *raw_value) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_read_node: null argument");
    if (tree < 0 || tree >= s->dev.T || node < 0 || node >= s->dev.N)
        return tg::fail(TG_ERR_ARG, "tg_search_read_node: tree/node out of range");
    const size_t A = s->A;
    const size_t rec = tg_pool::node_record_offset(tg_pool::kNumArrays, A);
    if (!s->node_host.get()) {
        int rc;
        if ((rc = s->node_dev.reserve(rec)) || (rc = s->node_host.alloc(rec))) return rc;
    }
    const unsigned char *node_host = s->node_host.get();
    hipStream_t st = s->last_stream;
    hipLaunchKernelGGL(gather_node_kernel, dim3(1), dim3(64), 0, st, s->dev, (int)A, tree, node, s->node_dev.get());
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(s->node_host.get(), s->node_dev.get(), rec, hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    const int32_t *head = reinterpret_cast<const int32_t *>(node_host);
    // another tree's sticky error is reported by the calls that read all trees; this one checks its own
    if (head[tg_pool::kHeadErr]) return fail_tree(tree, head[tg_pool::kHeadErr]);
    // the caller's name of every child array of the record, under the member's name (`action` has it already): an array added
    // to the list without a destination here does not compile - the reminder that tg_search_read_node's ABI has to grow with it
    void *const ch_index = children_index, *const ch_visits = children_visits, *const ch_vl = children_virtual_loss;
    void *const ch_vsum = children_value_sum, *const ch_policy = children_policy, *const ch_value = children_value;
    if (num_children) *num_children = head[tg_pool::kHeadChildren];
    if (node_visits) *node_visits = head[tg_pool::kHeadVisits];
    if (node_virtual_loss) *node_virtual_loss = head[tg_pool::kHeadVl];
    if (node_value_sum) std::memcpy(node_value_sum, &head[tg_pool::kHeadVsumBits], 4);
    if (raw_value) std::memcpy(raw_value, &head[tg_pool::kHeadRawBits], 4);
#define GET(field, E, per_child, remap) \
    if (field) std::memcpy(field, node_host + tg_pool::node_record_offset(tg_pool::k_##field, A), A * (sizeof(E) == 8 ? 8 : 4));
    TG_NODE_POOL_CHILD_ARRAYS(GET)
#undef GET
    return TG_OK;
}

int tg_search_read_node_links(tg_search *s, int tree, int node, int32_t *parent, int32_t *pedge) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_read_node_links: null argument");
    if (tree < 0 || tree >= s->dev.T || node < 0 || node >= s->dev.N)
        return tg::fail(TG_ERR_ARG, "tg_search_read_node_links: tree/node out of range");
    if (int rc = sync_launch_stream(s)) return rc;
    NodeRec rec;
    TG_HIP(hipMemcpy(&rec, s->dev.node + (size_t)tree * s->dev.N + node, sizeof(NodeRec), hipMemcpyDeviceToHost));
    if (parent) *parent = rec.parent;
    if (pedge) *pedge = rec.pedge;
    return TG_OK;
}

int tg_search_read_analysis(tg_search *s, int max_depth, int32_t *root_host, int32_t *action_host, int32_t *visits_host,
                            double *value_sum_host, double *policy_host, int16_t *pv_host, int32_t *pv_len_host,
                            int32_t *resume_host, void *stream) {
    if (!s || !root_host || !action_host || !visits_host || !value_sum_host || !policy_host || !pv_host || !pv_len_host ||
        !resume_host)
        return tg::fail(TG_ERR_ARG, "tg_search_read_analysis: null argument");
    if (max_depth < 1 || max_depth > kAnaMaxDepth)
        return tg::fail(TG_ERR_ARG, "tg_search_read_analysis: max_depth %d outside [1, %d]", max_depth, kAnaMaxDepth);
    const int T = s->dev.T, A = s->A;
    const size_t rec = tg_readout::analysis_record_bytes(A, max_depth), bytes = rec * T;
    if (bytes > s->ana_dev.capacity() || !s->ana_host.get()) {
        // growing releases the old records first: the launch stream, where the last read-out ran, is idle before that
        if (s->ana_dev.get() && s->stream_known) TG_HIP(hipStreamSynchronize(s->last_stream));
        s->ana_host.reset();
        int rc;
        if ((rc = s->ana_dev.reserve(bytes)) || (rc = s->ana_host.alloc(s->ana_dev.capacity()))) return rc;
    }
    hipStream_t st = use_stream(s, stream);
    hipLaunchKernelGGL(read_analysis_kernel, dim3((A + kAnaWaves - 1) / kAnaWaves, T), dim3(64 * kAnaWaves), 0, st, s->dev, A,
                       max_depth, s->ana_dev.get());
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(s->ana_host.get(), s->ana_dev.get(), bytes, hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    const size_t Az = A, pvn = Az * max_depth;
    for (int t = 0; t < T; ++t) {
        const unsigned char *r = s->ana_host.get() + rec * t;
        std::memcpy(root_host + (size_t)tg_readout::kAnaHeadWords * t, r, tg_readout::kAnaHeadWords * sizeof(int32_t));
        // every row to the caller's <row>_host: a row added to the list without a destination here does not compile
#define GET(row, E) std::memcpy(row##_host + Az * t, r + tg_readout::analysis_record_offset(tg_readout::kAna_##row, Az), Az * sizeof(E));
        TG_ANALYSIS_RECORD_ROWS(GET)
#undef GET
        std::memcpy(pv_host + pvn * t, r + tg_readout::analysis_pv_offset(Az), pvn * sizeof(int16_t));
    }
    return TG_OK;
}

int tg_search_read_improved_policy(tg_search *s, float *rows_dev, void *stream) {
    if (!s || !rows_dev) return tg::fail(TG_ERR_ARG, "tg_search_read_improved_policy: null argument");
    const int T = s->dev.T;
    for (int t = 0; t < T; ++t)
        if (s->roots.staged(t))                                // (a staged position: its tree is reset by the next root expansion)
            return tg::fail(TG_ERR_ARG, "tg_search_read_improved_policy: tree %d: the root is not expanded", t);
    if (!s->ip_bad_host.get()) {
        int rc;
        if ((rc = s->ip_bad_dev.reserve(T)) || (rc = s->ip_bad_host.alloc(T))) return rc;
    }
    hipStream_t st = use_stream(s, stream);
    with_board_size(s->S, [&](auto size) {
        hipLaunchKernelGGL(improved_policy_kernel<decltype(size)::value>, dim3(T), dim3(64), 0, st, s->dev, rows_dev,
                           s->ip_bad_dev.get());
    });
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(s->ip_bad_host.get(), s->ip_bad_dev.get(), (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    for (int t = 0; t < T; ++t)
        if (s->ip_bad_host.get()[t])
            return tg::fail(TG_ERR_ARG, "tg_search_read_improved_policy: tree %d: the root is not expanded", t);
    return TG_OK;
}

// num_nodes of the tree the last tg_search_read_node read, as of that read (it travels in the same record: a search's caller
// wants both - mcts/tree.py:57-105 reads the root and tree.num_nodes - and a second call would be a second host round trip)
int tg_search_node_record_num_nodes(tg_search *s, int32_t *num_nodes_host) {
    if (!s || !num_nodes_host) return tg::fail(TG_ERR_ARG, "tg_search_node_record_num_nodes: null argument");
    if (!s->node_host.get()) return tg::fail(TG_ERR_STATE, "tg_search_node_record_num_nodes: no node has been read");
    *num_nodes_host = reinterpret_cast<const int32_t *>(s->node_host.get())[tg_pool::kHeadNumNodes];
    return TG_OK;
}

}  // extern "C"

// ---- whole-tree read-out ----
namespace {

// One call's list of trees, checked and on its way to the device.  n: the listed trees (trees == null: all T, in order).
struct DumpCall {
    int n = 0;
    const int32_t *list_dev = nullptr;                        // null: all trees
    int64_t *sizes_dev = nullptr, *rec_at_dev = nullptr, *sums_dev = nullptr;
    int64_t *sizes_pin = nullptr, *rec_at_pin = nullptr, *sums_pin = nullptr;
};

// refusals first, nothing launched: a null handle, an empty list, a tree out of range, a duplicate
int dump_begin(tg_search *s, const char *entry, const int32_t *trees, int n, hipStream_t st, DumpCall *c) {
    const int T = s->dev.T;
    if (trees) {
        if (n < 1) return tg::fail(TG_ERR_ARG, "%s: the list holds %d trees", entry, n);
        std::vector<uint8_t> seen(T, 0);
        for (int j = 0; j < n; ++j) {
            if (trees[j] < 0 || trees[j] >= T) return tg::fail(TG_ERR_ARG, "%s: tree %d out of range (list entry %d)", entry, trees[j], j);
            if (seen[trees[j]]) return tg::fail(TG_ERR_ARG, "%s: tree %d is listed twice (list entry %d)", entry, trees[j], j);
            seen[trees[j]] = 1;
        }
    } else {
        n = T;
    }
    tg_search::TreeDump &d = s->dump;
    if ((size_t)n > d.pin_cap) {
        // (growing releases the old buffers: every call of this family left its stream idle)
        d.pin_cap = 0;
        int rc;
        if ((rc = d.list_dev.reserve(n)) || (rc = d.small_dev.reserve((size_t)n * 5)) || (rc = d.list_pin.alloc(n)) ||
            (rc = d.small_pin.alloc((size_t)n * 5)))
            return rc;
        d.pin_cap = n;
    }
    c->n = n;
    c->sizes_dev = d.small_dev.get(), c->rec_at_dev = c->sizes_dev + 2 * (size_t)n, c->sums_dev = c->rec_at_dev + n;
    c->sizes_pin = d.small_pin.get(), c->rec_at_pin = c->sizes_pin + 2 * (size_t)n, c->sums_pin = c->rec_at_pin + n;
    if (trees) {
        std::memcpy(d.list_pin.get(), trees, (size_t)n * sizeof(int32_t));
        TG_HIP(hipMemcpyAsync(d.list_dev.get(), d.list_pin.get(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        c->list_dev = d.list_dev.get();
    }
    return TG_OK;
}

// the scan of the listed trees and their sizes on the host (one launch, one copy, the stream waited for)
int dump_scan(tg_search *s, const DumpCall &c, hipStream_t st) {
    if (int rc = s->dump.first_dev.reserve((size_t)c.n * s->dev.N)) return rc;
    hipLaunchKernelGGL(dump_scan_kernel, dim3(c.n), dim3(tg_dump::kChunk), 0, st, s->dev, s->A, c.list_dev, s->dump.first_dev.get(),
                       c.sizes_dev);
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(c.sizes_pin, c.sizes_dev, (size_t)c.n * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    return TG_OK;
}

// the walk's grid: the list along y, a tree's nodes along x - enough workgroups for one large tree, few per tree for many trees
dim3 dump_grid(const tg_search *s, int n) {
    const long long per_tree = ((long long)s->dev.N + kDumpWaves - 1) / kDumpWaves;
    const long long share = std::max(8LL, 16384LL / n);
    return dim3((unsigned)std::max(1LL, std::min(per_tree, share)), (unsigned)std::min(n, 65535));
}

}  // namespace

extern "C" {

int tg_search_dump_sizes(tg_search *s, const int32_t *trees, int n, int64_t *num_nodes_host, int64_t *children_host, void *stream) {
    if (!s || !num_nodes_host || !children_host) return tg::fail(TG_ERR_ARG, "tg_search_dump_sizes: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DumpCall c;
    if (int rc = dump_begin(s, "tg_search_dump_sizes", trees, n, st, &c)) return rc;
    use_stream(s, stream);
    if (int rc = dump_scan(s, c, st)) return rc;
    for (int j = 0; j < c.n; ++j) {
        num_nodes_host[j] = c.sizes_pin[2 * j];
        children_host[j] = c.sizes_pin[2 * j + 1];
    }
    return TG_OK;
}

int tg_search_dump_trees(tg_search *s, const int32_t *trees, int n, unsigned char *records_host, size_t capacity,
                         int64_t *offsets_host, void *stream) {
    if (!s || !records_host || !offsets_host) return tg::fail(TG_ERR_ARG, "tg_search_dump_trees: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DumpCall c;
    if (int rc = dump_begin(s, "tg_search_dump_trees", trees, n, st, &c)) return rc;
    use_stream(s, stream);
    if (int rc = dump_scan(s, c, st)) return rc;
    size_t bytes = 0;
    for (int j = 0; j < c.n; ++j) {
        c.rec_at_pin[j] = (int64_t)bytes;
        bytes += tg_dump::record_bytes((size_t)c.sizes_pin[2 * j], (size_t)c.sizes_pin[2 * j + 1]);
    }
    if (bytes > capacity)                                      // (nothing of a record has been written anywhere on the host)
        return tg::fail(TG_ERR_ARG, "tg_search_dump_trees: the records take %zu bytes, capacity %zu", bytes, capacity);
    if (int rc = s->dump.out_dev.reserve(bytes)) return rc;
    TG_HIP(hipMemcpyAsync(c.rec_at_dev, c.rec_at_pin, (size_t)c.n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    // (the alignment gap between the 4-byte and the 8-byte rows of a record is written by nobody: zero, not stale)
    TG_HIP(hipMemsetAsync(s->dump.out_dev.get(), 0, bytes, st));
    hipLaunchKernelGGL((dump_walk_kernel<true, false>), dump_grid(s, c.n), dim3(64 * kDumpWaves), 0, st, s->dev, s->A, c.list_dev, c.n,
                       s->dump.first_dev.get(), c.sizes_dev, c.rec_at_dev, s->dump.out_dev.get(), (unsigned long long *)nullptr);
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(records_host, s->dump.out_dev.get(), bytes, hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < c.n; ++j) offsets_host[j] = c.rec_at_pin[j];
    offsets_host[c.n] = (int64_t)bytes;
    return TG_OK;
}

int tg_search_tree_digests(tg_search *s, const int32_t *trees, int n, uint64_t *digests_host, void *stream) {
    if (!s || !digests_host) return tg::fail(TG_ERR_ARG, "tg_search_tree_digests: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DumpCall c;
    if (int rc = dump_begin(s, "tg_search_tree_digests", trees, n, st, &c)) return rc;
    use_stream(s, stream);
    TG_HIP(hipMemsetAsync(c.sums_dev, 0, (size_t)c.n * 2 * sizeof(int64_t), st));
    hipLaunchKernelGGL((dump_walk_kernel<false, true>), dump_grid(s, c.n), dim3(64 * kDumpWaves), 0, st, s->dev, s->A, c.list_dev, c.n,
                       (const int64_t *)nullptr, (const int64_t *)nullptr, (const int64_t *)nullptr, (unsigned char *)nullptr,
                       reinterpret_cast<unsigned long long *>(c.sums_dev));
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(c.sums_pin, c.sums_dev, (size_t)c.n * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < c.n; ++j)
        for (int w = 0; w < 2; ++w)
            digests_host[2 * j + w] = tg_dump::DigestRule::finish(tg_dump::kSeed[w], (uint64_t)c.sums_pin[2 * j + w]);
    return TG_OK;
}

// ---- whole-tree write-in ----
// every record through tree_load.h's check_record: the first inadmissible one is the answer (rule, list entry, node, child)
static int check_records(const char *entry, int board_size, int tree_size, const unsigned char *records, const int64_t *offsets, int n) {
    if (board_size != 9 && board_size != 13 && board_size != 19) return tg::fail(TG_ERR_ARG, "%s: board size %d is not built", entry, board_size);
    if (tree_size < 1) return tg::fail(TG_ERR_ARG, "%s: tree_size %d", entry, tree_size);
    if (n < 1) return tg::fail(TG_ERR_ARG, "%s: the list holds %d records", entry, n);
    for (int j = 0; j < n; ++j) {
        if (offsets[j] < 0 || offsets[j + 1] < offsets[j])
            return tg::fail(TG_ERR_ARG, "%s: list entry %d: offsets %lld, %lld", entry, j, (long long)offsets[j], (long long)offsets[j + 1]);
        const tg_load::Verdict v = tg_load::check_record(records + offsets[j], (size_t)(offsets[j + 1] - offsets[j]), board_size * board_size + 1,
                                                         board_size + 2, tree_size);
        if (!v.ok())
            return tg::fail(TG_ERR_ARG, "%s: list entry %d: rule %d, node %d, child %d: %s", entry, j, v.rule, v.node, v.child,
                            tg_load::kRuleText[v.rule]);
    }
    return TG_OK;
}

int tg_search_check_records(int board_size, int tree_size, const unsigned char *records_host, const int64_t *offsets_host, int n) {
    if (!records_host || !offsets_host) return tg::fail(TG_ERR_ARG, "tg_search_check_records: null argument");
    return check_records("tg_search_check_records", board_size, tree_size, records_host, offsets_host, n);
}

int tg_search_load_trees(tg_search *s, const int32_t *trees, int n, const unsigned char *records_host, const int64_t *offsets_host,
                         int32_t *flags_host, void *stream) {
    if (!s || !records_host || !offsets_host || !flags_host) return tg::fail(TG_ERR_ARG, "tg_search_load_trees: null argument");
    SearchDev &D = s->dev;
    // refusals first, nothing uploaded or launched: the list (dump_begin's rules, restated: dump_begin queues the list's copy),
    // then every record
    if (trees) {
        if (n < 1) return tg::fail(TG_ERR_ARG, "tg_search_load_trees: the list holds %d trees", n);
        std::vector<uint8_t> seen(D.T, 0);
        for (int j = 0; j < n; ++j) {
            if (trees[j] < 0 || trees[j] >= D.T) return tg::fail(TG_ERR_ARG, "tg_search_load_trees: tree %d out of range (list entry %d)", trees[j], j);
            if (seen[trees[j]]) return tg::fail(TG_ERR_ARG, "tg_search_load_trees: tree %d is listed twice (list entry %d)", trees[j], j);
            seen[trees[j]] = 1;
        }
    } else {
        n = D.T;
    }
    if (int rc = check_records("tg_search_load_trees", s->S, D.N, records_host, offsets_host, n)) return rc;
    TG_HIP(hipSetDevice(s->cfg.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    DumpCall c;
    if (int rc = dump_begin(s, "tg_search_load_trees", trees, n, st, &c)) return rc;
    use_stream(s, stream);
    tg_search::TreeLoad &L = s->load;
    // (an admissible record is a multiple of 8 bytes long: packed behind each other, every record starts 8-byte aligned)
    size_t bytes = 0;
    for (int j = 0; j < n; ++j) {
        c.rec_at_pin[j] = (int64_t)bytes;
        bytes += (size_t)(offsets_host[j + 1] - offsets_host[j]);
    }
    int rc;
    if (bytes > L.in_cap) {
        L.in_cap = 0;
        if ((rc = L.in_dev.reserve(bytes)) || (rc = L.in_pin.alloc(bytes))) return rc;
        L.in_cap = bytes;
    }
    if ((size_t)n > L.flags_cap) {
        L.flags_cap = 0;
        if ((rc = L.flags_dev.reserve(n)) || (rc = L.flags_pin.alloc(n))) return rc;
        L.flags_cap = n;
    }
    // 1. the listed trees' staged positions, ahead of the load (as tg_search_reroot takes its trees'): a RootMeta with
    // num_nodes 0 cannot land behind it; other trees' staged positions stay staged
    bool staged = false;
    for (int j = 0; j < n; ++j) staged |= s->roots.staged(trees ? trees[j] : j);
    if (staged) {
        if ((rc = s->roots.begin())) return rc;
        for (int j = 0; j < n; ++j) {
            const int t = trees ? trees[j] : j;
            if (s->roots.staged(t) && (rc = s->roots.take(t, D, D.meta + t, st))) return rc;
        }
        if ((rc = s->roots.end(st))) return rc;
    }
    // 2. the records, one copy out of pinned memory
    for (int j = 0; j < n; ++j)
        std::memcpy(L.in_pin.get() + c.rec_at_pin[j], records_host + offsets_host[j], (size_t)(offsets_host[j + 1] - offsets_host[j]));
    TG_HIP(hipMemcpyAsync(L.in_dev.get(), L.in_pin.get(), bytes, hipMemcpyHostToDevice, st));
    TG_HIP(hipMemcpyAsync(c.rec_at_dev, c.rec_at_pin, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    // 3. one launch
    s->ranks.mark_stale();                                     // (a loaded tree may be live again)
    hipLaunchKernelGGL(load_walk_kernel, dump_grid(s, n), dim3(64 * kDumpWaves), 0, st, D, s->A, c.list_dev, n, c.rec_at_dev,
                       L.in_dev.get(), L.flags_dev.get(), s->halting.stopped_at.get());
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(L.flags_pin.get(), L.flags_dev.get(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    // 4. the call synchronises
    TG_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < n; ++j) {
        flags_host[j] = L.flags_pin.get()[j];
        if (!flags_host[j] && (rc = s->rng.clear_host_noise(trees ? trees[j] : j))) return rc;
    }
    return TG_OK;
}

}  // extern "C"

// ======================================================================================
// Self-play shard bookkeeping (host, C++): everything selfplay/worker.py:50-90 does per move and per board
// around the search - sequential-halving schedule (mcts/sequential_halving.py:7-60), final root choice
// (node.py:324-346), resign rule (tree.py:351-354), improved policy (node.py:281-321) and its ".3e" comment
// (sgf/selfplay_record.py:45-65), two-pass end + count_score (go_board.py:561-608), the SGF file
// (selfplay_record.py:67-110) - for all T boards of a search handle in ONE call per move, on host threads.
// Double arithmetic in the reference's evaluation order (np.sum's pairwise order, libm exp).
// ======================================================================================
namespace {

double host_np_sum_block(const double *a, int n) {
    if (n < 8) {
        double r = 0.;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}
double host_np_sum(const double *a, int n) {        // numpy's pairwise summation (blocks of <= 128)
    if (n <= 128) return host_np_sum_block(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return host_np_sum(a, n2) + host_np_sum(a + n2, n - n2);
}

struct SpGame {
    int index = -1;                 // -1: slot parked
    bool never_resign = false, done = true;
    bool fresh = false;             // started, root not expanded yet (chained moves: the slot sits out one lock-step move)
    int to_move = kBlack, pass_count = 0, moves_played = 0;
    std::string body;               // ";B[ee]C[...]" ...
    // the finished game's result (tg_selfplay_game_result): kept until the slot is restarted
    bool has_result = false, is_resign = false;
    int winner = kEmpty;            // kBlack / kWhite, kOob: a draw, kEmpty: none (the move limit)
    double score = 0.0;
};

// {considered actions: levels} in phase order (mcts/sequential_halving.py)
std::vector<std::pair<int, int>> halving_pairs(int max_considered, int sims) {
    std::vector<int> seq;
    if (max_considered <= 1) {
        for (int i = 0; i < sims; ++i) seq.push_back(i);
    } else {
        const int log2max = (int)std::ceil(std::log2((double)max_considered));
        std::vector<int> visits(max_considered, 0);
        int width = max_considered;
        while ((int)seq.size() < sims) {
            const int rounds = std::max(1, (int)((double)sims / (double)(log2max * width)));
            for (int r = 0; r < rounds; ++r)
                for (int i = 0; i < width; ++i) seq.push_back(visits[i]++);
            width = std::max(2, width / 2);
        }
        seq.resize(sims);
    }
    int mx = 0;
    for (int v : seq) mx = std::max(mx, v);
    std::vector<int> width_at_level(mx + 1, 0);
    for (int v : seq) ++width_at_level[v];
    std::vector<std::pair<int, int>> pairs;
    for (int w : width_at_level) {
        bool found = false;
        for (auto &pr : pairs)
            if (pr.first == w) { ++pr.second; found = true; break; }
        if (!found) pairs.emplace_back(w, 1);
    }
    return pairs;
}

}  // namespace

struct tg_selfplay {
    tg_search *s = nullptr;
    std::string save_dir, komi_text;
    double komi = 7.0;
    int visits = 16;
    std::vector<SpGame> games;                                   // [T]
    std::map<int, std::vector<std::pair<int, int>>> schedule_cache;   // root candidates -> phases
    // per-move scratch (root statistics of all trees)
    std::vector<int32_t> nc, nv, visits_a, vl_a;
    std::vector<float> raw;
    std::vector<double> vsum_a, pol_a;
    std::vector<uint8_t> cells;
    std::vector<int32_t> ph_nc, ph_mc, mv;
    std::vector<int64_t> consumed;
    bool nc_known = false;                 // nc holds the roots' child counts of the move in progress
    std::vector<int32_t> ph_seen;          // per tree: root children entered so far in this move (upper bound)       // tg_selfplay_play_move scratch
    bool force_feed = true;                          // a stream was (re)seeded: the next random window is regenerated
    std::string black_name = "TamaGo-Black", white_name = "TamaGo-White";   // PB[] / PW[] (tg_selfplay_set_players)
    bool unique = false;                             // tg_selfplay_set_unique_leaves: every phase in the UNIQUE leaf layout
    int64_t fwd_positions = 0;                       // positions handed to the network so far (tg_selfplay_forward_positions)
    tg_selfplay_observer observer = nullptr;         // audit hook (tg_selfplay_set_observer)
    void *observer_user = nullptr;
    std::vector<int32_t> nc_cursor;                  // root child counts as read off the draw cursor (cross-checked after the move)
    std::vector<int32_t> act32;                      // root actions of the move in progress (finish_move scratch)
    double t_acc[10] = {};                           // TG_SP_TIMING: host wall clock per section, per HANDLE (groups run on their own threads)
    long moves_timed = 0;
    // The improved-policy comment of a move (two softmaxes + up to 82 "%.3e" fields per board: most of finish_move's
    // host time) is not needed to go on - only the chosen move is.  finish_move saves what the comment is made of and
    // the text is appended to the game record later, while the NEXT move's kernels run (tg_selfplay_play_move, before
    // it waits for them), at the latest at the start of the next finish_move.
    struct PendingComment {
        bool valid = false;
        int n = 0, pos = 0, color = 0, nv = 0, max_count = 0;
        float raw = 0.f;
        std::vector<int32_t> act, vis;
        std::vector<double> pol, vsum;
    };
    std::vector<PendingComment> pending;             // [T]
    // chained moves (tg_selfplay_play_move, default): the device decides the move and goes on to the next root by itself
    bool chained = false;                            // this handle runs chained moves (set by the first tg_selfplay_play_move)
    bool sync_started = false;                       // ... or the round-trip scheme (TG_SP_CHAIN=0)
    bool scheme_told = false;                        // tg_selfplay_chained has told the caller `chained`: the first move keeps it
    tg_net *turn_net = nullptr;                      // two evaluators: the last call's net_next, which must search in this call
    bool chain_started = false;                      // a chain has run: the roots are expanded, c_phase / the cursors are valid
    std::vector<int64_t> c_phase;                    // per tree: draw cursor behind the phases of the last move (RootTail)
    std::vector<uint8_t> skip, skip_fresh;           // per tree: takes no part in this move / game just started
    std::vector<int32_t> state;                      // finish_roots_kernel's per-tree state [T][tg_readout::kStateWords]
    // sub-groups of a lock-step move (launch_phases_subgroups): streams 1.., events, the phase tables of a whole move
    static constexpr int kMaxSub = 16, kMaxPhases = 16;
    tg::Stream sub_stream[kMaxSub - 1];                              // (created as sub-groups are first used)
    tg::Event ev_start, ev_first_sel[kMaxSub], ev_sub_done[kMaxSub - 1];
    tg::DevBuf<int32_t> phase_all_dev;                               // [kMaxPhases][3 T]
    tg::StagingRing<int32_t, 2> phase_all_pin;                       // (pinned: a ring of two)
    // the caller's device buffers of a move (planes [T * batch_size][6][S][S], policy [..][A], value [..][3]) and its stream
    struct MoveBuffers {
        float *planes = nullptr, *policy = nullptr, *value = nullptr;
        void *stream = nullptr;
    };
    // A chained move between tg_selfplay_move_begin (everything queued) and tg_selfplay_move_end (records awaited, bookkeeping):
    // what the second half needs from the first.  Several handles (lanes of one shard, each with its own engine and stream) are
    // kept in this state at once by ONE host thread, so that the device always has other lanes' moves queued while the host
    // waits for one lane's records - boards of different lanes are on different moves (round 6).
    struct PendingMove {
        bool active = false, any_phase = false;
        int64_t leaves = 0;
        int32_t n_phases = 0;
        MoveBuffers bufs;
    } pend;
};

namespace {

std::string gtp_name(int pos, int S) {                           // board/coordinate.py:38-43
    if (pos == 0) return "pass";
    static const char *letters = "IABCDEFGHJKLMNOPQRSTUVWXYZ";
    const int W = S + 2, col = pos % W - 1, row = pos / W - 1;
    return std::string(1, letters[col + 1]) + std::to_string(S - row);
}
std::string sgf_name(int pos, int S) {                           // board/coordinate.py:45-49
    if (pos == 0) return "tt";
    const int W = S + 2, col = pos % W - 1, row = pos / W - 1;
    return std::string(1, (char)('a' + col)) + std::string(1, (char)('a' + row));
}

// go_board.py:561-608: stones in atari count as dead; an empty point takes the colour of its direct
// neighbours only (both colours -> neutral), in row-major order, earlier colourings feeding later points
int count_score_cells(const uint8_t *cells, int S) {
    const int W = S + 2, NC = W * W;
    std::vector<uint8_t> work(cells, cells + NC);
    std::vector<int> stack;
    std::vector<uint8_t> seen(NC), lib_seen(NC);
    for (int y = 1; y <= S; ++y)
        for (int x = 1; x <= S; ++x) {
            const int pos = y * W + x, c = cells[pos];
            if (c != kBlack && c != kWhite) continue;
            std::fill(seen.begin(), seen.end(), 0);
            std::fill(lib_seen.begin(), lib_seen.end(), 0);
            int libs = 0;
            stack.assign(1, pos);
            seen[pos] = 1;
            while (!stack.empty() && libs < 2) {
                const int p = stack.back();
                stack.pop_back();
                const int nb[4] = {p - W, p - 1, p + 1, p + W};
                for (int n : nb) {
                    if (cells[n] == kEmpty) { if (!lib_seen[n]) { lib_seen[n] = 1; ++libs; } }
                    else if (cells[n] == c && !seen[n]) { seen[n] = 1; stack.push_back(n); }
                }
            }
            if (libs == 1) work[pos] = kEmpty;
        }
    for (int y = 1; y <= S; ++y)
        for (int x = 1; x <= S; ++x) {
            const int pos = y * W + x;
            if (work[pos] != kEmpty) continue;
            int color = kEmpty;
            const int nb[4] = {pos - W, pos - 1, pos + 1, pos + W};
            for (int n : nb) {
                const int v = work[n];
                if (v == kBlack || v == kWhite) {
                    if (color == kEmpty) color = v;
                    else if (color != v) color = kOob;
                }
            }
            work[pos] = (uint8_t)color;
        }
    int score = 0;
    for (int i = 0; i < NC; ++i) score += (work[i] == kBlack) - (work[i] == kWhite);
    return score;
}

int write_sgf(const tg_selfplay *sp, const SpGame &g, int winner, bool is_resign, double score) {
    char buf[96];
    std::string text = "(;FF[4]GM[1]SZ[" + std::to_string(sp->s->S) + "]\n";
    text += "AP[TamaGo]PB[" + sp->black_name + "]PW[" + sp->white_name + "]";
    if (winner == kBlack) {
        if (is_resign) text += "RE[B+R]";
        else { snprintf(buf, sizeof(buf), "RE[B+%.1f]", score); text += buf; }
    } else if (winner == kWhite) {
        if (is_resign) text += "RE[W+R]";
        else { snprintf(buf, sizeof(buf), "RE[W+%.1f]", -score); text += buf; }
    } else {
        text += "RE[0]";
    }
    text += "KM[" + sp->komi_text + "]";
    text += g.body;
    text += "\n)";
    const std::string path = sp->save_dir + "/" + std::to_string(g.index) + ".sgf";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return tg::fail(TG_ERR_ARG, "tg_selfplay: cannot write %s", path.c_str());
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    fclose(f);
    return ok ? TG_OK : tg::fail(TG_ERR_ARG, "tg_selfplay: short write to %s", path.c_str());
}

// improved policy (node.py:281-321) -> ";B[ee]C[<n> <gtp>:<p:.3e> ...]" appended to the game record
void append_comment(tg_selfplay *sp, SpGame &g, const tg_selfplay::PendingComment &pc) {
    const int n = pc.n, S = sp->s->S;
    const double sigma_sel = (double)(50 + pc.max_count) * 1.0;
    std::vector<double> q(n), w1(n), w2(n);
    const double *pol = pc.pol.data(), *vsum = pc.vsum.data();
    const int32_t *vis = pc.vis.data(), *act = pc.act.data();
    for (int i = 0; i < n; ++i) q[i] = vis[i] > 0 ? vsum[i] / (double)vis[i] : 0.0;
    double mx = -INFINITY;
    for (int i = 0; i < n; ++i) mx = pol[i] > mx ? pol[i] : mx;
    for (int i = 0; i < n; ++i) w1[i] = std::exp(pol[i] - mx);
    const double s1 = host_np_sum(w1.data(), n);
    for (int i = 0; i < n; ++i) { w1[i] = w1[i] / s1; w2[i] = w1[i] * q[i]; }
    const double sum_prob = host_np_sum(w1.data(), n), v_pi = host_np_sum(w2.data(), n);
    const double nvd = (double)pc.nv;
    const double mixed = ((double)pc.raw * 1.0 + nvd * v_pi / sum_prob) / (nvd + 1.0);
    // np.max(self.children_visits) runs over the whole array (zeros beyond n): same value
    double mx2 = -INFINITY;
    for (int i = 0; i < n; ++i) {
        w2[i] = pol[i] + sigma_sel * (vis[i] > 0 ? q[i] : mixed);
        mx2 = w2[i] > mx2 ? w2[i] : mx2;
    }
    for (int i = 0; i < n; ++i) w1[i] = std::exp(w2[i] - mx2);
    const double s2 = host_np_sum(w1.data(), n);
    char buf[64];
    g.body += pc.color == kBlack ? ";B[" : ";W[";
    g.body += sgf_name(pc.pos, S);
    g.body += "]C[";
    g.body += std::to_string(n);
    for (int i = 0; i < n; ++i) {
        snprintf(buf, sizeof(buf), ":%.3e", w1[i] / s2);
        g.body += ' ';
        g.body += gtp_name(act[i], S);
        g.body += buf;
    }
    g.body += ']';
}

// The game in slot g is over: its result is kept for tg_selfplay_game_result and its record is written (an empty save_dir: no file).
int finish_game(const tg_selfplay *sp, SpGame &g, int winner, bool is_resign, double score) {
    g.has_result = true;
    g.winner = winner;
    g.is_resign = is_resign;
    g.score = score;
    g.done = true;
    return sp->save_dir.empty() ? TG_OK : write_sgf(sp, g, winner, is_resign, score);
}

void flush_comments(tg_selfplay *sp) {
    const int T = sp->s->dev.T;
    if ((int)sp->pending.size() != T) return;
    bool any = false;
    for (int t = 0; t < T; ++t) any |= sp->pending[t].valid;
    if (!any) return;
    parallel_trees(T, [&](int t) {
        tg_selfplay::PendingComment &pc = sp->pending[t];
        if (!pc.valid) return;
        append_comment(sp, sp->games[t], pc);
        pc.valid = false;
    });
}

}  // namespace

extern "C" {

int tg_search_count_scores(const uint8_t *cells_host, int board_size, int boards, int32_t *scores_host) {
    if (!cells_host || !scores_host) return tg::fail(TG_ERR_ARG, "tg_search_count_scores: null argument");
    if (board_size < 1 || board_size > 25 || boards < 0)
        return tg::fail(TG_ERR_ARG, "tg_search_count_scores: board size %d outside [1, 25] or %d boards", board_size, boards);
    const size_t NC = (size_t)(board_size + 2) * (board_size + 2);
    for (int g = 0; g < boards; ++g) scores_host[g] = count_score_cells(cells_host + (size_t)g * NC, board_size);
    return TG_OK;
}

int tg_selfplay_create(tg_search *s, const char *save_dir, int visits, double komi, const char *komi_text,
                       tg_selfplay **out) {
    if (!s || !save_dir || !komi_text || !out) return tg::fail(TG_ERR_ARG, "tg_selfplay_create: null argument");
    if (visits < 1) return tg::fail(TG_ERR_ARG, "tg_selfplay_create: visits must be >= 1");
    tg_selfplay *sp = new tg_selfplay;
    sp->s = s;
    sp->save_dir = save_dir;
    sp->komi = komi;
    sp->komi_text = komi_text;
    sp->visits = visits;
    sp->games.assign(s->dev.T, SpGame{});
    *out = sp;
    return TG_OK;
}

int tg_selfplay_destroy(tg_selfplay *sp) {
    if (!sp) return TG_OK;
    (void)hipSetDevice(sp->s->cfg.device);
    // the engine's launch stream is idle BEFORE any member is released; the sub-group streams wait for themselves (tg::Stream)
    if (sp->s->stream_known) (void)hipStreamSynchronize(sp->s->last_stream);
    delete sp;
    return TG_OK;
}

int tg_selfplay_start_game(tg_selfplay *sp, int slot, int index, int never_resign) {
    if (!sp) return tg::fail(TG_ERR_ARG, "tg_selfplay_start_game: null argument");
    if (slot < 0 || slot >= sp->s->dev.T) return tg::fail(TG_ERR_ARG, "tg_selfplay_start_game: slot %d out of range", slot);
    SpGame g;
    g.index = index;
    g.never_resign = never_resign != 0;
    g.done = index < 0;
    g.fresh = index >= 0;
    sp->games[slot] = g;
    if ((size_t)slot < sp->pending.size()) sp->pending[slot].valid = false;
    sp->force_feed = true;
    return TG_OK;
}

int tg_selfplay_schedule(tg_selfplay *sp, int32_t *num_considered_host, int32_t *max_count_host, int max_phases,
                         int32_t *n_phases_host) {
    if (!sp || !num_considered_host || !max_count_host || !n_phases_host)
        return tg::fail(TG_ERR_ARG, "tg_selfplay_schedule: null argument");
    tg_search *s = sp->s;
    const int T = s->dev.T;
    if (!sp->nc_known) {
        sp->nc.resize(T);
        int rc = tg_search_read_root_stats(s, sp->nc.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc) return rc;
    }
    sp->nc_known = false;
    std::fill(num_considered_host, num_considered_host + (size_t)max_phases * T, 0);
    std::fill(max_count_host, max_count_host + (size_t)max_phases * T, 0);
    int n_phases = 0;
    for (int t = 0; t < T; ++t) {
        if (sp->games[t].done || (sp->chained && sp->games[t].fresh)) continue;
        const int base = sp->nc[t] < 16 ? sp->nc[t] : 16;            // MAX_CONSIDERED_NODES (mcts/constant.py)
        auto it = sp->schedule_cache.find(base);
        if (it == sp->schedule_cache.end())
            it = sp->schedule_cache.emplace(base, halving_pairs(base, sp->visits)).first;
        const auto &pairs = it->second;
        if ((int)pairs.size() > max_phases) return tg::fail(TG_ERR_ARG, "tg_selfplay_schedule: %zu phases exceed max_phases", pairs.size());
        for (size_t ph = 0; ph < pairs.size(); ++ph) {
            num_considered_host[ph * T + t] = pairs[ph].first;
            max_count_host[ph * T + t] = pairs[ph].second;
        }
        n_phases = std::max(n_phases, (int)pairs.size());
    }
    *n_phases_host = n_phases;
    return TG_OK;
}

// tail != nullptr (chained moves): the root records are in roots_host already (launch_finish_roots, fin_ev waited for) and
// the device has decided the moves itself - the host's own decision below, from the same statistics, must be the same
static int finish_move_impl(tg_selfplay *sp, int32_t *moves_host, int32_t *finished_host, int64_t *stats_host, const RootTail *tail) {
    if (!sp || !moves_host || !finished_host) return tg::fail(TG_ERR_ARG, "tg_selfplay_finish_move: null argument");
    tg_search *s = sp->s;
    const SearchDev &D = s->dev;
    const int T = D.T, A = s->A, S = s->S;
    flush_comments(sp);                                               // the previous move's comments, if still waiting
    sp->pending.resize(T);
    sp->nc.resize(T); sp->nv.resize(T); sp->raw.resize(T);
    sp->visits_a.resize((size_t)T * A); sp->vl_a.resize((size_t)T * A);
    sp->vsum_a.resize((size_t)T * A); sp->pol_a.resize((size_t)T * A);
    std::vector<int32_t> &act32 = sp->act32;
    act32.resize((size_t)T * A);
    int rc = TG_OK;
    if (tail) {
        if ((rc = root_record_errors(s))) return rc;
        parse_root_records(s, sp->nc.data(), sp->nv.data(), sp->raw.data(), act32.data(), sp->visits_a.data(), sp->vl_a.data(),
                           sp->vsum_a.data(), sp->pol_a.data());
    } else {
        rc = tg_search_read_root_stats(s, sp->nc.data(), sp->nv.data(), sp->raw.data(), act32.data(), sp->visits_a.data(),
                                       sp->vl_a.data(), sp->vsum_a.data(), sp->pol_a.data());
    }
    if (rc) return rc;
    const double *noise_rows;
    size_t noise_count;
    if (int nrc = s->rng.host_noise(&noise_rows, &noise_count)) return nrc;      // (the device-drawn noise has long arrived)
    if (noise_count != (size_t)T * A) return tg::fail(TG_ERR_STATE, "tg_selfplay_finish_move: no root noise was set");
    // the boards are only needed to score a game that ends with this move, i.e. with a second pass in a row
    bool may_end = false;
    for (int t = 0; t < T; ++t) may_end |= !sp->games[t].done && sp->games[t].pass_count == 1 && (!tail || tail[t].kind == tg_readout::kSecondPass);
    sp->cells.resize((size_t)T * s->NC);
    if (may_end) TG_HIP(hipMemcpy(sp->cells.data(), D.root_cells, sp->cells.size(), hipMemcpyDeviceToHost));
    const int max_moves = S * S * 2;                                  // worker.py:44
    std::vector<int> status(T, TG_OK);
    std::vector<int64_t> n_moves(T, 0), n_games(T, 0);
    parallel_trees(T, [&](int t) {
        SpGame &g = sp->games[t];
        moves_host[t] = -1;
        finished_host[t] = 0;
        if (g.done || (tail && g.fresh)) return;
        const size_t o = (size_t)t * A;
        const int n = sp->nc[t];
        const int32_t *vis = &sp->visits_a[o], *vl = &sp->vl_a[o], *act = &act32[o];
        const double *vsum = &sp->vsum_a[o], *pol = &sp->pol_a[o], *noise = noise_rows + o;
        // ---- final root choice (tree.py:344, node.py:324-346 with count_threshold = PLAYOUTS = 100) ----
        int max_count = 0;
        for (int i = 0; i < n; ++i) max_count = std::max(max_count, vis[i]);
        const double sigma_sel = (double)(50 + max_count) * 1.0;
        int best = 0;
        double best_v = 0.0;
        for (int i = 0; i < n; ++i) {
            const double qi = vis[i] > 0 ? vsum[i] / (double)vis[i] : 0.0;
            const double ev = (vis[i] + vl[i] >= 100) ? -10000.0 : (pol[i] + noise[i]) + sigma_sel * qi;
            if (i == 0 || ev > best_v) { best_v = ev; best = i; }
        }
        const double value = vis[best] == 0 ? 0.5 : vsum[best] / (double)vis[best];
        n_moves[t] = 1;
        if (tail) {
            // what the device did with the same numbers (finish_roots_kernel): anything else is a bug, not a rounding matter
            const int p2 = act[best] == 0 ? g.pass_count + 1 : 0;
            using namespace tg_readout;
            const int kind = (!g.never_resign && value < 0.05) ? kResign : p2 == 2 ? kSecondPass : g.moves_played + 1 >= max_moves ? kMoveLimit : kMove;
            if (tail[t].best != best || tail[t].kind != kind || tail[t].pos != act[best]) {
                status[t] = tg::fail(TG_ERR_STATE, "tg_selfplay_play_move: board %d: the device chose child %d (point %d, kind %d), "
                                     "the host child %d (point %d, kind %d) from the same root statistics", t, tail[t].best,
                                     tail[t].pos, tail[t].kind, best, act[best], kind);
                return;
            }
        }
        if (!g.never_resign && value < 0.05) {                          // worker.py:59-62
            status[t] = finish_game(sp, g, 3 - g.to_move, true, 0.0);
            finished_host[t] = 1;
            n_games[t] = 1;
            return;
        }
        const int pos = act[best];
        // ---- improved policy (node.py:281-321) -> comment "<n> <gtp>:<p:.3e> ...": saved, formatted later ----
        tg_selfplay::PendingComment &pc = sp->pending[t];
        pc.valid = true;
        pc.n = n; pc.pos = pos; pc.color = g.to_move; pc.nv = sp->nv[t]; pc.raw = sp->raw[t]; pc.max_count = max_count;
        pc.act.assign(act, act + n);
        pc.vis.assign(vis, vis + n);
        pc.pol.assign(pol, pol + n);
        pc.vsum.assign(vsum, vsum + n);
        moves_host[t] = pos;
        g.pass_count = pos == 0 ? g.pass_count + 1 : 0;
        g.to_move = 3 - g.to_move;
        g.moves_played += 1;
        if (g.pass_count == 2 || g.moves_played >= max_moves) {         // the game ends here: its record is written now
            append_comment(sp, g, pc);
            pc.valid = false;
        }
        if (g.pass_count == 2) {                                        // worker.py:80-87 (a pass leaves the cells as they are)
            const double score = (double)count_score_cells(&sp->cells[(size_t)t * s->NC], S) - sp->komi;
            const int winner = score > 0.1 ? kBlack : (score < -0.1 ? kWhite : kOob);
            status[t] = finish_game(sp, g, winner, false, score);
        } else if (g.moves_played >= max_moves) {
            status[t] = finish_game(sp, g, kEmpty, false, 0.0);
        }
        if (g.done) {
            finished_host[t] = 1;
            n_games[t] = 1;
            moves_host[t] = -1;                                         // the slot gets a new root anyway
        }
    });
    for (int t = 0; t < T; ++t)
        if (status[t] != TG_OK) return status[t];
    if (stats_host) {
        stats_host[0] = 0;
        stats_host[1] = 0;
        for (int t = 0; t < T; ++t) { stats_host[0] += n_games[t]; stats_host[1] += n_moves[t]; }
    }
    return TG_OK;
}

int tg_selfplay_finish_move(tg_selfplay *sp, int32_t *moves_host, int32_t *finished_host, int64_t *stats_host) {
    return finish_move_impl(sp, moves_host, finished_host, stats_host, nullptr);
}

// UNIQUE leaf layout for every phase of this handle's moves (tg_search_select_gumbel with slots_per_tree -1), in every scheme:
// the descents of a phase through one root child end on the same leaf (nothing moves within a phase, tree.py:375-384), which
// the reference queues and evaluates once per descent (tree.py:412-416) - here it is evaluated once.  Same trees, games and
// records; the forward launches are sized by the plane ranges.  Between moves only.
int tg_selfplay_set_unique_leaves(tg_selfplay *sp, int on) {
    if (!sp) return tg::fail(TG_ERR_ARG, "tg_selfplay_set_unique_leaves: null argument");
    if (sp->pend.active) return tg::fail(TG_ERR_STATE, "tg_selfplay_set_unique_leaves: a move is in progress");
    sp->unique = on != 0;
    return TG_OK;
}

// Positions handed to the network so far by this handle's moves (roots and phases; tree.py:273-315 evaluates every queued leaf,
// which is what stats_host[2] of tg_selfplay_play_move keeps counting): equal to the queued leaves unless the UNIQUE layout is on.
int tg_selfplay_forward_positions(tg_selfplay *sp, int64_t *count_host) {
    if (!sp || !count_host) return tg::fail(TG_ERR_ARG, "tg_selfplay_forward_positions: null argument");
    *count_host = sp->fwd_positions;
    return TG_OK;
}

int tg_selfplay_set_observer(tg_selfplay *sp, tg_selfplay_observer fn, void *user) {
    if (!sp) return tg::fail(TG_ERR_ARG, "tg_selfplay_set_observer: null argument");
    sp->observer = fn;
    sp->observer_user = user;
    return TG_OK;
}

// The names write_sgf spells in PB[] / PW[] (a match between two evaluators, tg_selfplay_play_move2); NULL keeps a side's
// default, under which a self-play record keeps the reference's bytes.
int tg_selfplay_set_players(tg_selfplay *sp, const char *black, const char *white) {
    if (!sp) return tg::fail(TG_ERR_ARG, "tg_selfplay_set_players: null argument");
    for (const char *name : {black, white})
        if (name && strpbrk(name, "]\\\r\n"))
            return tg::fail(TG_ERR_ARG, "tg_selfplay_set_players: a name may not contain ']', a backslash or a line break");
    sp->black_name = black ? black : "TamaGo-Black";
    sp->white_name = white ? white : "TamaGo-White";
    return TG_OK;
}

// The result of the game that ended in `slot`: result_host[4] = {game index, winner (1 black, 2 white, 3 draw, 0 none: the move
// limit), resigned, moves played}, *score_host = count_score - komi (0 unless the game ended with two passes).
int tg_selfplay_game_result(tg_selfplay *sp, int slot, int32_t *result_host, double *score_host) {
    if (!sp || !result_host || !score_host) return tg::fail(TG_ERR_ARG, "tg_selfplay_game_result: null argument");
    if (slot < 0 || slot >= sp->s->dev.T) return tg::fail(TG_ERR_ARG, "tg_selfplay_game_result: slot %d out of range", slot);
    const SpGame &g = sp->games[slot];
    if (!g.has_result) return tg::fail(TG_ERR_STATE, "tg_selfplay_game_result: no game has ended in slot %d since it was started", slot);
    result_host[0] = g.index;
    result_host[1] = g.winner;
    result_host[2] = g.is_resign ? 1 : 0;
    result_host[3] = g.moves_played;
    *score_host = g.score;
    return TG_OK;
}

// PUCT mini-batches queued back to back (mcts/tree.py:146-152 with process_mini_batch, :273-315): ONE random window for all of them
// - uploaded in two parts, the first mini-batch's share in front of its selection launch, the rest behind it -, then per mini-batch
// selection, forward pass, backup on `stream`, with no host round trip in between.  The same launches on the same data as the
// per-mini-batch calls; for searches whose course does not depend on a mini-batch's outcome (STRICT_PLAYOUT, time_manager.py:160-161).
// The caller reads the cursors back afterwards (tg_search_advance_streams), as after a single mini-batch.
// (puct_chain_impl, below the stop rule's helpers: THE chain - this one, the early one and their compact variants are its options)
static int puct_chain_impl(tg_search *s, const char *who, tg_net *net, const int32_t *leaves_host, int n_batches, const int32_t *total_host,
                           int poll_every, int force_window, float *planes_dev, float *policy_dev, float *value_dev, void *stream,
                           int32_t *batches_run_host, bool compact, int64_t *positions_host, bool budget = false,
                           tg_net *const *group_nets = nullptr);
int tg_search_puct_chain(tg_search *s, tg_net *net, const int32_t *leaves_host, int n_batches, int force_window,
                         float *planes_dev, float *policy_dev, float *value_dev, void *stream) {
    return puct_chain_impl(s, "tg_search_puct_chain", net, leaves_host, n_batches, nullptr, 1, force_window, planes_dev, policy_dev,
                           value_dev, stream, nullptr, false, nullptr);
}

// ---- halt words and the device stop rule ----
static int halting_ready(tg_search *s) {
    tg_search::Halting &h = s->halting;
    if (h.mask.get()) return TG_OK;
    const size_t T = (size_t)s->dev.T;
    int rc;
    if ((rc = h.mask.alloc(T, hipHostMallocMapped)) || (rc = h.total.alloc(T, hipHostMallocMapped)) || (rc = h.stopped_at.alloc_zeroed(T)) ||
        (rc = h.live_back.alloc(1)))
        return rc;
    return TG_OK;
}

int tg_search_set_halt(tg_search *s, const uint8_t *halt_host, void *stream) {
    if (!s || !halt_host) return tg::fail(TG_ERR_ARG, "tg_search_set_halt: null argument");
    TG_HIP(hipSetDevice(s->cfg.device));
    hipStream_t st = use_stream(s, stream);
    tg_search::Halting &h = s->halting;
    int rc;
    if ((rc = halting_ready(s)) || (rc = h.inputs_read.wait_if_recorded())) return rc;
    const int T = s->dev.T;
    bool any = false;
    for (int t = 0; t < T; ++t) {
        h.mask.get()[t] = halt_host[t] ? 1 : 0;
        any |= halt_host[t] != 0;
    }
    if (!any) return TG_OK;
    hipLaunchKernelGGL(set_halt_kernel, dim3((T + 255) / 256), dim3(256), 0, st, s->dev, h.mask.dev(), h.stopped_at.get());
    TG_HIP(hipGetLastError());
    h.armed = true;
    s->ranks.mark_shrunk();
    return h.inputs_read.record(st);
}

int tg_search_read_halt(tg_search *s, uint8_t *halt_host, int32_t *stopped_at_host) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_read_halt: null argument");
    TG_HIP(hipSetDevice(s->cfg.device));
    if (int rc = sync_launch_stream(s)) return rc;
    const size_t T = (size_t)s->dev.T;
    std::vector<int32_t> words(2 * T, 0);                       // (a read-out allocates nothing on the device)
    int32_t *back = words.data();
    TG_HIP(hipMemcpy(back, s->dev.halt, T * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (s->halting.stopped_at.get())
        TG_HIP(hipMemcpy(back + T, s->halting.stopped_at.get(), T * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < T; ++t) {
        if (halt_host) halt_host[t] = back[t] ? 1 : 0;
        if (stopped_at_host) stopped_at_host[t] = back[t] ? back[T + t] : 0;
    }
    return TG_OK;
}

// the totals of the coming rule launches, into the host-mapped row the kernels read (the launches queued before are waited for)
static int stage_totals(tg_search *s, const char *who, const int32_t *total_host) {
    tg_search::Halting &h = s->halting;
    for (int t = 0; t < s->dev.T; ++t)
        if (total_host[t] < 1) return tg::fail(TG_ERR_ARG, "%s: tree %d: a total of %d visits (at least 1)", who, t, total_host[t]);
    int rc;
    if ((rc = halting_ready(s)) || (rc = h.inputs_read.wait_if_recorded())) return rc;
    std::memcpy(h.total.get(), total_host, (size_t)s->dev.T * sizeof(int32_t));
    return TG_OK;
}

// `n` live counters, zeroed on st (the launches that counted into the old ones are over: every caller has read or dropped them)
static int zero_live(tg_search *s, size_t n, hipStream_t st) {
    tg_search::Halting &h = s->halting;
    if (n > h.live.capacity()) {
        if (int rc = sync_launch_stream(s)) return rc;
        if (int rc = h.live.reserve(n)) return rc;
    }
    TG_HIP(hipMemsetAsync(h.live.get(), 0, n * sizeof(int32_t), st));
    return TG_OK;
}

static int launch_stop_rule(tg_search *s, int slot, hipStream_t st) {
    tg_search::Halting &h = s->halting;
    with_board_size(s->S, [&](auto size) {
        hipLaunchKernelGGL(stop_rule_kernel<decltype(size)::value>, dim3(s->dev.T), dim3(64), 0, st, s->dev, h.total.dev(),
                           h.stopped_at.get(), h.live.get() + slot);
    });
    TG_HIP(hipGetLastError());
    h.armed = true;
    s->ranks.mark_shrunk();
    return h.inputs_read.record(st);
}

// one device word on the host through the pinned word: the HOST waits for everything queued on st so far
static int read_word(tg_search *s, const int32_t *word_dev, hipStream_t st, int32_t *out) {
    tg_search::Halting &h = s->halting;
    TG_HIP(hipMemcpyAsync(h.live_back.get(), word_dev, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    *out = *h.live_back.get();
    return TG_OK;
}
// counter `slot` of the rule
static int read_live(tg_search *s, int slot, hipStream_t st, int32_t *out) { return read_word(s, s->halting.live.get() + slot, st, out); }

// ---- live ranks ----
static int live_ranks_ready(tg_search *s) {
    tg_search::LiveRanks &r = s->ranks;
    if (int rc = halting_ready(s)) return rc;                      // (the pinned word the count comes back through)
    if (r.rank.get()) return TG_OK;
    r.T = (size_t)s->dev.T;
    return r.rank.alloc_zeroed(r.T + 1);
}

// live_rank_kernel behind everything queued on st: the ranks in the table are those of the halt words as they stand there
static int launch_live_rank(tg_search *s, hipStream_t st) {
    tg_search::LiveRanks &r = s->ranks;
    hipLaunchKernelGGL(live_rank_kernel, dim3(1), dim3(tg_live::kChunk), 0, st, s->dev, r.rank.get(), r.count());
    TG_HIP(hipGetLastError());
    r.state = tg_search::LiveRanks::State::Fresh;
    r.grouped = false;
    return TG_OK;
}

int tg_search_compact_live(tg_search *s, int32_t *live_host, void *stream) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_compact_live: null argument");
    TG_HIP(hipSetDevice(s->cfg.device));
    int rc;
    if ((rc = live_ranks_ready(s))) return rc;
    hipStream_t st = use_stream(s, stream);
    if ((rc = launch_live_rank(s, st))) return rc;
    return live_host ? read_word(s, s->ranks.count(), st, live_host) : TG_OK;
}

int tg_search_read_live_rank(tg_search *s, int32_t *rank_host) {
    if (!s || !rank_host) return tg::fail(TG_ERR_ARG, "tg_search_read_live_rank: null argument");
    if (!s->ranks.rank.get()) return tg::fail(TG_ERR_STATE, "tg_search_read_live_rank: no live ranks were computed (tg_search_compact_live)");
    TG_HIP(hipSetDevice(s->cfg.device));
    if (int rc = sync_launch_stream(s)) return rc;
    TG_HIP(hipMemcpy(rank_host, s->ranks.rank.get(), s->ranks.T * sizeof(int32_t), hipMemcpyDeviceToHost));      // (a read-out allocates nothing)
    return TG_OK;
}

// ---- grouped ranks and rows by rank ----
int tg_search_group_live(tg_search *s, const int32_t *group_host, int n_groups, int32_t *count_host, void *stream) {
    if (!s || !group_host || !count_host) return tg::fail(TG_ERR_ARG, "tg_search_group_live: null argument");
    if (n_groups < 1 || n_groups > tg_group::kMaxGroups)
        return tg::fail(TG_ERR_ARG, "tg_search_group_live: n_groups %d outside [1, %d]", n_groups, tg_group::kMaxGroups);
    const int T = s->dev.T;
    for (int t = 0; t < T; ++t)
        if (group_host[t] < 0 || group_host[t] >= n_groups)
            return tg::fail(TG_ERR_ARG, "tg_search_group_live: tree %d: group %d outside [0, %d)", t, group_host[t], n_groups);
    TG_HIP(hipSetDevice(s->cfg.device));
    tg_search::LiveRanks &r = s->ranks;
    int rc;
    if ((rc = live_ranks_ready(s))) return rc;
    if (!r.group_in.get() && ((rc = r.group_in.alloc((size_t)T, hipHostMallocMapped)) || (rc = r.group_count_dev.alloc_zeroed(tg_group::kMaxGroups)) ||
                              (rc = r.group_count_back.alloc(tg_group::kMaxGroups))))
        return rc;
    hipStream_t st = use_stream(s, stream);
    // (every earlier call of this entry ended with its stream idle: the launch that read group_in is over)
    std::memcpy(r.group_in.get(), group_host, (size_t)T * sizeof(int32_t));
    hipLaunchKernelGGL(group_rank_kernel, dim3(1), dim3(tg_group::kChunk), 0, st, s->dev, r.group_in.dev(), n_groups, r.rank.get(),
                       r.group_count_dev.get());
    TG_HIP(hipGetLastError());
    r.state = tg_search::LiveRanks::State::Stale;          // (until the counts are back: a failure below leaves no grouped table in force)
    r.grouped = false;
    TG_HIP(hipMemcpyAsync(r.group_count_back.get(), r.group_count_dev.get(), (size_t)n_groups * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    int32_t offset = 0;
    for (int g = 0; g < n_groups; ++g) {
        count_host[g] = r.group_count[g] = r.group_count_back.get()[g];
        r.group_offset[g] = offset;
        offset += r.group_count[g];
    }
    r.n_groups = n_groups;
    r.grouped = true;
    r.state = tg_search::LiveRanks::State::Fresh;
    return TG_OK;
}

static int rows_by_rank(tg_search *s, const char *who, bool gather, const float *src_dev, float *dst_dev, int row_floats, void *stream) {
    if (!s || !src_dev || !dst_dev) return tg::fail(TG_ERR_ARG, "%s: null argument", who);
    if (row_floats < 1) return tg::fail(TG_ERR_ARG, "%s: rows of %d floats", who, row_floats);
    if (!s->ranks.rank.get() || s->ranks.state == tg_search::LiveRanks::State::Stale)
        return tg::fail(TG_ERR_STATE, "%s: no ranks in force (tg_search_group_live or tg_search_compact_live behind the last call that reset a root)", who);
    TG_HIP(hipSetDevice(s->cfg.device));
    hipStream_t st = use_stream(s, stream);
    const int T = s->dev.T;
    // the alignment every row's start really has: that of the buffers and of the row length
    const uintptr_t bits = reinterpret_cast<uintptr_t>(src_dev) | reinterpret_cast<uintptr_t>(dst_dev) | ((uintptr_t)row_floats * sizeof(float));
    if (bits % sizeof(float)) return tg::fail(TG_ERR_ARG, "%s: a buffer that is not aligned to a float", who);
    const int align = bits % 16 == 0 ? 16 : bits % 8 == 0 ? 8 : 4;
    const dim3 grid((unsigned)std::min((T + kRowWaves - 1) / kRowWaves, 4096)), block(64 * kRowWaves);
    auto launch = [&](auto g, auto a) {
        hipLaunchKernelGGL((rows_by_rank_kernel<decltype(g)::value, decltype(a)::value>), grid, block, 0, st, src_dev, dst_dev,
                           (const int32_t *)s->ranks.rank.get(), T, row_floats);
    };
    auto by_align = [&](auto g) {
        if (align == 16) launch(g, std::integral_constant<int, 16>{});
        else if (align == 8) launch(g, std::integral_constant<int, 8>{});
        else launch(g, std::integral_constant<int, 4>{});
    };
    if (gather) by_align(std::true_type{});
    else by_align(std::false_type{});
    TG_HIP(hipGetLastError());
    return TG_OK;
}

int tg_search_gather_rows_by_rank(tg_search *s, const float *src_dev, float *dst_dev, int row_floats, void *stream) {
    return rows_by_rank(s, "tg_search_gather_rows_by_rank", true, src_dev, dst_dev, row_floats, stream);
}

int tg_search_scatter_rows_by_rank(tg_search *s, const float *src_dev, float *dst_dev, int row_floats, void *stream) {
    return rows_by_rank(s, "tg_search_scatter_rows_by_rank", false, src_dev, dst_dev, row_floats, stream);
}

int tg_search_stop_rule(tg_search *s, const int32_t *total_host, int32_t *live_host, void *stream) {
    if (!s || !total_host) return tg::fail(TG_ERR_ARG, "tg_search_stop_rule: null argument");
    TG_HIP(hipSetDevice(s->cfg.device));
    int rc;
    if ((rc = stage_totals(s, "tg_search_stop_rule", total_host))) return rc;
    hipStream_t st = use_stream(s, stream);
    if ((rc = zero_live(s, 1, st)) || (rc = launch_stop_rule(s, 0, st))) return rc;
    return live_host ? read_live(s, 0, st, live_host) : TG_OK;
}

// the budget rule behind everything queued on st, counting into live counter `slot` (zeroed by the caller)
static int launch_budget_rule(tg_search *s, int slot, hipStream_t st) {
    tg_search::Halting &h = s->halting;
    const int T = s->dev.T;
    hipLaunchKernelGGL(budget_rule_kernel, dim3((T + 255) / 256), dim3(256), 0, st, s->dev, s->budgets.total.get(), h.stopped_at.get(),
                       h.live.get() + slot);
    TG_HIP(hipGetLastError());
    h.armed = true;
    s->ranks.mark_shrunk();
    return TG_OK;
}

int tg_search_budget_rule(tg_search *s, int32_t *live_host, void *stream) {
    if (!s) return tg::fail(TG_ERR_ARG, "tg_search_budget_rule: null argument");
    if (!s->budgets.on) return tg::fail(TG_ERR_STATE, "tg_search_budget_rule: no visit budgets are in force (tg_search_set_budget)");
    TG_HIP(hipSetDevice(s->cfg.device));
    int rc;
    if ((rc = halting_ready(s))) return rc;
    hipStream_t st = use_stream(s, stream);
    if ((rc = zero_live(s, 1, st)) || (rc = launch_budget_rule(s, 0, st))) return rc;
    return live_host ? read_live(s, 0, st, live_host) : TG_OK;
}

// tg_search_puct_chain with the stop rule queued behind the backup of every FULL mini-batch that has descents to follow - where
// MCTSTree.search tests is_move_decided (`leaves == batch_size and done < threshold`; batch_size: leaves_host[0]) -, and the live
// count read every poll_every mini-batches: the call returns once no tree is live.  The window covers the whole budget, as the
// chain's does; what a halted tree did not draw stays in it, and the cursors say what each tree consumed.
static int puct_chain_impl(tg_search *s, const char *who, tg_net *net, const int32_t *leaves_host, int n_batches, const int32_t *total_host,
                           int poll_every, int force_window, float *planes_dev, float *policy_dev, float *value_dev, void *stream,
                           int32_t *batches_run_host, bool compact, int64_t *positions_host, bool budget, tg_net *const *group_nets) {
    const bool early = total_host != nullptr;
    // GROUPED (tg_search_puct_chain_groups, which has checked the ranks and the networks): compact, by the grouped
    // ranks in force - group g's trees hold the rows [offset[g] * k, (offset[g] + count[g]) * k) and group_nets[g] evaluates them
    const bool grouped = group_nets != nullptr;
    if (!s || (!net && !grouped) || !leaves_host || !planes_dev || !policy_dev || !value_dev) return tg::fail(TG_ERR_ARG, "%s: null argument", who);
    if (n_batches < 1) return tg::fail(TG_ERR_ARG, "%s: no mini-batch", who);
    if (poll_every < 1) return tg::fail(TG_ERR_ARG, "%s: poll_every %d (at least 1)", who, poll_every);
    if (!grouped && tg_net_board_size(net) != s->S) return tg::fail(TG_ERR_ARG, "%s: network and search differ in board size", who);
    size_t total = 0;
    for (int b = 0; b < n_batches; ++b) {
        if (leaves_host[b] < 1 || leaves_host[b] > s->dev.K)
            return tg::fail(TG_ERR_ARG, "%s: mini-batch %d of %d leaves outside [1, batch_size]", who, b, leaves_host[b]);
        total += (size_t)leaves_host[b];
    }
    int rc;
    // BUDGET: the visit budgets in force bound every tree's descents, and the budget rule behind every backup
    // halts the trees that have spent theirs; the live count is looked at as the early chain looks at it
    if (early && s->budgets.on)
        return tg::fail(TG_ERR_ARG, "%s: an early-stop total while visit budgets are in force (tg_search_set_budget(NULL) first)", who);
    if (budget && !s->budgets.on) return tg::fail(TG_ERR_STATE, "%s: no visit budgets are in force (tg_search_set_budget)", who);
    if (early || compact || budget) TG_HIP(hipSetDevice(s->cfg.device));
    if (budget && (rc = halting_ready(s))) return rc;
    if (early && (rc = stage_totals(s, who, total_host))) return rc;
    if (early || budget) {
        if (!s->roots_expanded || s->roots.any())
            return tg::fail(TG_ERR_STATE, "%s: no root launch since a root was set, replaced or moved (tg_search_root_planes, forward, tg_search_backup first)", who);
    }
    if (compact && (rc = live_ranks_ready(s))) return rc;
    const size_t A = (size_t)s->A;
    // The window goes up one mini-batch's share at a time, each generated (MT19937 + log on this thread: ~90 us per 21 k draws)
    // and uploaded while the launches of the mini-batch before it run (select + forward + backup: 0.3 - 0.45 ms): a search that
    // starts from a freshly seeded stream - search_best_move hands numpy's state over per move - has nothing staged.
    if ((rc = feed_streams_impl(s, total * A, force_window, n_batches > 1 ? (size_t)leaves_host[0] * A : 0))) return rc;
    const bool pieces = s->win.book().in_parts();                              // (a new window was started and split)
    hipStream_t st = use_stream(s, stream);
    if ((early || budget) && (rc = zero_live(s, (size_t)n_batches, st))) return rc;
    // COMPACT: the forward passes cover the trees that were live at the last look - here, then at every poll, behind the rule.
    // Between two looks halt words are only set: a tree the selectors still take was live at the last one and has a rank
    // below `count`; one halted since keeps an idle slot until the next.
    int32_t count = s->dev.T;
    if (grouped) {
        count = 0;
        for (int g = 0; g < s->ranks.n_groups; ++g) count += s->ranks.group_count[g];
    } else if (compact && ((rc = launch_live_rank(s, st)) || (rc = read_word(s, s->ranks.count(), st, &count)))) {
        return rc;
    }
    size_t upto = 0;
    int run = 0, last_rule = -1;
    int64_t positions = 0;
    bool all_halted = count == 0;                                              // (compact: no tree is live, nothing is queued)
    for (int b = 0; b < n_batches && !all_halted; ++b) {
        const int k = leaves_host[b];
        upto += (size_t)k * A;
        if (b > 0 && pieces && (rc = s->win.extend(s->rng, upto, st))) return rc;
        if ((rc = select_puct_impl(s, who, k, planes_dev, nullptr, stream, compact))) return rc;
        if (grouped) {
            const tg_search::LiveRanks &r = s->ranks;
            for (int g = 0; g < r.n_groups; ++g) {
                const size_t row0 = (size_t)r.group_offset[g] * k;
                if (r.group_count[g] > 0 &&
                    (rc = tg_net_forward_dev(group_nets[g], planes_dev + row0 * 6 * (size_t)s->P, r.group_count[g] * k, 0,
                                             policy_dev + row0 * A, value_dev + row0 * 3, stream)))
                    return rc;
            }
        } else if ((rc = tg_net_forward_dev(net, planes_dev, count * k, 0, policy_dev, value_dev, stream))) {
            return rc;
        }
        positions += (int64_t)count * k;
        if ((rc = compact ? tg_search_backup_compact(s, policy_dev, value_dev, k, 0, stream)
                          : tg_search_backup(s, policy_dev, value_dev, k, 0, stream)))
            return rc;
        run = b + 1;
        if (early && k == leaves_host[0] && b + 1 < n_batches) {
            if ((rc = launch_stop_rule(s, b, st))) return rc;
            last_rule = b;
        }
        if (budget) {
            if ((rc = launch_budget_rule(s, b, st))) return rc;
            last_rule = b;
        }
        if ((early || budget) && run % poll_every == 0 && last_rule >= 0 && b + 1 < n_batches) {
            // (the compact count is the rule's live counter taken over every tree: the same predicate, one launch later)
            int32_t live = 0;
            if (compact) {
                if ((rc = launch_live_rank(s, st)) || (rc = read_word(s, s->ranks.count(), st, &live))) return rc;
                count = live;
            } else if ((rc = read_live(s, last_rule, st, &live))) {
                return rc;
            }
            all_halted = live == 0;
        }
    }
    if (batches_run_host) *batches_run_host = run;
    if (positions_host) *positions_host = positions;
    return s->win.complete_rest(s->rng);                                          // (what the mini-batches not run would have extended by)
}

int tg_search_puct_chain_early(tg_search *s, tg_net *net, const int32_t *leaves_host, int n_batches, const int32_t *total_host,
                               int poll_every, int force_window, float *planes_dev, float *policy_dev, float *value_dev, void *stream,
                               int32_t *batches_run_host) {
    if (!total_host) return tg::fail(TG_ERR_ARG, "tg_search_puct_chain_early: null argument");
    return puct_chain_impl(s, "tg_search_puct_chain_early", net, leaves_host, n_batches, total_host, poll_every, force_window, planes_dev,
                           policy_dev, value_dev, stream, batches_run_host, false, nullptr);
}

int tg_search_puct_chain_compact(tg_search *s, tg_net *net, const int32_t *leaves_host, int n_batches, const int32_t *total_host,
                                 int poll_every, int force_window, float *planes_dev, float *policy_dev, float *value_dev, void *stream,
                                 int32_t *batches_run_host, int64_t *positions_host) {
    return puct_chain_impl(s, "tg_search_puct_chain_compact", net, leaves_host, n_batches, total_host, total_host ? poll_every : 1,
                           force_window, planes_dev, policy_dev, value_dev, stream, batches_run_host, true, positions_host);
}

int tg_search_puct_chain_groups(tg_search *s, tg_net *const *nets, int n_groups, const int32_t *leaves_host, int n_batches, int force_window,
                                float *planes_dev, float *policy_dev, float *value_dev, void *stream, int64_t *positions_host) {
    const char *who = "tg_search_puct_chain_groups";
    if (!s || !nets) return tg::fail(TG_ERR_ARG, "%s: null argument", who);
    if (n_groups < 1 || n_groups > tg_group::kMaxGroups) return tg::fail(TG_ERR_ARG, "%s: n_groups %d outside [1, %d]", who, n_groups, tg_group::kMaxGroups);
    const tg_search::LiveRanks &r = s->ranks;
    if (r.state == tg_search::LiveRanks::State::Fresh && !r.grouped)
        return tg::fail(TG_ERR_STATE, "%s: the ranks in force are plain live ranks (tg_search_group_live behind the last tg_search_compact_live "
                        "or chained call that polled)", who);
    if (r.state != tg_search::LiveRanks::State::Fresh)
        return tg::fail(TG_ERR_STATE, "%s: no fresh grouped ranks (tg_search_group_live behind the last call that wrote halt words or reset a root)", who);
    if (r.n_groups != n_groups)
        return tg::fail(TG_ERR_ARG, "%s: %d networks for ranks of %d groups", who, n_groups, r.n_groups);
    if (s->budgets.on) return tg::fail(TG_ERR_ARG, "%s: visit budgets are in force (tg_search_set_budget(NULL) first): the grouped chain is strict", who);
    for (int g = 0; g < n_groups; ++g) {
        if (!nets[g]) {
            if (r.group_count[g] > 0) return tg::fail(TG_ERR_ARG, "%s: no network for group %d, which has %d live trees", who, g, r.group_count[g]);
            continue;
        }
        if (tg_net_board_size(nets[g]) != s->S) return tg::fail(TG_ERR_ARG, "%s: network %d and search differ in board size", who, g);
    }
    return puct_chain_impl(s, who, nullptr, leaves_host, n_batches, nullptr, 1, force_window, planes_dev, policy_dev, value_dev, stream,
                           nullptr, true, positions_host, false, nets);
}

int tg_search_puct_chain_budget(tg_search *s, tg_net *net, const int32_t *leaves_host, int n_batches, int poll_every, int compact,
                                int force_window, float *planes_dev, float *policy_dev, float *value_dev, void *stream,
                                int32_t *batches_run_host, int64_t *positions_host) {
    if (compact != 0 && compact != 1) return tg::fail(TG_ERR_ARG, "tg_search_puct_chain_budget: compact %d is neither 0 nor 1", compact);
    return puct_chain_impl(s, "tg_search_puct_chain_budget", net, leaves_host, n_batches, nullptr, poll_every, force_window, planes_dev,
                           policy_dev, value_dev, stream, batches_run_host, compact != 0, positions_host, true);
}

// ---- one lock-step move, three schemes (round trip, chained, chained in sub-groups): the pieces they share ------------------
using MoveBuffers = tg_selfplay::MoveBuffers;

static inline double sp_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// host-side wall clock per section of a move, per handle (TG_SP_TIMING=1: a line every 200 moves) - where a move's time goes
// when the GPU is not the bound.  lap(i) closes section i: each index belongs to ONE section of a scheme.
struct LapTimer {
    tg_selfplay *sp;
    double last;
    explicit LapTimer(tg_selfplay *sp_) : sp(enabled() ? sp_ : nullptr), last(sp ? sp_now() : 0.0) {}
    static bool enabled() { static const bool on = getenv("TG_SP_TIMING") != nullptr; return on; }
    void lap(int i) { if (sp) { const double t = sp_now(); sp->t_acc[i] += t - last; last = t; } }
    void report(const char *scheme, std::initializer_list<const char *> sections) {       // (the move is over: sections in lap order)
        if (!sp || ++sp->moves_timed % 200 != 0) return;
        std::string line;
        char buf[96];
        int i = 0;
        for (const char *name : sections) {
            snprintf(buf, sizeof(buf), "%s %s %.3f", i ? " |" : "", name, 1e3 * sp->t_acc[i] / sp->moves_timed);
            line += buf;
            ++i;
        }
        fprintf(stderr, "[selfplay timing%s, ms per move over %ld moves]%s\n", scheme, sp->moves_timed, line.c_str());
    }
};

// observer events (tg_selfplay_set_observer): a forward pass that has been queued (phase -1: the root evaluation) ...
static void emit_forward(tg_selfplay *sp, int phase, int64_t positions, const int32_t *nc, const int32_t *mc, const MoveBuffers &b) {
    if (!sp->observer) return;
    tg_selfplay_event ev{};
    ev.kind = 0; ev.phase = phase; ev.trees = sp->s->dev.T; ev.positions = (int32_t)positions;
    ev.num_considered = nc; ev.max_count = mc;
    ev.planes_dev = b.planes; ev.policy_dev = b.policy; ev.value_dev = b.value; ev.stream = b.stream;
    sp->observer(sp->observer_user, &ev);
}

// ... and a move that has been decided (finish_move_impl's root statistics and moves)
static void emit_move(tg_selfplay *sp, int n_phases, const int32_t *finished_host) {
    if (!sp->observer) return;
    tg_selfplay_event ev{};
    ev.kind = 1; ev.phase = n_phases; ev.trees = sp->s->dev.T;
    ev.num_children = sp->nc.data(); ev.action = sp->act32.data(); ev.children_visits = sp->visits_a.data();
    ev.children_value_sum = sp->vsum_a.data(); ev.moves = sp->mv.data(); ev.finished = finished_host;
    sp->observer(sp->observer_user, &ev);
}

// The root expansion is the only consumer of draws in its launch, and a Dirichlet prior takes one draw per child: the draws
// it consumed - sp->consumed, the cursors behind it, less `before`, the cursors ahead of it (null: 0) - ARE the root's child
// count (saves the schedule's own device read), provided nothing went wrong in that launch (a sticky device error - pool full,
// window exhausted - would leave a cursor that is not a child count): the count must be plausible here, and check_root_widths
// compares it with the root statistics read back behind the last phase, where the device error words are checked as well (no
// extra synchronisation here).  skip (may be null): boards that take no part in the move.
static int root_widths_from_draws(tg_selfplay *sp, const int64_t *before, const uint8_t *skip) {
    const int T = sp->s->dev.T, A = sp->s->A;
    sp->nc.assign(T, 0);
    for (int t = 0; t < T; ++t) {
        if (skip && skip[t]) continue;
        const int64_t n = sp->consumed[t] - (before ? before[t] : 0);
        if (n < 1 || n > A)
            return tg::fail(TG_ERR_STATE, "tg_selfplay_play_move: board %d consumed %lld draws at its root (expected 1..%d)",
                            t, (long long)n, A);
        sp->nc[t] = (int32_t)n;
    }
    sp->nc_known = true;
    sp->nc_cursor = sp->nc;
    return TG_OK;
}

// the roots' child counts in the records / the statistics read-back must be what the draw cursors said
static int check_root_widths(const tg_selfplay *sp, const uint8_t *skip) {
    const int T = sp->s->dev.T;
    for (int t = 0; t < T; ++t)
        if (!(skip && skip[t]) && sp->nc[t] != sp->nc_cursor[t])
            return tg::fail(TG_ERR_STATE, "tg_selfplay_play_move: board %d has %d root children but its root expansion "
                            "consumed %d draws - the halving schedule was built from a wrong width (cursor %lld behind the root, %lld "
                            "behind the phases before it; window %lld; game move %d)", t, sp->nc[t], sp->nc_cursor[t],
                            (long long)sp->consumed[t], (long long)(sp->consumed[t] - sp->nc_cursor[t]), (long long)sp->s->win.book().capacity(),
                            sp->games[t].moves_played);
    return TG_OK;
}

// What a move's phases will do, known on the host before any of them is launched: the halving schedule (sp->ph_nc / ph_mc,
// [n_phases][T]), per phase the leaves of all trees and of the widest tree, and the random window the phases can consume.
struct MovePlan {
    int32_t n_phases = 0;
    int64_t total[tg_selfplay::kMaxPhases] = {}, slots[tg_selfplay::kMaxPhases] = {};    // sum / max over the trees of nc * mc
    int64_t window = 0, first_window = 0;                                                  // draws per tree: all phases / the first one
};

static int plan_move(tg_selfplay *sp, MovePlan *out) {
    const int T = sp->s->dev.T, A = sp->s->A;
    *out = MovePlan{};
    // ---- sequential halving (tree.py:375-384) ----
    sp->ph_nc.resize((size_t)tg_selfplay::kMaxPhases * T);
    sp->ph_mc.resize((size_t)tg_selfplay::kMaxPhases * T);
    if (int rc = tg_selfplay_schedule(sp, sp->ph_nc.data(), sp->ph_mc.data(), tg_selfplay::kMaxPhases, &out->n_phases)) return rc;
    // Random draws the phases can consume: one Dirichlet prior (<= A draws) per EXPANSION, and only the first descent
    // through a root child can expand a node.  Root children entered in a phase: at most its width
    // (new ones: the picks among the unvisited children are nested prefixes of their score order, the first round's
    // being the largest) plus the children visited before the phase.  ONE window for all phases of the move is
    // generated and uploaded up front (the device cursor runs on from launch to launch) and the consumption is
    // read back once, behind the last phase - not a window, an upload and a host synchronisation per phase, each
    // sized as if every descent expanded (2.4x more draws).  The first part is what the first phase can consume; the
    // rest goes up while that phase runs.
    sp->ph_seen.assign(T, 0);
    for (int ph = 0; ph < out->n_phases; ++ph) {
        const int32_t *nc = &sp->ph_nc[(size_t)ph * T], *mc = &sp->ph_mc[(size_t)ph * T];
        int64_t expansions = 0;
        for (int t = 0; t < T; ++t) {
            const int64_t n = (int64_t)nc[t] * mc[t];
            out->total[ph] += n;
            out->slots[ph] = n > out->slots[ph] ? n : out->slots[ph];
            const int64_t entered = std::min<int64_t>(n, std::min<int64_t>(A, (int64_t)nc[t] + sp->ph_seen[t]));
            expansions = entered > expansions ? entered : expansions;
            sp->ph_seen[t] = (int32_t)std::min<int64_t>(A, sp->ph_seen[t] + entered);
        }
        out->window += expansions * A;
        if (ph == 0) out->first_window = out->window;
    }
    return TG_OK;
}

// The phases of a move with the whole lock-step group in one launch each: selection, forward pass, backup on the caller's
// stream, the rest of the random window going up behind the first launched phase.
static int run_phases_whole_group(tg_selfplay *sp, tg_net *net, const MovePlan &plan, const MoveBuffers &b, int64_t *leaves,
                                  int64_t *forwarded, bool *any_phase) {
    tg_search *s = sp->s;
    const int T = s->dev.T, layout = sp->unique ? -1 : 0;
    int rc;
    for (int ph = 0; ph < plan.n_phases; ++ph) {
        if (plan.slots[ph] == 0) continue;
        const int32_t *nc = &sp->ph_nc[(size_t)ph * T], *mc = &sp->ph_mc[(size_t)ph * T];
        if ((rc = tg_search_select_gumbel(s, nc, mc, layout, b.planes, b.stream))) return rc;
        const int64_t fwd = sp->unique ? s->last.planes : plan.total[ph];     // (UNIQUE: the plane ranges, known without a read-back)
        if ((rc = tg_net_forward_dev(net, b.planes, (int)fwd, 1, b.policy, b.value, b.stream))) return rc;
        if ((rc = tg_search_backup(s, b.policy, b.value, layout, 1, b.stream))) return rc;
        *forwarded += fwd;
        emit_forward(sp, ph, fwd, nc, mc, b);
        *leaves += plan.total[ph];
        if (!*any_phase && (rc = s->win.complete_rest(s->rng))) return rc;             // behind the first launched phase
        *any_phase = true;
    }
    return s->win.complete_rest(s->rng);                                               // (no phase was launched)
}

// The phases of a move with the boards in G sub-groups, each on a stream of its own and one selection behind the
// previous one: a sub-group's forward pass (most of the CUs) runs while the others' tree kernels (one workgroup per
// board) do - with ONE group the forward pass waits for the slowest board's selection and the selection for the whole
// forward pass, every phase.  Same kernels, on slices of the engine (sub_dev); leaf slots: sub-group g owns positions
// [first board x batch_size ...) of the caller's buffers, so sub-groups in different phases never share rows.
static int launch_phases_subgroups(tg_selfplay *sp, tg_net *net, const MovePlan &plan, int G, const MoveBuffers &b, int64_t *leaves,
                                   int64_t *forwarded, bool *any_phase) {
    tg_search *s = sp->s;
    const int T = s->dev.T, A = s->A, K = s->dev.K, n_phases = plan.n_phases;
    const size_t P = (size_t)s->P;
    constexpr int kMaxPhases = tg_selfplay::kMaxPhases;
    hipStream_t st = static_cast<hipStream_t>(b.stream);
    int rc;
    if ((rc = sp->phase_all_dev.reserve((size_t)kMaxPhases * 3 * T))) return rc;
    for (int g = 1; g < G; ++g)
        if ((rc = sp->sub_stream[g - 1].create())) return rc;
    int tb[tg_selfplay::kMaxSub + 1];
    for (int g = 0; g <= G; ++g) tb[g] = (int)((int64_t)g * T / G);
    int32_t *tab;
    int ring;
    if ((rc = sp->phase_all_pin.acquire((size_t)kMaxPhases * 3 * T, &tab, &ring))) return rc;
    const bool unique = sp->unique;
    const LeafLayout layout = unique ? LeafLayout::Unique : LeafLayout::Packed;
    PhaseLayout lay[kMaxPhases][tg_selfplay::kMaxSub];                 // per phase, each sub-group's launch
    for (int ph = 0; ph < n_phases; ++ph)
        for (int g = 0; g < G; ++g)
            if ((rc = layout_phase(s, "tg_selfplay_play_move", &sp->ph_nc[(size_t)ph * T], &sp->ph_mc[(size_t)ph * T], tb[g], tb[g + 1], K,
                                   layout, (int64_t)tb[g] * K, tab + (size_t)ph * 3 * T, nullptr, &lay[ph][g])))
                return rc;
    TG_HIP(hipMemcpyAsync(sp->phase_all_dev.get(), tab, (size_t)n_phases * 3 * T * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = sp->phase_all_pin.commit(ring, st))) return rc;
    use_stream(s, st);
    if ((rc = s->win.install(s->rng, &s->dev, st))) return rc;                          // (the first part of the window; the cursors back to 0)
    s->last.subgroups = true;                                          // (no whole-engine ranges: tg_search_unique_planes has nothing to report)
    s->last.layout = layout;
    if ((rc = sp->ev_start.record(st))) return rc;
    for (int g = 1; g < G; ++g) TG_HIP(hipStreamWaitEvent(sp->sub_stream[g - 1].get(), sp->ev_start.get(), 0));
    int launched[tg_selfplay::kMaxSub] = {};
    int last_started = -1;                                              // the last sub-group whose first selection is queued
    for (int ph = 0; ph < n_phases; ++ph) {
        const int32_t *row = sp->phase_all_dev.get() + (size_t)ph * 3 * T;
        for (int g = 0; g < G; ++g) {
            const int64_t count = lay[ph][g].positions;
            if (count == 0) continue;
            hipStream_t sg = g == 0 ? st : sp->sub_stream[g - 1].get();
            static const bool stagger = tg::knob("TG_SP_STAGGER") && atoi(tg::knob("TG_SP_STAGGER")) != 0;   // (measured: no gain at 16 boards, -3 % at 24 - the streams fall out of step by themselves)
            if (stagger && launched[g] == 0 && last_started >= 0) TG_HIP(hipStreamWaitEvent(sg, sp->ev_first_sel[last_started].get(), 0));
            if (launched[g] == 1 && *any_phase) TG_HIP(hipStreamWaitEvent(sg, s->win.rest_event(), 0));   // second part of the window
            const SearchDev D = sub_dev(s, tb[g], tb[g + 1] - tb[g]);
            const int32_t *off = row + 2 * (size_t)T + tb[g];
            if ((rc = launch_gumbel_select(s, D, row + tb[g], row + T + tb[g], off, K, lay[ph][g].max_n, b.planes, sg, unique))) return rc;
            if (launched[g] == 0) {
                if ((rc = sp->ev_first_sel[g].record(sg))) return rc;
                last_started = g;
            }
            const size_t o = (size_t)tb[g] * K;
            if ((rc = tg_net_forward_dev(net, b.planes + o * 6 * P, (int)count, 1, b.policy + o * A, b.value + o * 3, sg))) return rc;
            if ((rc = launch_backup(s, D, b.policy, b.value, 0, off, 1, sg, unique))) return rc;
            *leaves += lay[ph][g].queued;
            *forwarded += count;
            launched[g] += 1;
            if (!*any_phase) {
                *any_phase = true;
                if ((rc = s->win.complete_rest(s->rng))) return rc;           // behind the first launched selection
            }
        }
    }
    for (int g = 1; g < G; ++g) {
        if ((rc = sp->ev_sub_done[g - 1].record(sp->sub_stream[g - 1].get()))) return rc;
        TG_HIP(hipStreamWaitEvent(st, sp->ev_sub_done[g - 1].get(), 0));
    }
    return s->win.complete_rest(s->rng);                                       // (no phase was launched)
}

// Sub-groups of a move of T boards of size S on a device of num_cus CUs, and the CUs its forward launches are capped to
// (0: none).  False - one group - where the move cannot be split: an observer sees whole phases, no phase has nothing to split.
static bool choose_subgroups(int T, int S, int num_cus, bool observer, int n_phases, int *G, int *fwd_cap) {
    *G = 1;
    *fwd_cap = 0;
    if (observer || n_phases == 0) return false;
    // measured (tools/bench_selfplay.py, 400 simulations, leaf evaluations/s, one group -> sub-groups): 4 boards 1.06 -> 1.20 M
    // (2), 8: 1.71 -> 1.86 M (2), 16: 2.49 -> 2.84 M (3), 24: 3.00 -> 3.30 M (4); from 32 boards on a sub-group's forward pass
    // needs every CU or comes in launches too small to be efficient (32 boards: 3.26 M whole, 2.95 M in six)
    // More boards: two halves (29 .. 96 boards) or four quarters (.. 224), the forward launches kept off as many CUs as the
    // OTHER sub-groups' tree kernels need (a forward workgroup holds its CU for the whole launch - without the cap a
    // selection waits for it to end, with 8 CUs too few the forward pass waits for the selection): 32 boards 3.33 -> 3.57 M,
    // 48: 3.82 -> 4.16 M, 64: 4.09 -> 4.50 M, 96: 4.43 -> 4.72 M, 128: 4.62 -> 4.87 M, 192: 4.83 -> 4.97 M; 256: no gain.
    // (re-measured when the selection launch got shorter - the workers take whole entries, round 6 -: three sub-groups beat four
    // from 13 boards on - 20 boards 3.50 -> 4.01 M, 24: 3.95 -> 4.11 M, 28: 4.22 -> 4.41 M - and a forward cap pays from 24 boards:
    // 24: 4.17 -> 4.25 M, 28: 4.46 -> 4.62 M; 8 / 12 boards: two sub-groups as before)
    if (T >= 4 && T <= 12) *G = 2;
    else if (T > 12 && T <= 28) { *G = 3; if (T >= 24) *fwd_cap = num_cus - 32; }
    else if (T > 28 && T <= 96) { *G = 2; *fwd_cap = num_cus - std::max(32, T / 2); }
    else if (T > 96 && T <= 224) { *G = 4; *fwd_cap = num_cus - 32; }
    else if (T > 224 && T <= 384) { *G = 2; *fwd_cap = num_cus - 32; }     // (256 boards, one-axis forward kernel: 6.07 -> 6.30 M; 512: level)
    // (19x19: the pair kernel's launches follow each other across streams, net_device.h band_done - sub-groups only add launches:
    // 16 boards x 100 simulations 0.53 -> 0.55 M, 64 boards 0.86 -> 0.91 M leaf evaluations/s as one group)
    if (S == 19) { *G = 1; *fwd_cap = 0; }
    return true;
}

// Two evaluators, one per colour (tg_selfplay_play_move2 with net_to_move != net_next): a lock-step call has ONE mover colour.
// Every board that searches in the call has the same side to move; chained scheme: every board whose root the call's chain
// evaluates for the next call has the other one - the boards that moved have by themselves, a slot whose game was just started
// has black to move, so it may only sit out a call in which white moves.  Checked on the host before anything is launched:
// a violation is an error that names the slot, never an evaluation by the wrong network.
// The calls alternate between the two networks: the one a call names as net_next is the next call's net_to_move - a caller that
// hands the two over the wrong way round is caught from the second two-network call on, also where no board searches.  (Which
// of the two is black's is the caller's word in the first call: the library has no notion of whose network is whose.)
static int check_one_mover(const tg_selfplay *sp, bool chained, const tg_net *net_to_move) {
    const int T = sp->s->dev.T;
    if (sp->turn_net && net_to_move != sp->turn_net)
        return tg::fail(TG_ERR_STATE, "tg_selfplay_play_move2: net_to_move is not the network the last call named as net_next: "
                        "the two networks take turns call by call");
    int mover = kEmpty, mover_slot = -1;
    for (int t = 0; t < T; ++t) {
        const SpGame &g = sp->games[t];
        if (g.done || (chained && (g.fresh || !sp->chain_started))) continue;
        if (mover == kEmpty) { mover = g.to_move; mover_slot = t; }
        else if (g.to_move != mover)
            return tg::fail(TG_ERR_STATE, "tg_selfplay_play_move2: slot %d has %s to move but slot %d has %s: a call with two "
                            "networks moves one colour", t, g.to_move == kBlack ? "black" : "white", mover_slot,
                            mover == kBlack ? "black" : "white");
    }
    if (!chained || mover != kBlack) return TG_OK;
    for (int t = 0; t < T; ++t) {
        const SpGame &g = sp->games[t];
        if (!g.done && g.fresh)
            return tg::fail(TG_ERR_STATE, "tg_selfplay_play_move2: slot %d was started for a call in which black moves (slot %d): "
                            "its root would be evaluated by white's network", t, mover_slot);
    }
    return TG_OK;
}

// Chained moves.  A call = one lock-step move of every board whose root is expanded:
//   host   cursors of the last chain -> root child counts; Gumbel noise; halving schedule; random window (phases + next root)
//   device the phases (selection, forward, backup); finish_roots_kernel: root records + THE MOVE (choice, resign, game end);
//          play_kernel on the device's own moves; next root expansion, forward, backup          <- no host in between
//   host   (while that runs) last move's record comments, draws generated ahead; then waits for the RECORDS only (fin_ev,
//          recorded ahead of play_kernel), does the bookkeeping - checking the device's decision against its own - and returns
//          with the device still ~0.15 ms from the end of the root evaluation the next call starts from.
// A slot whose game has just been started (tg_selfplay_start_game) sits out one call: its root is expanded by that call's
// chain.  The first call of a handle therefore evaluates roots only.  Games, records and draws are those of the
// round-trip scheme (the draws of a game are consumed in the same order: root prior, noise, phases, next root prior ...).
// Two evaluators (tg_selfplay_play_move2): the phases run on `net`, the closing root evaluation on `net_next`.
static int chain_begin(tg_selfplay *sp, tg_net *net, tg_net *net_next, const MoveBuffers &b) {
    tg_search *s = sp->s;
    const int T = s->dev.T, A = s->A;
    hipStream_t st = static_cast<hipStream_t>(b.stream);
    int rc;
    LapTimer timer(sp);
    if ((rc = s->rng.check_seeded("tg_selfplay_play_move", nullptr))) return rc;
    if (net_next != net && (rc = check_one_mover(sp, true, net))) return rc;
    sp->skip.assign(T, 0);
    sp->skip_fresh.assign(T, 0);
    int64_t leaves = 0;
    for (int t = 0; t < T; ++t) {
        const SpGame &g = sp->games[t];
        sp->skip_fresh[t] = (!sp->chain_started || g.fresh) ? 1 : 0;          // (before the first chain no root is expanded)
        sp->skip[t] = (g.done || sp->skip_fresh[t]) ? 1 : 0;
        leaves += sp->skip[t] ? 0 : 1;                                        // the root evaluation this move starts from
    }
    int64_t forwarded = leaves;                                               // positions handed to the network (UNIQUE: fewer than leaves)
    // ---- the roots' child counts, off the draw cursors (before the first chain every board is skipped) ----
    sp->consumed.assign(T, 0);
    sp->c_phase.resize(T, 0);
    if (sp->chain_started) {
        TG_HIP(hipEventSynchronize(s->cur_ev.get()));
        if ((rc = advance_streams_impl(s, sp->consumed.data(), sp->skip_fresh.data(), s->cur_pin.get()))) return rc;
    }
    if ((rc = root_widths_from_draws(sp, sp->c_phase.data(), sp->skip.data()))) return rc;
    timer.lap(0);
    // (generated on the device, legacy_rng_device.h; the readers of the last noise - phases, finish_roots_kernel - lie before cur_ev)
    if ((rc = draw_noise_impl(s, nullptr, sp->skip_fresh.data(), sp->chain_started ? s->cur_ev.get() : nullptr))) return rc;
    timer.lap(1);
    MovePlan plan;
    if ((rc = plan_move(sp, &plan))) return rc;
    timer.lap(2);
    // one window for the phases and the next root's prior (<= A draws)
    if ((rc = feed_streams_impl(s, (size_t)(plan.window + A), 1, plan.window > 0 ? (size_t)plan.first_window : 0))) return rc;
    timer.lap(3);
    bool any_phase = false;
    int G, fwd_cap;
    if (choose_subgroups(T, s->S, s->num_cus, sp->observer != nullptr, plan.n_phases, &G, &fwd_cap)) {
        // (TG_SP_SUBGROUPS / TG_SP_FWD_CAP override; 1 = the whole lock-step group at once.  Read per call: tests toggle them)
        const int sub_env = tg::knob("TG_SP_SUBGROUPS") ? atoi(tg::knob("TG_SP_SUBGROUPS")) : 0;
        if (sub_env > 0) { G = sub_env; fwd_cap = 0; }
        if (tg::knob("TG_SP_FWD_CAP")) fwd_cap = atoi(tg::knob("TG_SP_FWD_CAP"));
        G = std::max(1, std::min(std::min(G, (int)tg_selfplay::kMaxSub), T));
    }
    if (G > 1) {
        const tg::LaunchCapsScope caps(16, fwd_cap > 0 ? fwd_cap : 0);   // (caps belong to this thread's launches, forward_plan.h)
        rc = launch_phases_subgroups(sp, net, plan, G, b, &leaves, &forwarded, &any_phase);
    } else {
        rc = run_phases_whole_group(sp, net, plan, b, &leaves, &forwarded, &any_phase);
    }
    if (rc) return rc;
    // No phase at all - every board's game has just been started (the first call of a handle; later: all games of the group
    // ended with the same move, which a one-board group does every game): the new window must be in place BEFORE
    // finish_roots_kernel notes each board's cursor "behind the phases", or that note is the OLD window's last cursor and the
    // next move reads a root of nc - that many children off it (found in round 6 with one-board lanes: "board 0 has 82 root
    // children but its root expansion consumed 81 draws").
    if (!any_phase && (rc = s->win.install(s->rng, &s->dev, st))) return rc;
    // ---- the chain: records + decision, the moves played, the next roots expanded and evaluated ----
    const int max_moves = s->S * s->S * 2;                             // worker.py:44
    sp->state.assign((size_t)tg_readout::kStateWords * T, 0);
    for (int t = 0; t < T; ++t) {
        const SpGame &g = sp->games[t];
        int32_t *st_t = &sp->state[(size_t)tg_readout::kStateWords * t];
        st_t[tg_readout::kStateFlags] = (sp->skip[t] ? tg_readout::kStateIdle : 0) | (g.never_resign ? tg_readout::kStateNeverResign : 0);
        st_t[tg_readout::kStatePasses] = g.pass_count;
        st_t[tg_readout::kStatePlayed] = g.moves_played;
    }
    use_stream(s, st);
    if ((rc = launch_finish_roots(s, sp->state.data(), max_moves, st)) || (rc = launch_play(s, st))) return rc;
    if ((rc = tg_search_root_planes(s, b.planes, b.stream))) return rc;           // (also uploads the roots of games just started)
    if (!s->cur_pin.get() && (rc = s->cur_pin.alloc((size_t)T, hipHostMallocMapped))) return rc;
    hipLaunchKernelGGL(publish_cursors_kernel, dim3((T + 255) / 256), dim3(256), 0, st, s->dev.rng_cursor, s->cur_pin.dev(), T);
    TG_HIP(hipGetLastError());
    if ((rc = s->cur_ev.record(st))) return rc;                                 // (the host needs the cursors, not the evaluation)
    if ((rc = tg_net_forward_dev(net_next, b.planes, T, 1, b.policy, b.value, b.stream))) return rc;   // (the next mover's network)
    if ((rc = tg_search_backup(s, b.policy, b.value, 1, 1, b.stream))) return rc;
    timer.lap(4);
    // ---- host work that nobody is waiting for: the previous move's record comments ----
    flush_comments(sp);
    timer.lap(5);
    sp->fwd_positions += forwarded;
    sp->turn_net = net_next != net ? net_next : nullptr;
    sp->pend = tg_selfplay::PendingMove{true, any_phase, leaves, plan.n_phases, b};
    return TG_OK;
}

static int chain_end(tg_selfplay *sp, int32_t *finished_host, int64_t *stats_host) {
    tg_search *s = sp->s;
    const int T = s->dev.T, A = s->A;
    int rc;
    LapTimer timer(sp);
    const tg_selfplay::PendingMove &pm = sp->pend;
    sp->pend.active = false;
    // ---- the records (not the stream): bookkeeping ----
    TG_HIP(hipEventSynchronize(s->fin_ev.get()));
    timer.lap(6);
    const RootTail *tail = reinterpret_cast<const RootTail *>(s->roots_host.get() + tg_readout::root_tail_offset(T, A));
    for (int t = 0; t < T; ++t) sp->c_phase[t] = tail[t].cursor;
    sp->mv.resize(T);
    int64_t counts[2] = {0, 0};
    if (pm.any_phase || sp->chain_started) {
        if ((rc = finish_move_impl(sp, sp->mv.data(), finished_host, counts, tail))) return rc;
        if ((rc = check_root_widths(sp, sp->skip.data()))) return rc;
        emit_move(sp, pm.n_phases, finished_host);
    } else {
        for (int t = 0; t < T; ++t) finished_host[t] = 0;
        if ((rc = root_record_errors(s))) return rc;
    }
    emit_forward(sp, -1, T, nullptr, nullptr, pm.bufs);              // the next root evaluation (its buffers are untouched since)
    for (int t = 0; t < T; ++t) sp->games[t].fresh = false;           // every root is expanded now (or about to be)
    sp->chain_started = true;
    timer.lap(7);
    timer.report(" (chained)", {"cursors", "noise", "schedule", "feed", "launches", "comments + draws ahead", "wait for records",
                                "bookkeeping"});
    if (stats_host) { stats_host[0] = counts[0]; stats_host[1] = counts[1]; stats_host[2] = pm.leaves; }
    return TG_OK;
}

static int play_move_chain(tg_selfplay *sp, tg_net *net, tg_net *net_next, const MoveBuffers &b, int32_t *finished_host,
                           int64_t *stats_host) {
    if (sp->pend.active) return tg::fail(TG_ERR_STATE, "tg_selfplay_play_move: a move begun with tg_selfplay_move_begin has not been ended");
    if (int rc = chain_begin(sp, net, net_next, b)) return rc;
    return chain_end(sp, finished_host, stats_host);
}

// The round-trip scheme (TG_SP_CHAIN=0): the move decided on the host, three host round trips per move.  The root evaluation and
// the phases both run on `net`; net_next != net (two evaluators): every live board has the same side to move, or nothing is
// launched, and net_next is only remembered as the network whose turn is next.
static int play_move_sync(tg_selfplay *sp, tg_net *net, tg_net *net_next, const MoveBuffers &b, int32_t *finished_host,
                          int64_t *stats_host) {
    tg_search *s = sp->s;
    const int T = s->dev.T, A = s->A;
    int rc;
    LapTimer timer(sp);
    if (net_next != net && (rc = check_one_mover(sp, false, net))) return rc;
    int64_t leaves = 0;
    for (int t = 0; t < T; ++t) leaves += sp->games[t].done ? 0 : 1;
    int64_t forwarded = leaves;
    // ---- root: expand, evaluate (tree.py:330-336) ----
    if ((rc = tg_search_feed_streams(s, (size_t)A, sp->force_feed ? 1 : 0))) return rc;
    sp->force_feed = false;
    timer.lap(0);
    if ((rc = tg_search_root_planes(s, b.planes, b.stream))) return rc;
    if ((rc = tg_net_forward_dev(net, b.planes, T, 1, b.policy, b.value, b.stream))) return rc;
    if ((rc = tg_search_backup(s, b.policy, b.value, 1, 1, b.stream))) return rc;
    sp->consumed.resize(T);
    if ((rc = tg_search_advance_streams(s, sp->consumed.data()))) return rc;
    if ((rc = root_widths_from_draws(sp, nullptr, nullptr))) return rc;
    emit_forward(sp, -1, T, nullptr, nullptr, b);                      // this move's root evaluation
    timer.lap(1);
    if ((rc = tg_search_draw_noise(s, nullptr))) return rc;
    timer.lap(2);
    MovePlan plan;
    if ((rc = plan_move(sp, &plan))) return rc;
    timer.lap(3);
    if (plan.window > 0 && (rc = feed_streams_impl(s, (size_t)plan.window, 0, (size_t)plan.first_window))) return rc;
    timer.lap(4);
    bool any_phase = false;
    if ((rc = run_phases_whole_group(sp, net, plan, b, &leaves, &forwarded, &any_phase))) return rc;
    timer.lap(5);
    // ---- host work that nobody is waiting for, while the phase kernels run: the previous move's record comments ----
    flush_comments(sp);
    timer.lap(6);
    if (any_phase && (rc = tg_search_advance_streams(s, nullptr))) return rc;
    timer.lap(7);
    // ---- move choice, records, finished games; play ----
    sp->mv.resize(T);
    int64_t counts[2] = {0, 0};
    if ((rc = tg_selfplay_finish_move(sp, sp->mv.data(), finished_host, counts))) return rc;
    if ((rc = check_errors(s))) return rc;          // (the stream is drained here: finish_move has read the roots back)
    if ((rc = check_root_widths(sp, nullptr))) return rc;
    emit_move(sp, plan.n_phases, finished_host);
    timer.lap(8);
    if ((rc = tg_search_play(s, sp->mv.data(), b.stream))) return rc;
    timer.lap(9);
    timer.report("", {"feed(root)", "root evaluation + cursors", "noise", "schedule", "feed(phases)", "launches", "comments",
                      "wait for phases", "finish_move", "play"});
    sp->fwd_positions += forwarded;
    sp->turn_net = net_next != net ? net_next : nullptr;
    if (stats_host) { stats_host[0] = counts[0]; stats_host[1] = counts[1]; stats_host[2] = leaves; }
    return TG_OK;
}

// One whole self-play move of every board, driven from here (no host-language code between the launches):
// root expansion + evaluation, Gumbel noise, halving schedule, every phase (selection, forward pass of the
// library's own network handle, backup), final choice / records / finished games, the moves played on the
// device-resident boards.  Buffers are the caller's (device): planes [T * batch_size][6][S][S],
// policy [T * batch_size][A], value [T * batch_size][3].
// chained unless the debug knob TG_SP_CHAIN says 0 (tg::knob: ignored without TG_DEBUG_KNOBS=1)
static bool new_handle_chained() {
    const char *v = tg::knob("TG_SP_CHAIN");
    return !v || atoi(v) != 0;
}

int tg_selfplay_play_move(tg_selfplay *sp, tg_net *net, float *planes_dev, float *policy_dev, float *value_dev,
                          void *stream, int32_t *finished_host, int64_t *stats_host) {
    return tg_selfplay_play_move2(sp, net, net, planes_dev, policy_dev, value_dev, stream, finished_host, stats_host);
}

// The same move with one evaluator per colour: net_to_move searches (round-trip scheme: and evaluates the roots it searches
// from), net_next evaluates the roots the chained scheme leaves for the next call.  net_to_move == net_next is
// tg_selfplay_play_move; two different handles put the call under the one-mover rule (check_one_mover).
int tg_selfplay_play_move2(tg_selfplay *sp, tg_net *net_to_move, tg_net *net_next, float *planes_dev, float *policy_dev,
                           float *value_dev, void *stream, int32_t *finished_host, int64_t *stats_host) {
    if (!sp || !net_to_move || !net_next || !planes_dev || !policy_dev || !value_dev || !finished_host)
        return tg::fail(TG_ERR_ARG, "tg_selfplay_play_move: null argument");
    const MoveBuffers b{planes_dev, policy_dev, value_dev, stream};
    // TG_SP_CHAIN=0: the round-trip scheme (kept for comparison; a handle stays with the scheme of its first move)
    if (!sp->chain_started && !sp->sync_started && !sp->scheme_told) sp->chained = new_handle_chained();
    if (sp->chained) return play_move_chain(sp, net_to_move, net_next, b, finished_host, stats_host);
    sp->sync_started = true;
    return play_move_sync(sp, net_to_move, net_next, b, finished_host, stats_host);
}

// The scheme of a handle's one-call moves, for a caller whose own decisions depend on it (a match: when a freed slot may take
// its next game): *chained_host = 1 chained, 0 round trip.  A handle that has not moved yet is told what its first
// tg_selfplay_play_move(2) would decide and stays with that answer.  sp == NULL: what a new handle would be told (no device).
int tg_selfplay_chained(tg_selfplay *sp, int *chained_host) {
    if (!chained_host) return tg::fail(TG_ERR_ARG, "tg_selfplay_chained: null argument");
    if (sp && !sp->chain_started && !sp->sync_started && !sp->scheme_told) {
        sp->chained = new_handle_chained();
        sp->scheme_told = true;
    }
    *chained_host = (sp ? sp->chained : new_handle_chained()) ? 1 : 0;
    return TG_OK;
}

// The two halves of a chained tg_selfplay_play_move (see PendingMove): `begin` queues the whole move on `stream` and returns with
// the device working; `end` waits for that move's records, does the bookkeeping and reports finished games.  Between the two
// the caller may run other handles' halves; slots are refilled (tg_selfplay_start_game) between an `end` and the next `begin`.
int tg_selfplay_move_begin(tg_selfplay *sp, tg_net *net, float *planes_dev, float *policy_dev, float *value_dev, void *stream) {
    return tg_selfplay_move_begin2(sp, net, net, planes_dev, policy_dev, value_dev, stream);
}

int tg_selfplay_move_begin2(tg_selfplay *sp, tg_net *net, tg_net *net_next, float *planes_dev, float *policy_dev, float *value_dev,
                            void *stream) {
    if (!sp || !net || !net_next || !planes_dev || !policy_dev || !value_dev)
        return tg::fail(TG_ERR_ARG, "tg_selfplay_move_begin: null argument");
    if (sp->sync_started || sp->observer)
        return tg::fail(TG_ERR_STATE, "tg_selfplay_move_begin: this handle runs the round-trip scheme / has an observer (whole moves only)");
    if (sp->pend.active) return tg::fail(TG_ERR_STATE, "tg_selfplay_move_begin: the previous move has not been ended");
    sp->chained = true;
    return chain_begin(sp, net, net_next, MoveBuffers{planes_dev, policy_dev, value_dev, stream});
}

int tg_selfplay_move_end(tg_selfplay *sp, int32_t *finished_host, int64_t *stats_host) {
    if (!sp || !finished_host) return tg::fail(TG_ERR_ARG, "tg_selfplay_move_end: null argument");
    if (!sp->pend.active) return tg::fail(TG_ERR_STATE, "tg_selfplay_move_end: no move has been begun");
    return chain_end(sp, finished_host, stats_host);
}


}  // extern "C"

// ---- policy-only play: the host side of policy_planes_kernel / policy_move_kernel -------------------------------------------
struct tg_policy {
    tg_search *s = nullptr;
    tg::DevBuf<uint32_t> mt;                      // [T][625] generator state per board
    tg::DevBuf<int32_t> moves, slot;              // [T] chosen moves; [T][4] games-mode slot records
    tg::PinBuf<int32_t> moves_back;               // pinned [T]: the moves on their way to moves_host
    tg::PinBuf<int32_t> fin_pub;                  // host-mapped [T]: games each slot has finished
    tg::PinBuf<uint32_t> state_back;              // pinned [625]: one state on its way down
    tg::DevBuf<uint8_t> no_superko;               // [T], allocated by the first tg_policy_set_superko(.., 0)
    // games mode
    tg::DevBuf<uint32_t> game_mt;                 // [games][625]
    tg::DevBuf<int32_t> log, len, reason;         // [games][max_moves], [games], [games]
    tg::DevBuf<uint8_t> final_cells;              // [games][NC]
    int games = 0, max_moves = 0, answer_pass = 0;
    int64_t ply = 0;
    bool games_on = false;
};

namespace {

PolicyDev policy_dev_view(const tg_policy *p, int flags) {
    PolicyDev v{};
    v.mt = p->mt.get();
    v.moves = p->moves.get();
    v.game_mt = p->game_mt.get();
    v.slot = p->slot.get();
    v.fin_pub = p->fin_pub.dev();
    v.log = p->log.get();
    v.len = p->len.get();
    v.reason = p->reason.get();
    v.final_cells = p->final_cells.get();
    v.no_superko = p->no_superko.get();
    v.games = p->games;
    v.max_moves = p->max_moves;
    v.ply = (int32_t)(p->ply & 0x3fffffff);      // (only its parity is used)
    v.flags = flags;
    return v;
}

int launch_policy_planes(tg_policy *p, float *planes_dev, int init, hipStream_t st) {
    tg_search *s = p->s;
    const PolicyDev v = policy_dev_view(p, init ? kPolGames : 0);
    with_board_size(s->S, [&](auto size) {
        hipLaunchKernelGGL(policy_planes_kernel<decltype(size)::value>, dim3(s->dev.T), dim3(64), 0, st, s->dev, v, planes_dev, init);
    });
    TG_HIP(hipGetLastError());
    return TG_OK;
}

int launch_policy_move(tg_policy *p, const float *policy_dev, int flags, float *next_planes, hipStream_t st) {
    tg_search *s = p->s;
    const PolicyDev v = policy_dev_view(p, flags);
    with_board_size(s->S, [&](auto size) {
        hipLaunchKernelGGL(policy_move_kernel<decltype(size)::value>, dim3(s->dev.T), dim3(64), 0, st, s->dev, v, policy_dev, next_planes);
    });
    TG_HIP(hipGetLastError());
    return TG_OK;
}

}  // namespace

extern "C" {

int tg_policy_create(tg_search *s, tg_policy **out) {
    if (!s || !out) return tg::fail(TG_ERR_ARG, "tg_policy_create: null argument");
    TG_HIP(hipSetDevice(s->cfg.device));
    std::unique_ptr<tg_policy> handle(new tg_policy);
    tg_policy *p = handle.get();
    p->s = s;
    const size_t T = (size_t)s->dev.T;
    int rc;
    if ((rc = p->mt.alloc_zeroed(T * tg_rng::kStateWords)) || (rc = p->moves.alloc_zeroed(T)) || (rc = p->slot.alloc_zeroed(T * 4)) ||
        (rc = p->moves_back.alloc(T)) || (rc = p->fin_pub.alloc(T, hipHostMallocMapped)) || (rc = p->state_back.alloc(tg_rng::kStateWords)))
        return rc;
    std::memset(p->fin_pub.get(), 0, T * sizeof(int32_t));
    // an unseeded board twists a zero state: give every board MT19937's position "twist first" at least
    std::vector<uint32_t> zero(T * tg_rng::kStateWords, 0u);
    for (size_t t = 0; t < T; ++t) zero[t * tg_rng::kStateWords + tg_rng::kMtN] = tg_rng::kMtN;
    TG_HIP(hipMemcpy(p->mt.get(), zero.data(), zero.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    *out = handle.release();
    return TG_OK;
}

int tg_policy_destroy(tg_policy *p) {
    if (!p) return TG_OK;
    (void)hipSetDevice(p->s->cfg.device);
    // the engine's launch stream is idle BEFORE any member is released
    if (p->s->stream_known) (void)hipStreamSynchronize(p->s->last_stream);
    delete p;
    return TG_OK;
}

int tg_policy_seed(tg_policy *p, int board, const uint32_t *mt_key, int mt_pos) {
    if (!p || !mt_key) return tg::fail(TG_ERR_ARG, "tg_policy_seed: null argument");
    if (board < 0 || board >= p->s->dev.T) return tg::fail(TG_ERR_ARG, "tg_policy_seed: board %d out of range", board);
    if (mt_pos < 0 || mt_pos > 624) return tg::fail(TG_ERR_ARG, "tg_policy_seed: MT19937 position %d outside [0, 624]", mt_pos);
    TG_HIP(hipSetDevice(p->s->cfg.device));
    int rc;
    if ((rc = sync_launch_stream(p->s))) return rc;          // (a launch in flight may still be drawing from the old state)
    uint32_t *dst = p->mt.get() + (size_t)board * tg_rng::kStateWords;
    const uint32_t pos = (uint32_t)mt_pos;
    TG_HIP(hipMemcpy(dst, mt_key, tg_rng::kMtN * sizeof(uint32_t), hipMemcpyHostToDevice));
    TG_HIP(hipMemcpy(dst + tg_rng::kMtN, &pos, sizeof(uint32_t), hipMemcpyHostToDevice));
    return TG_OK;
}

int tg_policy_state(tg_policy *p, int board, uint32_t *mt_key_out, int *mt_pos_out) {
    if (!p || !mt_key_out || !mt_pos_out) return tg::fail(TG_ERR_ARG, "tg_policy_state: null argument");
    if (board < 0 || board >= p->s->dev.T) return tg::fail(TG_ERR_ARG, "tg_policy_state: board %d out of range", board);
    TG_HIP(hipSetDevice(p->s->cfg.device));
    int rc;
    if ((rc = sync_launch_stream(p->s))) return rc;
    TG_HIP(hipMemcpy(p->state_back.get(), p->mt.get() + (size_t)board * tg_rng::kStateWords, tg_rng::kStateWords * sizeof(uint32_t),
                     hipMemcpyDeviceToHost));
    std::memcpy(mt_key_out, p->state_back.get(), tg_rng::kMtN * sizeof(uint32_t));
    *mt_pos_out = (int)p->state_back.get()[tg_rng::kMtN];
    return TG_OK;
}

int tg_policy_set_superko(tg_policy *p, int board, int check_superko) {
    if (!p) return tg::fail(TG_ERR_ARG, "tg_policy_set_superko: null argument");
    tg_search *s = p->s;
    if (board < 0 || board >= s->dev.T) return tg::fail(TG_ERR_ARG, "tg_policy_set_superko: board %d out of range", board);
    if (check_superko && !s->dev.superko)
        return tg::fail(TG_ERR_STATE, "tg_policy_set_superko: the search handle was created without check_superko (it keeps no history)");
    if (check_superko && !p->no_superko.get()) return TG_OK;
    TG_HIP(hipSetDevice(s->cfg.device));
    int rc;
    if ((rc = sync_launch_stream(s))) return rc;
    if (!p->no_superko.get() && (rc = p->no_superko.alloc_zeroed((size_t)s->dev.T))) return rc;
    const uint8_t off = check_superko ? 0 : 1;
    TG_HIP(hipMemcpy(p->no_superko.get() + board, &off, 1, hipMemcpyHostToDevice));
    return TG_OK;
}

int tg_policy_planes(tg_policy *p, float *planes_dev, void *stream) {
    if (!p || !planes_dev) return tg::fail(TG_ERR_ARG, "tg_policy_planes: null argument");
    hipStream_t st = use_stream(p->s, stream);
    if (int rc = flush_roots(p->s, st)) return rc;
    return launch_policy_planes(p, planes_dev, 0, st);
}

int tg_policy_moves(tg_policy *p, const float *policy_dev, int play, int answer_pass, int32_t *moves_dev, int32_t *moves_host,
                    void *stream) {
    if (!p || !policy_dev) return tg::fail(TG_ERR_ARG, "tg_policy_moves: null argument");
    if (p->games_on) return tg::fail(TG_ERR_STATE, "tg_policy_moves: a run of games is in progress (tg_policy_games_results ends it)");
    tg_search *s = p->s;
    hipStream_t st = use_stream(s, stream);
    int rc;
    if ((rc = flush_roots(s, st))) return rc;
    if ((rc = launch_policy_move(p, policy_dev, (play ? kPolPlay : 0) | (answer_pass ? kPolAnswerPass : 0), nullptr, st))) return rc;
    const size_t bytes = (size_t)s->dev.T * sizeof(int32_t);
    if (moves_dev) TG_HIP(hipMemcpyAsync(moves_dev, p->moves.get(), bytes, hipMemcpyDeviceToDevice, st));
    if (moves_host) {
        TG_HIP(hipMemcpyAsync(p->moves_back.get(), p->moves.get(), bytes, hipMemcpyDeviceToHost, st));
        TG_HIP(hipStreamSynchronize(st));
        std::memcpy(moves_host, p->moves_back.get(), bytes);
    }
    return TG_OK;
}

int tg_policy_seed_states(const uint32_t *seeds, size_t n, uint32_t *states_out) {
    if (!seeds || !states_out) return tg::fail(TG_ERR_ARG, "tg_policy_seed_states: null argument");
    // CPython _randommodule.c random_seed for a non-negative int below 2^32: init_by_array on the one-word key {seed}
    auto expand = [&](int g) {
        uint32_t *mt = states_out + (size_t)g * tg_rng::kStateWords;
        const uint32_t key = seeds[g];
        mt_init_genrand(19650218u, mt);
        int i = 1;
        for (int k = 624; k; --k) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key;      // + key[j] + j with j == 0 throughout
            if (++i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        for (int k = 623; k; --k) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            if (++i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        mt[0] = 0x80000000u;
        mt[624] = 624u;
    };
    parallel_trees((int)n, expand);
    return TG_OK;
}

int tg_policy_games_begin(tg_policy *p, int games, int max_moves, int answer_pass, const uint32_t *mt_states_host) {
    if (!p || !mt_states_host) return tg::fail(TG_ERR_ARG, "tg_policy_games_begin: null argument");
    if (games < 1 || max_moves < 1) return tg::fail(TG_ERR_ARG, "tg_policy_games_begin: games and max_moves must be >= 1");
    tg_search *s = p->s;
    if (max_moves >= s->HMAX)
        return tg::fail(TG_ERR_ARG, "tg_policy_games_begin: max_moves %d beyond the %d moves a board records", max_moves, s->HMAX - 1);
    for (int g = 0; g < games; ++g)
        if (mt_states_host[(size_t)g * tg_rng::kStateWords + tg_rng::kMtN] > (uint32_t)tg_rng::kMtN)
            return tg::fail(TG_ERR_ARG, "tg_policy_games_begin: game %d: MT19937 position outside [0, 624]", g);
    TG_HIP(hipSetDevice(s->cfg.device));
    int rc;
    if ((rc = sync_launch_stream(s))) return rc;             // (the buffers below may be re-allocated)
    const size_t G = (size_t)games;
    if ((rc = p->game_mt.reserve(G * tg_rng::kStateWords)) || (rc = p->log.alloc_zeroed(G * max_moves)) || (rc = p->len.alloc_zeroed(G)) ||
        (rc = p->reason.alloc_zeroed(G)) || (rc = p->final_cells.alloc_zeroed(G * s->NC)))
        return rc;
    TG_HIP(hipMemcpy(p->game_mt.get(), mt_states_host, G * tg_rng::kStateWords * sizeof(uint32_t), hipMemcpyHostToDevice));
    std::memset(p->fin_pub.get(), 0, (size_t)s->dev.T * sizeof(int32_t));
    // positions staged with tg_search_set_root are not part of a run of games: every slot starts from the empty board
    s->roots.drop_all();
    p->games = games;
    p->max_moves = max_moves;
    p->answer_pass = answer_pass != 0;
    p->ply = 0;
    p->games_on = true;
    return TG_OK;
}

int tg_policy_games_ply(tg_policy *p, tg_net *net, float *planes_dev, float *policy_dev, float *value_dev, float *policy_keep_dev,
                        void *stream) {
    if (!p || !net || !planes_dev || !policy_dev || !value_dev) return tg::fail(TG_ERR_ARG, "tg_policy_games_ply: null argument");
    if (!p->games_on) return tg::fail(TG_ERR_STATE, "tg_policy_games_ply: no run of games has been begun");
    tg_search *s = p->s;
    if (tg_net_board_size(net) != s->S) return tg::fail(TG_ERR_ARG, "tg_policy_games_ply: the network is for another board size");
    hipStream_t st = use_stream(s, stream);
    int rc;
    if (p->ply == 0 && (rc = launch_policy_planes(p, planes_dev, 1, st))) return rc;
    if ((rc = tg_net_forward_dev(net, planes_dev, s->dev.T, 0, policy_dev, value_dev, stream))) return rc;
    if (policy_keep_dev)
        TG_HIP(hipMemcpyAsync(policy_keep_dev, policy_dev, (size_t)s->dev.T * s->A * sizeof(float), hipMemcpyDeviceToDevice, st));
    if ((rc = launch_policy_move(p, policy_dev, kPolGames | kPolPlay | (p->answer_pass ? kPolAnswerPass : 0), planes_dev, st))) return rc;
    p->ply += 1;
    return TG_OK;
}

int tg_policy_games_finished(tg_policy *p, int32_t *finished_host) {
    if (!p || !finished_host) return tg::fail(TG_ERR_ARG, "tg_policy_games_finished: null argument");
    const volatile int32_t *fin = p->fin_pub.get();
    int64_t n = 0;
    for (int t = 0; t < p->s->dev.T; ++t) n += fin[t];
    *finished_host = (int32_t)n;
    return TG_OK;
}

int tg_policy_games_results(tg_policy *p, int32_t *moves_host, int32_t *lengths_host, int32_t *reasons_host, int32_t *scores_host,
                            uint8_t *cells_host, int64_t *plies_host) {
    if (!p) return tg::fail(TG_ERR_ARG, "tg_policy_games_results: null argument");
    if (!p->games_on) return tg::fail(TG_ERR_STATE, "tg_policy_games_results: no run of games has been begun");
    tg_search *s = p->s;
    TG_HIP(hipSetDevice(s->cfg.device));
    int rc;
    if ((rc = sync_launch_stream(s))) return rc;
    const size_t G = (size_t)p->games;
    if (moves_host) TG_HIP(hipMemcpy(moves_host, p->log.get(), G * p->max_moves * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (lengths_host) TG_HIP(hipMemcpy(lengths_host, p->len.get(), G * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (reasons_host) TG_HIP(hipMemcpy(reasons_host, p->reason.get(), G * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (scores_host || cells_host) {
        std::vector<uint8_t> cells(G * s->NC);
        TG_HIP(hipMemcpy(cells.data(), p->final_cells.get(), cells.size(), hipMemcpyDeviceToHost));
        if (cells_host) std::memcpy(cells_host, cells.data(), cells.size());
        if (scores_host) {
            std::vector<int32_t> why(G);
            TG_HIP(hipMemcpy(why.data(), p->reason.get(), G * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (size_t g = 0; g < G; ++g) scores_host[g] = why[g] ? count_score_cells(&cells[g * s->NC], s->S) : 0;
        }
    }
    if (plies_host) *plies_host = p->ply;
    p->games_on = false;
    return TG_OK;
}

}  // extern "C"

// ---- training samples from game records: the host side of replay_samples_kernel ----------------------------------------
struct tg_replay {
    int S = 0, device = 0, grid_cap = 0;
    tg::DevBuf<uint64_t> zob;                     // [4][NC] zero keys (put_stone's hash is not read by anything here)
    tg::DevBuf<uint64_t> cand_zob;                // [4][NC] keys of tg_replay_run_cand (superko reads the hashes), made at its first call
    tg::DevBuf<uint8_t> in;                       // one call's inputs, the layout of `stage`
    tg::DevBuf<int32_t> flags;                    // [games]
    tg::PinBuf<uint8_t> stage;                    // pinned: offsets, sample offsets, moves, sample plies, sample symmetries
    tg::PinBuf<int32_t> flags_back;               // pinned [games]: the flags on their way to flags_host
    size_t stage_cap = 0, flags_cap = 0;
};

extern "C" {

int tg_replay_create(int board_size, int device, tg_replay **out) {
    if (!out) return tg::fail(TG_ERR_ARG, "tg_replay_create: null argument");
    *out = nullptr;
    if (board_size != 9 && board_size != 13 && board_size != 19)
        return tg::fail(TG_ERR_ARG, "tg_replay_create: board size %d not built (9, 13 and 19 are)", board_size);
    TG_HIP(hipSetDevice(device));
    std::unique_ptr<tg_replay> handle(new tg_replay);
    tg_replay *r = handle.get();
    r->S = board_size;
    r->device = device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    r->grid_cap = cus * 32;                       // one-wave workgroups: the waves a CU holds (a 19x19 board's 19 KB of LDS admits 8 at a time)
    const size_t NC = (size_t)(board_size + 2) * (board_size + 2);
    if (int rc = r->zob.alloc_zeroed(4 * NC)) return rc;
    *out = handle.release();
    return TG_OK;
}

int tg_replay_destroy(tg_replay *r) {
    if (!r) return TG_OK;
    (void)hipSetDevice(r->device);
    delete r;                                     // (tg_replay_run returns with its stream idle: nothing queued uses a member)
    return TG_OK;
}

// tg_replay_run (cand_dev null: replay_samples_kernel under the zero keys, planes required) and tg_replay_run_cand (replay_cand_kernel
// under the handle's own keys; planes optional)
static int replay_run(const char *who, tg_replay *r, const int32_t *moves_host, const int64_t *offsets_host, int games,
                      const int32_t *sample_ply_host, const int8_t *sample_sym_host, const int64_t *sample_offsets_host,
                      float *planes_dev, int32_t *flags_host, bool with_cand, int superko, uint32_t *cand_dev, void *stream) {
    if (!r || !offsets_host || !sample_offsets_host || !flags_host)
        return tg::fail(TG_ERR_ARG, "%s: null argument", who);
    if (games < 0) return tg::fail(TG_ERR_ARG, "%s: negative number of games", who);
    if (games == 0) return TG_OK;
    if (offsets_host[0] != 0 || sample_offsets_host[0] != 0)
        return tg::fail(TG_ERR_ARG, "%s: offsets and sample offsets start at 0", who);
    for (int g = 0; g < games; ++g) {
        const int64_t n = offsets_host[g + 1] - offsets_host[g];
        if (n < 0 || sample_offsets_host[g + 1] < sample_offsets_host[g])
            return tg::fail(TG_ERR_ARG, "%s: game %d: offsets decrease", who, g);
    }
    const size_t M = (size_t)offsets_host[games], N = (size_t)sample_offsets_host[games];
    if ((M && !moves_host) || (N && (!sample_ply_host || !sample_sym_host || (with_cand ? !cand_dev : !planes_dev))))
        return tg::fail(TG_ERR_ARG, "%s: null argument", who);
    for (int g = 0; g < games; ++g) {
        const int64_t n = offsets_host[g + 1] - offsets_host[g];
        int64_t last = 0;
        for (int64_t i = sample_offsets_host[g]; i < sample_offsets_host[g + 1]; ++i) {
            const int64_t ply = sample_ply_host[i];
            if (ply < last || ply >= n || sample_sym_host[i] < 0 || sample_sym_host[i] > 7)
                return tg::fail(TG_ERR_ARG, "%s: game %d: sample %lld (ply %lld, symmetry %d) is out of order, "
                                "beyond the game's %lld moves or no symmetry", who, g, (long long)i, (long long)ply,
                                (int)sample_sym_host[i], (long long)n);
            last = ply;
        }
    }
    TG_HIP(hipSetDevice(r->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (with_cand && !r->cand_zob.get()) {
        // fixed-seed keys (splitmix64): superko compares hashes of one game with each other, which keys they are made of does not matter
        const size_t n_keys = 4 * (size_t)(r->S + 2) * (r->S + 2);
        std::vector<uint64_t> keys(n_keys);
        uint64_t x = 0x74616d61676f5a4bull;
        for (uint64_t &k : keys) {
            uint64_t z = (x += 0x9e3779b97f4a7c15ull);
            z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
            z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
            k = z ^ (z >> 31);
        }
        if (int rc = r->cand_zob.reserve(n_keys)) return rc;
        TG_HIP(hipMemcpy(r->cand_zob.get(), keys.data(), n_keys * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    // one pinned image, one copy: [offsets | sample offsets | moves | sample plies | sample symmetries]
    const size_t G1 = (size_t)games + 1;
    const size_t o_off = 0, o_soff = o_off + G1 * 8, o_moves = o_soff + G1 * 8, o_ply = o_moves + M * 4, o_sym = o_ply + N * 4;
    const size_t bytes = o_sym + N;
    int rc;
    if (bytes > r->stage_cap) {
        const size_t cap = bytes + bytes / 2;
        if ((rc = r->stage.alloc(cap)) || (rc = r->in.reserve(cap))) { r->stage_cap = 0; return rc; }
        r->stage_cap = cap;
    }
    if ((size_t)games > r->flags_cap) {
        const size_t cap = (size_t)games + (size_t)games / 2;
        if ((rc = r->flags_back.alloc(cap)) || (rc = r->flags.reserve(cap))) { r->flags_cap = 0; return rc; }
        r->flags_cap = cap;
    }
    uint8_t *pin = r->stage.get();
    std::memcpy(pin + o_off, offsets_host, G1 * 8);
    std::memcpy(pin + o_soff, sample_offsets_host, G1 * 8);
    if (M) std::memcpy(pin + o_moves, moves_host, M * 4);
    if (N) std::memcpy(pin + o_ply, sample_ply_host, N * 4);
    if (N) std::memcpy(pin + o_sym, sample_sym_host, N);
    TG_HIP(hipMemcpyAsync(r->in.get(), pin, bytes, hipMemcpyHostToDevice, st));
    ReplayDev R{};
    const uint8_t *base = r->in.get();
    R.offsets = reinterpret_cast<const int64_t *>(base + o_off);
    R.s_off = reinterpret_cast<const int64_t *>(base + o_soff);
    R.moves = reinterpret_cast<const int32_t *>(base + o_moves);
    R.s_ply = reinterpret_cast<const int32_t *>(base + o_ply);
    R.s_sym = reinterpret_cast<const int8_t *>(base + o_sym);
    R.planes = planes_dev;
    R.flags = r->flags.get();
    R.zob = with_cand ? r->cand_zob.get() : r->zob.get();
    R.games = games;
    const int grid = games < r->grid_cap ? games : r->grid_cap;
    with_board_size(r->S, [&](auto size) {
        if (with_cand)
            hipLaunchKernelGGL(replay_cand_kernel<decltype(size)::value>, dim3(grid), dim3(64), 0, st, R, cand_dev, superko ? 1 : 0);
        else
            hipLaunchKernelGGL(replay_samples_kernel<decltype(size)::value>, dim3(grid), dim3(64), 0, st, R);
    });
    TG_HIP(hipGetLastError());
    TG_HIP(hipMemcpyAsync(r->flags_back.get(), r->flags.get(), (size_t)games * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    std::memcpy(flags_host, r->flags_back.get(), (size_t)games * sizeof(int32_t));
    return TG_OK;
}

int tg_replay_run(tg_replay *r, const int32_t *moves_host, const int64_t *offsets_host, int games,
                  const int32_t *sample_ply_host, const int8_t *sample_sym_host, const int64_t *sample_offsets_host,
                  float *planes_dev, int32_t *flags_host, void *stream) {
    return replay_run("tg_replay_run", r, moves_host, offsets_host, games, sample_ply_host, sample_sym_host, sample_offsets_host,
                      planes_dev, flags_host, false, 0, nullptr, stream);
}

int tg_replay_run_cand(tg_replay *r, const int32_t *moves_host, const int64_t *offsets_host, int games,
                       const int32_t *sample_ply_host, const int8_t *sample_sym_host, const int64_t *sample_offsets_host,
                       float *planes_dev, int32_t *flags_host, int superko, uint32_t *cand_dev, void *stream) {
    return replay_run("tg_replay_run_cand", r, moves_host, offsets_host, games, sample_ply_host, sample_sym_host,
                      sample_offsets_host, planes_dev, flags_host, true, superko, cand_dev, stream);
}

}  // extern "C"
