// Whole-tree read-out: the packed record of one tree, the scan that places each node's children in it, and the
// digest of a tree.  Pure arithmetic and layout, no HIP: search.hip's dump_scan_kernel / dump_walk_kernel compile this text
// for the device, tests/tree_dump_driver.cpp for the host (tests/test_tree_dump_host.py), so the CPU checks the very rules the
// kernels apply.  The rule structs are template parameters: the tests put wrong rules in and show that the corpus tells them
// from the right ones.
//
// Record of one tree (8-byte aligned, a multiple of 8 bytes long):
//   head        kHeadWords int32: num_nodes, current_root, the tree's sticky error word, the side to move, the total number of
//               children (64 bits, low word first), 0, 0
//   nodes       num_nodes DumpNode: the tg_pool::NodeRec scalars (the two floats as their bits) and first_child, where the
//               node's entries start in every packed row
//   rows        one per child array of TG_NODE_POOL_CHILD_ARRAYS, `total` entries each: node 0's first `children` entries,
//               then node 1's, ... - first the arrays of up to four bytes per element, each widened to int32, then (8-byte
//               aligned) those of eight, in the list's order (the order of node_pool.h's node record)
// first_child is the exclusive scan of `children` over the nodes, total its end.  Pool contents at or beyond a node's
// `children` are stale by design: they enter neither the record nor the digest.
//
// Digest of one tree: two 64-bit words, the same rule under the two seeds kSeed[0], kSeed[1].  A word is
// finish(seed, wrap-around sum of term(seed, field, node, child, value bits)) over
//   (kFieldNumNodes, 0, 0, num_nodes), (kFieldCurrentRoot, 0, 0, current_root),
//   per node i: (kFieldVisits | kFieldVl | kFieldVsum | kFieldRaw | kFieldChildren, i, 0, the scalar),
//   per child array k, node i, child c < children: (kFieldArrays + k, i, c, the entry).
// Values enter by their bit patterns: an integer of up to 32 bits as its int32 (two's complement, zero-extended), a float32
// as its 32 bits, a float64 as its 64 bits (-0.0 and 0.0 differ).  A sum is order-independent: wavefronts add in any order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "node_pool.h"

#if defined(__HIPCC__)
#define TG_DUMP_FN __host__ __device__ inline
#else
#define TG_DUMP_FN inline
#endif

namespace tg_dump {

// ---- layout ----
enum Head : int { kHeadNumNodes, kHeadCurrentRoot, kHeadErr, kHeadToMove, kHeadTotalLo, kHeadTotalHi, kHeadPad0, kHeadPad1, kHeadWords };
constexpr size_t kHeadBytes = kHeadWords * sizeof(int32_t);

struct DumpNode {
    int32_t visits, vl;
    uint32_t vsum_bits, raw_bits;
    int32_t children, parent, pedge, pad;
    int64_t first_child;
};
static_assert(sizeof(DumpNode) == 40 && kHeadBytes % 8 == 0, "the nodes keep the rows 8-byte aligned");

TG_DUMP_FN size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }
TG_DUMP_FN size_t node_offset(size_t i) { return kHeadBytes + i * sizeof(DumpNode); }
// where row `id` (tg_pool::ArrayId of a child array; tg_pool::kNumArrays: the record's end) starts in the record of a tree of
// n nodes and `total` children
TG_DUMP_FN size_t row_offset(int id, size_t n, size_t total) {
    size_t at = node_offset(n);
    for (int wide = 0; wide < 2; ++wide) {
        if (wide) at = align8(at);
        for (int k = 0; k < tg_pool::kNumArrays; ++k) {
            if (!tg_pool::kArrays[k].per_child || (tg_pool::kArrays[k].elem_bytes == 8) != (wide == 1)) continue;
            if (k == id) return at;
            at += total * (wide ? 8 : 4);
        }
    }
    return align8(at);
}
TG_DUMP_FN size_t record_bytes(size_t n, size_t total) { return row_offset(tg_pool::kNumArrays, n, total); }

// what a node's `children` word counts for: never more than the pool row holds
TG_DUMP_FN int32_t clamp_children(int32_t children, int32_t A) { return children < 0 ? 0 : children > A ? A : children; }
TG_DUMP_FN int32_t clamp_nodes(int32_t num_nodes, int32_t N) { return num_nodes < 0 ? 0 : num_nodes > N ? N : num_nodes; }

// ---- the scan: first_child[i] = children[0] + ... + children[i - 1] ----
// How the kernel lays the nodes out (live_rank.h's form): one workgroup of kChunk threads takes them kChunk at a time, a
// wavefront of kLanes lanes scans its 64 counts, the wave totals are scanned across the workgroup, and `carry` - the children
// of the chunks before - goes from one chunk to the next.
constexpr int kLanes = 64;
constexpr int kChunk = 1024;
constexpr int kWaves = kChunk / kLanes;

struct ScanRule {
    static TG_DUMP_FN int32_t before(int32_t inclusive, int32_t own) { return inclusive - own; }
    static TG_DUMP_FN int64_t first(int64_t carry, int32_t waves_before, int32_t lanes_before) { return carry + waves_before + lanes_before; }
    static TG_DUMP_FN int64_t next_carry(int64_t carry, int32_t chunk_total) { return carry + chunk_total; }
};

// The kernel's order of operations on the host, under rule R: first[n] from children[n], the total returned.
template <class R = ScanRule>
inline int64_t scan_replay(const int32_t *children, int n, int64_t *first) {
    int64_t carry = 0;
    std::vector<int32_t> inclusive(kChunk);
    for (int c0 = 0; c0 < n; c0 += kChunk) {
        int32_t wave_total[kWaves];
        for (int w = 0; w < kWaves; ++w) {
            int32_t run = 0;
            for (int l = 0; l < kLanes; ++l) {
                const int i = c0 + w * kLanes + l;
                run += i < n ? children[i] : 0;
                inclusive[w * kLanes + l] = run;
            }
            wave_total[w] = run;
        }
        int32_t waves_before = 0;
        for (int w = 0; w < kWaves; ++w) {
            for (int l = 0; l < kLanes; ++l) {
                const int i = c0 + w * kLanes + l;
                if (i >= n) break;
                first[i] = R::first(carry, waves_before, R::before(inclusive[w * kLanes + l], children[i]));
            }
            waves_before += wave_total[w];
        }
        carry = R::next_carry(carry, waves_before);
    }
    return carry;
}

// ---- the digest ----
enum Field : int { kFieldNumNodes, kFieldCurrentRoot, kFieldVisits, kFieldVl, kFieldVsum, kFieldRaw, kFieldChildren, kFieldArrays = 16 };
constexpr uint64_t kSeed[2] = {0x243F6A8885A308D3ull, 0x13198A2E03707344ull};

TG_DUMP_FN uint64_t bits_of(int32_t v) { return (uint64_t)(uint32_t)v; }
TG_DUMP_FN uint64_t bits_of(int16_t v) { return (uint64_t)(uint32_t)(int32_t)v; }
TG_DUMP_FN uint64_t bits_of(uint32_t v) { return (uint64_t)v; }
TG_DUMP_FN uint64_t bits_of(float v) { uint32_t b; memcpy(&b, &v, 4); return (uint64_t)b; }
TG_DUMP_FN uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

struct DigestRule {
    static TG_DUMP_FN uint64_t mix(uint64_t x) {                                   // splitmix64's finaliser
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        return x ^ (x >> 31);
    }
    // field below 64, node below 2^31, child below 1024: the three share one word without overlap
    static TG_DUMP_FN uint64_t key(int field, int32_t node, int32_t child) {
        return ((uint64_t)(uint32_t)field << 42) | ((uint64_t)(uint32_t)node << 10) | (uint64_t)(uint32_t)child;
    }
    static TG_DUMP_FN uint64_t term(uint64_t seed, int field, int32_t node, int32_t child, uint64_t bits) {
        return mix(mix(key(field, node, child) ^ seed) + bits);
    }
    static TG_DUMP_FN uint64_t finish(uint64_t seed, uint64_t sum) { return mix(sum + seed); }
    // the entries of a pool row that belong to the node
    static TG_DUMP_FN int32_t used(int32_t children, int32_t A) { (void)A; return children; }
};

// two running sums, one per seed
struct Sums {
    uint64_t s[2] = {0, 0};
    template <class D>
    TG_DUMP_FN void add(int field, int32_t node, int32_t child, uint64_t bits) {
        s[0] += D::term(kSeed[0], field, node, child, bits);
        s[1] += D::term(kSeed[1], field, node, child, bits);
    }
};
template <class D>
TG_DUMP_FN void add_tree_terms(Sums &sums, int32_t num_nodes, int32_t current_root) {
    sums.add<D>(kFieldNumNodes, 0, 0, bits_of(num_nodes));
    sums.add<D>(kFieldCurrentRoot, 0, 0, bits_of(current_root));
}
template <class D>
TG_DUMP_FN void add_node_terms(Sums &sums, int32_t i, const tg_pool::NodeRec &r, int32_t children) {
    sums.add<D>(kFieldVisits, i, 0, bits_of(r.visits));
    sums.add<D>(kFieldVl, i, 0, bits_of(r.vl));
    sums.add<D>(kFieldVsum, i, 0, bits_of(r.vsum));
    sums.add<D>(kFieldRaw, i, 0, bits_of(r.raw));
    sums.add<D>(kFieldChildren, i, 0, bits_of(children));
}

// ---- a tree on the host: what the kernels read of one tree of the pool ([N][A] per child array, [N] node records) ----
struct HostTree {
    int32_t A = 0, num_nodes = 0, current_root = 0, err = 0, to_move = 0;
    std::vector<tg_pool::NodeRec> node;
#define TG_DUMP_MEMBER(member, E, per_child, remap) std::vector<E> member;
    TG_NODE_POOL_CHILD_ARRAYS(TG_DUMP_MEMBER)
#undef TG_DUMP_MEMBER
};

// the digest in the kernel's terms, under digest rule D
template <class D = DigestRule>
inline void digest_replay(const HostTree &t, uint64_t out[2]) {
    using namespace tg_pool;
    Sums sums;
    add_tree_terms<D>(sums, t.num_nodes, t.current_root);
    for (int32_t i = 0; i < t.num_nodes; ++i) {
        const int32_t c = clamp_children(t.node[i].children, t.A);
        add_node_terms<D>(sums, i, t.node[i], c);
        const int32_t used = clamp_children(D::used(c, t.A), t.A);
#define TG_DUMP_TERMS(member, E, per_child, remap) \
        for (int32_t k = 0; k < used; ++k) sums.add<D>(kFieldArrays + k_##member, i, k, bits_of(t.member[(size_t)i * t.A + k]));
        TG_NODE_POOL_CHILD_ARRAYS(TG_DUMP_TERMS)
#undef TG_DUMP_TERMS
    }
    out[0] = D::finish(kSeed[0], sums.s[0]);
    out[1] = D::finish(kSeed[1], sums.s[1]);
}

// the packed record in the kernel's terms, under scan rule R (a wrong rule may place entries out of range: they are dropped)
template <class R = ScanRule>
inline std::vector<unsigned char> pack_replay(const HostTree &t) {
    using namespace tg_pool;
    const int32_t n = t.num_nodes;
    std::vector<int32_t> children(n);
    for (int32_t i = 0; i < n; ++i) children[i] = clamp_children(t.node[i].children, t.A);
    std::vector<int64_t> first(n);
    int64_t total = 0;
    for (int32_t i = 0; i < n; ++i) total += children[i];
    scan_replay<R>(children.data(), n, first.data());
    std::vector<unsigned char> rec(record_bytes(n, total), 0);
    int32_t head[kHeadWords] = {};
    head[kHeadNumNodes] = n, head[kHeadCurrentRoot] = t.current_root, head[kHeadErr] = t.err, head[kHeadToMove] = t.to_move;
    head[kHeadTotalLo] = (int32_t)(uint32_t)total, head[kHeadTotalHi] = (int32_t)(uint32_t)((uint64_t)total >> 32);
    std::memcpy(rec.data(), head, kHeadBytes);
    for (int32_t i = 0; i < n; ++i) {
        const NodeRec &r = t.node[i];
        DumpNode d{r.visits, r.vl, (uint32_t)bits_of(r.vsum), (uint32_t)bits_of(r.raw), children[i], r.parent, r.pedge, 0, first[i]};
        std::memcpy(rec.data() + node_offset(i), &d, sizeof(d));
#define TG_DUMP_PUT(member, E, per_child, remap)                                                        \
        for (int32_t k = 0; k < children[i]; ++k) {                                                     \
            using W = std::conditional_t<sizeof(E) == 8, E, int32_t>;                                   \
            const int64_t at = first[i] + k;                                                            \
            if (at < 0 || at >= total) continue;                                                        \
            const W v = (W)t.member[(size_t)i * t.A + k];                                               \
            std::memcpy(rec.data() + row_offset(k_##member, n, total) + (size_t)at * sizeof(W), &v, sizeof(W)); \
        }
        TG_NODE_POOL_CHILD_ARRAYS(TG_DUMP_PUT)
#undef TG_DUMP_PUT
    }
    return rec;
}

}  // namespace tg_dump
