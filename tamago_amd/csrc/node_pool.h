// The node pool of the device search: WHICH arrays a node consists of, stated once (DESIGN.md 3 "Node pool").  No HIP and
// nothing from search.hip: tests/test_node_pool_host.py compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tg_pool {

constexpr int kNotExpanded = -1;

struct NodeRec {
    int32_t visits, vl;         // node_visits, virtual_loss
    float vsum, raw;            // node_value_sum (float32 like the reference's np.float32 accumulator), raw_value
    int32_t children, parent, pedge, pad;
};
static_assert(sizeof(NodeRec) == 32, "two node records per 64-byte line");

}  // namespace tg_pool

// Every per-node array of the pool, [T][N][per node]: X(SearchDev member, element type (names of tg_pool), one element per
// CHILD (A per node) or one per node, holds node indices: remapped when a tree is compacted).  Allocation, growth, the
// sub-group view, the compaction's moves and tg_search_read_node's record are expansions of this list: a new array is added
// HERE (plus what it means: its initial value in expand_node / expand_fill, its loads at the selection sites that read it).
#define TG_NODE_POOL_CHILD_ARRAYS(X)      \
    X(ch_index, int32_t, true, true)      \
    X(ch_visits, int32_t, true, false)    \
    X(ch_vl, int32_t, true, false)        \
    X(ch_vsum, double, true, false)       \
    X(ch_policy, double, true, false)     \
    X(ch_value, double, true, false)      \
    X(action, int16_t, true, false)
#define TG_NODE_POOL_ARRAYS(X) TG_NODE_POOL_CHILD_ARRAYS(X) X(node, NodeRec, false, false)

namespace tg_pool {

struct ArrayInfo {
    const char *name;
    size_t elem_bytes;
    bool per_child, remap;
};
#define TG_POOL_INFO(member, E, per_child, remap) {#member, sizeof(E), per_child, remap},
constexpr ArrayInfo kArrays[] = {TG_NODE_POOL_ARRAYS(TG_POOL_INFO)};
#undef TG_POOL_INFO
constexpr int kNumArrays = (int)(sizeof(kArrays) / sizeof(kArrays[0]));
#define TG_POOL_ID(member, E, per_child, remap) k_##member,
enum ArrayId : int { TG_NODE_POOL_ARRAYS(TG_POOL_ID) };
#undef TG_POOL_ID

constexpr size_t per_node(bool per_child, size_t A) { return per_child ? A : 1; }
constexpr size_t bytes_per_node(size_t A) {      // 38 A + 32 today
    size_t b = 0;
    for (const ArrayInfo &a : kArrays) b += a.elem_bytes * per_node(a.per_child, A);
    return b;
}

// tg_search_read_node's record of one node: a 32-byte head, then the child arrays in the list's order - first those of up
// to four bytes per element, each widened to int32, then (8-byte aligned) those of eight.  -> where array `id` starts
// (kNumArrays: the record's size).  The head's int32 words: the node's scalars (the two floats as their bits), the tree's
// sticky error flags and its num_nodes as of the read
enum NodeHead : int { kHeadChildren, kHeadVisits, kHeadVl, kHeadVsumBits, kHeadRawBits, kHeadErr, kHeadNumNodes, kHeadPad, kNodeHeadWords };
constexpr size_t kNodeRecordHead = kNodeHeadWords * sizeof(int32_t);
static_assert(kNodeRecordHead == 32, "the head keeps the rows 8-byte aligned");
constexpr size_t node_record_offset(int id, size_t A) {
    size_t at = kNodeRecordHead;
    for (int wide = 0; wide < 2; ++wide) {
        if (wide) at = (at + 7) & ~(size_t)7;
        for (int k = 0; k < kNumArrays; ++k) {
            if (!kArrays[k].per_child || (kArrays[k].elem_bytes == 8) != (wide == 1)) continue;
            if (k == id) return at;
            at += A * (wide ? 8 : 4);
        }
    }
    return at;
}

}  // namespace tg_pool
