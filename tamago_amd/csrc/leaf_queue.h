// The leaf queue of the device search: what the selection kernels hand to backup_kernel, stated once (DESIGN.md 3 "Leaf
// queue").  No HIP and nothing from search.hip: tests/test_leaf_queue_host.py compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tg_queue {

constexpr int kPathCap = 48;                 // levels of a recorded path (24 until round 5: the last mini-batches of a 1 600-visit 19x19 search walk 25 levels and fell to the one-wave backup, 560 us instead of 30)
constexpr int kPathEdgeBits = 10;            // a path entry is node << kPathEdgeBits | edge
constexpr int kPackedPathNodes = 1 << 21;    // nodes per tree a path entry has room for: bigger pools record no paths
constexpr int kLargestA = 19 * 19 + 1;       // edges of a node on the largest board
constexpr int kPass = 0;                     // the move that is a pass, as the kernels' boards record it

}  // namespace tg_queue

// Every array of the queue, [T][K][per slot]: X(SearchDev member, element type, elements per slot).  Allocation and the
// sub-group view are expansions of this list; one entry is written by search.hip's write_queue_entry.
//   q_node, q_pnode, q_pedge: the leaf to evaluate (< 0: the reference's node[-1]), its parent and the parent's edge
//   q_depth, q_path: optional root->leaf path of a queued leaf, path_entry(node, edge) per level, kPathCap entries per slot;
//     q_depth = number of levels (0: not recorded - the backup then follows the parent pointers)
//   q_src: UNIQUE leaf layout (tg_search_select_gumbel with slots_per_tree -1): the plane, within its tree's range, that
//     holds queued leaf k's position (written by the unique selection kernels, read by the unique backup; unused otherwise)
#define TG_LEAF_QUEUE_ARRAYS(X)            \
    X(q_node, int32_t, 1)                  \
    X(q_pnode, int32_t, 1)                 \
    X(q_pedge, int32_t, 1)                 \
    X(q_depth, int32_t, 1)                 \
    X(q_path, int32_t, tg_queue::kPathCap) \
    X(q_src, int32_t, 1)

namespace tg_queue {

struct ArrayInfo {
    const char *name;
    size_t elem_bytes, per_slot;
};
#define TG_QUEUE_INFO(member, E, per_slot) {#member, sizeof(E), (size_t)(per_slot)},
constexpr ArrayInfo kArrays[] = {TG_LEAF_QUEUE_ARRAYS(TG_QUEUE_INFO)};
#undef TG_QUEUE_INFO

constexpr int32_t path_entry(int node, int edge) { return (node << kPathEdgeBits) | edge; }
constexpr int path_node(int32_t entry) { return entry >> kPathEdgeBits; }
constexpr int path_edge(int32_t entry) { return entry & ((1 << kPathEdgeBits) - 1); }
static_assert(kLargestA - 1 < (1 << kPathEdgeBits), "an edge of the largest board fits kPathEdgeBits");
static_assert((int64_t)(kPackedPathNodes - 1) << kPathEdgeBits <= INT32_MAX - ((1 << kPathEdgeBits) - 1),
              "the entry of the last packable node is a non-negative int32_t");
static_assert(path_node(path_entry(kPackedPathNodes - 1, kLargestA - 1)) == kPackedPathNodes - 1 &&
              path_edge(path_entry(kPackedPathNodes - 1, kLargestA - 1)) == kLargestA - 1, "packing round-trips");

// q_depth of a leaf `depth` levels below the root in a pool of `nodes_per_tree`: depth where its q_path holds the whole
// path, else 0 - to the backup "not recorded": it follows the parent pointers instead of a truncated or unpackable path
constexpr int kNoRecordedPath = 0;
constexpr int recorded_depth(int depth, int nodes_per_tree) {
    return (depth <= kPathCap && nodes_per_tree <= kPackedPathNodes) ? depth : kNoRecordedPath;
}

// tree.py:224-229, where a PUCT descent ends: on an edge without a visit (its count, virtual loss included, is below
// expand_threshold + 1) - and after two consecutive passes never (the threshold is out of reach), so that nothing is
// expanded below a finished game.  moves_after: the board's move count once the edge's move is played; last_move: that move
constexpr bool puct_descent_ends(int edge_count_after_virtual_loss, int moves_after, int last_move, int move_before) {
    const bool two_pass = moves_after > 2 && last_move == kPass && move_before == kPass;
    const int threshold = two_pass ? 10000000 : 1;
    return edge_count_after_virtual_loss < threshold + 1;
}

}  // namespace tg_queue
