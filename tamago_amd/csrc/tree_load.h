// Whole-tree write-in: which packed records (tree_dump.h) may enter a pool, and how a record becomes pool rows.
// Pure arithmetic and layout, no HIP: search.hip's load_walk_kernel compiles the fill rule for the device and
// tg_search_check_records / tg_search_load_trees the check for the host; tests/tree_load_driver.cpp compiles both for the host
// (tests/test_tree_load_host.py), so the CPU checks the very rules the library applies.  The fill rule is a template
// parameter: the tests put wrong rules in and show that the corpus tells them from the right one.
//
// An admissible record (check_record; the first violated rule is reported, in this order):
//   head       len >= the head; the two pad words 0; 0 <= num_nodes <= N; current_root 0; the error word 0; to_move 1 or 2
//              (an empty record may carry any); the nodes lie within len
//   per node   1 <= children <= A (an expanded node holds at least the pass); first_child is the exclusive scan of children;
//              pad 0; visits >= 0; vl >= 0
//   sizes      total == the sum of the nodes' children; len == record_bytes(num_nodes, total) exactly
//   ch_index   every entry is -1 or lies in (i, num_nodes): children are created after their parents and a reroot keeps
//              creation order, so every walk is acyclic and bounded; every node i >= 1 is named by exactly one edge (p, e) and
//              its parent / pedge are that p / e; node 0 carries what expand_node writes for a root: parent -1, pedge -1
//   action     kPass, or the padded coordinate of an on-board point of this board size (it is stored as int16)
//   counts     ch_visits >= 0, ch_vl >= 0; float fields may hold any bits
// What is NOT checked, here or on the device: that the tree belongs to the root position it is loaded under (its actions legal
// there, its priors and values those of that position).  mcts/tree.py's verify replays the paths on a host board.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "root_position.h"
#include "tree_dump.h"

namespace tg_load {

using tg_dump::DumpNode;
using tg_dump::HostTree;

// ---- the fill rule: what entry k of a node's pool row becomes ----
// The kernel takes a row in passes of kLanes entries, a lane per entry, ceil(A / kLanes) passes: entry k comes from the record
// where the rule says so, else it gets the canonical tail - what expand_node leaves in a fresh row (ch_index kNotExpanded,
// everything else 0) - where the rule says the tail is written.
struct FillRule {
    static TG_DUMP_FN bool from_record(int32_t k, int32_t children) { return k < children; }
    static TG_DUMP_FN bool writes_tail() { return true; }
};
template <class E>
TG_DUMP_FN E tail_value(int array_id) { return array_id == tg_pool::k_ch_index ? (E)tg_pool::kNotExpanded : (E)0; }

// ---- the check ----
enum Rule : int {
    kOk, kLength, kHeadPad, kNumNodes, kCurrentRoot, kErrWord, kToMove, kChildren, kFirstChild, kNodePad, kNodeCount, kTotal,
    kChildIndex, kEdges, kParent, kRoot, kAction, kChildCount, kRules
};
constexpr const char *kRuleText[kRules] = {
    "ok",
    "the length is not the record's (head, nodes and rows of num_nodes nodes and `total` children)",
    "a pad word of the head is not 0",
    "num_nodes is negative or exceeds the pool's tree_size",
    "current_root is not 0",
    "the error word is set",
    "to_move is neither 1 nor 2",
    "children is outside [1, actions]",
    "first_child is not the exclusive scan of children",
    "a node's pad word is not 0",
    "a node's visits or virtual loss is negative",
    "total is not the sum of the nodes' children",
    "a child index is neither -1 nor in (node, num_nodes)",
    "a node is not named by exactly one edge",
    "a node's parent / pedge are not the edge that names it",
    "node 0 is not a root (parent -1, pedge -1)",
    "an action is neither the pass nor an on-board point",
    "a child's visits or virtual loss is negative",
};
struct Verdict {
    int rule = kOk;
    int32_t node = -1, child = -1;
    bool ok() const { return rule == kOk; }
};
inline std::string verdict_text(const Verdict &v) {
    std::string s = kRuleText[v.rule >= 0 && v.rule < kRules ? v.rule : 0];
    if (v.node >= 0) s += " (node " + std::to_string(v.node) + (v.child >= 0 ? ", child " + std::to_string(v.child) : std::string()) + ")";
    return s;
}

// (records come out of byte buffers: no alignment is assumed on the host)
template <class E>
inline E read_at(const unsigned char *rec, size_t offset) { E v; std::memcpy(&v, rec + offset, sizeof(E)); return v; }
inline int64_t head_total(const int32_t *head) {
    return (int64_t)((uint64_t)(uint32_t)head[tg_dump::kHeadTotalLo] | ((uint64_t)(uint32_t)head[tg_dump::kHeadTotalHi] << 32));
}

// an action of a board of width W (S + 2): the pass, or a point inside the border
inline bool action_on_board(int32_t a, int W) {
    if (a == tg_root::kPass) return true;
    if (a < 0 || a >= W * W) return false;
    return tg_root::empty_board_cell(a, W) == tg_root::kEmpty;
}

// A: actions per node (S * S + 1), W: board width with the border (S + 2), N: nodes a tree of the pool holds
inline Verdict check_record(const unsigned char *rec, size_t len, int32_t A, int W, int32_t N) {
    using namespace tg_dump;
    if (len < kHeadBytes) return {kLength, -1, -1};
    int32_t head[kHeadWords];
    std::memcpy(head, rec, kHeadBytes);
    if (head[kHeadPad0] != 0 || head[kHeadPad1] != 0) return {kHeadPad, -1, -1};
    const int32_t n = head[kHeadNumNodes];
    if (n < 0 || n > N) return {kNumNodes, -1, -1};
    if (head[kHeadCurrentRoot] != 0) return {kCurrentRoot, -1, -1};
    if (head[kHeadErr] != 0) return {kErrWord, -1, -1};
    if (n > 0 && head[kHeadToMove] != tg_root::kBlack && head[kHeadToMove] != tg_root::kWhite) return {kToMove, -1, -1};
    if (len < node_offset((size_t)n)) return {kLength, -1, -1};
    const int64_t total = head_total(head);
    int64_t sum = 0;
    for (int32_t i = 0; i < n; ++i) {
        const DumpNode d = read_at<DumpNode>(rec, node_offset((size_t)i));
        if (d.children < 1 || d.children > A) return {kChildren, i, -1};
        if (d.first_child != sum) return {kFirstChild, i, -1};
        if (d.pad != 0) return {kNodePad, i, -1};
        if (d.visits < 0 || d.vl < 0) return {kNodeCount, i, -1};
        sum += d.children;
    }
    if (total != sum) return {kTotal, -1, -1};
    if (len != record_bytes((size_t)n, (size_t)total)) return {kLength, -1, -1};
    const size_t at_index = row_offset(tg_pool::k_ch_index, n, total), at_visits = row_offset(tg_pool::k_ch_visits, n, total),
                 at_vl = row_offset(tg_pool::k_ch_vl, n, total), at_action = row_offset(tg_pool::k_action, n, total);
    // edges: who names each node (-1: nobody yet)
    std::vector<int32_t> by_node((size_t)n, -1), by_edge((size_t)n, -1);
    for (int32_t i = 0; i < n; ++i) {
        const DumpNode d = read_at<DumpNode>(rec, node_offset((size_t)i));
        for (int32_t k = 0; k < d.children; ++k) {
            const size_t e = (size_t)(d.first_child + k) * sizeof(int32_t);
            const int32_t c = read_at<int32_t>(rec, at_index + e);
            if (c != tg_pool::kNotExpanded) {
                if (c <= i || c >= n) return {kChildIndex, i, k};
                if (by_node[c] >= 0) return {kEdges, c, -1};
                by_node[c] = i, by_edge[c] = k;
            }
            if (!action_on_board(read_at<int32_t>(rec, at_action + e), W)) return {kAction, i, k};
            if (read_at<int32_t>(rec, at_visits + e) < 0 || read_at<int32_t>(rec, at_vl + e) < 0) return {kChildCount, i, k};
        }
    }
    for (int32_t i = 0; i < n; ++i) {
        const DumpNode d = read_at<DumpNode>(rec, node_offset((size_t)i));
        if (i == 0) {
            if (d.parent != -1 || d.pedge != -1) return {kRoot, 0, -1};
            continue;
        }
        if (by_node[i] < 0) return {kEdges, i, -1};
        if (d.parent != by_node[i] || d.pedge != by_edge[i]) return {kParent, i, -1};
    }
    return {};
}

// ---- the kernel's order of operations on the host, under fill rule F ----
// `pool` is the tree as it was (its rows of A entries per node, at least the record's num_nodes of them: stale contents
// included); the record's nodes are written over it as load_walk_kernel writes them, and the tree-level words set.
template <class F = FillRule>
inline void unpack_replay(const unsigned char *rec, HostTree &pool) {
    using namespace tg_dump;
    using namespace tg_pool;
    int32_t head[kHeadWords];
    std::memcpy(head, rec, kHeadBytes);
    const int32_t A = pool.A, n = clamp_nodes(head[tg_dump::kHeadNumNodes], (int32_t)pool.node.size());
    const int64_t total = head_total(head);
    for (int32_t i = 0; i < n; ++i) {
        const DumpNode d = read_at<DumpNode>(rec, node_offset((size_t)i));
        const int32_t c = clamp_children(d.children, A);
        NodeRec r{};
        r.visits = d.visits, r.vl = d.vl, r.children = c, r.parent = d.parent, r.pedge = d.pedge, r.pad = 0;
        std::memcpy(&r.vsum, &d.vsum_bits, 4);
        std::memcpy(&r.raw, &d.raw_bits, 4);
        pool.node[i] = r;
        for (int32_t k0 = 0; k0 < A; k0 += kLanes)
            for (int32_t k = k0; k < k0 + kLanes && k < A; ++k) {
                const int64_t at = d.first_child + k;
#define TG_LOAD_PUT(member, E, per_child, remap)                                                                        \
                {                                                                                                       \
                    using Wd = std::conditional_t<sizeof(E) == 8, E, int32_t>;                                         \
                    E &dst = pool.member[(size_t)i * A + k];                                                            \
                    if (F::from_record(k, c)) {                                                                         \
                        if (at >= 0 && at < total) /* (a wrong rule may reach beyond the record's rows: dropped) */    \
                            dst = (E)read_at<Wd>(rec, row_offset(k_##member, n, total) + (size_t)at * sizeof(Wd));      \
                    } else if (F::writes_tail()) {                                                                      \
                        dst = tail_value<E>(k_##member);                                                                \
                    }                                                                                                   \
                }
                TG_NODE_POOL_CHILD_ARRAYS(TG_LOAD_PUT)
#undef TG_LOAD_PUT
            }
    }
    pool.num_nodes = n, pool.current_root = 0, pool.err = 0, pool.to_move = head[tg_dump::kHeadToMove];
}

}  // namespace tg_load
