// Per-tree visit budgets of the PUCT selectors: a tree that keeps a subtree across moves owes its search
// `total - kept root visits` descents, a number that differs from tree to tree, so the last mini-batch of a lock-step launch
// is partial by a different amount per tree.  Pure arithmetic, no HIP: search.hip's selectors and budget_rule_kernel compile
// this text for the device, tests/visit_budget_driver.cpp for the host (tests/test_visit_budget_host.py), so the CPU checks
// the very rules the kernels apply.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TG_BUDGET_FN __host__ __device__ inline
#else
#define TG_BUDGET_FN inline
#endif

namespace tg_budget {

// The descents a tree makes in a mini-batch of max_leaves slots: what its budget still owes, at most the slots, never less
// than none (a kept root may already hold more visits than the total).  total >= 1 and root_visits >= 0 (the entry points
// refuse other totals, a node's visits only grow from 0): the difference cannot overflow.  int32 throughout.
TG_BUDGET_FN int32_t descents(int32_t total, int32_t root_visits, int32_t max_leaves) {
    const int32_t owed = total - root_visits;
    return owed < 0 ? 0 : (owed < max_leaves ? owed : (max_leaves < 0 ? 0 : max_leaves));
}

// Nothing is owed any more: the tree's search is over (tg_search_budget_rule halts it).
TG_BUDGET_FN bool spent(int32_t total, int32_t root_visits) { return total - root_visits <= 0; }

}  // namespace tg_budget
