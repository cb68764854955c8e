// The early stop of a CONSTANT_PLAYOUT search (mcts/time_manager.py:146-163 is_move_decided, tested in mcts/tree.py:150-152):
// the search ends once the visits still to come cannot lift the runner-up child over the leader.  Pure arithmetic, no HIP:
// search.hip's stop_rule_kernel compiles this text for the device, tests/stop_rule_driver.cpp for the host
// (tests/test_stop_rule_host.py), so the CPU checks the very rule the kernel applies.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TG_STOP_FN __host__ __device__ inline
#else
#define TG_STOP_FN inline
#endif

namespace tg_stop {

// The two largest values of a multiset of visit counts (counts are >= 0; duplicates count: {5, 5, 1} has first = second = 5,
// as sorted(v)[-1], sorted(v)[-2] have).  Top2{0, 0}: the empty set - unused child slots hold 0 and change nothing.
struct Top2 { int32_t first, second; };

// one more value
TG_STOP_FN Top2 push(Top2 a, int32_t v) {
    if (v > a.first) return Top2{v, a.first};
    return Top2{a.first, v > a.second ? v : a.second};
}

// The pair-merge step of the butterfly: the two largest of the union of two multisets, from their two largest each.
TG_STOP_FN Top2 merge(Top2 a, Top2 b) {
    if (a.first >= b.first) return Top2{a.first, b.first > a.second ? b.first : a.second};
    return Top2{b.first, a.first > b.second ? a.first : b.second};
}

// time_manager.py:155-163: remaining = threshold - root visits, cutoff = first - second, decided iff remaining < cutoff.
// int32 throughout, strict <.
TG_STOP_FN bool decided(int32_t total, int32_t node_visits, Top2 top) { return total - node_visits < top.first - top.second; }

// How the kernel lays a row of A child slots over a wavefront: lane l holds slots l, l + 64, ... (ceil(A / 64) passes, the last
// one tail-masked).  What lane `lane` holds of `visits`, for the host driver to replay the kernel's order of operations.
constexpr int kLanes = 64;
constexpr int passes(int A) { return (A + kLanes - 1) / kLanes; }
TG_STOP_FN Top2 lane_top2(const int32_t *visits, int A, int lane) {
    Top2 top{0, 0};
    for (int r = 0; r < passes(A); ++r) {
        const int i = lane + kLanes * r;
        if (i < A) top = push(top, visits[i]);
    }
    return top;
}

}  // namespace tg_stop
