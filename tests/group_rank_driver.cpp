// Stand-alone driver of csrc/group_rank.h for tests/test_group_rank_host.py (host compiler, no HIP): group_rank_kernel's order
// of operations on the CPU - the selectors' predicate per tree, a counting pass over the chunks, the offsets, an assigning
// pass with the per-group carry from chunk to chunk - under the header's rule (0) or one of five wrong ones: inclusive
// offsets (1), a position within the group that counts the tree itself (2), the chunk carry dropped (3), the chunk carry
// taken as the chunk's total over all groups (4), the groups laid out in descending order (5).  One case per input line, one
// output line each.
//   rule T G  err[0] halt[0] num_nodes[0] group[0] ... err[T-1] halt[T-1] num_nodes[T-1] group[T-1]
// ->  count[0..G) offset[0..G) rank[0..T)
#include <cstdio>
#include <vector>

#include "../tamago_amd/csrc/group_rank.h"

struct InclusiveOffsetRule : tg_group::Rule {
    static int32_t offset(int32_t inclusive, int32_t) { return inclusive; }
};
struct CountsItselfRule : tg_group::Rule {
    static int32_t within(int32_t lanes_upto) { return lanes_upto; }
};
struct DroppedCarryRule : tg_group::Rule {
    static int32_t next_carry(int32_t, const int32_t *chunk_total, int g, int) { return chunk_total[g]; }
};
struct AllGroupsCarryRule : tg_group::Rule {
    static int32_t next_carry(int32_t carry, const int32_t *chunk_total, int, int) {
        int32_t all = 0;
        for (int g = 0; g < tg_group::kMaxGroups; ++g) all += chunk_total[g];
        return carry + all;
    }
};
struct DescendingRule : tg_group::Rule {
    static int place(int g, int n_groups) { return n_groups - 1 - g; }
};

int main() {
    for (;;) {
        int rule, T, G;
        if (scanf("%d", &rule) != 1) return 0;
        if (scanf("%d %d", &T, &G) != 2 || T < 1 || G < 1 || G > tg_group::kMaxGroups || rule < 0 || rule > 5) return 2;
        std::vector<uint8_t> flag(T);
        std::vector<int32_t> group(T);
        for (int t = 0; t < T; ++t) {
            int err, halt, nodes, g;
            if (scanf("%d %d %d %d", &err, &halt, &nodes, &g) != 4) return 2;
            flag[t] = tg_live::live(err, halt, nodes) ? 1 : 0;
            group[t] = g;
        }
        std::vector<int32_t> rank(T), count(G), offset(G);
        auto run = [&](auto r) {
            tg_group::replay<decltype(r)>(flag.data(), group.data(), T, G, rank.data(), count.data(), offset.data());
        };
        switch (rule) {
        case 0: run(tg_group::Rule{}); break;
        case 1: run(InclusiveOffsetRule{}); break;
        case 2: run(CountsItselfRule{}); break;
        case 3: run(DroppedCarryRule{}); break;
        case 4: run(AllGroupsCarryRule{}); break;
        default: run(DescendingRule{}); break;
        }
        for (int g = 0; g < G; ++g) printf("%d ", count[g]);
        for (int g = 0; g < G; ++g) printf("%d ", offset[g]);
        for (int t = 0; t < T; ++t) printf("%d%c", rank[t], t + 1 < T ? ' ' : '\n');
    }
}
