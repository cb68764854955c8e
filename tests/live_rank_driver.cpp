// Stand-alone driver of csrc/live_rank.h for tests/test_live_rank_host.py (host compiler, no HIP): live_rank_kernel's order of
// operations on the CPU - the selectors' predicate per tree, the trees a chunk at a time, every wavefront's inclusive scan, the
// wave totals across the chunk, the carry into the next chunk - under the header's rule (0) or one of two wrong ones: an
// inclusive scan (1), a carry dropped between chunks (2).  One case per input line, one output line each.
//   rule T  err[0] halt[0] num_nodes[0] ... err[T-1] halt[T-1] num_nodes[T-1]
// ->  count rank[0] ... rank[T-1]
#include <cstdio>
#include <vector>

#include "../tamago_amd/csrc/live_rank.h"

struct InclusiveRule : tg_live::Rule {
    static int32_t before(int32_t inclusive, int32_t) { return inclusive; }
};
struct DroppedCarryRule : tg_live::Rule {
    static int32_t next_carry(int32_t, int32_t chunk_total) { return chunk_total; }
};

int main() {
    for (;;) {
        int rule, T;
        if (scanf("%d", &rule) != 1) return 0;
        if (scanf("%d", &T) != 1 || T < 1 || rule < 0 || rule > 2) return 2;
        std::vector<uint8_t> flag(T);
        for (int t = 0; t < T; ++t) {
            int err, halt, nodes;
            if (scanf("%d %d %d", &err, &halt, &nodes) != 3) return 2;
            flag[t] = tg_live::live(err, halt, nodes) ? 1 : 0;
        }
        std::vector<int32_t> rank(T);
        const int32_t count = rule == 0   ? tg_live::replay<tg_live::Rule>(flag.data(), T, rank.data())
                              : rule == 1 ? tg_live::replay<InclusiveRule>(flag.data(), T, rank.data())
                                          : tg_live::replay<DroppedCarryRule>(flag.data(), T, rank.data());
        printf("%d", count);
        for (int t = 0; t < T; ++t) printf(" %d", rank[t]);
        printf("\n");
    }
}
