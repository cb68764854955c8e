// Stand-alone driver of csrc/stop_rule.h for tests/test_stop_rule_host.py (host compiler, no HIP): stop_rule_kernel's order of
// operations on the CPU - every lane's slots pushed pass by pass (the last pass tail-masked), then the six butterfly steps of
// pair merges, lane l with lane l ^ (1 << step) (the kernel pairs lanes by mirrors in two of the steps: any pairing that joins the
// two halves of a group serves an all-reduce) - and the predicate.  One case per input line, one output line each.
//   A total node_visits v[0] ... v[A-1]
// ->  first second decided agree     (agree: 1 when every lane ends the butterfly with the same pair)
#include <cstdio>
#include <vector>

#include "../tamago_amd/csrc/stop_rule.h"

int main() {
    for (;;) {
        int A, total, node_visits;
        if (scanf("%d", &A) != 1) return 0;
        if (A < 1 || scanf("%d %d", &total, &node_visits) != 2) return 2;
        std::vector<int32_t> v(A);
        for (int i = 0; i < A; ++i)
            if (scanf("%d", &v[i]) != 1) return 2;
        tg_stop::Top2 lane[tg_stop::kLanes], next[tg_stop::kLanes];
        for (int l = 0; l < tg_stop::kLanes; ++l) lane[l] = tg_stop::lane_top2(v.data(), A, l);
        for (int step = 0; step < 6; ++step) {
            for (int l = 0; l < tg_stop::kLanes; ++l) next[l] = tg_stop::merge(lane[l], lane[l ^ (1 << step)]);
            for (int l = 0; l < tg_stop::kLanes; ++l) lane[l] = next[l];
        }
        int agree = 1;
        for (int l = 1; l < tg_stop::kLanes; ++l) agree &= lane[l].first == lane[0].first && lane[l].second == lane[0].second;
        printf("%d %d %d %d\n", lane[0].first, lane[0].second, (int)tg_stop::decided(total, node_visits, lane[0]), agree);
    }
}
