// Stand-alone driver of csrc/leaf_queue.h for tests/test_leaf_queue_host.py (host compiler, no HIP): the enumeration of the
// queue's arrays, one per line - name, element bytes, elements per slot -, then one line per query read from stdin:
//   pack n e        -> entry, path_node(entry), path_edge(entry)
//   depth d N       -> recorded_depth(d, N)
//   ends c m l b    -> puct_descent_ends(c, m, l, b)
#include <cstdio>
#include <cstring>

#include "../tamago_amd/csrc/leaf_queue.h"

int main() {
    for (const tg_queue::ArrayInfo &a : tg_queue::kArrays) printf("array %s %zu %zu\n", a.name, a.elem_bytes, a.per_slot);
    char what[16];
    int a, b, c, d;
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "pack") && scanf("%d %d", &a, &b) == 2) {
            const int32_t entry = tg_queue::path_entry(a, b);
            printf("pack %d %d %d\n", (int)entry, tg_queue::path_node(entry), tg_queue::path_edge(entry));
        } else if (!strcmp(what, "depth") && scanf("%d %d", &a, &b) == 2) {
            printf("depth %d\n", tg_queue::recorded_depth(a, b));
        } else if (!strcmp(what, "ends") && scanf("%d %d %d %d", &a, &b, &c, &d) == 4) {
            printf("ends %d\n", tg_queue::puct_descent_ends(a, b, c, d) ? 1 : 0);
        } else {
            return 1;
        }
    }
    return 0;
}
