// Stand-alone driver of csrc/node_pool.h for tests/test_node_pool_host.py (host compiler, no HIP): the enumeration of the
// pool's per-node arrays, one per line - name, element bytes, elements per node at the board sizes' A, remap flag -, then the
// bytes of one node and the size of tg_search_read_node's record at each A.
#include <cstdio>

#include "../tamago_amd/csrc/node_pool.h"

int main() {
    const size_t As[] = {82, 170, 362};
    for (const tg_pool::ArrayInfo &a : tg_pool::kArrays) {
        printf("array %s %zu", a.name, a.elem_bytes);
        for (size_t A : As) printf(" %zu", tg_pool::per_node(a.per_child, A));
        printf(" %d\n", a.remap ? 1 : 0);
    }
    for (size_t A : As)
        printf("node %zu %zu %zu\n", A, tg_pool::bytes_per_node(A), tg_pool::node_record_offset(tg_pool::kNumArrays, A));
    return 0;
}
