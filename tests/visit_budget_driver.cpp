// Host driver of csrc/visit_budget.h (tests/test_visit_budget_host.py): reads "total root_visits max_leaves" rows from stdin
// and prints "descents spent" per row - the very functions the PUCT selectors and budget_rule_kernel compile for the device.
#include <cstdio>

#include "../tamago_amd/csrc/visit_budget.h"

int main() {
    int total, visits, max_leaves;
    while (scanf("%d %d %d", &total, &visits, &max_leaves) == 3)
        printf("%d %d\n", (int)tg_budget::descents(total, visits, max_leaves), tg_budget::spent(total, visits) ? 1 : 0);
    return 0;
}
