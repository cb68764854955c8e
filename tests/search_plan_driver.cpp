// Stand-alone driver of csrc/search_plan.h for tests/test_search_plan_host.py (host compiler, no HIP): one case per input
// line, the plan's name per output line.
//   family S T launch_trees N most unique prof shared_device num_cus split_per_cu split_prof_build
//   serial mpipe_prof mpipe_max_trees split split_cfg mpipe_cfg gumbel_workers
#include <cstdio>

#include "../tamago_amd/csrc/search_plan.h"

int main() {
    int family, v[18];
    char name[160];
    for (;;) {
        if (scanf("%d", &family) != 1) return 0;
        for (int &x : v)
            if (scanf("%d", &x) != 1) return 2;
        tg_plan::PlanInputs in;
        in.S = v[0], in.T = v[1], in.launch_trees = v[2], in.N = v[3], in.most = v[4], in.unique = v[5] != 0, in.prof = v[6] != 0;
        in.shared_device = v[7] != 0, in.num_cus = v[8], in.split_per_cu = v[9], in.split_prof_build = v[10] != 0;
        tg_plan::SearchKnobs k;
        k.serial = v[11] != 0, k.mpipe_prof = v[12] != 0, k.mpipe_max_trees = v[13], k.split = v[14] != 0;
        k.split_cfg = v[15], k.mpipe_cfg = v[16], k.gumbel_workers = v[17];
        const tg_plan::LaunchPlan plan = family == 0   ? tg_plan::plan_select_puct(in, k)
                                         : family == 1 ? tg_plan::plan_select_gumbel(in, k)
                                                       : tg_plan::plan_backup(in);
        plan.name(name, sizeof(name));
        puts(name);
    }
}
