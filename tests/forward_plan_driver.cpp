// Stand-alone driver of csrc/forward_plan.h for tests/test_forward_plan_host.py (host compiler, no HIP): one case per input
// line, one output line each.  Knobs come as the strings the environment would hold ("-": unset) and go through the header's parsers.
//   S batch num_cus spread_w1d spread_split shared_device band_timeouts guard_cap forward_cap
//   TG_FWD_ALGO TG_FWD_BANDS TG_FWD_GROUP TG_FWD_WINO TG_FWD_NO_TAIL TG_FWD_SPREAD_GUARD TG_FWD_CUS TG_SPLIT_SPAN
// ->  name | flops | peak | dtype | family group bands tail guarded grid guard_grid span demoted      (doubles as %a: exact)
#include <cstdio>

#include "../tamago_amd/csrc/forward_plan.h"

int main() {
    for (;;) {
        tg_fwd::PlanInputs in;
        int shared;
        char s[8][64];
        if (scanf("%d", &in.S) != 1) return 0;
        if (scanf("%d %d %lf %lf %d %u %d %d", &in.batch, &in.num_cus, &in.spread_w1d, &in.spread_split, &shared, &in.band_timeouts,
                  &in.caps.guard, &in.caps.forward) != 8)
            return 2;
        in.shared_device = shared != 0;
        for (auto &word : s)
            if (scanf("%63s", word) != 1) return 2;
        const auto env = [&](int i) -> const char * { return s[i][0] == '-' && !s[i][1] ? nullptr : s[i]; };
        tg_fwd::ForwardKnobs k;
        k.algo = tg_fwd::parse_algo(env(0));
        k.bands = tg_fwd::parse_bands(env(1));
        k.group = tg_fwd::parse_int(env(2), 0);
        k.wino = tg_fwd::parse_int(env(3), 0);
        k.no_tail = env(4) != nullptr;
        k.spread_guard_off = tg_fwd::parse_int(env(5), 1) == 0;
        k.fwd_cus = tg_fwd::parse_int(env(6), 0);
        k.split_span = tg_fwd::parse_int(env(7), 0);
        const tg_fwd::ForwardPlan p = tg_fwd::plan_forward(in, k);
        const tg_fwd::Executed e = tg_fwd::executed(in, k);
        printf("%s|%a|%a|%s|%d %d %d %d %d %d %d %d %d\n", tg_fwd::kernel_name(p), e.flops, e.peak, e.dtype, (int)p.family, p.group,
               p.bands, p.tail, (int)p.guarded, p.grid, p.guard_grid, p.span, (int)p.demoted);
    }
}
