// Which tree kernel a search launch gets: pure functions of the launch's shape and the knobs' values (DESIGN.md 4.4 "Search
// launch plans" states the rules and what was measured for them).  No HIP, nothing from search.hip: the launcher there looks up
// the instantiation a plan names, tg_search_launch_name renders the same plan, tests/test_search_plan_host.py compiles this alone.
#pragma once
#include <cstddef>
#include <cstdio>

#include "leaf_queue.h"

namespace tg_plan {

constexpr int kPipeMaxLeaves = 1024;        // descents per launch the pipelined PUCT kernels have tables for
constexpr int kGumbelPipeMaxN = 512;        // ... and a tree's descents per phase of the pipelined Gumbel kernel
using tg_queue::kPackedPathNodes;           // pools beyond it: the kernels that work from recorded paths are not chosen
constexpr int kSplitMaxTrees = 16;

// Every selection knob, as values (read in one place: search.hip launch_context)
struct SearchKnobs {
    bool serial = false;             // TG_SELECT_SERIAL
    bool mpipe_prof = false;         // TG_MPIPE_PROF: the multi-selector kernel keeps the phase counters
    int mpipe_max_trees = 256;       // TG_SELECT_MPIPE_TREES
    bool split = true;               // TG_SELECT_SPLIT unset or non-zero
    int split_cfg = 0, mpipe_cfg = 0;   // TG_SPLIT_CFG, TG_MPIPE_CFG
    int gumbel_workers = 0;          // TG_GUMBEL_WORKERS (0: unset)
    bool split_test_mute = false, gumbel_one_by_one = false;   // TG_SPLIT_TEST_MUTE, TG_GUMBEL_ONE_BY_ONE: kernel arguments, no part of the choice
};

struct PlanInputs {
    int S = 9;                       // board size
    int T = 1;                       // the ENGINE's trees: how crowded the CUs are
    int launch_trees = 1;            // trees of this launch (a sub-group's slice: the grid of the Gumbel and backup kernels)
    int N = 2;                       // nodes per tree
    int most = 0;                    // PUCT: max_leaves; Gumbel: max_n, the most descents a tree of the launch makes
    bool unique = false;             // the UNIQUE leaf layout
    bool prof = false;               // tg_search_profile is on
    bool shared_device = false;      // TG_SHARED_DEVICE
    int num_cus = 256;
    int split_per_cu = -1;           // resident select_puct_split_kernel workgroups per CU: asked for only where split_wanted()
    bool split_prof_build = false;   // built with -DTG_SPLIT_PROF
};

enum class Kernel { Puct, PuctPipe, PuctMPipe, PuctSplit, Gumbel, GumbelPipe, Backup };

// One launch: kernel<S, p..., unique> on grid x block.  p: <NNODE, NWRK, NSHIP, NWG> (PuctSplit), <NSEL, NWRK> (PuctMPipe),
// <NW> (GumbelPipe), <NWAVE> (Backup); `unique` is a template argument of the Gumbel and backup kernels only
struct LaunchPlan {
    Kernel kernel;
    int S, p[4];
    bool unique;
    int grid, block;
    int name(char *out, size_t cap) const {
        char k[96] = "";
        const char *u = unique ? "true" : "false";
        switch (kernel) {
        case Kernel::Puct: snprintf(k, sizeof(k), "select_puct_kernel<%d>", S); break;
        case Kernel::PuctPipe: snprintf(k, sizeof(k), "select_puct_pipe_kernel<%d>", S); break;
        case Kernel::PuctMPipe: snprintf(k, sizeof(k), "select_puct_mpipe_kernel<%d, %d, %d>", S, p[0], p[1]); break;
        case Kernel::PuctSplit: snprintf(k, sizeof(k), "select_puct_split_kernel<%d, %d, %d, %d, %d>", S, p[0], p[1], p[2], p[3]); break;
        case Kernel::Gumbel: snprintf(k, sizeof(k), "select_gumbel_kernel<%d, %s>", S, u); break;
        case Kernel::GumbelPipe: snprintf(k, sizeof(k), "select_gumbel_pipe_kernel<%d, %d, %s>", S, p[0], u); break;
        case Kernel::Backup: snprintf(k, sizeof(k), "backup_kernel<%d, %d, %s>", S, p[0], u); break;
        }
        return snprintf(out, cap, "%s grid=%d block=%d", k, grid, block);
    }
};
using SelectPuctPlan = LaunchPlan;
using SelectGumbelPlan = LaunchPlan;
using BackupPlan = LaunchPlan;

inline bool puct_pipelined(const PlanInputs &in, const SearchKnobs &k) {
    return !k.serial && (!in.prof || k.mpipe_prof) && in.most <= kPipeMaxLeaves;
}
// Every condition of the split kernel but the room for its workgroups: where this holds the caller fills in.split_per_cu
inline bool split_wanted(const PlanInputs &in, const SearchKnobs &k) {
    return puct_pipelined(in, k) && !in.shared_device && k.split && (!in.prof || in.split_prof_build) && in.S != 13 &&
           in.T <= kSplitMaxTrees && in.N <= kPackedPathNodes;
}

// The instantiations a tuning knob chooses among: the first row of the board size whose cfg matches; cfg 0 closes a size's
// rows (anything else)
struct CfgRow { int S, cfg, p[4]; };
constexpr CfgRow kSplitRows[] = {       // TG_SPLIT_CFG -> <NNODE, NWRK, NSHIP, NWG>
    {9, 616, {6, 16, 3, 1}},    {9, 816, {8, 16, 3, 1}},   {9, 1016, {10, 16, 2, 1}},  {9, 912, {9, 12, 3, 1}},
    {9, 11016, {10, 16, 3, 1}}, {9, 30916, {9, 16, 3, 3}}, {9, 0, {9, 16, 3, 2}},
    {19, 607, {6, 7, 3, 1}},    {19, 1207, {12, 7, 2, 1}}, {19, 11007, {10, 7, 3, 1}}, {19, 31007, {10, 7, 3, 3}},
    {19, 0, {10, 7, 3, 2}},
};
constexpr CfgRow kMPipeRows[] = {       // TG_MPIPE_CFG (selectors * 100 + workers) -> <NSEL, NWRK>
    {9, 404, {4, 4}},  {9, 408, {4, 8}},  {9, 412, {4, 12}}, {9, 808, {8, 8}}, {9, 0, {6, 10}},
    {13, 404, {4, 4}}, {13, 605, {6, 5}}, {13, 806, {8, 6}}, {13, 0, {6, 6}},
    {19, 404, {4, 4}}, {19, 605, {6, 5}}, {19, 806, {8, 6}}, {19, 0, {6, 6}},
};
template <size_t R>
inline void cfg_params(const CfgRow (&rows)[R], int S, int cfg, int p[4]) {
    for (const CfgRow &r : rows)
        if (r.S == S && (r.cfg == cfg || r.cfg == 0)) {
            for (int i = 0; i < 4; ++i) p[i] = r.p[i];
            return;
        }
}

inline SelectPuctPlan plan_select_puct(const PlanInputs &in, const SearchKnobs &k) {
    LaunchPlan plan{Kernel::Puct, in.S, {0, 0, 0, 0}, false, in.T, 64};
    if (!puct_pipelined(in, k)) return plan;
    if (split_wanted(in, k)) {
        cfg_params(kSplitRows, in.S, k.split_cfg, plan.p);
        // a tree's workgroups wait for each other through memory: all of them must be resident at once
        const long long grid = (long long)(1 + plan.p[3]) * in.T;
        if (grid <= (long long)in.split_per_cu * in.num_cus) {
            plan.kernel = Kernel::PuctSplit;
            plan.grid = (int)grid;
            plan.block = 1024;
            return plan;
        }
        plan.p[0] = plan.p[1] = plan.p[2] = plan.p[3] = 0;
    }
    if (in.T <= k.mpipe_max_trees) {
        plan.kernel = Kernel::PuctMPipe;
        cfg_params(kMPipeRows, in.S, k.mpipe_cfg, plan.p);
        plan.block = 64 * (plan.p[0] + plan.p[1]);
    } else {
        plan.kernel = Kernel::PuctPipe;
        plan.block = 192;
    }
    return plan;
}

inline SelectGumbelPlan plan_select_gumbel(const PlanInputs &in, const SearchKnobs &k) {
    LaunchPlan plan{Kernel::Gumbel, in.S, {0, 0, 0, 0}, in.unique, in.launch_trees, 64};
    if (k.serial || in.most > kGumbelPipeMaxN || in.N > kPackedPathNodes) return plan;
    const int w = k.gumbel_workers ? k.gumbel_workers : (in.T <= 28 ? 10 : (in.T <= 128 ? 6 : 2));
    plan.kernel = Kernel::GumbelPipe;
    if (in.S == 9) plan.p[0] = w == 15 || w == 10 || w == 6 || w == 4 ? w : 2;
    else if (in.S == 13) plan.p[0] = w >= 6 ? 6 : 2;
    else plan.p[0] = w >= 4 || !k.gumbel_workers ? 4 : 2;
    plan.block = 64 * (1 + plan.p[0]);
    return plan;
}

inline BackupPlan plan_backup(const PlanInputs &in) {
    const int waves = in.S != 13 && in.T <= 64 ? 16 : 8;
    return {Kernel::Backup, in.S, {waves, 0, 0, 0}, in.unique, in.launch_trees, 64 * waves};
}

}  // namespace tg_plan
