"""The search launch rules (DESIGN.md 4.4 "Search launch plans"), stated independently of csrc/search_plan.h: what
tests/test_search_plan_host.py holds the plan functions to and tests/test_gpu_search_plan.py the handles' launch names."""

SPLIT_CFG = {9: {616: (6, 16, 3, 1), 816: (8, 16, 3, 1), 1016: (10, 16, 2, 1), 912: (9, 12, 3, 1), 11016: (10, 16, 3, 1),
                 30916: (9, 16, 3, 3)},
             19: {607: (6, 7, 3, 1), 1207: (12, 7, 2, 1), 11007: (10, 7, 3, 1), 31007: (10, 7, 3, 3)}}
SPLIT_DEFAULT = {9: (9, 16, 3, 2), 19: (10, 7, 3, 2)}
MPIPE_CFG = {9: {404: (4, 4), 408: (4, 8), 412: (4, 12), 808: (8, 8)},
             13: {404: (4, 4), 605: (6, 5), 806: (8, 6)},
             19: {404: (4, 4), 605: (6, 5), 806: (8, 6)}}
MPIPE_DEFAULT = {9: (6, 10), 13: (6, 6), 19: (6, 6)}

# knob values as the plan functions get them; "unset" is the default of each
DEFAULT_KNOBS = dict(serial=0, mpipe_prof=0, mpipe_max_trees=256, split=1, split_cfg=0, mpipe_cfg=0, gumbel_workers=0)


def _bool(b):
    return "true" if b else "false"


def split_params(S, knobs):
    return SPLIT_CFG[S].get(knobs["split_cfg"], SPLIT_DEFAULT[S])


def puct_name(S, T, N, max_leaves, prof, shared_device, num_cus, per_cu, knobs, split_prof_build=False):
    pipelined = not knobs["serial"] and (not prof or knobs["mpipe_prof"]) and max_leaves <= 1024
    if (pipelined and not shared_device and knobs["split"] and (not prof or split_prof_build) and S != 13 and T <= 16
            and N <= 2 ** 21):
        nnode, nwrk, nship, nwg = split_params(S, knobs)
        if (1 + nwg) * T <= per_cu * num_cus:
            return f"select_puct_split_kernel<{S}, {nnode}, {nwrk}, {nship}, {nwg}> grid={(1 + nwg) * T} block=1024"
    if pipelined and T <= knobs["mpipe_max_trees"]:
        nsel, nwrk = MPIPE_CFG[S].get(knobs["mpipe_cfg"], MPIPE_DEFAULT[S])
        return f"select_puct_mpipe_kernel<{S}, {nsel}, {nwrk}> grid={T} block={64 * (nsel + nwrk)}"
    if pipelined:
        return f"select_puct_pipe_kernel<{S}> grid={T} block=192"
    return f"select_puct_kernel<{S}> grid={T} block=64"


def gumbel_pipelined(N, max_n, knobs):
    return not knobs["serial"] and max_n <= 512 and N <= 2 ** 21


def gumbel_name(S, T, launch_trees, N, max_n, unique, knobs):
    if not gumbel_pipelined(N, max_n, knobs):
        return f"select_gumbel_kernel<{S}, {_bool(unique)}> grid={launch_trees} block=64"
    env = knobs["gumbel_workers"]
    workers = env if env else (10 if T <= 28 else (6 if T <= 128 else 2))
    if S == 9:
        nw = workers if workers in (15, 10, 6, 4) else 2
    elif S == 13:
        nw = 6 if workers >= 6 else 2
    else:
        nw = 4 if (workers >= 4 or not env) else 2
    return f"select_gumbel_pipe_kernel<{S}, {nw}, {_bool(unique)}> grid={launch_trees} block={64 * (1 + nw)}"


def backup_name(S, T, launch_trees, unique):
    waves = 8 if S == 13 else (16 if T <= 64 else 8)
    return f"backup_kernel<{S}, {waves}, {_bool(unique)}> grid={launch_trees} block={64 * waves}"


def built_kernels():
    """The selection and backup instantiations of csrc/search.hip: 65 of the 94 kernels of its code object."""
    names = set()
    for S in (9, 19):
        for p in list(SPLIT_CFG[S].values()) + [SPLIT_DEFAULT[S]]:
            names.add(f"select_puct_split_kernel<{S}, {p[0]}, {p[1]}, {p[2]}, {p[3]}>")
    for S in (9, 13, 19):
        for p in list(MPIPE_CFG[S].values()) + [MPIPE_DEFAULT[S]]:
            names.add(f"select_puct_mpipe_kernel<{S}, {p[0]}, {p[1]}>")
        names.add(f"select_puct_pipe_kernel<{S}>")
        names.add(f"select_puct_kernel<{S}>")
    for u in ("false", "true"):
        for S, nws in ((9, (15, 10, 6, 4, 2)), (13, (6, 2)), (19, (4, 2))):
            names.add(f"select_gumbel_kernel<{S}, {u}>")
            for nw in nws:
                names.add(f"select_gumbel_pipe_kernel<{S}, {nw}, {u}>")
        for S, waves in ((9, 16), (9, 8), (13, 8), (19, 16), (19, 8)):
            names.add(f"backup_kernel<{S}, {waves}, {u}>")
    assert len(names) == 12 + 13 + 3 + 3 + 24 + 10
    return names
