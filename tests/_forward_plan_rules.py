"""The forward launch rules (DESIGN.md 4.1 "How a launch is chosen": the table, row by row), stated independently of
csrc/forward_plan.h: what tests/test_forward_plan_host.py holds plan_forward to.  Knob values are the strings the environment
would hold (None: unset)."""

LIMIT_W1D, LIMIT_SPLIT = 128.0, 262144.0

DEFAULT_KNOBS = dict(algo=None, bands=None, group=None, wino=None, no_tail=False, guard_off=False, fwd_cus=None, split_span=None)

# the instantiations the launch tables hold (csrc/net_forward.hip kExactRows, csrc/net_forward_split.hip kSplitRows, the two-way
# choices of w1d_forward and band_forward, the pair kernel): what a plan can name
EXACT_ROWS = {("wino", 19, 1), ("direct", 19, 1), ("wino", 9, 3), ("wino", 9, 1), ("wino", 9, 2), ("wino", 13, 1),
              ("direct", 13, 1), ("direct", 9, 3), ("direct", 9, 1)}
SPLIT_ROWS = {(13, 1, 6), (19, 1, 6), (9, 3, 2), (9, 3, 3), (9, 3, 4), (9, 3, 8), (9, 3, 6), (9, 1, 6)}
OTHER_ROWS = {("w1d", 3), ("w1d", 1), ("band", 4), ("band", 2), ("pair",)}
DIRECT_WORKGROUPS_PER_CU = {(9, 1): 2, (9, 3): 2, (13, 1): 2, (19, 1): 1}

F16_FAMILIES = ("w1d", "split16", "w1dband")


def _cap(n, cap):
    return cap if 0 < cap < n else n


def _groups(batch, group):
    return -(-batch // group)


def plan(S, batch, knobs, cus=256, spread_w1d=1.0, spread_split=1.0, shared=False, timeouts=0, guard_cap=0, fwd_cap=0):
    """family, group, bands, tail, guarded, grid (with a tail: the head launch's), guard_grid, span, demoted"""
    algo = knobs["algo"]
    out = dict(group=1, bands=0, tail=0, guarded=False, grid=0, guard_grid=0, span=6, demoted="none")
    guard_on = not knobs["guard_off"]
    # rows 1 and 2: is an f16 family asked for, and may this network have one
    asked = algo == "split16" if S == 13 else (algo is None or algo in F16_FAMILIES)
    if asked and guard_on and spread_split > LIMIT_SPLIT:
        asked, out["demoted"] = False, "spread_split"
    if not asked:
        # row 3: exact fp32
        if algo == "direct" or S == 13:
            out["family"] = "direct"
            if S == 9:
                forced = int(knobs["group"]) if knobs["group"] is not None else 0
                out["group"] = forced if forced in (1, 3) else (3 if batch > 2 * cus else 1)
            out["grid"] = min(_groups(batch, out["group"]), cus * DIRECT_WORKGROUPS_PER_CU[S, out["group"]])
        else:
            out["family"] = "wino"
            if S == 9:
                forced = int(knobs["wino"]) % 10 if knobs["wino"] is not None else 0
                out["group"] = forced if forced in (1, 2, 3) else (1 if batch <= cus else (2 if batch <= 2 * cus else 3))
            out["grid"] = min(_groups(batch, out["group"]), cus)
        return out
    out["guarded"] = True
    one_axis_fits = not guard_on or spread_w1d <= LIMIT_W1D
    bands_set = knobs["bands"] is not None
    if S == 13:
        out["family"] = "split13"                                   # row 4
    elif S == 19:
        pair = algo in (None, "w1dband")                            # row 5
        if pair and not one_axis_fits:
            pair, out["demoted"] = False, "spread_w1d"
        if pair and algo is None:
            if bands_set or shared:
                pair = False
            elif timeouts > 0:
                pair, out["demoted"] = False, "band_timeouts"
        if pair:
            pairs = min(batch, _cap(cus, fwd_cap) // 2)
            if pairs >= 8:
                pairs -= pairs % 8
            out.update(family="pair19", grid=2 * pairs)
        else:                                                       # row 6
            forced = int(knobs["bands"]) if bands_set else None
            if forced is not None and forced < 0:
                forced = None
            room = cus // 4 if guard_cap > 0 else cus
            if forced == 0 or fwd_cap > 0 or (forced is None and (shared or timeouts > 0)):
                bands = 0
            elif forced in (None, 4) and 4 * batch <= room:
                bands = 4
            elif forced in (None, 2, 4) and 2 * batch <= room:
                bands = 2
            else:
                bands = 0
            out.update(family="band19" if bands else "split19", bands=bands)
    else:
        one_axis = algo in (None, "w1d")                            # row 7
        if one_axis and not one_axis_fits:
            one_axis, out["demoted"] = False, "spread_w1d"
        out["family"] = "w1d9" if one_axis else "split9"
        out["group"] = 3 if batch > cus else 1
        a_round = 3 * _cap(cus, fwd_cap)
        left = batch % a_round
        if not knobs["no_tail"] and batch > a_round and 0 < left <= a_round // 3:
            out["tail"] = left
    # row 8: grids
    groups = _groups(batch - out["tail"], out["group"])
    if out["family"] == "w1d9":
        out["grid"] = _cap(min(groups, cus), fwd_cap)
    elif out["family"] == "band19":
        out["grid"] = batch * out["bands"]
    elif out["family"] != "pair19":
        out["grid"] = min(groups, _cap(cus, int(knobs["fwd_cus"]) if knobs["fwd_cus"] is not None else 0))
    if out["family"] == "split9" and out["group"] == 3 and knobs["split_span"] in ("2", "3", "4", "8"):
        out["span"] = int(knobs["split_span"])
    out["guard_grid"] = _cap(min(groups, cus), guard_cap)
    return out


def name(p, S):
    f, g = p["family"], p["group"]
    if f == "pair19":
        return "dualnet_fwd_w1dband_kernel + dualnet_heads19_kernel"
    if f == "band19":
        return f"dualnet_fwd_band_kernel<{p['bands']}>"
    if f == "split13":
        return "dualnet_fwd_split_kernel<13, 1, f16x2> + dualnet_fwd_wino8_kernel<13, 1> (range guard, per board)"
    if f in ("w1d9", "split9", "split19"):
        kernel = "dualnet_fwd_w1d_kernel<%d>" if f == "w1d9" else f"dualnet_fwd_split_kernel<{S}, %d, f16x2>"
        if p["tail"] > 0:
            return f"{kernel % 3} + {kernel % 1} (ragged tail)"
        return kernel % g
    if f == "wino":
        return "dualnet_fwd_wino8_kernel<19, 1, global scratch>" if S == 19 else f"dualnet_fwd_wino8_kernel<{S}, {g}>"
    return f"dualnet_fwd_kernel<{S}, {g}>"


def rows(p, S):
    """The launch-table rows the plan's launches look up (a ragged tail: the one-board launch behind the head, too)."""
    f, g = p["family"], p["group"]
    if f in ("wino", "direct"):
        return {(f, S, g)}
    out = {("wino", S, g)}                                          # the range guard behind every f16 launch
    if f in ("split9", "split13", "split19"):
        out.add((S, g, p["span"]))
        if p["tail"] > 0:
            out |= {(S, 1, 6), ("wino", S, 1)}
    elif f == "w1d9":
        out.add(("w1d", g))
        if p["tail"] > 0:
            out |= {("w1d", 1), ("wino", S, 1)}
    elif f == "band19":
        out.add(("band", p["bands"]))
    else:
        out.add(("pair",))
    return out
