"""The forward launch rules on the CPU: csrc/forward_plan.h, compiled alone into tests/forward_plan_driver.cpp with the host
compiler (-ffp-contract=off, as the library is built: the recorded FLOP means must come out bit for bit), against every row of
tests/golden/forward_plan.json and the independent statement of DESIGN.md 4.1's table in tests/_forward_plan_rules.py."""
import itertools
import json
import math
import os
import re
import shutil
import subprocess

import pytest

from tests import _forward_plan_rules as rules

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "tamago_amd", "csrc")
FAMILIES = ("direct", "wino", "split9", "w1d9", "split13", "split19", "band19", "pair19")      # enum Family, in its order
DEMOTED = ("none", "spread_w1d", "spread_split", "band_timeouts")                              # enum Demoted
ALGOS = (None, "w1d", "split16", "w1dband", "wino", "direct", "no-such-algorithm")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("forward_plan") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(HERE, "forward_plan_driver.cpp"), "-o", exe])

    def run(cases):
        """cases: dicts of plan()'s arguments -> per case (name, flops, peak, dtype, plan dict)"""
        lines = []
        for c in cases:
            k = dict(rules.DEFAULT_KNOBS, **c.get("knobs", {}))
            env = [k["algo"], k["bands"], k["group"], k["wino"], "1" if k["no_tail"] else None, "0" if k["guard_off"] else None,
                   k["fwd_cus"], k["split_span"]]
            lines.append("%d %d %d %r %r %d %d %d %d %s" % (
                c["S"], c["batch"], c.get("cus", 256), c.get("spread_w1d", 1.0), c.get("spread_split", 1.0), c.get("shared", False),
                c.get("timeouts", 0), c.get("guard_cap", 0), c.get("fwd_cap", 0), " ".join("-" if v is None else v for v in env)))
        res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        out = []
        for line in res.stdout.splitlines():
            name, flops, peak, dtype, rest = line.split("|")
            v = [int(x) for x in rest.split()]
            out.append((name, float.fromhex(flops), float.fromhex(peak), dtype,
                        dict(family=FAMILIES[v[0]], group=v[1], bands=v[2], tail=v[3], guarded=bool(v[4]), grid=v[5], guard_grid=v[6],
                             span=v[7], demoted=DEMOTED[v[8]])))
        assert len(out) == len(cases)
        return out
    return run


def test_every_recorded_row_holds(driver, golden_dir):
    """(a) name, FLOPs, peak and operand format of all rows of the fixture, on its own CU count and spreads: caps 0 / 0, no time-outs"""
    with open(os.path.join(golden_dir, "forward_plan.json")) as f:
        fix = json.load(f)
    assert fix["columns"] == ["network", "size", "batch", "algo", "bands", "shared", "name", "flops", "peak", "dtype"]
    cases = []
    for network, size, batch, algo, bands, shared in (r[:6] for r in fix["rows"]):
        w1d, split = fix["channel_spread_w1d_split"][f"{network}/{size}"]
        cases.append(dict(S=size, batch=batch, cus=fix["num_cus"], spread_w1d=w1d, spread_split=split, shared=shared,
                          knobs=dict(algo=algo, bands=bands)))
    assert len(cases) >= 510
    got = driver(cases)
    wrong = [(r[:6], g[:4], r[6:]) for r, g in zip(fix["rows"], got) if list(g[:4]) != r[6:]]      # (the doubles: ==)
    assert not wrong, f"{len(wrong)} of {len(cases)} rows differ (case, got, recorded); the first: {wrong[:5]}"


def _knob_settings(S):
    """All knobs unset, then each knob alone."""
    yield {}
    yield {"guard_off": True}
    for v in ("100", "300"):
        yield {"fwd_cus": v}
    if S == 9:
        for v in ("1", "2", "3"):
            yield {"group": v}
        for v in ("81", "82", "83", "84", "1", "2", "3"):
            yield {"wino": v}
        yield {"no_tail": True}
        for v in ("2", "3", "4", "8", "5"):
            yield {"split_span": v}
    if S == 19:
        for v in ("0", "2", "4", "3", "-1"):
            yield {"bands": v}


def _cases():
    above = lambda x: math.nextafter(x, math.inf)
    spreads = ((1.0, 1.0), (rules.LIMIT_W1D, 1.0), (above(rules.LIMIT_W1D), 1.0), (1.0, rules.LIMIT_SPLIT),
               (above(rules.LIMIT_W1D), above(rules.LIMIT_SPLIT)), (1.0, above(rules.LIMIT_SPLIT)))
    caps = ((0, 0), (16, 0), (16, 224), (0, 224), (0, 300), (16, 100))
    batches = {9: (1, 5, 256, 257, 512, 513, 768, 769, 896, 1000, 3200, 65536), 13: (1, 300, 700),
               19: (1, 5, 13, 16, 17, 32, 33, 64, 65, 128, 129, 4096)}
    for S in (9, 13, 19):
        for batch, algo, knobs in itertools.product(batches[S], ALGOS, _knob_settings(S)):
            for (guard_cap, fwd_cap), shared, timeouts in itertools.product(caps, (False, True), (0, 1)):
                if S != 19 and (shared or timeouts):
                    continue
                yield dict(S=S, batch=batch, knobs=dict(knobs, algo=algo), guard_cap=guard_cap, fwd_cap=fwd_cap, shared=shared,
                           timeouts=timeouts)
            for w1d, split in spreads[1:]:
                yield dict(S=S, batch=batch, knobs=dict(knobs, algo=algo), spread_w1d=w1d, spread_split=split)
    # another CU count: the thresholds and the direct kernel's workgroups per CU follow it
    for S, batch, algo in itertools.product((9, 19), (1, 60, 61, 200, 304, 305, 3000), ALGOS):
        yield dict(S=S, batch=batch, cus=304, knobs=dict(algo=algo))


def _expected(c):
    args = {k: v for k, v in c.items() if k not in ("S", "batch", "knobs")}
    return rules.plan(c["S"], c["batch"], dict(rules.DEFAULT_KNOBS, **c["knobs"]), **args)


def _built_rows():
    """The launch tables as the sources hold them: kExactRows, kSplitRows and the two-way choices."""
    with open(os.path.join(CSRC, "net_forward.hip")) as f:
        exact = re.search(r"kExactRows\[\] = \{(.*?)\n\};", f.read(), re.S).group(1)
    with open(os.path.join(CSRC, "net_forward_split.hip")) as f:
        split = re.search(r"kSplitRows\[\] = \{(.*?)\n\};", f.read(), re.S).group(1)
    rows = set()
    for wino, S, g, fn, fS, fg in re.findall(r"\{(true|false), (\d+), (\d+), (launch_wino8|launch)<(\d+), (\d+)[,>]", exact):
        assert (fS, fg) == (S, g) and (fn == "launch_wino8") == (wino == "true"), "a row's key and its instantiation differ"
        rows.add(("wino" if wino == "true" else "direct", int(S), int(g)))
    for S, g, span, fS, fg, fspan in re.findall(r"\{(\d+), (\d+), (\d+), launch_split<(\d+), (\d+), FmtF16(?:, (\d+))?>\}", split):
        assert (fS, fg, fspan or "6") == (S, g, span), "a row's key and its instantiation differ"
        rows.add((int(S), int(g), int(span)))
    return rows


def test_plan_follows_the_rules(driver):
    """(b) grids, caps, tails, bands, demotions and knobs the fixture does not reach, and every row of the launch tables"""
    cases = list(_cases())
    got = driver(cases)
    wrong, reached = [], set()
    for c, (name, _, _, _, p) in zip(cases, got):
        want = _expected(c)
        if p != want or name != rules.name(want, c["S"]):
            wrong.append((c, name, p, want))
        reached |= rules.rows(p, c["S"])
    assert not wrong, f"{len(wrong)} of {len(cases)} plans differ from the rules (case, name, got, rules); the first: {wrong[:3]}"
    built = rules.EXACT_ROWS | rules.SPLIT_ROWS | rules.OTHER_ROWS
    assert reached <= built, sorted(map(str, reached - built))
    assert reached == built, sorted(map(str, built - reached))
    assert _built_rows() == rules.EXACT_ROWS | rules.SPLIT_ROWS


def test_the_rules_statement_itself(driver):
    """Spot values by hand from the parent's code on 256 CUs, against the rules AND the header (a typo in the rules would
    otherwise only have to agree with the header's)."""
    def both(S, batch, **kw):
        knobs = {k: kw.pop(k) for k in list(kw) if k in rules.DEFAULT_KNOBS}
        c = dict(S=S, batch=batch, knobs=knobs, **kw)
        (name, _, _, _, p), = driver([c])
        want = _expected(c)
        assert p == want and name == rules.name(want, S), (c, name, p, want)
        return dict(p, name=name)

    def sub(p, **want):
        return {k: p[k] for k in want} == want

    # ragged tail under a forward cap (9x9 default, 3 200 positions: 4 rounds of 768 + 128 | 672 x 4 + 512)
    assert sub(both(9, 3200), family="w1d9", tail=128, group=3, grid=256,
               name="dualnet_fwd_w1d_kernel<3> + dualnet_fwd_w1d_kernel<1> (ragged tail)")
    assert sub(both(9, 3200, fwd_cap=224), tail=0, grid=224, name="dualnet_fwd_w1d_kernel<3>")
    assert sub(both(9, 3200, no_tail=True), tail=0, grid=256)
    assert both(9, 3200, fwd_cap=300) == both(9, 3200)
    # split grid: TG_FWD_CUS only
    assert sub(both(9, 3200, algo="split16"), family="split9", grid=256, span=6)
    assert sub(both(9, 3200, algo="split16", fwd_cus="100"), grid=100)
    assert sub(both(9, 3200, algo="split16", fwd_cap=224), grid=256)
    # guard launch grid
    assert sub(both(9, 3200), guard_grid=256)
    assert sub(both(9, 3200, guard_cap=16), guard_grid=16)
    assert sub(both(9, 3200, algo="wino", guard_cap=16), family="wino", guarded=False, grid=256, guard_grid=0)
    # bands (19x19 split16)
    for batch, bands in ((16, 4), (17, 2), (32, 2), (33, 0)):
        assert sub(both(19, batch, algo="split16", guard_cap=16), family="band19" if bands else "split19", bands=bands, grid=batch * bands or batch)
    for fwd_cap in (1, 224, 300):
        assert sub(both(19, 4, algo="split16", fwd_cap=fwd_cap, bands="2"), family="split19", bands=0)
    assert sub(both(19, 65, algo="split16", bands="4"), family="band19", bands=2, grid=130)
    assert sub(both(19, 64, algo="split16", bands="4"), bands=4, grid=256)
    assert sub(both(19, 1, algo="split16", bands="0"), family="split19", bands=0)
    # pair kernel (19x19 default): workgroups
    for batch, fwd_cap, grid in ((5, 0, 10), (13, 0, 16), (4096, 0, 256), (4096, 100, 96)):
        assert sub(both(19, batch, fwd_cap=fwd_cap), family="pair19", grid=grid, demoted="none")
    assert sub(both(19, 16, timeouts=1), family="split19", demoted="band_timeouts")
    assert sub(both(19, 16, algo="w1dband", timeouts=1, shared=True), family="pair19", demoted="none")
    # spread limits: the limit itself passes, the next double does not
    up = lambda x: math.nextafter(x, math.inf)
    assert sub(both(9, 1, spread_w1d=128.0), family="w1d9", demoted="none")
    assert sub(both(9, 1, spread_w1d=up(128.0)), family="split9", demoted="spread_w1d")
    assert sub(both(19, 1, spread_w1d=up(128.0)), family="band19", demoted="spread_w1d")
    assert sub(both(9, 1, spread_split=262144.0), family="w1d9", demoted="none")
    assert sub(both(9, 1, spread_split=up(262144.0)), family="wino", demoted="spread_split", guarded=False)
    assert sub(both(9, 1, spread_w1d=1e9, spread_split=1e9, guard_off=True), family="w1d9", demoted="none")
    assert sub(both(13, 1, spread_split=1e9), family="direct", demoted="none")
    assert sub(both(13, 1, spread_split=1e9, algo="split16"), family="direct", demoted="spread_split")
    assert sub(both(13, 1, algo="split16"), family="split13", guarded=True, guard_grid=1)
    # TG_FWD_GROUP (9x9 direct), TG_FWD_WINO (9x9 wino)
    assert sub(both(9, 1, algo="direct", group="3"), name="dualnet_fwd_kernel<9, 3>", grid=1)
    assert sub(both(9, 1, algo="direct", group="2"), name="dualnet_fwd_kernel<9, 1>")
    assert sub(both(9, 3200, algo="direct"), name="dualnet_fwd_kernel<9, 3>", grid=512)
    for batch in (1, 3200):
        for v, g in (("81", 1), ("82", 2), ("83", 3), ("1", 1), ("2", 2), ("3", 3)):
            assert sub(both(9, batch, algo="wino", wino=v), name=f"dualnet_fwd_wino8_kernel<9, {g}>")
        assert sub(both(9, batch, algo="wino", wino="84"), group=1 if batch == 1 else 3)
