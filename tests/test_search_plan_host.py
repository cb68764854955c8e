"""The search launch rules on the CPU: csrc/search_plan.h, compiled alone into tests/search_plan_driver.cpp with the host
compiler, against the independent statement of DESIGN.md 4.4's tables in tests/_search_plan_rules.py."""
import itertools
import os
import shutil
import subprocess

import pytest

from tests import _search_plan_rules as rules

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = (9, 13, 19)
TREES = (1, 4, 16, 17, 28, 29, 64, 65, 128, 129, 256, 257, 2048)
NODES = (1024, 2 ** 21, 2 ** 21 + 1)
MAX_LEAVES = (0, 1, 1024, 1025)
MAX_N = (1, 512, 513)
NUM_CUS = 256


def _knob_settings():
    """All knobs unset, then each knob alone."""
    yield "unset", {}
    split_cfgs = sorted({c for S in rules.SPLIT_CFG for c in rules.SPLIT_CFG[S]}) + [4242]
    mpipe_cfgs = sorted({c for S in rules.MPIPE_CFG for c in rules.MPIPE_CFG[S]}) + [4242]
    for c in split_cfgs:
        yield f"TG_SPLIT_CFG={c}", {"split_cfg": c}
    for c in mpipe_cfgs:
        yield f"TG_MPIPE_CFG={c}", {"mpipe_cfg": c}
    for w in range(17):
        yield f"TG_GUMBEL_WORKERS={w}", {"gumbel_workers": w}
    for t in (0, 300):
        yield f"TG_SELECT_MPIPE_TREES={t}", {"mpipe_max_trees": t}
    for v in (0, 1):
        yield f"TG_SELECT_SPLIT={v}", {"split": v}
    yield "TG_SELECT_SERIAL", {"serial": 1}
    yield "TG_MPIPE_PROF", {"mpipe_prof": 1}


def _cases():
    """(label, driver input line, expected name)"""
    for label, setting in _knob_settings():
        knobs = dict(rules.DEFAULT_KNOBS, **setting)
        kline = "{serial} {mpipe_prof} {mpipe_max_trees} {split} {split_cfg} {mpipe_cfg} {gumbel_workers}".format(**knobs)
        for S, T, N in itertools.product(SIZES, TREES, NODES):
            # PUCT.  Split room: a CU count of 256 with one workgroup per CU and with none; and, at the boundary itself, a
            # device of exactly (1 + NWG) T CUs and one with a CU less (per_cu * num_cus cannot meet (1 + NWG) T at 256 CUs)
            need = (1 + rules.split_params(S if S != 13 else 9, knobs)[3]) * T
            rooms = ((NUM_CUS, 1), (NUM_CUS, 0), (need, 1), (need - 1, 1))
            for max_leaves, prof, shared, (cus, per_cu) in itertools.product(MAX_LEAVES, (0, 1), (0, 1), rooms):
                want = rules.puct_name(S, T, N, max_leaves, prof, shared, cus, per_cu, knobs)
                yield (f"{label} puct S{S} T{T} N{N} leaves{max_leaves} prof{prof} shared{shared} cus{cus}x{per_cu}",
                       f"0 {S} {T} {T} {N} {max_leaves} 0 {prof} {shared} {cus} {per_cu} 0 {kline}", want)
            # Gumbel and backup: the whole engine, and a slice of it (the grid follows the slice, the kernel the engine)
            for trees, unique in itertools.product(sorted({T, max(1, T // 2)}), (0, 1)):
                for max_n in MAX_N:
                    yield (f"{label} gumbel S{S} T{T}/{trees} N{N} n{max_n} unique{unique}",
                           f"1 {S} {T} {trees} {N} {max_n} {unique} 0 0 {NUM_CUS} 1 0 {kline}",
                           rules.gumbel_name(S, T, trees, N, max_n, unique, knobs))
                yield (f"{label} backup S{S} T{T}/{trees} unique{unique}",
                       f"2 {S} {T} {trees} {N} 0 {unique} 0 0 {NUM_CUS} 1 0 {kline}", rules.backup_name(S, T, trees, unique))
    # a TG_SPLIT_PROF build keeps the split kernel while the profile buffer is on
    knobs = rules.DEFAULT_KNOBS
    yield ("split_prof build", "0 9 4 4 1024 8 0 1 0 256 1 1 0 1 256 1 0 0 0",
           rules.puct_name(9, 4, 1024, 8, 1, 0, 256, 1, dict(knobs, mpipe_prof=1), split_prof_build=True))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("search_plan") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", os.path.join(HERE, "search_plan_driver.cpp"), "-o", exe])
    return exe


def test_plan_functions_follow_the_rules(driver):
    cases = list(_cases())
    res = subprocess.run([driver], input="\n".join(c[1] for c in cases) + "\n", capture_output=True, text=True, check=True)
    got = res.stdout.splitlines()
    assert len(got) == len(cases)
    wrong = [(label, g, want) for (label, _, want), g in zip(cases, got) if g != want]
    assert not wrong, f"{len(wrong)} of {len(cases)} plans differ from the rules, first: {wrong[:5]}"
    # every name a plan can render is an instantiation the library builds - and the grid reaches every one of them
    built = rules.built_kernels()
    named = {g.split(" grid=")[0] for g in got}
    assert named <= built, sorted(named - built)
    assert named == built, sorted(built - named)


def test_the_rules_statement_itself():
    """Spot values of the independent statement, by hand from DESIGN.md 4.4 (a typo there would otherwise only have to agree
    with the header's)."""
    k = rules.DEFAULT_KNOBS
    assert rules.puct_name(9, 1, 64, 8, 0, 0, 256, 1, k) == "select_puct_split_kernel<9, 9, 16, 3, 2> grid=3 block=1024"
    assert rules.puct_name(19, 16, 64, 8, 0, 0, 256, 1, k) == "select_puct_split_kernel<19, 10, 7, 3, 2> grid=48 block=1024"
    assert rules.puct_name(9, 17, 64, 8, 0, 0, 256, 1, k) == "select_puct_mpipe_kernel<9, 6, 10> grid=17 block=1024"
    assert rules.puct_name(13, 2, 64, 8, 0, 0, 256, 1, k) == "select_puct_mpipe_kernel<13, 6, 6> grid=2 block=768"
    assert rules.puct_name(9, 300, 64, 8, 0, 0, 256, 1, k) == "select_puct_pipe_kernel<9> grid=300 block=192"
    assert rules.puct_name(9, 1, 64, 8, 1, 0, 256, 1, k) == "select_puct_kernel<9> grid=1 block=64"
    assert rules.gumbel_name(9, 1, 1, 64, 8, 0, k) == "select_gumbel_pipe_kernel<9, 10, false> grid=1 block=704"
    assert rules.gumbel_name(19, 300, 300, 64, 8, 1, k) == "select_gumbel_pipe_kernel<19, 4, true> grid=300 block=320"
    assert rules.gumbel_name(13, 2, 2, 64, 513, 0, k) == "select_gumbel_kernel<13, false> grid=2 block=64"
    assert rules.backup_name(9, 64, 64, 0) == "backup_kernel<9, 16, false> grid=64 block=1024"
    assert rules.backup_name(13, 2, 2, 1) == "backup_kernel<13, 8, true> grid=2 block=512"
