"""The wiring of the search launch plans on real handles: tg_search_launch_name - the name of the plan the launcher gets
from the same call - equals the rules of DESIGN.md 4.4 (tests/_search_plan_rules.py) evaluated with the device's CU count.
Nothing is launched but what handle creation does."""
import json
import os
import subprocess
import sys

import pytest

from tests import _search_plan_rules as rules

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("TG_SELECT_SERIAL", "TG_MPIPE_PROF", "TG_SELECT_MPIPE_TREES", "TG_SPLIT_CFG", "TG_MPIPE_CFG", "TG_GUMBEL_WORKERS",
         "TG_SELECT_SPLIT", "TG_SPLIT_TEST_MUTE", "TG_GUMBEL_ONE_BY_ONE", "TG_SHARED_DEVICE")
# select_puct_split_kernel: 1024 threads and more than 80 of a CU's 160 KB of LDS - one workgroup per CU
SPLIT_PER_CU = 1


@pytest.fixture(scope="module")
def reported():
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env["TG_DEBUG_KNOBS"] = "1"
    res = subprocess.run([sys.executable, os.path.join(HERE, "_search_plan_names.py")], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    line = next(l for l in res.stdout.splitlines() if l.startswith("NAMES "))
    return json.loads(line[len("NAMES "):])


def _expected(S, T, cus, prof=False):
    from tests._search_plan_names import BATCH, TREE_SIZE
    k = rules.DEFAULT_KNOBS
    return {"puct": rules.puct_name(S, T, TREE_SIZE, BATCH, prof, False, cus, SPLIT_PER_CU, k),
            "gumbel": rules.gumbel_name(S, T, T, TREE_SIZE, BATCH, False, k),
            "gumbel_unique": rules.gumbel_name(S, T, T, TREE_SIZE, BATCH, True, k),
            "gumbel_513": rules.gumbel_name(S, T, T, TREE_SIZE, 513, True, k),
            "backup": rules.backup_name(S, T, T, False),
            "backup_unique": rules.backup_name(S, T, T, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("S,T", [(9, 1), (9, 17), (9, 300), (13, 2), (19, 2)])
def test_launch_names_follow_the_rules(reported, S, T):
    cus = reported["cus"]
    got = reported["handles"][f"{S},{T}"]
    assert got["plain"] == _expected(S, T, cus)
    if "split_kernel" in got["plain"]["puct"]:                   # a split name only where all the tree's workgroups fit
        nwg = rules.split_params(S, rules.DEFAULT_KNOBS)[3]
        assert (1 + nwg) * T <= SPLIT_PER_CU * cus
    built = rules.built_kernels()
    assert {n.split(" grid=")[0] for n in got["plain"].values()} <= built


@pytest.mark.gpu
def test_profile_buffer_and_per_call_knob(reported):
    cus = reported["cus"]
    got = reported["handles"]["9,1"]
    assert got["profile"] == _expected(9, 1, cus, prof=True)
    assert got["profile"]["puct"] == "select_puct_kernel<9> grid=1 block=64"
    assert got["one_by_one"] == got["plain"] == got["again"]
