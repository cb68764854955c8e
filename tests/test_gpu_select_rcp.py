"""The PUCT selection kernels build, bit for bit, the trees recorded in tests/golden/select_rcp_digests.json
(tools/gen_golden_select_rcp.py: the one-wavefront kernel at commit 38f7062 - IEEE divisions and __dsqrt_rn, every node read
from the pool at every step).  A comparison among the kernels of one build would not notice an error they share; the recorded
digests do.  What they pin: select_puct_pipe_kernel scoring the root from registers it loads once per launch and keeps in
step with its own virtual losses and expansions, and the reciprocal-table quotients of the split selector up to and past the
table's end.

Cases (tests/_select_rcp_digest.py CASES, one child process per run - the kernel variant is read from the environment once):
ragged opening roots, tree 1 on a superko position of the rule corpus; 9x9 with 5 trees, 96 visits as 32/32/32 and 100 as
32/32/32/4; 19x19 with 2 trees, 48 visits as 16/16/16; and 9x9 with 2 trees whose root count passes kRcpN inside the search."""
import functools
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _select_rcp_digest import CASES, K_RCP_N  # noqa: E402

pytestmark = pytest.mark.gpu

# selection kernel -> environment (TG_SELECT_SPLIT=0 unless named: up to 16 trees the split kernel would take the launch)
VARIANTS = {
    "pipe": {"TG_SELECT_MPIPE_TREES": "0"},           # select_puct_pipe_kernel, the many-tree kernel, forced at a small tree count
    "mpipe": {},                                      # select_puct_mpipe_kernel: the default up to 256 trees
    "serial": {"TG_SELECT_SERIAL": "1"},              # select_puct_kernel
    "split": {"TG_SELECT_SPLIT": "1"},                # select_puct_split_kernel: quotients from its reciprocal table
}


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(HERE, "golden", "select_rcp_digests.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def run(case, variant):
    """(digest, nodes, largest root visit count) of one child process."""
    env = dict(os.environ, TG_DEBUG_KNOBS="1", TG_SELECT_SPLIT="0")
    for name in ("TG_SELECT_SERIAL", "TG_SELECT_MPIPE_TREES", "TG_SPLIT_CFG"):
        env.pop(name, None)
    env.update(VARIANTS[variant])
    res = subprocess.run([sys.executable, os.path.join(HERE, "_select_rcp_digest.py")] + CASES[case].split(), env=env,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    digest, nodes, root_visits = res.stdout.strip().splitlines()[-1].split()
    return digest, int(nodes), int(root_visits)


def check(case, variant):
    want = golden()[case]
    assert want["argv"] == CASES[case], "the recorded digest belongs to another configuration: tools/gen_golden_select_rcp.py"
    got = run(case, variant)
    assert got == (want["digest"], want["nodes"], want["max_root_visits"]), (case, variant, got, want)


@pytest.mark.parametrize("case", ["9x9_96", "9x9_100_short_last", "19x19_48"])
def test_pipe_kernel_at_a_small_tree_count_builds_the_recorded_trees(case):
    check(case, "pipe")


@pytest.mark.parametrize("variant", ["pipe", "split"])
def test_root_count_passing_the_table_size(variant):
    """kRcpN + 64 visits in mini-batches of 64.  pipe: 33 launches that each load the root into registers and score it from
    there, up to a count of 2 112.  split: the root's quotients come from the reciprocal table, then - in the same tree, once a
    count reaches kRcpN - from the division sequence."""
    assert golden()["9x9_boundary"]["max_root_visits"] >= K_RCP_N + 64
    check("9x9_boundary", variant)


@pytest.mark.parametrize("variant", ["mpipe", "serial"])
def test_mpipe_and_serial_kernels_build_the_recorded_trees(variant):
    check("9x9_96", variant)
