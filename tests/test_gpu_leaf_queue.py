"""The device leaf queue itself (csrc/leaf_queue.h), not the trees after its backup: every PUCT selection kernel leaves the
same queue - counts, node indices, root-first paths - after each of two selection launches (tests/_leaf_queue_digest.py)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("TG_SELECT_SERIAL", "TG_MPIPE_PROF", "TG_SELECT_MPIPE_TREES", "TG_SPLIT_CFG", "TG_MPIPE_CFG", "TG_SELECT_SPLIT",
         "TG_SPLIT_TEST_MUTE", "TG_SHARED_DEVICE")
# (the setting, the kernel it is there to run)
VARIANTS = (
    ({}, "select_puct_split_kernel<"),
    ({"TG_SELECT_SPLIT": "0"}, "select_puct_mpipe_kernel<"),
    ({"TG_SELECT_SPLIT": "0", "TG_SELECT_MPIPE_TREES": "0"}, "select_puct_pipe_kernel<"),
    ({"TG_SELECT_SERIAL": "1"}, "select_puct_kernel<"),
)


@pytest.mark.gpu
def test_every_puct_selection_kernel_leaves_the_same_queue():
    script = os.path.join(HERE, "_leaf_queue_digest.py")
    ran = {}
    for setting, kernel in VARIANTS:                        # one after the other, each in a process and under a limit of its own
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(setting, TG_DEBUG_KNOBS="1")
        res = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
        _, name, digest = next(l for l in res.stdout.splitlines() if l.startswith("QUEUE ")).split()
        print(setting, name, digest)
        if name.startswith(kernel):                         # (a device without room for the split kernel's workgroups plans another)
            ran[name] = digest
    # the three kernels every device's plan chooses, and four different ones where the split kernel has room
    assert len(ran) >= 3 and any(n.startswith("select_puct_kernel<") for n in ran), ran
    assert len(set(ran.values())) == 1, ran
