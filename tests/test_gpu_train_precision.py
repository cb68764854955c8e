"""The HIP training step (tamago_amd/csrc/train.hip) against an fp64 reference of the same step, tensor by tensor (needs a GPU).

One HipTrainer.step per case; every tensor it saves or leaves behind - 13 Z_l, 7 Y_b, 13 D_l, the heads' hD and dL/dlogits, the
three losses, every momentum buffer (the gradient + weight decay on a first step), every parameter and running statistic - is
held to oracle.train_ref.reference_step at fp64 with the device's own ReLU masks pinned:
    err(x) = max|x - x64| / max|x64|,   err_hip <= FACTOR[family] * err_ref32 + 4 * 2^-23
(tools/train_step_precision.py: the bound, the mask rule, the cases and why each batch size is there; the CPU side of it,
tests/test_train_precision_host.py, shows that this bound catches a dropped board, a flipped mask element, plain momentum and a
dropped statistic replica).  The references cost a second or two of CPU time per case and are computed once per case."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import train_step_precision as tsp  # noqa: E402


def _hold(name, rows, flips):
    print(f"{name}: {flips} mask elements differ from the fp64 masks\n{tsp.report(rows)}")
    bad = tsp.violations(rows)
    assert not bad, [(r[0], f"err_ref32 {r[2]:.3e} err_hip {r[3]:.3e} bound {r[4]:.3e}") for r in bad]


@pytest.mark.parametrize("name", list(tsp.CASES))
def test_one_step_against_fp64_with_the_masks_pinned(name):
    """First steps at every launch shape the host code can choose (tsp.CASES), and one step with preloaded momentum and
    non-trivial running statistics: mu, Nesterov and weight decay against the formulas, not through a trajectory."""
    _hold(name, *tsp.run_case(tsp.CASES[name]))


@pytest.mark.parametrize("name", list(tsp.SECOND_STEP_CASES))
def test_second_step_from_the_devices_own_state(name):
    """Step 1, the device's parameters / momentum / statistics read back, step 2 on another batch held to the reference
    started from that state, at the bound of a first step: no drift to absorb, and statistics, partial weight-gradient
    images or loss accumulators that were not cleared between the steps would show."""
    _hold(name, *tsp.run_second_step_case(tsp.SECOND_STEP_CASES[name]))


def test_debug_read_refuses_what_it_does_not_hold():
    """tg_trainer_debug_read: an index beyond the 13 layers / 7 block outputs and a `which` without a tensor are errors."""
    import numpy as np
    import torch
    from tamago_amd import lib as tl
    from tamago_amd.nn import learn
    state, _, _ = tsp.make_inputs(tsp.CASES["s9-b2-rl"])
    hip = learn.HipTrainer(torch.device("cuda", 0), 9, 2, state)
    out = np.zeros((2, 81, 64), dtype=np.float32)
    lib = tl.load()
    try:
        for which, index in ((0, 13), (1, 7), (2, -1), (3, 0), (7, 0), (-1, 0)):
            assert lib.tg_trainer_debug_read(hip.handle, which, index, out.ctypes.data) != 0, (which, index)
        for which, index in ((0, 12), (1, 6), (2, 0), (4, 0), (5, 0), (6, 0)):
            assert lib.tg_trainer_debug_read(hip.handle, which, index, out.ctypes.data) == 0, (which, index)
    finally:
        hip.close()
