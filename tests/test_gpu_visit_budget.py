"""Per-tree visit budgets in the four PUCT selection kernels (csrc/visit_budget.h, tg_search_set_budget, tg_search_budget_rule,
tg_search_puct_chain_budget): every tree of a lock-step launch under budgets is the same tree searched alone
with puct_batch(cap), in the strided and in the compact layout.  A fresh child process per kernel (tests/_visit_budget_kernels.py):
the selection knobs are read once per process.  Every comparison is exact."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _visit_budget_kernels as helper
from tests.test_gpu_compact_idle import KERNELS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ERR_ARG, ERR_STATE = -1, -3


@functools.lru_cache(maxsize=None)
def _kernel_run(kernel, layout):
    env = dict(os.environ, TG_DEBUG_KNOBS="1", TG_SELECT_SPLIT="0")
    for name in ("TG_SELECT_SERIAL", "TG_SELECT_MPIPE_TREES", "TG_SPLIT_CFG", "TG_MPIPE_CFG", "TG_SPLIT_TEST_MUTE", "TG_SHARED_DEVICE"):
        env.pop(name, None)
    env.update(KERNELS[kernel][0])
    res = subprocess.run([sys.executable, os.path.join(HERE, "_visit_budget_kernels.py"), layout], env=env, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(next(line for line in res.stdout.splitlines() if line.startswith("BUDGET "))[len("BUDGET "):])


def _visits(stage):
    return [state[1] for state in stage]


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_each_selection_kernel_under_budgets(kernel):
    """Six trees at K = 8 after three plain mini-batches, totals for caps (8, 8, 3, 1, 0, 0): a budgeted mini-batch, a second
    one (caps 8, 4, 0, 0, 0, 0), then a plain one with the budgets off."""
    run = _kernel_run(kernel, "strided")
    assert KERNELS[kernel][1] in run["kernel"]
    warm = helper.WARM * helper.BATCH
    assert _visits(run["stages"][0]) == [warm] * 6
    assert [min(helper.BATCH, max(0, total - warm)) for total in helper.TOTALS] == list(helper.CAPS[0])
    for stage, alone in zip(run["stages"], run["alone"]):
        assert stage == alone                                        # every tree: the same tree searched alone with puct_batch(cap)
    assert run["leaves"] == [list(helper.CAPS[0]), list(helper.CAPS[1]), [helper.BATCH] * 6]
    assert run["planes_ok"] == [True, True, True]                    # leaf j of tree t at row t * 8 + j
    assert run["positions"] == [6 * helper.BATCH] * 3               # the stride stays max_leaves
    first, second, plain = run["stages"][1:]
    assert _visits(first) == [32, 32, 27, 25, 24, 24] and _visits(second) == [40, 36, 27, 25, 24, 24]
    for t in (4, 5):                                                 # cap 0: the tree and its stream cursor are untouched
        assert run["stages"][0][t] == first[t] == second[t]
    for t in (2, 3):
        assert first[t] == second[t]
    assert _visits(plain) == [v + helper.BATCH for v in _visits(second)]


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_each_selection_kernel_under_budgets_compact(kernel):
    """The same behind budget_rule and compact_live: the spent trees have rank -1, the forward passes cover live * 8
    positions, and the trees are those of the strided run - but for the last, plain mini-batch, which the halted trees sit out."""
    run, strided = _kernel_run(kernel, "compact"), _kernel_run(kernel, "strided")
    assert KERNELS[kernel][1] in run["kernel"] and run["kernel"] == strided["kernel"]
    assert run["live"] == [4, 2, 2]
    assert run["rank"] == [[0, 1, 2, 3, -1, -1], [0, 1, -1, -1, -1, -1], [0, 1, -1, -1, -1, -1]]
    assert run["positions"] == [4 * helper.BATCH, 2 * helper.BATCH, 2 * helper.BATCH]
    assert run["planes_ok"] == [True, True, True]                    # leaf j of tree t at row rank[t] * 8 + j
    assert run["leaves"] == [list(helper.CAPS[0]), list(helper.CAPS[1]), [8, 8, 0, 0, 0, 0]]
    for stage, alone in zip(run["stages"], run["alone"]):
        assert stage == alone
    assert run["stages"][:3] == strided["stages"][:3]
    assert _visits(run["stages"][3]) == [48, 44, 27, 25, 24, 24]


def _dualnet_engine(trees, host_streams=False):
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    from tests import _early_stop_cases as cases
    from tests.test_gpu_early_stop import _dualnet
    eng = SearchEngine(9, trees, 96, 8, DeviceEvaluator(_dualnet(9)), host_streams=host_streams)
    for t in range(trees):
        eng.set_root(t, cases.product_board((0, 4, 10, 20)[t % 4]), 1, np.random.RandomState(40 + t).get_state())
    eng.root_eval(False)
    eng.puct_batch(8)
    return eng


@pytest.mark.parametrize("compact", [False, True], ids=["strided", "compact"])
def test_chained_budget_search_equals_the_mini_batches_one_by_one(compact):
    """tg_search_puct_chain_budget on a DualNet (totals 40, 26, 8, 5 after 8 visits: the trees stop after 4, 3, 0 and 0
    mini-batches) against the same mini-batches sent one by one with the rule in between (an engine that cannot chain)."""
    from tests.test_gpu_early_stop import _tree_state
    totals, batches = [40, 26, 8, 5], [8, 8, 8, 8, 8]
    chained, stepped = _dualnet_engine(4), _dualnet_engine(4, host_streams=True)
    try:
        assert chained.can_chain(40) and not stepped.can_chain(40)
        ran = chained.puct_chain(batches, budget=totals, poll_every=1, compact=compact)
        ran_stepped = stepped.puct_chain(batches, budget=totals, poll_every=1, compact=compact)
        assert ran == ran_stepped == 4                               # the fifth mini-batch is never queued: no tree is live
        for t in range(4):
            a, b = _tree_state(chained, t), _tree_state(stepped, t)
            assert a[:4] == b[:4], t
        assert chained.read_root_stats()["node_visits"].tolist() == [40, 26, 8, 8]
        halted, stopped = chained.read_halt()
        assert halted.tolist() == [True] * 4 and stopped.tolist() == [40, 26, 8, 8]
        if compact:
            assert chained.evaluator.batches[-1] == (4 + 2 + 2 + 1) * 8   # live trees at each look: 4 (no rule yet), 2, 2, 1
    finally:
        chained.close()
        stepped.close()


def test_refusals():
    """Budgets together with an early total: TG_ERR_ARG; totals below 1: TG_ERR_ARG; the rule and the chain without budgets in
    force: TG_ERR_STATE; nothing is launched by a refused call."""
    import ctypes
    import torch
    eng = _dualnet_engine(2)
    try:
        arr = np.array([8, 8], dtype=np.int32)
        totals = np.array([30, 30], dtype=np.int32)
        policy = torch.empty((16, 82), dtype=torch.float32, device=eng.device)
        value = torch.empty((16, 3), dtype=torch.float32, device=eng.device)
        ran, pos = ctypes.c_int32(0), ctypes.c_int64(0)

        def budget_chain():
            return eng.lib.tg_search_puct_chain_budget(eng.handle, eng.evaluator.network.handle, arr.ctypes.data, 2, 1, 0, 1,
                                                       eng.planes.data_ptr(), policy.data_ptr(), value.data_ptr(), eng._stream(),
                                                       ctypes.byref(ran), ctypes.byref(pos))

        def early_chain():
            return eng.lib.tg_search_puct_chain_early(eng.handle, eng.evaluator.network.handle, arr.ctypes.data, 2, totals.ctypes.data,
                                                      1, 1, eng.planes.data_ptr(), policy.data_ptr(), value.data_ptr(), eng._stream(),
                                                      ctypes.byref(ran))
        assert eng.lib.tg_search_budget_rule(eng.handle, None, eng._stream()) == ERR_STATE
        assert budget_chain() == ERR_STATE
        bad = np.array([30, 0], dtype=np.int32)
        assert eng.lib.tg_search_set_budget(eng.handle, bad.ctypes.data, eng._stream()) == ERR_ARG
        eng.set_budget(30)
        assert early_chain() == ERR_ARG
        with pytest.raises(ValueError):
            eng.puct_chain([8, 8], budget=True, early_total=30)
        assert eng.read_root_stats()["node_visits"].tolist() == [8, 8]
        eng.set_budget(None)
        assert eng.lib.tg_search_budget_rule(eng.handle, None, eng._stream()) == ERR_STATE
    finally:
        eng.close()
