"""CPU side of the head-epilogue check (tools/head_epilogue_precision.py, tests/test_gpu_head_epilogue.py): the crafted cases
are what the criterion presupposes, the criterion passes the undamaged epilogue and fails with each fault model on named cases,
and the 1e-4 absolute check of tests/test_gpu_net.py lets the faults of average weight through.

FAULT_TABLE is what the GPU test's teeth rest on: a kernel copy with one of these faults misses the criterion on the cases
named there, which the GPU test runs on every family."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import head_epilogue_precision as hep  # noqa: E402

OLD_TOL = 1e-4                           # tests/test_gpu_net.py: TOL, absolute

# fault -> cases (of every board size unless the name carries an index that only some have) on which the criterion must fail.
# `mixed` = hep.mixed_rows: different rows on the boards of a workgroup, which on the GPU the real-network test supplies.
# `nan-prefill` = the crafted case run into outputs that hold NaN (forward_device(out=...)).
FAULT_TABLE = {
    "sum_omits_last_stripe": ["equal0", "equal1e4", "tail", "rampup", "peak{pass}", "tower{pass}"],
    "sum_omits_last_entry": ["equal0", "equal1e4", "peak{pass}", "tower{pass}", "rampup"],
    "max_omits_last_stripe": ["tower{pass}"],                      # (expf(120) overflows; a maximum of -20 or -40 still serves)
    "no_max_subtraction": ["equal1e4", "wide"],
    "pass_not_stored": ["nan-prefill"],
    "boards_exchange_inv": ["mixed"],
    "value_takes_neighbour_exp": ["peak0", "peak63", "peak64"],    # (they carry value biases (30, 0, -30), (30, -30, 0), (0, 30, -30))
}


def _case(size, name):
    A = hep.actions(size)
    name = name.replace("{pass}", str(A - 1))
    return next(c for c in hep.cases(size) if c[0] == name)


def _launch(size, name, boards=4):
    """A workgroup's boards: `boards` copies of a crafted case, or the mixed launch."""
    if name == "mixed":
        return hep.mixed_rows(size)
    _, row, vrow = _case(size, name)
    return np.tile(row, (boards, 1)), np.tile(vrow, (boards, 1))


def _passes(policy, value, logits, vlogits):
    return hep.within(policy, logits) and hep.within(value, vlogits)


@pytest.mark.parametrize("size", hep.SIZES)
def test_cases_are_what_the_criterion_presupposes(size):
    """Tiny entries only where the issue allows them, the fp32 reference within 3 (19 on normal*) ulp, every bias a multiple of
    2^-6, every value case carried, PASS in the second, third and sixth stripe."""
    hep.condition(size)
    A = hep.actions(size)
    assert hep.last_stripe(A) // 64 == {82: 1, 170: 2, 362: 5}[A]
    names = hep.case_names(size)
    assert len(names) == len(set(names)) == (17 if size == 9 else 19)
    carried = set()
    for name, row, vrow in hep.cases(size):
        assert row.dtype == np.float32 and row.shape == (A,) and vrow.shape == (3,)
        assert np.array_equal(row * 64.0, np.round(row * 64.0)), name
        l = row.astype(np.float64)
        assert np.array_equal((row - row.max()).astype(np.float64), l - l.max()), name       # l - m is exact in fp32
        carried.add(tuple(float(v) for v in vrow))
    assert carried == {tuple(float(np.float32(v)) for v in c) for c in hep.VALUE_CASES} and len(carried) == 11


@pytest.mark.parametrize("size", hep.SIZES)
def test_undamaged_epilogue_passes_every_case(size):
    """The restated epilogue (striped per-lane sums, butterfly) without a fault is within the criterion on every case, on the
    mixed launch and into NaN-prefilled outputs - the fault models fail for their fault alone."""
    for name in hep.case_names(size) + ["mixed"]:
        logits, vlogits = _launch(size, name)
        policy, value = hep.epilogue32(logits, vlogits)
        assert _passes(policy, value, logits, vlogits), name


@pytest.mark.parametrize("fault", list(hep.FAULTS))
@pytest.mark.parametrize("size", hep.SIZES)
def test_each_fault_violates_the_criterion_on_its_named_cases(size, fault):
    for name in FAULT_TABLE[fault]:
        logits, vlogits = _launch(size, "equal0" if name == "nan-prefill" else name)
        policy, value = hep.epilogue32(logits, vlogits, fault)
        assert not _passes(policy, value, logits, vlogits), (fault, name)
        if fault == "value_takes_neighbour_exp":
            assert hep.within(policy, logits) and not hep.within(value, vlogits), name       # the value check alone sees it


def test_faults_of_average_weight_pass_the_absolute_check_on_a_flat_19x19_row():
    """Why the criterion is relative.  A flat 19x19 row (probabilities near 1/362 = 2.8e-3) under the 1e-4 absolute check:
    a sum without its last term moves every probability by 7.7e-6; an entry A - 1 that is not stored keeps what the previous
    launch of the same positions left in the staging buffer, the same value; two boards with each other's 1 / sum are off by
    the relative difference of two sums of 362 near-equal terms.  All three pass.  (The whole-stripe form of the first fault
    leaves out 42 of 362 terms and moves a flat row by 3.6e-4: the absolute check sees it on a flat row - and on no peaked one.)"""
    A = hep.actions(19)
    rs = np.random.RandomState(19)
    logits = hep._q(rs.standard_normal((2, A)) * 0.05)                 # two near-flat rows that differ ...
    logits[:, 0] = 0.25                                                # ... with the same maximum (1 / sum is relative to it)
    vlogits = np.zeros((2, 3), np.float32)
    want = hep.softmax64(logits)
    earlier, _ = hep.epilogue32(logits, vlogits)                       # what an earlier launch stored
    for fault in ("sum_omits_last_entry", "pass_not_stored", "boards_exchange_inv"):
        policy, value = hep.epilogue32(logits, vlogits, fault, prefill=earlier[:, -1:])
        assert np.abs(policy - want).max() < OLD_TOL, fault
        if fault != "pass_not_stored":
            assert not hep.within(policy, logits), fault
    policy, _ = hep.epilogue32(logits, vlogits, "pass_not_stored")     # (what the new test does: outputs prefilled with NaN)
    assert not hep.within(policy, logits)
    policy, _ = hep.epilogue32(logits, vlogits, "sum_omits_last_stripe")
    assert np.abs(policy - want).max() > 3 * OLD_TOL


def test_criterion_arithmetic():
    """rel_err ignores entries under 2^-100, tiny_ok holds them to [0, 2^-99], NaN never passes."""
    logits = np.array([0.0, -100.0], np.float32)
    p64 = hep.softmax64(logits)
    assert p64[1] < hep.TINY
    assert hep.within(np.array([1.0, 0.0], np.float32), logits)
    assert hep.within(np.array([1.0, 2.0 ** -99], np.float32), logits)
    assert not hep.within(np.array([1.0, 2.0 ** -98], np.float32), logits)
    assert not hep.within(np.array([1.0, -0.5], np.float32), logits)
    assert not hep.within(np.array([1.0, np.nan], np.float32), logits)
    assert not hep.within(np.array([np.nan, 0.0], np.float32), logits)
    assert not hep.within(np.array([1.0 + 8 * hep.ULP, 0.0], np.float32), logits)
    assert hep.bound(0.0) == 4 * 2.0 ** -23 and hep.bound(1e-6) == 4e-6 + 4 * 2.0 ** -23
