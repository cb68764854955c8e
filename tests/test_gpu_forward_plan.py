"""The forward dispatch's choice, pinned: which kernel a launch gets, and the FLOP count, peak and operand format
bench.py prices it with, against tests/golden/forward_plan.json (tools/gen_golden_forward_plan.py, recorded before the
name, the FLOP figure and the launch sequence came from one plan).  Nothing is launched."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden_forward_plan as gen  # noqa: E402


def test_every_recorded_choice_holds(golden_dir):
    import torch
    with open(os.path.join(golden_dir, "forward_plan.json")) as f:
        fix = json.load(f)
    c = torch.cuda.get_device_properties(0).multi_processor_count
    assert c == fix["num_cus"], (f"this device has {c} CUs, tests/golden/forward_plan.json was recorded on {fix['num_cus']}: the "
                                 "launch sizes around the thresholds are multiples of the CU count - regenerate the fixture "
                                 "(tools/gen_golden_forward_plan.py) on the parent commit on this device")
    assert tuple(fix["columns"]) == gen.COLUMNS
    rows = {tuple(r[:6]): tuple(r[6:]) for r in fix["rows"]}
    cases = gen.cases(c)
    assert len(rows) == len(fix["rows"]) and set(rows) == set(cases)
    nets = gen.make_networks()
    wrong = []
    for case in cases:
        got = gen.query(nets, case)          # (name and dtype: strings; FLOPs and peak: doubles, compared exactly)
        if got != rows[case]:
            wrong.append((case, got, rows[case]))
    assert not wrong, f"{len(wrong)} of {len(cases)} rows differ (case, got, recorded); the first: {wrong[:5]}"
