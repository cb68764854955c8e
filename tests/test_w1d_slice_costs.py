"""Structure of the emitted three-board tower of dualnet_fwd_w1d_kernel<3, false>, read with tools/slice_costs.py from the
object tamago_amd.build makes (CPU test: cross-compiles for gfx950, needs no GPU).

The tower's riders are placed by hand, slice by slice (a slice = one MFMA and what follows it up to the next MFMA); the
placement only holds if hipcc emits it as written.  Three facts are asserted; the modelled cycle totals are printed, not
asserted - they are a model.

* Rows.  The block loop's body holds two layers of nine rows: 18 emitted rows of 72 slices, 48 in rows 0 and 8; a group
  executes the body six times, 108 rows.
* In rows 1-7 no slice carries a weight request together with any other vector-memory or LDS instruction.
* In rows 1-7 no slice carries more than three vector-issue instructions (VALU, LDS, vector memory) besides its MFMA,
  with the exceptions listed in EXCEPTIONS - at most two per row."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import slice_costs  # noqa: E402

# (layer parity, slice) -> reason.  Slices 16 and 17 carry a residual read (layers with a residual: parity 1) with the step
# of its cursor, and a cell read with its address XOR or cursor step: the eight cell reads need eight slices outside the four
# ahead of the row barrier's wait, the exchange traffic, the epilogue's arithmetic and the transform's tail, and a row has six.
EXCEPTIONS = {(1, 16): "residual read + cursor step + cell read + address", (1, 17): "residual read + cursor step + cell read + address"}


@pytest.fixture(scope="module")
def tower():
    from tamago_amd import build
    build.build(verbose=False)
    return slice_costs.analyse(os.path.join(build.OBJ_DIR, "net_forward_w1d.hip.o"), "dualnet_fwd_w1d_kernelILi3ELb0EE")


def test_rows_and_slices(tower):
    rows = tower["rows"]
    assert len(rows) == 18 and tower["rows_per_group"] == 108
    for r in rows:
        assert len(r["slices"]) == (48 if r["row"] in (0, 8) else 72), (r["layer"], r["row"])
    for l in tower["layers"]:
        print(f"layer parity {l['layer']}: MFMAs alone {l['mfma_floor']}, sum of issue costs {l['issue_sum']}, modelled {l['model']}")
    for r in rows:
        print(f"  parity {r['layer']} row {r['row']}: sum of issue costs {r['issue_sum']}, modelled {r['model']}")


def test_a_weight_request_shares_its_slice_with_no_other_memory_instruction(tower):
    bad = [(r["layer"], r["row"], m, s) for r in tower["rows"] if 1 <= r["row"] <= 7
           for m, s in enumerate(r["slices"]) if s["requests"] and (s["vmem"] > s["requests"] or s["lds"] or s["requests"] > 1)]
    assert not bad, bad
    # 16-byte loads in the body: a layer's 48 fragments, both parities, and the second layer's shift vector (behind the first
    # layer's last MFMA; the first layer's is loaded in front of the body's first MFMA, in no slice)
    assert sum(s["requests"] for r in tower["rows"] for s in r["slices"]) == 2 * 48 + 1


def test_at_most_three_vector_issue_riders_a_slice(tower):
    per_row = {}
    bad = []
    for r in tower["rows"]:
        if not 1 <= r["row"] <= 7:
            continue
        for m, s in enumerate(r["slices"]):
            n = s["valu"] + s["lds"] + s["vmem"]
            if n <= 3:
                continue
            if (r["layer"], m) in EXCEPTIONS:
                per_row[(r["layer"], r["row"])] = per_row.get((r["layer"], r["row"]), 0) + 1
            else:
                bad.append((r["layer"], r["row"], m, n))
    assert not bad, bad
    assert all(v <= 2 for v in per_row.values()), per_row
