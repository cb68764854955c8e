#!/usr/bin/env python3
"""Per-slice issue cost of the 9x9 forward tower, read from the EMITTED gfx950 code (no GPU needed).

The three-board tower of `dualnet_fwd_w1d_kernel` is hand-scheduled as "slices": one `v_mfma` plus whatever rides along
until the next one, fenced by `sched_barrier(0)`.  A row of the board is 72 slices (rows 0 and 8: 48), a layer 9 rows, and
the block loop's body holds two layers (conv1 = parity 0, conv2 + residual = parity 1): 18 emitted rows, executed
6 times per group = 108 rows.  This tool cuts that loop body at consecutive MFMAs and prints, per slice, the
instructions between the MFMAs by class and a modelled cost; per row and per layer it prints sum(max(16, cost)).

    python tools/slice_costs.py build/obj/net_forward_w1d.hip.o w1d_kernelILi3ELb0 [--json out.json] [--rows]

The model (one wave per SIMD, `v_mfma_f32_16x16x32_f16`; constants in cycles):

    MFMA   8    an MFMA holds the SIMD's vector issue for 8 of its 16 cycles
    VALU   4    v_add_f32 / v_fma_f32 / v_max3_f32 / conversions / register moves / lane operations
    LDS    4    one issue slot per ds_read / ds_write (the transfer of a 16-byte store's data runs beside the issue)
    VMEM  16    a 1 KB weight request: four waves' requests pass the CU's vector L1 at 64 B per clock
    NOP    4    per slot; `s_nop k` is k + 1 slots
    s_waitcnt, s_barrier, scalar ALU: printed, priced 0 (scalar issue is a port of its own; a wait is priced as satisfied)

Issue costs add; a gap between two MFMAs runs max(16, 8 + its riders).  What follows a row's last MFMA up to the next
row's first one (the wait at the top of row 1, the cursor bookkeeping at the end of a layer) is counted to that last slice.
A model of issue slots, not of time: LDS latency, bank conflicts and the clock are not in it.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_check import disassemble, kernels

COST = {"mfma": 8, "valu": 4, "lds": 4, "vmem": 16, "nop": 4, "wait": 0, "barrier": 0, "salu": 0}
MFMA_CYCLES = 16
ROW_SLICES = [48, 72, 72, 72, 72, 72, 72, 72, 48]     # MFMAs of rows 0 .. 8 of a layer
LAYERS_IN_BODY = 2                                       # the block loop's body: conv1, conv2
BLOCKS = 6                                               # executions of the body per group
CLASSES = ["valu", "lds", "vmem", "nop", "wait", "barrier", "salu"]


def classify(op):
    if op.startswith("v_mfma"): return "mfma"
    if op.startswith("v_"): return "valu"                # lane operations and v_accvgpr moves included
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")): return "vmem"
    if op == "s_nop": return "nop"
    if op == "s_waitcnt": return "wait"
    if op == "s_barrier": return "barrier"
    return "salu"                                        # scalar ALU, scalar memory, branches


def tower_body(insts):
    """The instructions of the block loop's body: the span of the backward branch that holds exactly the MFMAs of two layers."""
    want = LAYERS_IN_BODY * sum(ROW_SLICES)
    index = {a: i for i, (a, _, _, _) in enumerate(insts)}
    for i, (addr, op, _, tgt) in enumerate(insts):
        if tgt is None or tgt >= addr or tgt not in index:
            continue
        span = insts[index[tgt]:i + 1]
        if sum(1 for _, o, _, _ in span if o.startswith("v_mfma")) == want:
            return span
    raise RuntimeError(f"no loop with {want} MFMAs found: not the three-board tower?")


def slices_of(body):
    """-> [{'ops': [(mnemonic, operands), ..]}] one per MFMA: the instructions behind it up to the next MFMA."""
    out = []
    for _, op, args, _ in body:
        if op.startswith("v_mfma"):
            out.append([])
        elif out:
            out[-1].append((op, args))
    return out


def slice_record(ops):
    rec = {c: 0 for c in CLASSES}
    rec["requests"] = 0
    cost = COST["mfma"]
    for op, args in ops:
        c = classify(op)
        rec[c] += 1
        if c == "nop":
            slots = int(args.strip() or 0) + 1
            rec["nop_slots"] = rec.get("nop_slots", 0) + slots
            cost += COST["nop"] * slots
        else:
            cost += COST[c]
        if c == "vmem" and op.startswith("global_load_dwordx4"):
            rec["requests"] += 1
    rec.setdefault("nop_slots", 0)
    rec["cost"] = cost
    return rec


def analyse(obj, flt):
    """-> {'kernel': name, 'rows': [{'layer': parity, 'row': y, 'slices': [...], 'mfma_floor', 'issue_sum', 'model'}], 'layers': [...]}"""
    found = [(n, ins) for n, ins in kernels(disassemble(obj)).items() if flt in n]
    if len(found) != 1:
        raise RuntimeError(f"{len(found)} kernels match {flt!r}: {[n for n, _ in found]}")
    name, insts = found[0]
    sl = slices_of(tower_body(insts))
    rows, k = [], 0
    for layer in range(LAYERS_IN_BODY):
        for y, n in enumerate(ROW_SLICES):
            recs = [slice_record(ops) for ops in sl[k:k + n]]
            k += n
            rows.append({"layer": layer, "row": y, "slices": recs, "mfma_floor": MFMA_CYCLES * n,
                         "issue_sum": sum(r["cost"] for r in recs),
                         "model": sum(max(MFMA_CYCLES, r["cost"]) for r in recs)})
    layers = [{"layer": l, "mfma_floor": sum(r["mfma_floor"] for r in rows if r["layer"] == l),
               "issue_sum": sum(r["issue_sum"] for r in rows if r["layer"] == l),
               "model": sum(r["model"] for r in rows if r["layer"] == l)} for l in range(LAYERS_IN_BODY)]
    return {"kernel": name, "constants": COST, "emitted_rows": len(rows), "rows_per_group": len(rows) * BLOCKS,
            "rows": rows, "layers": layers}


def summary(res):
    """What profiles/ keeps: per row the totals and the slices that overflow, not every slice."""
    return {"kernel": res["kernel"], "constants": res["constants"], "emitted_rows": res["emitted_rows"],
            "rows_per_group": res["rows_per_group"], "layers": res["layers"],
            "rows": [{"layer": r["layer"], "row": r["row"], "slices": len(r["slices"]), "mfma_floor": r["mfma_floor"],
                      "issue_sum": r["issue_sum"], "model": r["model"],
                      "valu": sum(s["valu"] for s in r["slices"]), "lds": sum(s["lds"] for s in r["slices"]),
                      "vmem": sum(s["vmem"] for s in r["slices"]), "nop_slots": sum(s["nop_slots"] for s in r["slices"]),
                      "cost_by_slice": [s["cost"] for s in r["slices"]]} for r in res["rows"]]}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    obj, flt = args[0], args[1]
    res = analyse(obj, flt)
    print(res["kernel"])
    print("constants:", " ".join(f"{k}={v}" for k, v in COST.items()), "| a gap runs max(16, cost)")
    for r in res["rows"]:
        print(f"layer parity {r['layer']} row {r['row']}: {len(r['slices'])} slices, MFMAs alone {r['mfma_floor']}, "
              f"sum of issue costs {r['issue_sum']}, modelled sum(max(16, cost)) {r['model']}")
        if "--rows" in sys.argv:
            continue
        print("   m  " + " ".join(f"{c:>7s}" for c in CLASSES) + "    cost")
        for m, s in enumerate(r["slices"]):
            nop = f"{s['nop']}({s['nop_slots']})" if s["nop"] else "0"
            cells = [nop if c == "nop" else str(s[c]) for c in CLASSES]
            print(f"  {m:2d}  " + " ".join(f"{v:>7s}" for v in cells) + f"  {s['cost']:6d}" + ("  *" if s["cost"] > MFMA_CYCLES else ""))
    for l in res["layers"]:
        print(f"layer parity {l['layer']}: MFMAs alone {l['mfma_floor']}, sum of issue costs {l['issue_sum']}, modelled {l['model']}")
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(summary(res), f, indent=1)


if __name__ == "__main__":
    main()
