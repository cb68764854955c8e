#!/usr/bin/env python3
"""Static count of a kernel's emitted instructions by class (the whole kernel: every wave role, every path), as JSON: what a
change to the arithmetic of a kernel removed or added, before any run.  fp64 VALU work is split out: the division sequence
(v_div_scale / v_div_fmas / v_div_fixup / v_rcp), square roots (v_rsq / v_sqrt), fused multiply-adds, the rest.

    python tools/kernel_instruction_mix.py build/obj/search.hip.o select_puct_pipe_kernelILi9E"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_check import disassemble, kernels  # noqa: E402


def classify(op):
    if op in ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32"): return "lane"
    if op.startswith("v_") and "_f64" in op:
        if op.startswith(("v_div_", "v_rcp_")): return "valu_f64_div"
        if op.startswith(("v_rsq_", "v_sqrt_")): return "valu_f64_sqrt"
        if op.startswith("v_fma_"): return "valu_f64_fma"
        return "valu_f64_other"
    if op.startswith("v_"): return "valu"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_load", "buffer_load", "flat_load", "scratch_load")): return "vmem_load"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")): return "vmem_store_atomic"
    if op.startswith(("s_load", "s_buffer_load")): return "smem_load"
    if op == "s_nop": return "nop"
    if op == "s_waitcnt": return "wait"
    if op == "s_barrier": return "barrier"
    if op.startswith("s_cbranch") or op == "s_branch": return "branch"
    if op.startswith("s_"): return "salu"
    return "other"


def mix(obj, flt):
    out = {}
    for name, ins in kernels(disassemble(obj)).items():
        if flt not in name:
            continue
        counts = {}
        for _addr, op, _args, _tgt in ins:
            c = classify(op)
            counts[c] = counts.get(c, 0) + 1
        counts["total"] = len(ins)
        out[name] = dict(sorted(counts.items()))
    return out


if __name__ == "__main__":
    print(json.dumps(mix(sys.argv[1], sys.argv[2]), indent=1))
