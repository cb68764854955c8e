#!/usr/bin/env python3
"""The policy and value softmax of every forward kernel family (want_logits = 0) against an fp64 softmax of the same logits.

The heads' epilogue - row maximum, expf, wave-reduced sum, one reciprocal, the stores, the three-way value softmax - exists in
six hand-written copies with their own lane striping (run_heads in net_device.h, two in split_common.h, the w1d one,
dualnet_heads19_fin_kernel, dualnet_heads19_kernel<16>).  The rest of the suite holds logits to fp64 and probabilities to 1e-4
absolute, which at 19x19 is 3.6 % of an average probability.  Here the probabilities are held relative to their own size.

Exactly known logits.  A network whose two FC weight matrices are zero puts out the FC biases as logits in every family (the
fp32 paths compute fmaf(h, 0, bias), the MFMA paths fmaf(0, down2x, 0 * down2) + bias, the 19x19 heads
((0 + 0) + (0 + 0)) + bias), whatever the tower (oracle.net.make_state_dict(size, 7, 1.5), unchanged) hands them.  CASES are
bias rows in multiples of 2^-6: l - max is exact in fp32, so the epilogue alone is measured.

Criterion (per row).  p64 = fp64 softmax of the fp32 logits.  Over the entries with p64 >= 2^-100:
    err = max |p - p64| / p64,      err_hip <= 4 * err_ref32 + 4 * 2^-23,
err_ref32 = the same error of softmax32 below (numpy float32: subtract the maximum, exp, sum in sequence, one reciprocal, one
product).  The factor is the project's (forward_precision_ladder.bound), the floor is train_step_precision's: the half-ulp
operations of a correctly rounded epilogue (expf <= 1 ulp, the sum, the reciprocal, the product), with margin; the library is
built without fast-math and with -ffp-contract=off.  Entries with p64 < 2^-100 must be finite, >= 0 and <= 2^-99; such entries
exist only in the tower* cases (all but index k) and in wide (the odd indices) - asserted on the reference (condition()), never
on a device output.

What is guarded in front of the epilogue.  The 9x9 f16 kernels (run_heads_x32, run_heads_mfma) write the two policy 1x1-convolution
features as f16 pieces; a feature at or beyond kHeadRangeLimit (60 000, split_common.h) raises the f16 range flag - and the group's
bit where the kernel keeps a bitmap - and the exact kernel redoes the group, like a tower layer output beyond its limit or an input
plane value beyond it.  The value features, and both heads at 13x13 and 19x19, are fp32.  tests/test_gpu_net_magnitude.py holds
that; the cases here stay far inside (the tower is make_state_dict's: features below 60).

FAULTS are numpy fp32 restatements of the epilogue with one defect each; tests/test_head_epilogue_host.py shows that the
criterion catches each of them on named cases and that the 1e-4 absolute check does not.

GPU box:  python tools/head_epilogue_precision.py [--out profiles/head_epilogue_precision.json]
tests/test_gpu_head_epilogue.py takes cases, reference and criterion from here."""
import argparse
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np
import torch

import forward_precision_ladder as fpl  # noqa: E402

SIZES = (9, 13, 19)
FLOOR = 4 * 2.0 ** -23                  # train_step_precision.FLOOR
FACTOR = 4.0                            # forward_precision_ladder.bound
TINY = 2.0 ** -100                      # below it an entry is only held to [0, 2 * TINY]
ULP = 2.0 ** -23
BIG_19 = 529                            # 33 * 16 + 1: dualnet_heads19_kernel<16> with a one-board last workgroup
QUANTUM = 2.0 ** -6


def actions(size):
    return size * size + 1


def last_stripe(A):
    """First index of the 64-lane stripe that holds PASS (index A - 1)."""
    return 64 * ((A - 1) // 64)


def _q(x):
    """Round to multiples of 2^-6 (exact in fp32 at these magnitudes)."""
    return (np.round(np.asarray(x, np.float64) / QUANTUM) * QUANTUM).astype(np.float32)


def peak_indices(A):
    return sorted({k for k in (0, 63, 64, 127, 128, A - 2, A - 1) if 0 <= k < A})


def tower_indices(A):
    return (0, 64, A - 1)


def policy_cases(A):
    """name -> fp32 bias row [A], in a fixed order."""
    out = {"equal0": np.zeros(A, np.float32), "equal1e4": np.full(A, 10000.0, np.float32)}
    for k in peak_indices(A):
        row = np.full(A, -20.0, np.float32)
        row[k] = 3.0
        out[f"peak{k}"] = row
    row = np.full(A, -40.0, np.float32)
    row[last_stripe(A):] = 0.0
    out["tail"] = row
    ramp = _q(-64.0 * np.arange(A) / (A - 1))
    out["ramp"], out["rampup"] = ramp, ramp[::-1].copy()
    for scale in (1, 8, 20):
        draws = np.random.RandomState(1000 * A + scale).standard_normal(A)
        out[f"normal{scale}"] = _q(np.clip(draws * scale, -32.0, 32.0))
    for k in tower_indices(A):
        row = np.full(A, -60.0, np.float32)
        row[k] = 60.0
        out[f"tower{k}"] = row
    row = np.full(A, -100.0, np.float32)
    row[0::2] = 100.0
    out["wide"] = row
    return out


VALUE_CASES = tuple(
    [(0.0, 0.0, 0.0), (1e4, 1e4, 1e4)] + sorted(itertools.permutations((30.0, 0.0, -30.0)), reverse=True)
    + [(90.0, 0.0, -90.0), (-90.0, 0.0, 90.0), (QUANTUM, 0.0, -QUANTUM)])


def cases(size):
    """[(name, policy bias [A], value bias [3])]: policy case i carries value case i mod n - every value case rides on a network
    that is loaded anyway."""
    pol = policy_cases(actions(size))
    assert len(pol) >= len(VALUE_CASES)
    return [(name, row, np.asarray(VALUE_CASES[i % len(VALUE_CASES)], np.float32)) for i, (name, row) in enumerate(pol.items())]


def case_names(size):
    return list(policy_cases(actions(size)))


def may_have_tiny(name):
    return name.startswith("tower") or name == "wide"


# ---------------------------------------------------------------------------------------------- references and criterion
def softmax64(logits):
    """fp64 softmax of fp32 logits, rows along the last axis."""
    l = np.asarray(logits, np.float32).astype(np.float64)
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax32(logits):
    """The plain fp32 evaluation: subtract the maximum, exp, sum in sequence, one reciprocal, one product."""
    l = np.asarray(logits, np.float32)
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    s = np.cumsum(e, axis=-1, dtype=np.float32)[..., -1:]                # (np.sum adds pairwise; cumsum adds in sequence)
    return e * (np.float32(1.0) / s)


def rel_err(p, p64):
    """Per row: max |p - p64| / p64 over the entries with p64 >= TINY (0 for a row without any).  NaN counts as infinite."""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(p64 >= TINY, np.abs(p - p64) / p64, 0.0)
    rel = np.where(np.isnan(rel), np.inf, rel)
    return rel.max(axis=-1)


def tiny_ok(p, p64):
    """Per row: every entry with p64 < TINY is finite, >= 0 and <= 2 * TINY."""
    p = np.asarray(p, np.float64)
    small = p64 < TINY
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p) & (p >= 0.0) & (p <= 2.0 * TINY)
    return (ok | ~small).all(axis=-1)


def bound(err_ref32):
    return FACTOR * err_ref32 + FLOOR


def judge(p, logits):
    """Probabilities `p` [..., n] against the logits they were made from -> dict of per-row arrays: err, err_ref32, bound,
    ok (the criterion, tiny entries included)."""
    p64 = softmax64(logits)
    err, ref = rel_err(p, p64), rel_err(softmax32(logits), p64)
    return {"err": err, "err_ref32": ref, "bound": bound(ref), "ok": (err <= bound(ref)) & tiny_ok(p, p64)}


def within(p, logits):
    return bool(np.all(judge(p, logits)["ok"]))


def worst(verdict):
    """(err, err_ref32) of the row closest to (or farthest beyond) its bound."""
    err, ref = np.atleast_1d(verdict["err"]), np.atleast_1d(verdict["err_ref32"])
    with np.errstate(invalid="ignore"):
        i = int(np.argmax(np.where(np.isfinite(err), err / bound(ref), np.inf)))
    return float(err[i]), float(ref[i])


def condition(size):
    """What the criterion presupposes, asserted on the references alone: entries below TINY exist only in tower* (all but
    index k) and wide (the odd indices), the value rows have them only under (+-90, 0, -+90), and the fp32 reference is itself
    within the criterion's reach (3 ulp on the equal, peak, tail and ramp cases, 19 ulp on the normal ones)."""
    A = actions(size)
    for name, row, vrow in cases(size):
        p64 = softmax64(row)
        small = np.flatnonzero(p64 < TINY)
        if name.startswith("tower"):
            k = int(name[5:])
            assert small.tolist() == [a for a in range(A) if a != k], name
        elif name == "wide":
            assert small.tolist() == list(range(1, A, 2)), name
        else:
            assert small.size == 0, name
            ref = float(rel_err(softmax32(row), p64))
            assert ref < (19 if name.startswith("normal") else 3) * ULP, (name, ref)
        assert tiny_ok(softmax32(row), p64), name
        v64 = softmax64(vrow)
        assert (v64 < TINY).any() == (abs(float(vrow[0])) == 90.0), (name, vrow)
        assert tiny_ok(softmax32(vrow), v64) and float(rel_err(softmax32(vrow), v64)) < 3 * ULP, (name, vrow)


# ------------------------------------------------------------------------------------------------------- fault models
def epilogue32(logits, vlogits, fault=None, prefill=np.nan):
    """A numpy fp32 restatement of the kernels' epilogue on a workgroup's boards: logits [G, A], value logits [G, 3] ->
    (policy [G, A], value [G, 3]).  Per board, 64 lanes walk the row in stripes of 64 (a = lane, lane + 64, ...): the maximum,
    the per-lane sums of exp(l - m) reduced over the lanes, inv = 1 / sum, the stores of exp(l - m) * inv into an output that
    holds `prefill`; the value softmax by lanes 0..2.  `fault`: None or one of FAULTS."""
    assert fault is None or fault in FAULTS, fault
    l = np.asarray(logits, np.float32)
    G, A = l.shape
    cut = last_stripe(A)
    f32 = np.float32
    lane_rows = -(-A // 64) * 64
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = (l[:, :cut] if fault == "max_omits_last_stripe" else l).max(axis=1, keepdims=True)
        if fault == "no_max_subtraction":
            m = np.zeros_like(m)
        e = np.exp(l - m).astype(f32)
        summed = e.copy()
        if fault == "sum_omits_last_stripe":
            summed[:, cut:] = 0
        if fault == "sum_omits_last_entry":
            summed[:, A - 1:] = 0
        lanes = np.zeros((G, lane_rows), f32)
        lanes[:, :A] = summed
        per_lane = np.cumsum(lanes.reshape(G, -1, 64), axis=1, dtype=f32)[:, -1, :]         # a lane's stripes in sequence
        o = 32
        while o:                                                                              # the xor butterfly over the lanes
            per_lane = per_lane + per_lane[:, np.arange(64) ^ o]
            o >>= 1
        inv = (f32(1.0) / per_lane[:, :1]).astype(f32)
        if fault == "boards_exchange_inv":
            swap = np.arange(G) ^ 1
            swap[swap >= G] = G - 1
            inv = inv[swap]
        policy = np.full((G, A), prefill, f32)
        stored = A - 1 if fault == "pass_not_stored" else A
        policy[:, :stored] = (e * inv)[:, :stored]
        v = np.asarray(vlogits, f32)
        ev = np.exp(v - v.max(axis=1, keepdims=True)).astype(f32)
        es = (ev[:, 0] + ev[:, 1] + ev[:, 2])[:, None]
        value = (ev[:, [1, 2, 0]] if fault == "value_takes_neighbour_exp" else ev) / es
    return policy, value.astype(f32)


# name -> what it restates.  sum_omits_last_entry is the one-term form of the first (a sum loop bounded at A - 1): the term of
# average weight that the 1e-4 absolute check cannot see at any board size.
FAULTS = {
    "sum_omits_last_stripe": "the sum of exponentials leaves out the stripe that holds PASS",
    "sum_omits_last_entry": "the sum of exponentials leaves out entry A - 1",
    "max_omits_last_stripe": "the row maximum leaves out the stripe that holds PASS",
    "no_max_subtraction": "exp(l) in place of exp(l - max)",
    "pass_not_stored": "entry A - 1 is not stored: the output keeps what the buffer held",
    "boards_exchange_inv": "boards 2i and 2i + 1 of a workgroup use each other's 1 / sum",
    "value_takes_neighbour_exp": "value class c puts out the exponential of class c + 1",
}


def mixed_rows(size):
    """The `mixed` launch of the host test: the rows of every case without tiny entries, one per board - boards of a workgroup
    differ, as on a real network."""
    picked = [(row, vrow) for name, row, vrow in cases(size) if not may_have_tiny(name)]
    return np.stack([r for r, _ in picked]), np.stack([v for _, v in picked])


# ------------------------------------------------------------------------------------------------------------ device
def zero_fc_state(size, policy_bias, value_bias):
    """make_state_dict(size, 7, 1.5) with both FC weight matrices zero and the given FC biases."""
    from oracle.net import make_state_dict
    sd = dict(make_state_dict(size, 7, 1.5))
    for head, bias in (("policy_head", policy_bias), ("value_head", value_bias)):
        sd[f"{head}.fc_layer.weight"] = torch.zeros_like(sd[f"{head}.fc_layer.weight"])
        sd[f"{head}.fc_layer.bias"] = torch.from_numpy(np.asarray(bias, np.float32).copy())
    return sd


def launches(size):
    """[(family id, batch, algo, shared, exact, kernel name)] of a size: every family at its batch - among them the 19x19
    default path at BIG_19 boards."""
    assert fpl.family(f"19-pair-{BIG_19}")[2:4] == (BIG_19, None)
    return [(fid, batch, algo, shared, exact, name) for fid, s, batch, algo, shared, exact, name in fpl.FAMILIES if s == size]


def forward(net, x, algo, shared, want_logits):
    """(policy, value, kernel name) of one host-side forward under TG_FWD_ALGO = algo."""
    with fpl.environment(TG_FWD_ALGO=algo, TG_FWD_BANDS=None):
        net.set_shared_device(shared)
        try:
            name = net._lib.tg_net_kernel_name(net.handle, x.shape[0]).decode()
            pol, val = net.inference_with_policy_logits(x) if want_logits else net.inference(x)
        finally:
            net.set_shared_device(False)
    return pol, val, name


def forward_prefilled(net, x, algo, shared):
    """forward_device(out=...) into outputs that hold NaN -> (policy, value) on the host."""
    b, A = x.shape[0], actions(net.board_size)
    out = (torch.full((b, A), float("nan"), device="cuda"), torch.full((b, 3), float("nan"), device="cuda"))
    with fpl.environment(TG_FWD_ALGO=algo, TG_FWD_BANDS=None):
        net.set_shared_device(shared)
        try:
            net.forward_device(x.cuda(), out=out)
            torch.cuda.synchronize()
        finally:
            net.set_shared_device(False)
    return out[0].cpu(), out[1].cpu()


def measure_case(net, size, launch, planes, row, vrow):
    """One crafted network on one launch -> record (figures of the worst board) and the verdicts."""
    label, batch, algo, shared, exact, want_name = launch
    reps = (batch + planes.shape[0] - 1) // planes.shape[0]
    x = planes.repeat(reps, 1, 1, 1)[:batch].contiguous()
    logits, _, name = forward(net, x, algo, shared, True)
    pol, val, _ = forward(net, x, algo, shared, False)
    lg = logits.numpy()
    vp = judge(pol.numpy(), lg)
    vv = judge(val.numpy(), np.broadcast_to(vrow, (batch, 3)))
    (pe, pr), (ve, vr) = worst(vp), worst(vv)
    return {"family": label, "kernel": name, "kernel_as_expected": name == want_name, "batch": batch,
            "logits_equal_bias": bool(np.array_equal(lg, np.broadcast_to(row, lg.shape))),
            "policy_err_hip": pe, "policy_err_ref32": pr, "policy_bound": bound(pr), "policy_ok": bool(vp["ok"].all()),
            "value_err_hip": ve, "value_err_ref32": vr, "value_bound": bound(vr), "value_ok": bool(vv["ok"].all()),
            "range_fallbacks": net.range_fallbacks(), "band_timeouts": net.band_timeouts()}


def measure(sizes=SIZES):
    records = []
    for size in sizes:
        planes = fpl.plane_sets(size)["uniform"]
        for name, row, vrow in cases(size):
            net = fpl.make_net(size, zero_fc_state(size, row, vrow))
            for launch in launches(size):
                rec = {"size": size, "case": name, **measure_case(net, size, launch, planes, row, vrow)}
                records.append(rec)
                print(json.dumps(rec), flush=True)
    return records


def summary(records):
    """Per launch the largest figures over the cases, and the cases that miss."""
    out = {}
    for r in records:
        s = out.setdefault(r["family"], {"policy_err_hip_max": 0.0, "policy_err_hip_max_case": None, "value_err_hip_max": 0.0,
                                         "policy_err_hip_over_floor_max": 0.0, "cases": 0, "misses": []})
        s["cases"] += 1
        if r["policy_err_hip"] > s["policy_err_hip_max"]:
            s["policy_err_hip_max"], s["policy_err_hip_max_case"] = r["policy_err_hip"], r["case"]
        s["policy_err_hip_over_floor_max"] = max(s["policy_err_hip_over_floor_max"], r["policy_err_hip"] / FLOOR)
        s["value_err_hip_max"] = max(s["value_err_hip_max"], r["value_err_hip"])
        if not (r["policy_ok"] and r["value_ok"] and r["logits_equal_bias"]):
            s["misses"].append(r["case"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "head_epilogue_precision.json"))
    args = ap.parse_args()
    for size in SIZES:
        condition(size)
    records = measure()
    doc = {"what": "policy and value softmax of every forward kernel family on crafted logits (zero FC weights: logits = FC "
                   "biases) against the fp64 softmax; figures of the worst board of each launch; relative errors",
           "criterion": "err_hip <= 4 * err_ref32 + 4 * 2^-23 over entries with p64 >= 2^-100", "floor": FLOOR,
           "summary": summary(records)}
    with open(args.out, "w") as f:                                    # (the summary indented, one record per line)
        f.write(json.dumps(doc, indent=1)[:-2] + ',\n "records": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in records) + "\n ]\n}\n")
    return 0 if all(not s["misses"] for s in doc["summary"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
