#!/usr/bin/env python3
"""Every forward kernel family against the oracle's fp64 forward, on networks whose mid-block channel scales spread over 2^S
(oracle.net.rescale_mid_channels: the same function, bit for bit in fp32 and fp64, at every S).

One JSON line per (size, family, S): err_hip = max |logits - fp64 logits|, err_ref = the oracle's own fp32 forward against
the same fp64 forward, the bound 4 * err_ref + 1e-6 of the project's accuracy contract, the kernel that ran, the channel
spreads the load-time guard of the f16 towers saw (tg_net_channel_spread) and the fallback counters.  The rungs are run
twice: with the guard as the library has it ("guard": true) and, in a child process, with the guard switched off by its debug
knob (TG_DEBUG_KNOBS=1 TG_FWD_SPREAD_GUARD=0; "guard": false) - the second is what the limits in csrc/net_forward.hip are
read from.

GPU box:  python tools/forward_precision_ladder.py [--rungs 0,8,12,16,20] > profiles/forward_precision_ladder.json
          python tools/forward_precision_ladder.py --magnitude > profiles/forward_magnitude_ladder.json
(--magnitude: activations going UP instead - oracle.net.scale_tower / scale_head, the f16 range guard's side; see below.)

tests/test_gpu_net_precision.py takes the family table, the plane sets and the measuring code from here."""
import argparse
import contextlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np
import torch

RUNGS = (0, 8, 12, 16, 20)
POSITIONS = 16                      # distinct positions per plane set; larger launches tile them
VALUE_TOL = 1e-4                    # value softmax (the API hands out no value logits)

SPLIT13 = "dualnet_fwd_split_kernel<13, 1, f16x2> + dualnet_fwd_wino8_kernel<13, 1> (range guard, per board)"
# id, board size, launch size, TG_FWD_ALGO (None: the default), shared device, exact fp32, kernel of a 256-CU device
FAMILIES = (
    ("9-w1d-1", 9, 6, "w1d", False, False, "dualnet_fwd_w1d_kernel<1>"),
    ("9-w1d-3", 9, 300, "w1d", False, False, "dualnet_fwd_w1d_kernel<3>"),
    ("9-split16-1", 9, 6, "split16", False, False, "dualnet_fwd_split_kernel<9, 1, f16x2>"),
    ("9-split16-3", 9, 300, "split16", False, False, "dualnet_fwd_split_kernel<9, 3, f16x2>"),
    ("9-wino-1", 9, 6, "wino", False, True, "dualnet_fwd_wino8_kernel<9, 1>"),
    ("9-wino-2", 9, 300, "wino", False, True, "dualnet_fwd_wino8_kernel<9, 2>"),
    ("9-direct-1", 9, 6, "direct", False, True, "dualnet_fwd_kernel<9, 1>"),
    ("9-direct-300", 9, 300, "direct", False, True, "dualnet_fwd_kernel<9, 1>"),
    ("13-default", 13, 5, None, False, True, "dualnet_fwd_kernel<13, 1>"),
    ("13-split16", 13, 5, "split16", False, False, SPLIT13),
    ("19-pair", 19, 3, None, False, False, "dualnet_fwd_w1dband_kernel + dualnet_heads19_kernel"),
    # (more than 512 boards: dualnet_heads19_kernel<16> in place of the part + fin pair; 33 * 16 + 1 - a one-board last workgroup)
    ("19-pair-529", 19, 529, None, False, False, "dualnet_fwd_w1dband_kernel + dualnet_heads19_kernel"),
    ("19-band4", 19, 3, "split16", False, False, "dualnet_fwd_band_kernel<4>"),
    ("19-band2", 19, 100, "split16", False, False, "dualnet_fwd_band_kernel<2>"),
    ("19-split16-shared", 19, 3, "split16", True, False, "dualnet_fwd_split_kernel<19, 1, f16x2>"),
    ("19-wino", 19, 3, "wino", False, True, "dualnet_fwd_wino8_kernel<19, 1, global scratch>"),
    ("19-direct", 19, 3, "direct", False, True, "dualnet_fwd_kernel<19, 1>"),
)
FAMILY_IDS = tuple(f[0] for f in FAMILIES)


def family(fid):
    return FAMILIES[FAMILY_IDS.index(fid)]


def is_exact_kernel(name):
    """The exact-fp32 kernels' names (tg_net_kernel_name); an f16 launch names its f16 kernel first."""
    return name.startswith("dualnet_fwd_wino8_kernel") or name.startswith("dualnet_fwd_kernel")


def plane_sets(size):
    """name -> fp32 planes [POSITIONS, 6, size, size].  randint: what the rest of the suite feeds (exact in f16: the stem's low
    activation piece is zero); uniform, thirds: not exact in f16; feat: recorded feature planes (tests/golden/feat_s*.npz)."""
    from tests.helpers import load_npz
    rs = np.random.RandomState(100 + size)
    shape = (POSITIONS, 6, size, size)
    sets = {
        "randint": rs.randint(-1, 2, size=shape).astype(np.float32),
        "uniform": rs.random_sample(shape).astype(np.float32),
        "thirds": (rs.randint(0, 4, size=shape).astype(np.float64) / 3.0).astype(np.float32),
        "feat": load_npz(f"feat_s{size}.npz")["planes"][:POSITIONS].astype(np.float32),
    }
    assert sets["feat"].shape == shape
    return {k: torch.from_numpy(v) for k, v in sets.items()}


def reference(sd, planes):
    """(fp64 logits, fp64 value softmax, fp32 logits, fp32 value softmax) of the oracle, float64 tensors."""
    from oracle.net import forward_logits
    with torch.no_grad():
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        l64, v64 = forward_logits(sd64, planes.double())
        l32, v32 = forward_logits(sd, planes)
    return l64, torch.softmax(v64, dim=1), l32.double(), torch.softmax(v32, dim=1).double()


@contextlib.contextmanager
def environment(**values):
    """Set (a string) or unset (None) process environment variables for the block."""
    saved = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_net(size, sd):
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), size)
    net.load_state_dict(sd)
    return net


def run(net, batch, algo, shared, planes):
    """Forward `planes`, tiled to a launch of `batch` positions, with TG_FWD_ALGO = algo (None: unset) -> (logits, value
    softmax, kernel name), the outputs cut to the positions of the first copy."""
    n = min(batch, planes.shape[0])
    reps = (batch + planes.shape[0] - 1) // planes.shape[0]
    x = planes.repeat(reps, 1, 1, 1)[:batch].contiguous()
    with environment(TG_FWD_ALGO=algo, TG_FWD_BANDS=None):
        net.set_shared_device(shared)
        try:
            name = net._lib.tg_net_kernel_name(net.handle, batch).decode()
            logits, value = net.inference_with_policy_logits(x)
        finally:
            net.set_shared_device(False)
    return logits[:n], value[:n], name


def run_family(net, fid, planes):
    _, _, batch, algo, shared, _, _ = family(fid)
    return run(net, batch, algo, shared, planes)


def errors(logits, value, ref):
    """err_hip, err_ref, value softmax error against fp64 - over the positions that `logits` holds."""
    n = logits.shape[0]
    l64, v64, l32, _ = ref
    return (float((logits.double() - l64[:n]).abs().max()), float((l32[:n] - l64[:n]).abs().max()),
            float((value.double() - v64[:n]).abs().max()))


def bound(err_ref):
    return 4.0 * err_ref + 1e-6


# ------------------------------------------------------------------------------------------------ magnitudes going UP
# oracle.net.scale_tower / scale_head: the same function bit for bit with the tower's activations, or one head's features, 2^k
# times as large.  tests/test_net_magnitude_host.py and tests/test_gpu_net_magnitude.py take everything below from here.
TOWER_RUNGS = (0, 4, 6, 7, 8, 9, 10, 12, 16)
HEAD_RUNGS = (4, 8, 12, 13, 14, 16, 20)
F16_MAX = 65504.0
HEAD_FREE = 16000.0                 # a policy feature below this must not cost a redo; at or above F16_MAX it must
BAND = 2.0 ** -10                   # no guarded quantity of a chosen case lies within limit * (1 +- BAND)
BASES = {9: ((7, 1.5),), 13: ((7, 1.5),), 19: ((7, 1.5), (3, 1.4))}      # (seed, gain) of make_state_dict; the first is the precision suite's
# f16 family -> (the tower guard's limit: kWsRangeLimit of w1d_common.h or the split kernels' 60 000; boards per redone unit, 0 =
# the launch: what the kernel marks in the group bitmap; the heads write the policy features as f16 pieces)
GUARDS = {
    "9-w1d-1": (16000.0, 1, True), "9-w1d-3": (16000.0, 3, True),
    "9-split16-1": (60000.0, 0, True), "9-split16-3": (60000.0, 0, True),
    "13-split16": (60000.0, 1, False),
    "19-pair": (16000.0, 1, False), "19-pair-529": (16000.0, 1, False),
    "19-band4": (60000.0, 0, False), "19-band2": (60000.0, 0, False), "19-split16-shared": (60000.0, 0, False),
}
LAST_ROW_CHANNEL = 5                # oracle.net.spike_last_row's channel in the tests
LARGE = ("9-w1d-3", "9-split16-3", "19-pair-529", "19-band2")          # these take the first tripping rungs only


def classify(maxima, fid):
    """(must, may) per position, bool arrays: the family's guard must / may send the position to the exact kernel.  Tower: hot
    (must) when an input plane value, the stem or a layer output reaches limit * (1 + BAND), cold below limit * (1 - BAND).  Heads that write f16 feature
    pieces: must from F16_MAX on, free below HEAD_FREE, either in between.  A quantity inside a band: ValueError."""
    limit, _, head = GUARDS[fid]
    tower = np.maximum(np.maximum(maxima["planes"], maxima["stem"]), maxima["layers"].max(axis=0))
    edges = [(tower, limit)] + ([(maxima["policy_head"], F16_MAX), (maxima["policy_head"], HEAD_FREE)] if head else [])
    for q, edge in edges:
        inside = (q >= edge * (1 - BAND)) & (q < edge * (1 + BAND))
        if inside.any():
            raise ValueError(f"{fid}: position {int(np.argmax(inside))} has {q[inside][0]!r} inside the band around {edge}")
    must = tower >= limit
    may = np.zeros_like(must)
    if head:
        must = must | (maxima["policy_head"] >= F16_MAX)
        may = (maxima["policy_head"] >= HEAD_FREE) & ~must
    return must, may


def predicted_redo(must, may, fid):
    """must, may: classify()'s answer for each position of ONE launch of the family, in launch order [batch].  -> (redone [batch]
    bool: the whole units - groups of the kernel's bitmap, or the launch - that hold a must position; undecided [batch] bool: the
    units with a may and no must position).  The counters of the launch must say redone.sum() positions, plus any of undecided."""
    batch, unit = family(fid)[2], GUARDS[fid][1] or family(fid)[2]
    assert len(must) == batch and len(may) == batch
    redone, undecided = np.zeros(batch, bool), np.zeros(batch, bool)
    for lo in range(0, batch, unit):
        if must[lo:lo + unit].any():
            redone[lo:lo + unit] = True
        elif may[lo:lo + unit].any():
            undecided[lo:lo + unit] = True
    return redone, undecided


def run_launch(net, fid, x):
    """One launch of the family on exactly the positions x (as many as the family's launch has) -> (logits, value softmax, kernel
    name, launches redone, positions redone): every position's output and what the fallback counters moved by."""
    _, _, batch, algo, shared, _, _ = family(fid)
    assert x.shape[0] == batch, (fid, x.shape)
    before = (net.range_fallbacks(), net.range_fallback_positions())
    logits, value, name = run(net, batch, algo, shared, x)
    return logits, value, name, net.range_fallbacks() - before[0], net.range_fallback_positions() - before[1]


def magnitude_net(base, ladder_name, k):
    from oracle.net import scale_head, scale_tower
    return scale_tower(base, k) if ladder_name == "tower" else scale_head(base, ladder_name, k)


def magnitude_rungs(ladder_name):
    return TOWER_RUNGS if ladder_name == "tower" else HEAD_RUNGS


def magnitude_ladders():
    """--magnitude: the three ladders for every f16 family on the first base network of its size, one JSON line per rung."""
    from oracle.net import layer_maxima, make_state_dict
    for size in (9, 13, 19):
        seed, gain = BASES[size][0]
        base = make_state_dict(size, seed, gain)
        planes = plane_sets(size)["randint"]
        ref = reference(base, planes)
        for name in ("tower", "policy_head", "value_head"):
            for k in magnitude_rungs(name):
                sd = magnitude_net(base, name, k)
                maxima = layer_maxima(sd, planes)
                net = make_net(size, sd)
                for fid in GUARDS:
                    if family(fid)[1] != size:
                        continue
                    before = (net.range_fallbacks(), net.range_fallback_positions())
                    logits, value, kernel = run_family(net, fid, planes)
                    err_hip, err_ref, err_val = errors(logits, value, ref)
                    n = logits.shape[0]                                   # (the launch's distinct positions: the maxima are theirs)
                    print(json.dumps({
                        "size": size, "family": fid, "launch": family(fid)[2], "ladder": name, "k": k, "kernel": kernel,
                        "finite": bool(torch.isfinite(logits).all()),
                        "err_hip": err_hip, "err_ref": err_ref, "bound": bound(err_ref), "err_hip_over_bound": err_hip / bound(err_ref),
                        "err_value_softmax": err_val,
                        "largest_tower_activation": float(max(maxima["stem"][:n].max(), maxima["layers"][:, :n].max())),
                        "largest_policy_feature": float(maxima["policy_head"][:n].max()),
                        "largest_value_feature": float(maxima["value_head"][:n].max()),
                        "range_fallbacks": net.range_fallbacks() - before[0],
                        "range_fallback_positions": net.range_fallback_positions() - before[1]}), flush=True)


def ladder(rungs, guard_on):
    from oracle.net import make_state_dict, rescale_mid_channels
    for size in (9, 13, 19):
        base = make_state_dict(size, 7, 1.5)
        planes = plane_sets(size)["randint"]
        ref = reference(base, planes)
        for S in rungs:
            net = make_net(size, rescale_mid_channels(base, S, seed=1))
            for fid in FAMILY_IDS:
                if family(fid)[1] != size or (family(fid)[5] and not guard_on):       # (exact kernels: no guard to switch off)
                    continue
                logits, value, name = run_family(net, fid, planes)
                err_hip, err_ref, err_val = errors(logits, value, ref)
                print(json.dumps({
                    "size": size, "family": fid, "S": S, "guard": guard_on, "kernel": name, "err_hip": err_hip, "err_ref": err_ref,
                    "bound": bound(err_ref), "within_bound": err_hip < bound(err_ref), "err_value_softmax": err_val,
                    "spread_w1d": net._lib.tg_net_channel_spread(net.handle, 0),
                    "spread_split": net._lib.tg_net_channel_spread(net.handle, 1),
                    "range_fallbacks": net.range_fallbacks(), "range_fallback_positions": net.range_fallback_positions(),
                    "band_timeouts": net.band_timeouts()}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rungs", default=",".join(str(S) for S in RUNGS), help="comma-separated exponents S")
    ap.add_argument("--guard-off", action="store_true", help="this process was started with the guard's debug knob set")
    ap.add_argument("--magnitude", action="store_true", help="the tower, policy-head and value-head ladders (activations going up) instead")
    args = ap.parse_args()
    if args.magnitude:
        return magnitude_ladders()
    rungs = [int(v) for v in args.rungs.split(",")]
    if args.guard_off:
        return ladder(rungs, False)
    ladder(rungs, True)
    import subprocess                                            # (the knob is read once per process: a fresh child)
    env = dict(os.environ, TG_DEBUG_KNOBS="1", TG_FWD_SPREAD_GUARD="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--rungs", args.rungs, "--guard-off"], env=env, check=True)


if __name__ == "__main__":
    main()
