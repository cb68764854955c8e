"""The HIP training step against an fp64 reference of the same step, tensor by tensor, with the ReLU masks pinned.

    python tools/train_step_precision.py [--out FILE]     # needs a GPU; writes profiles/train_step_precision.json

What is held to what (tests/test_gpu_train_precision.py asserts it, tests/test_train_precision_host.py gives it teeth on the
CPU): every tensor the step saves or leaves behind - the 13 convolution outputs Z_l, the 7 block outputs Y_b, the 13
D_l = dL/d(batch-norm output), the heads' hD and dL/dlogits, the three losses, every momentum buffer (= gradient + weight decay
on a first step), every parameter and every running statistic after the step - against oracle.train_ref.reference_step at
fp64:  err(x) = max|x - x64| / max|x64|,  err_hip <= FACTOR[family] * err_ref32 + 4 * 2^-23,  where err_ref32 is the same
reference run at fp32 on the CPU (an honest fp32 implementation's error) and the floor is fp32 rounding of the tensor's largest
value.

The mask rule.  A pre-activation within rounding of zero may land on either side of a ReLU in two correct implementations, and
one flipped element moves gradients by percents.  So the masks are taken out of the comparison: per case, fp64 and fp32 run with
their natural masks; margin = 4 * max|o32 - o64| per ReLU; the device's masks are read back (Y_b > 0 for the stem and the block
outputs, hact > 0 for the heads, D_l != 0 for the conv1 ReLUs whose activation is never materialised - D_l is the back-propagated
gradient times the very mask the kernels rebuild) and may differ from the fp64 natural ones only where |o64| < margin, at most
MAX_FLIPS elements a step; then fp64 and fp32 are rerun with the device's masks, and those runs are compared.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_train import make_case  # noqa: E402  (seeded parameter tables only)
from oracle import train_ref  # noqa: E402
from tamago_amd.nn.learn import BLOCKS  # noqa: E402

FLOOR = 4 * 2.0 ** -23
MAX_FLIPS = 16              # device masks against the fp64 natural ones, per step
MAX_FLIPS_REF32 = 8         # the fp32 CPU run alone
# err_hip <= FACTOR * err_ref32 + FLOOR per tensor family.  4 is the forward test's factor (tests/test_gpu_net_precision.py); a
# family measured above it on healthy code gets twice its measured ratio, at most 16, with the reason in DESIGN.md §4.5.
# mom.tiny = the momentum buffers (gradients) of the tensors of one to three elements (TINY below): err_ref32 of such a tensor
# is one draw of the fp32 CPU run's rounding, not a maximum over many elements - over the cases the same scalar's err_ref32
# spreads from 7e-8 to 1.3e-5 - so the ratio to it is as noisy.  Measured (profiles/train_step_precision.json): the largest factor
# a tiny tensor needs is 8.79 (value_head.bn_layer.bias at 19x19 batch 65: err_hip 1.47e-6 against an err_ref32 of 1.13e-7 - a sum
# of 23 465 gradients accumulated per thread, then by butterfly, where the CPU sums pairwise); twice that is above the cap of 16.
# Every other family needs at most 3.2 and stays at 4.
FACTOR = {"Z": 4.0, "Y": 4.0, "D": 4.0, "head": 4.0, "loss": 4.0, "mom.conv": 4.0, "mom.bn": 4.0, "mom.head": 4.0,
          "mom.tiny": 16.0, "param": 4.0, "stat": 4.0}

# id: board size, batch, objective; `same_class`: every board has one value class; `history`: preloaded momentum (not a first step).
# 9x9:  2 = the minimum (fewer boards than statistic replicas and than head_fc_grad's batch slices), 17 = the replica index wraps,
#       65 = 64 weight-gradient chunks of which one walks two boards, 260 = 256 workgroups of which four walk two boards, chunks of
#       four and five boards.   19x19: 3 and 64 = four workgroups per board (64: exactly 256 of them), 65 = one, ragged chunks.
# (Seeds of the three large cases: picked among eight for few pre-activations at a ReLU threshold - the fp32 CPU run flips 0 to 1
# mask elements on them, 0 to 11 over the eight - so that its cap of MAX_FLIPS_REF32 keeps headroom on a host that rounds otherwise.)
CASES = {
    "s9-b2-rl": dict(size=9, batch=2, mode="rl", seed=11),
    "s9-b17-sl-oneclass": dict(size=9, batch=17, mode="sl", seed=12, same_class=True),
    "s9-b65-rl": dict(size=9, batch=65, mode="rl", seed=13),
    "s9-b65-sl-history": dict(size=9, batch=65, mode="sl", seed=14, history=True),
    "s9-b260-sl": dict(size=9, batch=260, mode="sl", seed=37),
    "s19-b3-sl": dict(size=19, batch=3, mode="sl", seed=16),
    "s19-b64-rl": dict(size=19, batch=64, mode="rl", seed=31),
    "s19-b65-sl": dict(size=19, batch=65, mode="sl", seed=35),
}
# a second step from the device's own state after a first one, on another batch
SECOND_STEP_CASES = {
    "s9-b17-rl-step2": dict(size=9, batch=17, mode="rl", seed=21),
    "s19-b3-rl-step2": dict(size=19, batch=3, mode="rl", seed=22),
}
LR = 0.01


# ------------------------------------------------------------------------------------------------ inputs
def make_batch(size, batch, mode, seed, same_class=False):
    """Planes binary in four channels and uniform in two; policy rows = normalised gamma draws with about half the entries
    exactly 0, the last row one-hot, the one before it (batch >= 3) 1 on PASS only, in RL mode the one before that (batch >= 4)
    summing to 0.5; value classes: all three (batch >= 3) unless `same_class`."""
    rng = np.random.RandomState(seed)
    A = size * size + 1
    planes = np.empty((batch, 6, size, size), np.float32)
    planes[:, :4] = rng.randint(0, 2, size=(batch, 4, size, size))
    planes[:, 4:] = rng.uniform(size=(batch, 2, size, size))
    pol = rng.gamma(0.3, size=(batch, A))
    pol[rng.uniform(size=(batch, A)) < 0.5] = 0.0
    pol[np.arange(batch), rng.randint(0, A, batch)] += 0.1           # (no empty row)
    pol /= pol.sum(1, keepdims=True)
    pol[batch - 1] = 0.0
    pol[batch - 1, rng.randint(0, A - 1)] = 1.0
    if batch >= 3:
        pol[batch - 2] = 0.0
        pol[batch - 2, A - 1] = 1.0
    if batch >= 4 and mode == "rl":
        pol[batch - 3] *= 0.5
    val = rng.randint(0, 3, batch).astype(np.int64)
    if same_class:
        val[:] = 1
    elif batch >= 3:
        val[:3] = [0, 1, 2]
    return torch.from_numpy(planes), torch.from_numpy(pol.astype(np.float32)), torch.from_numpy(val)


def make_momentum(state, seed):
    """Random momentum buffers of the size gradients have (max|g| 0.003 .. 0.25 on these networks)."""
    rng = np.random.RandomState(seed)
    return {k: torch.from_numpy(rng.normal(0, 0.02, tuple(v.shape)).astype(np.float32)) for k, v in state.items()
            if not k.endswith(("running_mean", "running_var"))}


def make_inputs(spec):
    """(state, momentum or None, batch) of a case."""
    state, _ = make_case(seed=3000 + spec["seed"], SIZE=spec["size"])
    momentum = make_momentum(state, 4000 + spec["seed"]) if spec.get("history") else None
    return state, momentum, make_batch(spec["size"], spec["batch"], spec["mode"], 5000 + spec["seed"], spec.get("same_class", False))


# ------------------------------------------------------------------------------------------- the references
def reference(state, momentum, batch, mode, dtype, masks=None):
    torch.set_num_threads(4)               # (as tests/test_train_step.py: the fp32 run's summation order does not follow the host)
    return train_ref.reference_step(state, *batch, mode=mode, lr=LR, dtype=dtype, masks=masks, momentum=momentum)


def natural_runs(state, momentum, batch, mode):
    """fp64 and fp32 with their own masks -> (pre64, masks64, masks32, margin): what the mask rule needs, nothing else kept."""
    r64 = reference(state, momentum, batch, mode, torch.float64)
    pre64, masks64 = r64["pre"], r64["masks"]
    del r64
    r32 = reference(state, momentum, batch, mode, torch.float32)
    margin = {k: 4.0 * float((r32["pre"][k].double() - pre64[k]).abs().max()) for k in train_ref.RELU_NAMES}
    return pre64, masks64, r32["masks"], margin


def mask_disagreements(masks, pre64, masks64, margin):
    """(elements where `masks` differ from the fp64 natural masks, those of them with |o64| >= margin: none are allowed)."""
    total = outside = 0
    for k in train_ref.RELU_NAMES:
        diff = masks[k].reshape(masks64[k].shape) != masks64[k]
        total += int(diff.sum())
        outside += int((diff & (pre64[k].abs() >= margin[k])).sum())
    return total, outside


def check_masks(masks, pre64, masks64, margin, cap=MAX_FLIPS):
    total, outside = mask_disagreements(masks, pre64, masks64, margin)
    assert outside == 0, f"{outside} ReLU mask elements differ from the fp64 masks outside the rounding margin"
    assert total <= cap, f"{total} ReLU mask elements differ from the fp64 masks (at most {cap})"
    return total


# ------------------------------------------------------------------------------------------------ comparing
TINY = ("policy_head.bn_layer.weight", "policy_head.bn_layer.bias", "value_head.bn_layer.weight", "value_head.bn_layer.bias",
        "value_head.fc_layer.bias")          # tensors of one to three elements


def family_of(name):
    kind, _, key = name.partition(":")
    if kind != "mom":
        return kind
    if key in TINY:
        return "mom.tiny"
    if ".bn" in key or key.startswith("bn_layer"):
        return "mom.bn"
    return "mom.head" if "head" in key else "mom.conv"


def tensors_of(run):
    """name -> tensor, for every quantity that is compared; names are 'family:what'."""
    out = {}
    for l in range(13):
        out[f"Z:{l}"], out[f"D:{l}"] = run["Z"][l], run["D"][l]
    for b in range(BLOCKS + 1):
        out[f"Y:{b}"] = run["Y"][b]
    out["head:hD"], out["head:dlog"] = run["hD"], run["dlog"]
    for i, k in enumerate(("total", "policy", "value")):
        out[f"loss:{k}"] = run["losses"][i]
    for k, v in run["mom"].items():
        out[f"mom:{k}"] = v
    for k, v in run["param"].items():
        out[f"param:{k}"] = v
    for k, v in run["stat"].items():
        out[f"stat:{k}"] = v
    return out


def err(x, x64):
    scale = float(x64.abs().max())
    return float((x.double().reshape(x64.shape) - x64).abs().max()) / (scale if scale > 0 else 1.0)


def compare(dev, ref64, ref32):
    """Rows (name, family, err_ref32, err_hip, bound) for every tensor of the step."""
    d, r64, r32 = tensors_of(dev), tensors_of(ref64), tensors_of(ref32)
    assert set(d) == set(r64) == set(r32)
    rows = []
    for name in r64:
        e32, ehip = err(r32[name], r64[name]), err(d[name], r64[name])
        rows.append((name, family_of(name), e32, ehip, FACTOR[family_of(name)] * e32 + FLOOR))
    return rows


def violations(rows):
    return [r for r in rows if not r[3] <= r[4]]


def by_family(rows):
    """family -> the tensor with the largest err_hip / bound: {err_ref32, err_hip, ratio = err_hip / err_ref32,
    needed = the factor that tensor needs under the floor, tensor}."""
    out = {}
    for name, fam, e32, ehip, bound in rows:
        cur = out.get(fam)
        if cur is None or ehip / bound > cur["_load"]:
            out[fam] = {"tensor": name, "err_ref32": e32, "err_hip": ehip, "ratio": ehip / e32 if e32 > 0 else None,
                        "needed": max(ehip - FLOOR, 0.0) / e32 if e32 > 0 else None, "_load": ehip / bound}
    for v in out.values():
        del v["_load"]
    return out


def report(rows):
    return "\n".join(f"  {fam:9s} {v['tensor']:45s} err_ref32 {v['err_ref32']:.3e} err_hip {v['err_hip']:.3e} "
                     f"needed factor {v['needed'] if v['needed'] is None else round(v['needed'], 2)}" for fam, v in by_family(rows).items())


# --------------------------------------------------------------------------------------------------- device
def to_momentum_list(state, momentum):
    return [momentum[k] for k in state if k in momentum]


def device_step(hip, state_keys, batch, mode):
    """One HipTrainer.step and everything it saved or left behind, in reference_step's layout (fp32 CPU tensors)."""
    from tamago_amd import lib as tl
    dev = hip.device
    size, bsz, P = hip.board_size, hip.batch_size, hip.board_size ** 2
    hip.take_losses()                                          # (accumulators start from zero)
    hip.step(*(a.to(dev) for a in batch), mode=mode, lr=LR)
    losses = hip.take_losses()
    lib = tl.load()

    def read(which, index, shape):
        out = np.zeros(shape, dtype=np.float32)
        tl.check(lib.tg_trainer_debug_read(hip.handle, which, index, out.ctypes.data), "tg_trainer_debug_read")
        return torch.from_numpy(out)

    def board(which, index):
        return read(which, index, (bsz, P, 64)).permute(0, 2, 1).reshape(bsz, 64, size, size)

    run = {"Z": [board(0, l) for l in range(13)], "Y": [board(1, b) for b in range(BLOCKS + 1)],
           "D": [board(2, l) for l in range(13)]}
    hact = read(4, 0, (bsz, 3, size, size))
    run["hD"] = read(5, 0, (bsz, P, 4)).permute(0, 2, 1)[:, :3].reshape(bsz, 3, size, size)
    run["dlog"] = read(6, 0, (bsz, P + 4))
    run["losses"] = torch.tensor([losses["loss"], losses["policy"], losses["value"]], dtype=torch.float64)
    masks = {"stem": run["Y"][0] > 0, "policy_head": hact[:, :2] > 0, "value_head": hact[:, 2:] > 0}
    for b in range(BLOCKS):
        masks[f"blocks.{b}.conv1"] = run["D"][1 + 2 * b] != 0
        masks[f"blocks.{b}.out"] = run["Y"][b + 1] > 0
    run["masks"] = masks
    now = hip.state_dict()
    trainable = [k for k in state_keys if not k.endswith(("running_mean", "running_var"))]
    run["param"] = {k: now[k] for k in trainable}
    run["stat"] = {k: now[k] for k in state_keys if k.endswith(("running_mean", "running_var"))}
    run["mom"] = dict(zip(trainable, hip.momentum_buffers()))
    return run


def pinned_comparison(state, momentum, batch, mode, dev_run):
    """The mask rule, then the rows of the device's step against fp64 / fp32 rerun with the device's masks; (rows, flips)."""
    pre64, masks64, _, margin = natural_runs(state, momentum, batch, mode)
    flips = check_masks(dev_run["masks"], pre64, masks64, margin)
    del pre64, masks64
    ref64 = reference(state, momentum, batch, mode, torch.float64, dev_run["masks"])
    ref32 = reference(state, momentum, batch, mode, torch.float32, dev_run["masks"])
    return compare(dev_run, ref64, ref32), flips


def run_case(spec):
    """A case of CASES on the device: (rows, flips)."""
    from tamago_amd.nn import learn
    state, momentum, batch = make_inputs(spec)
    hip = learn.HipTrainer(torch.device("cuda", 0), spec["size"], spec["batch"], state)
    try:
        if momentum is not None:
            hip.load_momentum_buffers(to_momentum_list(state, momentum))
        dev_run = device_step(hip, list(state), batch, spec["mode"])
    finally:
        hip.close()
    return pinned_comparison(state, momentum, batch, spec["mode"], dev_run)


def run_second_step_case(spec):
    """Step 1, then step 2 on another batch held to the reference started from the device's own state after step 1."""
    from tamago_amd.nn import learn
    state, _, first = make_inputs(spec)
    second = make_batch(spec["size"], spec["batch"], spec["mode"], 6000 + spec["seed"])
    hip = learn.HipTrainer(torch.device("cuda", 0), spec["size"], spec["batch"], state)
    try:
        hip.step(*(a.to(hip.device) for a in first), mode=spec["mode"], lr=LR)
        mid = {k: v for k, v in hip.state_dict().items() if k in state}
        momentum = dict(zip([k for k in state if not k.endswith(("running_mean", "running_var"))], hip.momentum_buffers()))
        dev_run = device_step(hip, list(state), second, spec["mode"])
    finally:
        hip.close()
    moved = max(float((mid[k] - state[k]).abs().max()) for k in state)
    assert moved > 1e-3, moved                                  # step 1 happened
    return pinned_comparison(mid, momentum, second, spec["mode"], dev_run)


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_precision.json"))
    args = ap.parse_args()
    record = {"bound": "err_hip <= FACTOR[family] * err_ref32 + 4 * 2^-23, err(x) = max|x - x64| / max|x64|",
              "factor": FACTOR, "cases": {}}
    for runner, cases in ((run_case, CASES), (run_second_step_case, SECOND_STEP_CASES)):
        for name, spec in cases.items():
            rows, flips = runner(spec)
            print(f"{name}: {flips} mask elements differ from fp64, {len(violations(rows))} tensors above their bound")
            print(report(rows), flush=True)
            record["cases"][name] = {"mask_flips": flips, "violations": [r[0] for r in violations(rows)], "families": by_family(rows)}
    path = args.out
    with open(path, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
