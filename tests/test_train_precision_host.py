"""CPU side of the training-step precision check (tools/train_step_precision.py, tests/test_gpu_train_precision.py): the fp64
reference step is pinned to the reference project's vectors and to the existing fp32 steps, the inputs of every case flip few
masks, and the bound has teeth - the fp32 CPU run stands in for the device, passes undamaged and fails with each of four
defects the older tolerances let through."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import train_step_precision as tsp  # noqa: E402
from gen_golden_train import make_case, sample_of  # noqa: E402

from oracle import train_ref  # noqa: E402
from tamago_amd.nn import learn  # noqa: E402
from tamago_amd.nn.network.dual_net import state_dict_keys  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "train_s9.npz"))
TOL_LOSS, TOL_PARAM = 2e-5, 2e-6             # tests/test_train_step.py: TOL["cpu"]


def _trainable(state):
    return [k for k in state if not k.endswith(("running_mean", "running_var"))]


@pytest.mark.parametrize("mode", ["rl", "sl"])
def test_fp64_reference_step_matches_the_reference_projects_vectors(mode):
    """Natural masks, step 1 of tests/golden/train_s9.npz: losses and the sampled parameters."""
    state, batches = make_case()
    run = train_ref.reference_step(state, *(torch.from_numpy(a) for a in batches[0]), mode=mode, lr=0.01)
    np.testing.assert_allclose(run["losses"].numpy(), GOLD[f"{mode}_losses"][0], rtol=0, atol=TOL_LOSS)
    moved = 0.0
    for key in _trainable(state):
        got = sample_of(run["param"][key].numpy())
        np.testing.assert_allclose(got, GOLD[f"{mode}/step1/{key}"], rtol=0, atol=TOL_PARAM, err_msg=key)
        moved = max(moved, float(np.abs(got - sample_of(state[key].numpy())).max()))
    assert moved > 1e-3


@pytest.mark.parametrize("mode", ["rl", "sl"])
def test_fp32_instance_is_the_existing_autograd_step(mode):
    """rl_train_step / sl_train_step + torch.optim.SGD (what tests/test_train_step.py compares the kernels with) against the
    reference at fp32: parameters, momentum buffers, statistics and losses agree within rounding of each tensor's largest value
    times the factor two fp32 evaluations of a gradient may be apart (each within err_ref32 of fp64), and the existing step
    passes the device's bound against fp64."""
    state, batches = make_case()
    batch = tuple(torch.from_numpy(a) for a in batches[0])
    net = train_ref.TrainableDualNet(torch.device("cpu"), 9, state).train()
    opt = learn.make_optimizer(net, 0.01)
    part = (train_ref.rl_train_step if mode == "rl" else train_ref.sl_train_step)(net, opt, *batch)
    r64 = train_ref.reference_step(state, *batch, mode=mode, lr=0.01, dtype=torch.float64)
    r32 = train_ref.reference_step(state, *batch, mode=mode, lr=0.01, dtype=torch.float32)
    assert all(r32["param"][k].dtype == torch.float32 for k in r32["param"])
    assert tsp.mask_disagreements(r32["masks"], r64["pre"], r64["masks"], {k: 0.0 for k in train_ref.RELU_NAMES})[0] == 0
    now = net.state_dict()
    theirs = {"loss": torch.tensor([part["loss"], part["policy"], part["value"]], dtype=torch.float64),
              "param": {k: now[k] for k in _trainable(state)},
              "mom": {k: opt.state[net.t[k]]["momentum_buffer"] for k in _trainable(state)},
              "stat": {k: now[k] for k in state if k not in _trainable(state)}}
    for fam, mine64, mine32 in (("param", r64["param"], r32["param"]), ("mom", r64["mom"], r32["mom"]), ("stat", r64["stat"], r32["stat"])):
        for k in mine64:
            e32, e_theirs = tsp.err(mine32[k], mine64[k]), tsp.err(theirs[fam][k], mine64[k])
            assert e_theirs <= 4 * e32 + tsp.FLOOR, (fam, k, e32, e_theirs)
            assert tsp.err(theirs[fam][k], mine32[k].double()) <= 2 * e32 + tsp.FLOOR, (fam, k)
    for i in range(3):
        assert tsp.err(theirs["loss"][i], r64["losses"][i]) <= 4 * tsp.err(r32["losses"][i], r64["losses"][i]) + tsp.FLOOR, i


@pytest.mark.parametrize("name", list(tsp.CASES))
def test_inputs_of_every_case_flip_few_masks_between_fp32_and_fp64(name):
    """The fp32 CPU run alone: its masks differ from the fp64 ones only inside the margin and in at most 8 elements - the
    device's allowance of 16 is not an artefact of inputs that sit on ReLU thresholds."""
    spec = tsp.CASES[name]
    state, momentum, batch = tsp.make_inputs(spec)
    pre64, masks64, masks32, margin = tsp.natural_runs(state, momentum, batch, spec["mode"])
    flips = tsp.check_masks(masks32, pre64, masks64, margin, cap=tsp.MAX_FLIPS_REF32)
    print(name, "flips", flips)
    pol = batch[1]
    assert float((pol == 0).float().mean()) > 0.3 and bool((pol.sum(1) - 1).abs().max() < 1e-5 or spec["mode"] == "rl")


# ---------------------------------------------------------------------------------------------------- teeth
TEETH_CASE = "s9-b65-sl-history"
_teeth = {}


def _stand_in():
    """The fp32 CPU run with its own masks as the device; fp64 / fp32 pinned to those masks as the references."""
    if not _teeth:
        spec = tsp.CASES[TEETH_CASE]
        state, momentum, batch = tsp.make_inputs(spec)
        pre64, masks64, masks32, margin = tsp.natural_runs(state, momentum, batch, spec["mode"])
        ref64 = tsp.reference(state, momentum, batch, spec["mode"], torch.float64, masks32)
        ref32 = tsp.reference(state, momentum, batch, spec["mode"], torch.float32, masks32)
        _teeth.update(spec=spec, state=state, momentum=momentum, batch=batch, pre64=pre64, masks64=masks64, masks32=masks32,
                      margin=margin, ref64=ref64, ref32=ref32)
    return _teeth


def _device_copy(run):
    dev = dict(run)
    for k in ("mom", "param", "stat"):
        dev[k] = dict(run[k])
    return dev


def _bad(dev):
    t = _stand_in()
    return {r[0] for r in tsp.violations(tsp.compare(dev, t["ref64"], t["ref32"]))}


def test_undamaged_stand_in_passes():
    t = _stand_in()
    tsp.check_masks(t["masks32"], t["pre64"], t["masks64"], t["margin"], cap=tsp.MAX_FLIPS_REF32)
    assert _bad(_device_copy(t["ref32"])) == set()


def test_teeth_one_board_left_out_of_a_weight_gradient():
    """(a) blocks.2.conv1 (layer 5) without the last of 65 boards - the second board of the one two-board chunk."""
    t = _stand_in()
    run, key, b = t["ref32"], "blocks.2.conv1.weight", t["spec"]["batch"] - 1
    share = torch.nn.grad.conv2d_weight(run["Y"][2][b:b + 1], run["grad"][key].shape, run["dZ"][5][b:b + 1], padding=1)
    whole = torch.nn.grad.conv2d_weight(run["Y"][2], run["grad"][key].shape, run["dZ"][5], padding=1)
    assert tsp.err(whole, run["grad"][key].double()) < 1e-5 and float(share.abs().max()) > 0     # the shares add up to the gradient
    dev = _device_copy(run)
    dev["mom"][key] = run["mom"][key] - share
    dev["param"][key] = run["param"][key] + tsp.LR * (1 + learn.MOMENTUM) * share
    assert f"mom:{key}" in _bad(dev)


def test_teeth_one_mask_element_flipped_and_not_pinned():
    """(b) one element of blocks.3.conv1's mask, ten margins away from zero: the mask rule refuses it, and against
    references that do not know of it the gradients break the bound."""
    t = _stand_in()
    name = "blocks.3.conv1"
    o = t["pre64"][name].abs().flatten()
    o = torch.where(o > 10 * t["margin"][name], o, torch.full_like(o, float("inf")))
    masks = dict(t["masks32"])
    flipped = masks[name].clone().flatten()
    flipped[int(o.argmin())] ^= True
    masks[name] = flipped.reshape(masks[name].shape)
    with pytest.raises(AssertionError, match="outside the rounding margin"):
        tsp.check_masks(masks, t["pre64"], t["masks64"], t["margin"])
    dev = tsp.reference(t["state"], t["momentum"], t["batch"], t["spec"]["mode"], torch.float32, masks)
    bad = _bad(dev)
    assert "D:7" in bad and "mom:blocks.3.conv1.weight" in bad, sorted(bad)


def test_teeth_plain_momentum_instead_of_nesterov():
    """(c) w -= lr * buf."""
    t = _stand_in()
    dev = _device_copy(t["ref32"])
    for k in dev["param"]:
        dev["param"][k] = t["state"][k] - tsp.LR * dev["mom"][k]
    bad = _bad(dev)
    assert {f"param:{k}" for k in dev["param"]} <= bad and not any(n.startswith("mom:") for n in bad), sorted(bad)


def test_teeth_one_replica_missing_from_a_batch_norm_backward_sum():
    """(d) blocks.1.bn2 (layer 4): S1 = sum D and S2 = sum D * xhat without the boards of replica 3 (b % 16 == 3)."""
    t = _stand_in()
    run, l, pre = t["ref32"], 4, "blocks.1.bn2"
    z, d = run["Z"][l], run["D"][l]
    mean = z.mean(dim=(0, 2, 3), keepdim=True)
    xhat = (z - mean) / torch.sqrt(((z - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True) + learn._BODY_BN[0])
    assert tsp.err((d * xhat).sum(dim=(0, 2, 3)), run["grad"][pre + ".weight"].double()) < 1e-5       # S2 is d gamma
    boards = torch.arange(z.shape[0]) % 16 == 3
    dev = _device_copy(run)
    for leaf, share in (("weight", (d * xhat)[boards].sum(dim=(0, 2, 3))), ("bias", d[boards].sum(dim=(0, 2, 3)))):
        dev["mom"][f"{pre}.{leaf}"] = run["mom"][f"{pre}.{leaf}"] - share
        dev["param"][f"{pre}.{leaf}"] = run["param"][f"{pre}.{leaf}"] + tsp.LR * (1 + learn.MOMENTUM) * share
    assert {f"mom:{pre}.weight", f"mom:{pre}.bias"} <= _bad(dev)
