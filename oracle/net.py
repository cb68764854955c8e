"""Oracle DualNet forward (TEST INFRASTRUCTURE - see oracle/__init__.py).

Restates nn/network/dual_net.py:17-106, res_block.py:8-38, head/policy_head.py:7-39
and head/value_head.py:7-39 as a functional PyTorch-CPU fp32 forward over a plain
``state_dict`` with the reference's key names (nn/utility.py:139-159 loads exactly
these).  Inference mode only: BatchNorm uses running statistics.
"""
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn.functional as F

FILTERS = 64      # dual_net.py:26
BLOCKS = 6        # dual_net.py:27
EPS_STEM = 1e-5   # nn.BatchNorm2d default, dual_net.py:32
EPS_BODY = 2e-5   # res_block.py:22-23, policy_head.py:19, value_head.py:20


def state_dict_shapes(board_size: int) -> Dict[str, Tuple[int, ...]]:
    """Key -> shape of every tensor ``load_network`` expects (nn/utility.py:139-159)."""
    p = board_size * board_size
    shapes = {"conv_layer.weight": (FILTERS, 6, 3, 3)}

    def bn(prefix, c):
        shapes[prefix + ".weight"] = (c,)
        shapes[prefix + ".bias"] = (c,)
        shapes[prefix + ".running_mean"] = (c,)
        shapes[prefix + ".running_var"] = (c,)
        shapes[prefix + ".num_batches_tracked"] = ()

    bn("bn_layer", FILTERS)
    for b in range(BLOCKS):
        shapes[f"blocks.{b}.conv1.weight"] = (FILTERS, FILTERS, 3, 3)
        shapes[f"blocks.{b}.conv2.weight"] = (FILTERS, FILTERS, 3, 3)
        bn(f"blocks.{b}.bn1", FILTERS)
        bn(f"blocks.{b}.bn2", FILTERS)
    shapes["policy_head.conv_layer.weight"] = (2, FILTERS, 1, 1)
    bn("policy_head.bn_layer", 2)
    shapes["policy_head.fc_layer.weight"] = (p + 1, 2 * p)
    shapes["policy_head.fc_layer.bias"] = (p + 1,)
    shapes["value_head.conv_layer.weight"] = (1, FILTERS, 1, 1)
    bn("value_head.bn_layer", 1)
    shapes["value_head.fc_layer.weight"] = (3, p)
    shapes["value_head.fc_layer.bias"] = (3,)
    return shapes


def make_state_dict(board_size: int, seed: int, gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """Seeded synthetic weights (no trained weights exist - model/.gitkeep only).
    Only ``RandomState.random_sample`` plus exact float64 arithmetic is used so the
    values are bit-identical on every machine.  BN statistics are non-trivial on
    purpose (mean != 0, var != 1) so that folding errors show up."""
    rs = np.random.RandomState(seed)
    out = {}
    for key, shape in state_dict_shapes(board_size).items():
        if key.endswith("num_batches_tracked"):
            out[key] = torch.tensor(0, dtype=torch.long)
            continue
        n = int(np.prod(shape)) if shape else 1
        u = rs.random_sample(n)
        if key.endswith("running_var"):
            v = 0.5 + u                                  # [0.5, 1.5)
        elif key.endswith("running_mean"):
            v = (u - 0.5) * 0.2
        elif ".bn" in key or key.startswith("bn_layer"):
            v = 0.75 + 0.5 * u if key.endswith("weight") else (u - 0.5) * 0.2
        elif key.endswith("fc_layer.bias"):
            v = (u - 0.5) * 0.2
        else:
            fan_in = int(np.prod(shape[1:]))
            v = (u - 0.5) * 2.0 * gain * (3.0 / fan_in) ** 0.5
        out[key] = torch.from_numpy(v.astype(np.float32).reshape(shape))
    return out


def rescale_mid_channels(sd: Dict[str, torch.Tensor], S: int, seed: int) -> Dict[str, torch.Tensor]:
    """The same function with another scale inside every residual block: mid-block channel c
    of block b carries k_c = 2^j_c times its activation (bn1 weight and bias x k_c) and conv2
    reads it back through weights / k_c.  j_c is drawn from [-S, 0] (j_0 = -S, j_1 = 0: the
    spread inside a layer is exactly 2^S).  ReLU commutes with a positive factor, powers of
    two commute with every fp32 / fp64 rounding short of under- and overflow, and the
    exponents only go down, so the logits keep their bits while the per-channel scales a
    kernel folds or carries spread by 2^S.  Returns a new dict; ``sd`` is left alone."""
    rs = np.random.RandomState(seed)
    out = dict(sd)
    for b in range(BLOCKS):
        j = rs.randint(-S, 1, size=FILTERS)
        j[0], j[1] = -S, 0
        k = torch.from_numpy(np.ldexp(1.0, j))                      # float64, exact
        for leaf in ("weight", "bias"):
            t = sd[f"blocks.{b}.bn1.{leaf}"]
            out[f"blocks.{b}.bn1.{leaf}"] = t * k.to(t.dtype)
        w = sd[f"blocks.{b}.conv2.weight"]
        out[f"blocks.{b}.conv2.weight"] = w / k.to(w.dtype).reshape(1, FILTERS, 1, 1)
    return out


def _pow2(t: torch.Tensor, k: int) -> torch.Tensor:
    return t * (2.0 ** k)                                            # (a power of two: exact in every float format short of its range)


def scale_tower(sd: Dict[str, torch.Tensor], k: int) -> Dict[str, torch.Tensor]:
    """The same function with every tower activation (stem output, the twelve layer outputs) carried 2^k times as large.  The stem
    batch norm's weight and bias are x 2^k; a block's convolutions are linear, so its batch norms see 2^k times their input:
    their running_mean and bias are x 2^k (bn(2^k c) = 2^k bn(c) term by term), and the residual sum adds two values of the same
    scale.  The two head batch norms undo it: running_mean x 2^k, weight / 2^k.  ReLU commutes with a positive factor and a power
    of two commutes with every fp32 / fp64 rounding short of over- and underflow, so policy logits and value logits keep their
    bits while the activations climb past whatever limit a kernel has.  Returns a new dict; ``sd`` is left alone."""
    out = dict(sd)
    for leaf in ("weight", "bias"):
        out[f"bn_layer.{leaf}"] = _pow2(sd[f"bn_layer.{leaf}"], k)
    for b in range(BLOCKS):
        for bn in ("bn1", "bn2"):
            for leaf in ("bias", "running_mean"):
                out[f"blocks.{b}.{bn}.{leaf}"] = _pow2(sd[f"blocks.{b}.{bn}.{leaf}"], k)
    for head in ("policy_head", "value_head"):
        out[f"{head}.bn_layer.weight"] = _pow2(sd[f"{head}.bn_layer.weight"], -k)
        out[f"{head}.bn_layer.running_mean"] = _pow2(sd[f"{head}.bn_layer.running_mean"], k)
    return out


def scale_head(sd: Dict[str, torch.Tensor], head: str, k: int) -> Dict[str, torch.Tensor]:
    """The same function with the features of one head (``policy_head`` or ``value_head``: its 1x1 convolution behind batch norm
    and ReLU) carried 2^k times as large: the head's batch-norm weight and bias are x 2^k, its FC weight / 2^k, the FC bias
    stays.  The tower is untouched.  ReLU commutes with a positive factor, the FC's products keep their significands and only
    shift exponents back, so every partial sum - and the logits - keep their bits (powers of two, short of over- and
    underflow).  Returns a new dict; ``sd`` is left alone."""
    assert head in ("policy_head", "value_head"), head
    out = dict(sd)
    for leaf in ("weight", "bias"):
        out[f"{head}.bn_layer.{leaf}"] = _pow2(sd[f"{head}.bn_layer.{leaf}"], k)
    out[f"{head}.fc_layer.weight"] = _pow2(sd[f"{head}.fc_layer.weight"], -k)
    return out


TOWER_LAYERS = 2 * BLOCKS


def spike_channel(sd: Dict[str, torch.Tensor], layer: int, c: int, height: float) -> Dict[str, torch.Tensor]:
    """ANOTHER function (its own reference): exactly one tower layer's output is ``height`` higher in channel c, everywhere on
    the board, and nothing downstream reads it.  layer = 2 b: the mid-block output of block b (bn1.bias[c] += height; conv2 of
    the block no longer reads channel c).  layer = 2 b + 1: the output of block b (bn2.bias[c] += height; block b + 1 takes the
    height off again through bn2.bias[c], so that channel c is hot on that block's residual input only and its output is back
    in range).  No later reader takes channel c of the residual stream: conv1 of every later block and both head convolutions
    have zero weights for it - not only the next one, because fp32 carries height + x at a quantum of 2^-7 (height = 120 000)
    and what comes back down has lost ten bits: read downstream, the fp32 ORACLE's value softmax is 1e-3 off its fp64 one, and
    the case would measure the construction, not a kernel.  Returns a new dict; ``sd`` is left alone."""
    assert 0 <= layer < TOWER_LAYERS and 0 <= c < FILTERS
    out = dict(sd)

    def bump(key, by):
        t = sd[key].clone()
        t[c] += by
        out[key] = t

    def blind(key):
        w = sd[key].clone()
        w[:, c] = 0
        out[key] = w

    b = layer // 2
    if layer % 2 == 0:
        bump(f"blocks.{b}.bn1.bias", height)
        blind(f"blocks.{b}.conv2.weight")
    else:
        bump(f"blocks.{b}.bn2.bias", height)
        if b + 1 < BLOCKS:
            bump(f"blocks.{b + 1}.bn2.bias", -height)
        for later in range(b + 1, BLOCKS):
            blind(f"blocks.{later}.conv1.weight")
        blind("policy_head.conv_layer.weight")
        blind("value_head.conv_layer.weight")
    return out


def spike_last_row(sd: Dict[str, torch.Tensor], c: int, height: float) -> Dict[str, torch.Tensor]:
    """ANOTHER function (its own reference): the tower's LAST layer output is ``height`` higher in channel c on the board's last
    row only - what a kernel that finishes its last rows apart from the others must still see.  Weights are the same at every
    point, so the row comes from the zero padding: mid-block channel c + 1 of the last block is the constant height / 4
    (bn1.weight = 0), read by output channel c alone, through the three taps that look one row DOWN, with the weight that
    sums to - height over two taps; bn2.bias[c] += height.  The last row sees padding there and keeps the height; every
    other point loses at least all of it (corners of a row: two taps inside).  Both heads' weights for channel c are zero.
    Returns a new dict; ``sd`` is left alone."""
    b, cm, level = BLOCKS - 1, (c + 1) % FILTERS, height / 4.0
    out = dict(sd)
    for leaf, value in (("weight", 0.0), ("bias", level)):
        t = sd[f"blocks.{b}.bn1.{leaf}"].clone()
        t[cm] = value
        out[f"blocks.{b}.bn1.{leaf}"] = t
    g = float(sd[f"blocks.{b}.bn2.weight"][c].double() / torch.sqrt(sd[f"blocks.{b}.bn2.running_var"][c].double() + EPS_BODY))
    w = sd[f"blocks.{b}.conv2.weight"].clone()
    w[:, cm] = 0
    w[c] = 0
    w[c, cm, 2, :] = -height / (2.0 * level * g)
    out[f"blocks.{b}.conv2.weight"] = w
    t = sd[f"blocks.{b}.bn2.bias"].clone()
    t[c] += height
    out[f"blocks.{b}.bn2.bias"] = t
    for head in ("policy_head", "value_head"):
        w = sd[f"{head}.conv_layer.weight"].clone()
        w[:, c] = 0
        out[f"{head}.conv_layer.weight"] = w
    return out


def spike_points(size: int):
    """The board points of the point spikes: the corners (0, 0), (S-1, S-1), (S-1, 0), the centre, the middle of the last row."""
    s = size
    return ((0, 0), (s - 1, s - 1), (s - 1, 0), (s // 2, s // 2), (s - 1, s // 2))


def spike_point(sd: Dict[str, torch.Tensor], planes: torch.Tensor, board: int, point, height: float) -> torch.Tensor:
    """Planes with ONE entry of ``board`` multiplied: of the six entries at ``point`` = (y, x) the non-zero one that some stem
    channel reads most strongly, by the factor that lifts that channel's output at the point by ``height``.  A 3x3 stem
    convolution carries one entry to the point's 3x3 neighbourhood only: the stem output is hot there and unchanged everywhere
    else (stem_output shows it); the tower then spreads it over the board.  Returns new planes; ``planes`` is left alone."""
    y, x = point
    g = (sd["bn_layer.weight"] / torch.sqrt(sd["bn_layer.running_var"] + EPS_STEM)).double()
    gain = sd["conv_layer.weight"][:, :, 1, 1].double() * g[:, None] * planes[board, :, y, x].double()[None, :]   # [o][plane]
    best = float(gain.max())
    assert best > 0.0, "every entry at the point is zero: choose another plane seed"
    ch = int(gain.max(dim=0).values.argmax())
    out = planes.clone()
    out[board, ch, y, x] *= float(np.float32(1.0 + height / best))
    return out


def stem_output(sd: Dict[str, torch.Tensor], planes: torch.Tensor) -> torch.Tensor:
    """The stem's output [N, 64, S, S] (dual_net.py:43)."""
    with torch.no_grad():
        return F.relu(_bn(F.conv2d(planes, sd["conv_layer.weight"], padding=1), sd, "bn_layer", EPS_STEM))


def _bn(x, sd, prefix, eps):
    return F.batch_norm(x, sd[prefix + ".running_mean"], sd[prefix + ".running_var"],
                        sd[prefix + ".weight"], sd[prefix + ".bias"], False, 0.0, eps)


def forward_logits(sd: Dict[str, torch.Tensor], planes: torch.Tensor):
    """DualNet.forward, dual_net.py:41-52."""
    x = F.relu(_bn(F.conv2d(planes, sd["conv_layer.weight"], padding=1), sd, "bn_layer",
                   EPS_STEM))
    for b in range(BLOCKS):                                          # res_block.py:36-39
        h = F.relu(_bn(F.conv2d(x, sd[f"blocks.{b}.conv1.weight"], padding=1), sd,
                       f"blocks.{b}.bn1", EPS_BODY))
        h = _bn(F.conv2d(h, sd[f"blocks.{b}.conv2.weight"], padding=1), sd,
                f"blocks.{b}.bn2", EPS_BODY)
        x = F.relu(x + h)
    batch = x.shape[0]
    ph = F.relu(_bn(F.conv2d(x, sd["policy_head.conv_layer.weight"]), sd,
                    "policy_head.bn_layer", EPS_BODY))               # policy_head.py:33-39
    policy = F.linear(ph.reshape(batch, -1), sd["policy_head.fc_layer.weight"],
                      sd["policy_head.fc_layer.bias"])
    vh = F.relu(_bn(F.conv2d(x, sd["value_head.conv_layer.weight"]), sd,
                    "value_head.bn_layer", EPS_BODY))                # value_head.py:33-39
    value = F.linear(vh.reshape(batch, -1), sd["value_head.fc_layer.weight"],
                     sd["value_head.fc_layer.bias"])
    return policy, value


def layer_maxima(sd: Dict[str, torch.Tensor], planes: torch.Tensor, dtype=torch.float64) -> Dict[str, np.ndarray]:
    """Per position, the largest value of everything a kernel's f16 range guard has to look at, from a forward in ``dtype``:
    "planes" [N] (the largest |input|: the f16 kernels split the planes into f16 pieces as well), "stem" [N], "layers" [12, N] (each tower layer's output behind its ReLU: 2 b = mid-block, 2 b + 1 = output of block b),
    "policy_head" [N] and "value_head" [N] (the head's features behind batch norm and ReLU) - and, over all positions, per
    channel: "layer_channels" [12, 64], "policy_channels" [2].  float64 arrays.  The same operations as forward_logits."""
    with torch.no_grad():
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        x = F.relu(_bn(F.conv2d(planes.to(dtype), sd["conv_layer.weight"], padding=1), sd, "bn_layer", EPS_STEM))
        top = lambda t: t.flatten(1).max(dim=1).values.double().numpy()                      # noqa: E731
        per_channel = lambda t: t.transpose(0, 1).flatten(1).max(dim=1).values.double().numpy()   # noqa: E731
        out = {"planes": top(planes.to(dtype).abs()), "stem": top(x)}
        layers = []
        for b in range(BLOCKS):
            h = F.relu(_bn(F.conv2d(x, sd[f"blocks.{b}.conv1.weight"], padding=1), sd, f"blocks.{b}.bn1", EPS_BODY))
            layers.append(h)
            h = _bn(F.conv2d(h, sd[f"blocks.{b}.conv2.weight"], padding=1), sd, f"blocks.{b}.bn2", EPS_BODY)
            x = F.relu(x + h)
            layers.append(x)
        out["layers"] = np.stack([top(t) for t in layers])
        out["layer_channels"] = np.stack([per_channel(t) for t in layers])
        for head in ("policy_head", "value_head"):
            f = F.relu(_bn(F.conv2d(x, sd[f"{head}.conv_layer.weight"]), sd, f"{head}.bn_layer", EPS_BODY))
            out[head] = top(f)
        out["policy_channels"] = per_channel(F.relu(_bn(F.conv2d(x, sd["policy_head.conv_layer.weight"]), sd,
                                                        "policy_head.bn_layer", EPS_BODY)))
    return out


def tower_output(sd: Dict[str, torch.Tensor], planes: torch.Tensor) -> torch.Tensor:
    """The last block's output [N, 64, S, S]: what both heads read (dual_net.py:44-47)."""
    with torch.no_grad():
        x = stem_output(sd, planes)
        for b in range(BLOCKS):
            h = F.relu(_bn(F.conv2d(x, sd[f"blocks.{b}.conv1.weight"], padding=1), sd, f"blocks.{b}.bn1", EPS_BODY))
            x = F.relu(x + _bn(F.conv2d(h, sd[f"blocks.{b}.conv2.weight"], padding=1), sd, f"blocks.{b}.bn2", EPS_BODY))
        return x


class OracleNet:
    """The two inference entry points the search uses (dual_net.py:81-106), CPU only."""

    def __init__(self, state_dict: Dict[str, torch.Tensor]):
        self.sd = state_dict

    def inference(self, planes: torch.Tensor):
        with torch.no_grad():
            policy, value = forward_logits(self.sd, planes)
            return torch.softmax(policy, dim=1), torch.softmax(value, dim=1)

    def inference_with_policy_logits(self, planes: torch.Tensor):
        with torch.no_grad():
            policy, value = forward_logits(self.sd, planes)
            return policy, torch.softmax(value, dim=1)
