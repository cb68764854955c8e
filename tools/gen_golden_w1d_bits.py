#!/usr/bin/env python3
"""Bit pin of the 9x9 one-axis Winograd forward kernel (TG_FWD_ALGO=w1d): policy logits, policy probabilities and value of
seeded inputs at batches 1, 3, 4, 7, 260 and 1300 -> tests/golden/w1d_bits_s9.npz.

The file pins what the kernel computed BEFORE a change that must not move a bit (staging, addressing, load placement).  So
it is generated on a GPU with the library of the PARENT commit of such a change, never with the code under test:

    TAMAGO_HIP_LIB=<parent checkout>/tamago_amd/libtamago_hip.so python tools/gen_golden_w1d_bits.py

tests/test_gpu_net_w1d_phases.py compares the raw float32 bits (and holds the same outputs to the oracle's tolerance, so a
file generated wrongly cannot hide behind itself).

Inputs (`planes(b)` below, imported by the test): weights make_state_dict(9, SEED, GAIN); planes of batch b from
RandomState(PLANE_SEED + b), uniform in [-1, 1) times 1.2345 - NOT f16-exact, the low pieces of the operand split are
non-zero -; the LAST position of every batch is zero in the interior and keeps its values on the 32 corner and edge cells of
each plane only (what a 3x3 tap reads across the border of the board).  The planes are not stored: the file carries their
SHA-256 per batch, which the test checks after regenerating them.

Which kernel a batch runs (256 compute units; KERNEL below, asserted here and in the test through tg_net_kernel_name): up to
the CU count dualnet_fwd_w1d_kernel<1>, one board per workgroup - batches 1, 3, 4 and 7 are one to seven workgroups of one
group each.  Above it dualnet_fwd_w1d_kernel<3>: 260 is 87 groups (the last of two boards) on 87 workgroups, one group each;
1300 = 433 * 3 + 1 is 434 groups on 256 workgroups, no second launch for the tail (1300 mod 768 = 532 > 256), so 178 groups
are handed out by the ticket counter and run as a workgroup's SECOND group - next planes prefetched behind the tower, border
and padding zeroed again over what the first group left there - and the last group is ragged with ONE board, the border
position.  The arrays of batch 1300 would be 0.9 MB: the file carries their SHA-256 (HASHED)."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "w1d_bits_s9.npz")

SEED, GAIN = 13, 1.4
PLANE_SEED = 9000
BATCHES = (1, 3, 4, 7, 260, 1300)
HASHED = (1300,)                                       # SHA-256 of each output array instead of the array
KERNEL = {1: "dualnet_fwd_w1d_kernel<1>", 3: "dualnet_fwd_w1d_kernel<1>", 4: "dualnet_fwd_w1d_kernel<1>",
          7: "dualnet_fwd_w1d_kernel<1>", 260: "dualnet_fwd_w1d_kernel<3>", 1300: "dualnet_fwd_w1d_kernel<3>"}


def planes(b: int) -> np.ndarray:
    rs = np.random.RandomState(PLANE_SEED + b)
    x = (rs.uniform(-1.0, 1.0, size=(b, 6, 9, 9)) * 1.2345).astype(np.float32)
    x[b - 1, :, 1:8, 1:8] = 0.0
    return x


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main() -> None:
    sys.path.insert(0, REPO)
    os.environ["TG_FWD_ALGO"] = "w1d"
    import torch
    from oracle.net import make_state_dict
    from tamago_amd import lib as tl
    from tamago_amd.nn.network.dual_net import DualNet

    net = DualNet(torch.device("cuda:0"), 9)
    net.load_state_dict(make_state_dict(9, SEED, GAIN))
    out = {"seed": np.int64(SEED), "gain": np.float64(GAIN), "plane_seed": np.int64(PLANE_SEED),
           "batches": np.asarray(BATCHES, dtype=np.int64)}
    for b in BATCHES:
        x = planes(b)
        assert np.count_nonzero(x.astype(np.float16).astype(np.float32) != x) > np.count_nonzero(x) // 2
        t = torch.from_numpy(x)
        pol, val = net.inference(t)
        lg, val2 = net.inference_with_policy_logits(t)
        assert torch.equal(val, val2)
        out[f"b{b}_planes_sha256"] = np.asarray(sha(x))
        name = tl.load().tg_net_kernel_name(net.handle, b).decode()
        assert name == KERNEL[b], (b, name)
        for key, a in (("policy", pol), ("logits", lg), ("value", val)):
            a = a.numpy().astype(np.float32)
            if b in HASHED:
                out[f"b{b}_{key}_sha256"] = np.asarray(sha(a))
            else:
                out[f"b{b}_{key}"] = a
        print(f"batch {b:4d}: kernel {name}, policy sha {sha(pol.numpy().astype(np.float32))[:12]}")
    np.savez_compressed(GOLD, **out)
    print(f"wrote {GOLD} ({os.path.getsize(GOLD)} bytes) with library {tl.LIB_PATH}")


if __name__ == "__main__":
    main()
