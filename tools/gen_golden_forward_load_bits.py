#!/usr/bin/env python3
"""Bit pin of what a loaded network computes, per board size and forward family -> tests/golden/forward_load_bits.json.

A weight image that moved one bit moves these outputs: the file pins what the forward kernels computed from the images
BEFORE a change to the load path (the blob layout, the image builders of csrc/net_weights.cpp, tg_net_create) that must not
move a bit.  So it is generated on a GPU with the library of the PARENT commit of such a change, never with the code under test:

    TAMAGO_HIP_LIB=<parent checkout>/tamago_amd/libtamago_hip.so python tools/gen_golden_forward_load_bits.py

tests/test_gpu_net_load_bits.py runs `measure()` below on the library under test and compares.

Networks: the plain random blobs of tests/_net_blobs.py ("s9", "s13", "s19").  Planes: RandomState(PLANE_SEED + size), binary.
Batches 5 / 2 / 2 at 9x9 / 13x13 / 19x19 - launch size does not matter to a weight image; these are the smallest batches that
reach every family.  TG_FWD_ALGO unset and w1d, split16, wino, direct; where a size has no kernel of the family asked for, the
plan's choice runs - the file records tg_net_kernel_name beside each digest, so it shows which kernel that was."""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "forward_load_bits.json")

PLANE_SEED = 7100
BATCH = {9: 5, 13: 2, 19: 2}
ALGOS = (None, "w1d", "split16", "wino", "direct")


def planes(size: int) -> np.ndarray:
    return np.random.RandomState(PLANE_SEED + size).randint(0, 2, size=(BATCH[size], 6, size, size)).astype(np.float32)


def sha(t) -> str:
    return hashlib.sha256(np.ascontiguousarray(t.numpy().astype(np.float32)).tobytes()).hexdigest()


def measure(size: int) -> dict:
    """{algo or "default": {"kernel", "policy", "value", "logits"}} of the network "s<size>" on cuda:0."""
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import torch
    from tamago_amd import lib as tl
    from tamago_amd.nn.network.dual_net import DualNet
    from tests._net_blobs import make_state

    saved = os.environ.pop("TG_FWD_ALGO", None)
    try:
        net = DualNet(torch.device("cuda:0"), size)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in make_state(f"s{size}")[1].items()})
        x = torch.from_numpy(planes(size))
        out = {}
        for algo in ALGOS:
            if algo is None:
                os.environ.pop("TG_FWD_ALGO", None)
            else:
                os.environ["TG_FWD_ALGO"] = algo
            pol, val = net.inference(x)
            lg, val2 = net.inference_with_policy_logits(x)
            assert torch.equal(val, val2)
            out[algo or "default"] = {"kernel": tl.load().tg_net_kernel_name(net.handle, BATCH[size]).decode(),
                                      "policy": sha(pol), "value": sha(val), "logits": sha(lg)}
        return out
    finally:
        os.environ.pop("TG_FWD_ALGO", None)
        if saved is not None:
            os.environ["TG_FWD_ALGO"] = saved


def main() -> None:
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from tamago_amd import lib as tl
    out = {str(size): measure(size) for size in BATCH}
    for size, rows in out.items():
        for algo, row in rows.items():
            print(f"{size:>2} {algo:8s} {row['kernel']:40s} policy {row['policy'][:12]}")
    with open(GOLD, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLD} with library {tl.LIB_PATH}")


if __name__ == "__main__":
    main()
