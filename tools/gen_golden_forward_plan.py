#!/usr/bin/env python3
"""Which forward kernel a launch gets, as the library itself reports it: tg_net_kernel_name and
tg_net_executed_flops_per_position (FLOPs per position, the pipe's peak, the operand format) over board sizes, launch sizes
around every threshold of the choice (in units of the device's CU count c), TG_FWD_ALGO, TG_FWD_BANDS and the shared-device
switch - plus networks whose mid-block channels are rescaled beyond the spread limit of the one-axis Winograd kernels (they
fall through to the direct split kernels) and beyond both limits (exact fp32).  Nothing is launched.

GPU box:  python tools/gen_golden_forward_plan.py [--out FILE]            (default: tests/golden/forward_plan.json)

tests/test_gpu_forward_plan.py takes the case list and the query from here and holds every recorded row against the
library it runs on."""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
os.environ.setdefault("TG_DEBUG_KNOBS", "1")          # TG_FWD_BANDS is a debug knob (csrc/common.h tg::knob)

OUT = os.path.join(REPO, "tests", "golden", "forward_plan.json")
ALGOS = (None, "w1d", "split16", "w1dband", "wino", "direct", "no-such-algorithm")
BANDS = (None, "0", "2", "4")
# network -> exponent S of oracle.net.rescale_mid_channels (spread 2^S inside a layer; the limits: csrc/forward_plan.h)
NETWORKS = {"plain": 0, "beyond-w1d-limit": 8, "beyond-split-limit": 20}
COLUMNS = ("network", "size", "batch", "algo", "bands", "shared", "name", "flops", "peak", "dtype")
# what else the choice reads from the environment: unset while the rows are taken
_UNSET = ("TG_FWD_GROUP", "TG_FWD_WINO", "TG_FWD_NO_TAIL", "TG_FWD_TEST_GUARD_CAP", "TG_SHARED_DEVICE", "TG_FWD_SPREAD_GUARD")


def cases(c):
    """(network, size, batch, algo, bands, shared) of every recorded row on a device of c CUs."""
    out = []
    for batch in (1, c, c + 1, 2 * c, 2 * c + 1, 3 * c, 3 * c + 1, 4 * c, 6 * c, 6 * c + 64, 7 * c, 7 * c + 1):
        out += [("plain", 9, batch, algo, None, False) for algo in ALGOS]
    for batch in (1, 300):
        out += [("plain", 13, batch, algo, None, False) for algo in ALGOS]
    for batch in (1, 64, 65, 128, 129, 4096):
        out += [("plain", 19, batch, algo, bands, shared) for algo in ALGOS for bands in BANDS for shared in (False, True)]
    for network in ("beyond-w1d-limit", "beyond-split-limit"):
        for size, batches in ((9, (1, c + 1, 6 * c + 64)), (13, (1,)), (19, (1, 4096))):
            out += [(network, size, batch, algo, None, False) for batch in batches for algo in ALGOS]
    return out


def make_networks():
    """(network, size) -> DualNet on cuda:0."""
    import torch
    from oracle.net import make_state_dict, rescale_mid_channels
    from tamago_amd.nn.network.dual_net import DualNet
    for k in _UNSET:
        os.environ.pop(k, None)
    nets = {}
    for size in (9, 13, 19):
        base = make_state_dict(size, 7, 1.5)
        for network, S in NETWORKS.items():
            net = DualNet(torch.device("cuda:0"), size)
            net.load_state_dict(rescale_mid_channels(base, S, seed=1) if S else base)
            nets[network, size] = net
    return nets


def query(nets, case):
    """(name, FLOPs per position, peak TFLOP/s, operand format) the library reports for the case."""
    network, size, batch, algo, bands, shared = case
    net = nets[network, size]
    saved = {k: os.environ.get(k) for k in ("TG_FWD_ALGO", "TG_FWD_BANDS") + _UNSET}
    try:
        for k, v in (("TG_FWD_ALGO", algo), ("TG_FWD_BANDS", bands)) + tuple((k, None) for k in _UNSET):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        net.set_shared_device(shared)
        peak, dtype = ctypes.c_double(0.0), ctypes.c_char_p()
        name = net._lib.tg_net_kernel_name(net.handle, batch).decode()
        flops = net._lib.tg_net_executed_flops_per_position(net.handle, batch, ctypes.byref(peak), ctypes.byref(dtype))
        return name, float(flops), float(peak.value), dtype.value.decode()
    finally:
        net.set_shared_device(False)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    import argparse
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=OUT)
    out = ap.parse_args().out
    c = torch.cuda.get_device_properties(0).multi_processor_count
    nets = make_networks()
    rows = [list(case) + list(query(nets, case)) for case in cases(c)]
    spreads = {f"{network}/{size}": [net._lib.tg_net_channel_spread(net.handle, 0), net._lib.tg_net_channel_spread(net.handle, 1)]
               for (network, size), net in nets.items()}
    with open(out, "w") as f:
        f.write('{"num_cus": %d,\n "channel_spread_w1d_split": %s,\n "columns": %s,\n "rows": [\n' %
                (c, json.dumps(spreads), json.dumps(COLUMNS)))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print(f"{out}: {len(rows)} rows, {c} CUs")


if __name__ == "__main__":
    main()
