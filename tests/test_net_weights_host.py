"""The parameter blob's layout and every weight image of the forward kernels on the CPU: csrc/net_params.h and
csrc/net_weights.cpp compiled alone with the host compiler into tests/net_weights_driver.cpp (DESIGN.md 3 "Parameter blob and
weight images").  The image digests in golden/net_weight_images.json were recorded from the builders as they stood inside
tg_net_create / split_prepare / heads_prepare / w1d_prepare, moved verbatim, before they were restructured:
``python tests/test_net_weights_host.py --record [net_weights.cpp]`` rewrites them."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tamago_amd.nn.network.dual_net import state_dict_keys  # noqa: E402
from tests._net_blobs import BLOBS, make_blob, make_state  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "net_weight_images.json")
SOURCE = os.path.join(REPO, "tamago_amd", "csrc", "net_weights.cpp")
IMAGES = {"w0frag": np.float32, "wfrag": np.float32, "wwino": np.float32, "scale": np.float32, "shift": np.float32,
          "hp_w": np.float32, "hv_w": np.float32, "head_ss": np.float32, "pfc_wT": np.float32, "pfc_b": np.float32,
          "vfc_w": np.float32, "vfc_b": np.float32, "wsplit": np.uint16, "sscale": np.float32,
          "hd1_img": np.uint16, "hd1_tab": np.float32, "pfc_img": np.uint16, "pfc_tab": np.float32,
          "w1_w": np.uint16, "w1_shift": np.float32, "w1_down": np.float32}
HEADS_9X9_ONLY = ("hd1_img", "hd1_tab", "pfc_img", "pfc_tab")


def build_driver(workdir: str, source: str = SOURCE) -> str:
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = os.path.join(workdir, "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.dirname(SOURCE),
                           os.path.join(HERE, "net_weights_driver.cpp"), source, "-o", exe])
    return exe


def run_blob(exe: str, workdir: str, name: str):
    """-> (stdout rows, the image directory) of the driver on blob `name`."""
    size, blob = make_blob(name)
    out = os.path.join(workdir, name)
    os.makedirs(out, exist_ok=True)
    path = os.path.join(workdir, name + ".f32")
    blob.tofile(path)
    res = subprocess.run([exe, str(size), path, out], capture_output=True, text=True, check=True)
    os.remove(path)
    return [line.split() for line in res.stdout.splitlines()], out


def digest(rows, out):
    images = {}
    for name in sorted(os.listdir(out)):
        with open(os.path.join(out, name), "rb") as f:
            images[name[:-len(".bin")]] = hashlib.sha256(f.read()).hexdigest()
    spreads = {r[1]: float.fromhex(r[2]).hex() for r in rows if r[0] == "spread"}
    return {"images": images, "spread_split": spreads["split"], "spread_w1d": spreads["w1d"]}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("net_weights"))
    return build_driver(work), work


@pytest.fixture(scope="module")
def runs(driver):
    exe, work = driver
    return {name: run_blob(exe, work, name) for name in BLOBS}


def load(out, name):
    return np.fromfile(os.path.join(out, name + ".bin"), dtype=IMAGES[name])


# ---- layout ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,total", [("s9", 462968), ("s13", None), ("s19", 712168)])
def test_layout_is_the_running_sum_over_state_dict_keys(runs, name, total):
    rows, _ = runs[name]
    size = BLOBS[name][0]
    got = [(r[1], int(r[2]), int(r[3])) for r in rows if r[0] == "layout"]
    want, o = [], 0
    for key, shape in state_dict_keys(size):
        want.append((key, o, int(np.prod(shape))))
        o += int(np.prod(shape))
    assert got == want
    assert [int(r[1]) for r in rows if r[0] == "total"] == [o]
    if total is not None:
        assert o == total


# ---- recorded bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BLOBS))
def test_images_have_the_recorded_bits(runs, name):
    with open(GOLDEN) as f:
        golden = json.load(f)[name]
    got = digest(*runs[name])
    size = BLOBS[name][0]
    assert sorted(got["images"]) == sorted(k for k in IMAGES if size == 9 or k not in HEADS_9X9_ONLY)
    assert got["spread_split"] == golden["spread_split"] and got["spread_w1d"] == golden["spread_w1d"]
    assert got["images"] == golden["images"]


def test_the_edited_blobs_reach_their_paths(runs):
    spread = {name: {r[1]: float.fromhex(r[2]) for r in runs[name][0] if r[0] == "spread"} for name in BLOBS}
    assert spread["s9_spread"]["w1d"] > 2048 and spread["s9_spread"]["split"] > 2048      # the 2^-12 channel: beyond w1d's 128
    assert spread["s9_spread_wide"]["w1d"] > 2.0 ** 19 and spread["s9_spread_wide"]["split"] > 2.0 ** 19     # ... and split's 2^18
    for name in ("s9", "s13", "s19", "s9_zeros", "s9_tiny"):
        assert 1.0 <= spread[name]["w1d"] < 8 and 1.0 <= spread[name]["split"] < 8
    out = runs["s9_zeros"][1]
    assert not load(out, "pfc_img").any() and load(out, "pfc_tab")[0] == 1.0             # mx == 0: exponent 0
    assert load(out, "w1_down")[4] == 1.0 and not load(out, "w1_w").reshape(12, -1)[4].any()
    def down(name, key):               # 2^-e of the layer: its largest weight into [2^9, 2^10)
        return 2.0 ** (np.frexp(np.abs(make_state(name)[1][key]).max())[1] - 10)
    stem = load(runs["s9_spread"][1], "sscale").astype(np.float64)[:64] / load(runs["s9_spread"][1], "scale").astype(np.float64)[:64]
    assert down("s9_spread", "conv_layer.weight") >= 2.0 ** 7 and (stem == down("s9_spread", "conv_layer.weight")).all()   # e < 0
    tiny = runs["s9_tiny"][1]
    assert (load(tiny, "w1_down") == 2.0 ** -40).all() and load(tiny, "hd1_tab")[16] == 2.0 ** -40         # clamped
    ratio = load(tiny, "sscale").astype(np.float64)[64:128] / load(tiny, "scale").astype(np.float64)[64:128]
    assert down("s9_tiny", "blocks.0.conv1.weight") < 2.0 ** -70 and (ratio == down("s9_tiny", "blocks.0.conv1.weight")).all()   # not clamped
    nonfinite = load(runs["s9_nonfinite"][1], "wsplit")
    assert ((nonfinite & 0x7FFF) > 0x7C00).any() and ((nonfinite & 0x7FFF) == 0x7C00).any()               # NaN and inf pieces


# ---- against numpy, no recorded bits ---------------------------------------------------------------------------------
def test_fold_bn_against_float64(runs):
    for name in ("s9", "s19", "s9_nonfinite"):
        size, state = make_state(name)
        out = runs[name][1]

        def fold(prefix, eps):
            w, b, m, v = (state[f"{prefix}.{leaf}"].astype(np.float64) for leaf in ("weight", "bias", "running_mean", "running_var"))
            s = w / np.sqrt(v + eps)
            return s.astype(np.float32), (b - m * s).astype(np.float32)
        layers = [fold("bn_layer", 1e-5)] + [fold(f"blocks.{b}.bn{c}", 2e-5) for b in range(6) for c in (1, 2)]
        assert np.array_equal(load(out, "scale"), np.concatenate([s for s, _ in layers]))
        assert np.array_equal(load(out, "shift"), np.concatenate([t for _, t in layers]))
        (ps, pt), (vs, vt) = fold("policy_head.bn_layer", 2e-5), fold("value_head.bn_layer", 2e-5)
        assert np.array_equal(load(out, "head_ss"), np.array([ps[0], pt[0], ps[1], pt[1], vs[0], vt[0]], dtype=np.float32))


def test_pfc_wT_is_the_padded_transpose(runs):
    for name in ("s9", "s13", "s19"):
        size, state = make_state(name)
        p = size * size
        got = load(runs[name][1], "pfc_wT")
        assert got.size % 1024 == 0 and 0 <= got.size - 2 * p * (p + 1) < 1024
        assert np.array_equal(got[:2 * p * (p + 1)].reshape(2 * p, p + 1), state["policy_head.fc_layer.weight"].T)
        assert not got[2 * p * (p + 1):].any()


def test_wfrag_index_formula(runs):
    # NetDev: wfrag [12 layer][4 wave][9 tap][4 s][64 lane][4] = w[cout = 16 wave + (lane & 15)][cin = 16 s + 4 (lane >> 4) + j][tap]
    size, state = make_state("s9")
    got = load(runs["s9"][1], "wfrag").reshape(12, 4, 9, 4, 64, 4)
    lane = np.arange(64)
    for layer in range(12):
        w = state[f"blocks.{layer // 2}.conv{layer % 2 + 1}.weight"].reshape(64, 64, 9)
        wave, tap, s, ln, j = np.meshgrid(np.arange(4), np.arange(9), np.arange(4), lane, np.arange(4), indexing="ij")
        assert np.array_equal(got[layer], w[16 * wave + (ln & 15), 16 * s + 4 * (ln >> 4) + j, tap])


# ---- f16 conversions -------------------------------------------------------------------------------------------------
def test_f16_conversions_against_numpy(driver):
    exe, work = driver
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    exact = bits.view(np.float16).astype(np.float32)
    finite = np.sort(exact[np.isfinite(exact) & (exact >= 0)])
    mid = ((finite[:-1].astype(np.float64) + finite[1:].astype(np.float64)) / 2).astype(np.float32)     # the ties, exact in float32
    assert np.array_equal(mid.astype(np.float64) * 2, finite[:-1].astype(np.float64) + finite[1:])
    edge = np.array([65504.0, 65519.996, 65520.0, 65536.0, 2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
                     2.0 ** -26, 2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), np.float32(0)), 1e-45, 3e38], dtype=np.float32)
    pos = np.concatenate([finite, mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf)), edge])
    values = np.concatenate([pos, -pos, np.array([np.inf, -np.inf, np.nan], dtype=np.float32)]).astype(np.float32)
    path = os.path.join(work, "values.f32")
    values.tofile(path)
    subprocess.run([exe, "f16", path, work], check=True)
    widened = np.fromfile(os.path.join(work, "f16_to_f32.bin"), dtype=np.float32)
    nan = np.isnan(exact)
    assert np.array_equal(np.isnan(widened), nan)
    assert np.array_equal(widened[~nan].view(np.uint32), exact[~nan].view(np.uint32))
    narrowed = np.fromfile(os.path.join(work, "f32_to_f16.bin"), dtype=np.uint16)
    with np.errstate(over="ignore"):
        want = values.astype(np.float16)
    nan = np.isnan(want)
    assert nan.sum() == 1 and np.array_equal(np.isnan(narrowed.view(np.float16)), nan)
    assert np.array_equal(narrowed[~nan], want[~nan].view(np.uint16))


if __name__ == "__main__":
    import tempfile
    assert sys.argv[1:2] == ["--record"], __doc__
    with tempfile.TemporaryDirectory() as tmp:
        binary = build_driver(tmp, *sys.argv[2:3])
        recorded = {blob: digest(*run_blob(binary, tmp, blob)) for blob in BLOBS}
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
