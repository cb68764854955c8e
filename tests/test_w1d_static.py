"""Register budget of the 9x9 one-axis Winograd forward kernel, read from the code object metadata hipcc emits for gfx950
(CPU test: cross-compiles net_forward_w1d.hip with the flags of tamago_amd.build, needs no GPU).

The production instantiations dualnet_fwd_w1d_kernel<3, false> and <1, false> keep a layer's weight fragments in the
accumulation half of the register file and fill the other half: a change outside the tower that costs a few registers
shows up as scratch traffic inside it.  They must not spill a vector register and must use no scratch."""
import os
import re
import shutil
import subprocess

import pytest

from tamago_amd import build

SRC = os.path.join(build.CSRC, "net_forward_w1d.hip")


def _hipcc():
    try:
        return build._hipcc()
    except RuntimeError:
        return None


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None or shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("w1d_static") / "net_forward_w1d.s"
    cmd = [hipcc] + build.FLAGS + build.EXTRA_FLAGS["net_forward_w1d.hip"] + \
        ["-x", "hip", "--cuda-device-only", "-S", SRC, "-o", str(out)]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    kernels = {}
    name = None
    for line in out.read_text().splitlines():
        m = re.match(r"\s+\.(name|vgpr_spill_count|private_segment_fixed_size|vgpr_count|agpr_count):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "name":
            name = m.group(2)
            kernels[name] = {}
        elif name is not None:
            kernels[name][m.group(1)] = int(m.group(2))
    return kernels


@pytest.mark.parametrize("g", [3, 1])
def test_production_instantiation_spills_nothing(metadata, g):
    # Itanium mangling of dualnet_fwd_w1d_kernel<G, false>: template arguments ILi<G>ELb0EE
    names = [n for n in metadata if "dualnet_fwd_w1d_kernel" in n and f"ILi{g}ELb0EE" in n]
    assert len(names) == 1, sorted(metadata)
    md = metadata[names[0]]
    assert md["vgpr_spill_count"] == 0, md
    assert md["private_segment_fixed_size"] == 0, md
