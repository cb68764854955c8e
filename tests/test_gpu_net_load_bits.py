"""A loaded network computes the bits it computed before the load path was reworked: golden/forward_load_bits.json
(tools/gen_golden_forward_load_bits.py, generated with the library of the commit BEFORE csrc/net_params.h and
csrc/net_weights.cpp took over the blob layout and the weight images) pins policy, value and logits of seeded binary planes
per board size and forward family, with the name of the kernel that ran."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import gen_golden_forward_load_bits as gen  # noqa: E402


@pytest.mark.parametrize("size", sorted(gen.BATCH))
def test_forward_bits_of_a_loaded_network(size):
    with open(gen.GOLD) as f:
        golden = json.load(f)[str(size)]
    got = gen.measure(size)
    assert sorted(got) == sorted(golden) == sorted(a or "default" for a in gen.ALGOS)
    for algo in got:
        print(f"{size} {algo}: {got[algo]['kernel']}", flush=True)
        assert got[algo] == golden[algo], (size, algo)
