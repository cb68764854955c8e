"""The node pool's enumeration on the CPU: csrc/node_pool.h, compiled alone into tests/node_pool_driver.cpp with the host
compiler, against the list of arrays written out here (DESIGN.md 3 "Node pool")."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = (82, 170, 362)                       # A = S * S + 1 at 9x9, 13x13, 19x19
# (SearchDev member, element bytes, one element per child, holds node indices)
ARRAYS = [
    ("ch_index", 4, True, True),
    ("ch_visits", 4, True, False),
    ("ch_vl", 4, True, False),
    ("ch_vsum", 8, True, False),
    ("ch_policy", 8, True, False),
    ("ch_value", 8, True, False),
    ("action", 2, True, False),
    ("node", 32, False, False),
]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("node_pool") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(HERE, "node_pool_driver.cpp"), "-o", exe])
    return [line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]


def test_the_enumeration_is_the_pool(listing):
    got = [(r[1], int(r[2]), tuple(int(x) for x in r[3:6]), int(r[6])) for r in listing if r[0] == "array"]
    want = [(name, size, tuple(a if per_child else 1 for a in SIZES), int(remap)) for name, size, per_child, remap in ARRAYS]
    assert got == want
    assert [g[0] for g in got if g[3]] == ["ch_index"]                  # the one array a compaction remaps
    assert [g[1] for g in got if g[2][0] != 1] == [4, 4, 4, 8, 8, 8, 2]    # the seven child arrays


def test_bytes_per_node_and_the_node_record(listing):
    rows = {int(r[1]): (int(r[2]), int(r[3])) for r in listing if r[0] == "node"}
    assert sorted(rows) == list(SIZES)
    for a in SIZES:
        per_node, record = rows[a]
        assert per_node == 38 * a + 32 == sum(size * (a if per_child else 1) for _, size, per_child, _ in ARRAYS)
        # tg_search_read_node's record: a 32-byte head, four int32 rows (index, visits, virtual loss, action widened), 8-byte
        # alignment, three float64 rows
        assert record == ((32 + 4 * 4 * a + 7) & ~7) + 3 * 8 * a
