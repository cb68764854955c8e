"""The leaf queue's contract on the CPU: csrc/leaf_queue.h, compiled alone into tests/leaf_queue_driver.cpp with the host
compiler, against the arrays, the packing and the two rules written out here (DESIGN.md 3 "Leaf queue")."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

PATH_CAP = 48
# (SearchDev member, element bytes, elements per slot)
ARRAYS = [
    ("q_node", 4, 1),
    ("q_pnode", 4, 1),
    ("q_pedge", 4, 1),
    ("q_depth", 4, 1),
    ("q_path", 4, PATH_CAP),
    ("q_src", 4, 1),
]
PASS = 0

PACK = list(itertools.product((0, 1, 2 ** 21 - 1), (0, 81, 169, 361, 1023)))
DEPTH = list(itertools.product((0, 1, 47, 48, 49), (2 ** 21, 2 ** 21 + 1)))
# edge count after the virtual loss, moves after the move, the move, the move before it
ENDS = list(itertools.product((1, 2, 3), (1, 2, 3, 4), (PASS, 5), (PASS, 5)))


def _descent_ends(count, moves, last, before):
    """mcts/tree.py:224-229 of the reference, restated"""
    expand_threshold = 1
    if moves > 2:
        if last == PASS and before == PASS:
            expand_threshold = 10000000
    return count < expand_threshold + 1


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("leaf_queue") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(HERE, "leaf_queue_driver.cpp"), "-o", exe])
    queries = [f"pack {n} {e}" for n, e in PACK] + [f"depth {d} {n}" for d, n in DEPTH] + \
              ["ends %d %d %d %d" % q for q in ENDS]
    out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()]
    return {kind: [r[1:] for r in rows if r[0] == kind] for kind in ("array", "pack", "depth", "ends")}


def test_the_enumeration_is_the_queue(answers):
    assert [(r[0], int(r[1]), int(r[2])) for r in answers["array"]] == ARRAYS


def test_a_path_entry_round_trips(answers):
    got = [tuple(int(x) for x in r) for r in answers["pack"]]
    assert len(got) == len(PACK)
    for (n, e), (entry, node, edge) in zip(PACK, got):
        assert 0 <= entry < 2 ** 31, (n, e, entry)                 # a non-negative int32
        assert (node, edge) == (n, e), (n, e, entry)


def test_recorded_depth_is_the_rule(answers):
    got = [int(r[0]) for r in answers["depth"]]
    want = [d if d <= PATH_CAP and n <= 2 ** 21 else 0 for d, n in DEPTH]
    assert got == want


def test_a_puct_descent_ends_where_the_reference_ends_it(answers):
    got = [bool(int(r[0])) for r in answers["ends"]]
    want = [_descent_ends(*q) for q in ENDS]
    assert got == want
    assert any(want) and not all(want)
