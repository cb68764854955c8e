"""The read-out records on the CPU: csrc/readout.h, compiled alone into tests/readout_driver.cpp with the host compiler,
against the layouts written out by hand here (DESIGN.md 3 "Read-out records")."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = (82, 170, 362)                       # A = S * S + 1 at 9x9, 13x13, 19x19
ODD = (5, 7)                                 # no board size gives an odd A: the root record's alignment pad, exercised
DEPTHS = (1, 3, 32)
POOL, RNG, PIPE, REROOT = 1, 2, 4, 8
ERROR_WORDS = [(0, POOL), (1, RNG), (2, PIPE), (3, REROOT), (4, POOL | PIPE), (5, RNG | PIPE), (6, PIPE | (7 << 8)), (7, 0),
               (8, POOL | RNG | PIPE | REROOT)]
TEXT = {POOL: "node pool full", RNG: "random window exhausted", PIPE: "pipeline stalled", REROOT: "new root beyond the tree's nodes"}


def align8(n):
    return (n + 7) & ~7


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("readout") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(HERE, "readout_driver.cpp"), "-o", exe])
    args = [str(x) for pair in ERROR_WORDS for x in pair]
    return [line.split() for line in subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.splitlines()]


def rows_of(fields):
    return [(name, int(size), int(at)) for name, size, at in (f.split(":") for f in fields)]


def test_root_record(listing):
    got = {int(r[1]): (int(r[2]), rows_of(r[3:])) for r in listing if r[0] == "root"}
    assert sorted(got) == sorted(SIZES + ODD)
    for a in SIZES:
        size, rows = got[a]
        assert size == 16 + 12 * a + 16 * a
        assert rows == [("visits", 4, 16), ("virtual_loss", 4, 16 + 4 * a), ("action", 4, 16 + 8 * a),
                        ("value_sum", 8, 16 + 12 * a), ("policy", 8, 16 + 20 * a)]
    for a in ODD:                                                     # 16 + 12 A is 4 mod 8: the float64 rows move up by 4
        size, rows = got[a]
        at = dict((name, off) for name, _, off in rows)
        assert [at["visits"], at["virtual_loss"], at["action"]] == [16, 16 + 4 * a, 16 + 8 * a]
        assert (16 + 12 * a) % 8 == 4 and at["value_sum"] == 16 + 12 * a + 4 and at["value_sum"] % 8 == 0
        assert at["policy"] == at["value_sum"] + 8 * a and at["policy"] % 8 == 0
        assert size == 16 + 12 * a + 16 * a + 4


def test_selfplay_tail_and_state(listing):
    tails = [tuple(int(x) for x in r[1:]) for r in listing if r[0] == "tail"]
    assert {(a, t) for a, t, *_ in tails} == {(a, t) for a in SIZES + ODD for t in (1, 3, 16)}
    for a, trees, t, at, total in tails:
        rec = 16 + 12 * a + 16 * a + (4 if a % 2 else 0)
        assert at == trees * rec + 32 * t and total == trees * (rec + 32)
    (tail,) = [r for r in listing if r[0] == "tail_struct"]
    assert [int(x) for x in tail[1:]] == [32, 0, 4, 8, 16]            # {best, kind, pos, pad; cursor (int64), pad}
    (state,) = [r for r in listing if r[0] == "state"]
    assert [int(x) for x in state[1:]] == [0, 1, 2, 4, 1, 2]           # words: flags, passes, played of 4; bits: idle, never resign
    (kinds,) = [r for r in listing if r[0] == "kinds"]
    assert [int(x) for x in kinds[1:]] == [0, 1, 2, 3, 4]              # move, resign, second pass, move limit, idle


def test_analysis_record(listing):
    got = {(int(r[1]), int(r[2])): (int(r[3]), int(r[4]), rows_of(r[5:])) for r in listing if r[0] == "analysis"}
    for a in SIZES:
        for d in DEPTHS:
            size, pv, rows = got[(a, d)]
            ints = align8(16 + 16 * a)
            assert ints == 16 + 16 * a
            assert rows == [("action", 4, 16), ("visits", 4, 16 + 4 * a), ("pv_len", 4, 16 + 8 * a), ("resume", 4, 16 + 12 * a),
                            ("value_sum", 8, ints), ("policy", 8, ints + 8 * a)]
            assert pv == ints + 16 * a and pv % 8 == 0
            assert size - pv == align8(2 * a * d)
            # the size formula the record had before the header stated its layout
            assert size == ((16 + 16 * a + 7) & ~7) + 16 * a + ((2 * a * d + 7) & ~7)
    (head,) = [r for r in listing if r[0] == "analysis_head"]
    assert [int(x) for x in head[1:]] == [0, 1, 2, 3, 4]               # children, visits, value sum bits, err; 4 words
    (limits,) = [r for r in listing if r[0] == "analysis_limits"]
    assert [int(x) for x in limits[1:]] == [4, 1024]


def test_node_record_and_the_heads(listing):
    nodes = {int(r[1]): int(r[2]) for r in listing if r[0] == "node"}
    for a in SIZES:                                                    # (what tests/test_node_pool_host.py asserts)
        assert nodes[a] == ((32 + 4 * 4 * a + 7) & ~7) + 3 * 8 * a
    (head,) = [r for r in listing if r[0] == "node_head"]
    # children, visits, virtual loss, value sum bits, raw value bits, err, num_nodes, pad; 8 words = 32 bytes
    assert [int(x) for x in head[1:]] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 32]
    (root,) = [r for r in listing if r[0] == "root_head"]
    assert [int(x) for x in root[1:]] == [0, 1, 2, 3, 4]               # children, visits, raw value bits, err; 4 words


def test_error_text(listing):
    (flags,) = [r for r in listing if r[0] == "flags"]
    assert [int(x) for x in flags[1:]] == [POOL, RNG, PIPE, REROOT]
    text = {}
    for r in listing:
        if r[0] == "error":
            text[(int(r[1]), int(r[2]))] = " ".join(r[3:])[1:-1]
    assert sorted(text) == sorted(ERROR_WORDS)

    def said(tree, word):
        return {flag for flag, sub in TEXT.items() if sub in text[(tree, word)]}
    for tree, word in ERROR_WORDS[:4]:                                 # each flag alone: its text and no other
        assert said(tree, word) == {word}
    assert said(4, POOL | PIPE) >= {POOL}
    assert said(5, RNG | PIPE) == {RNG}                                # the random window takes precedence over the pipeline
    assert said(6, PIPE | (7 << 8)) == {PIPE}                          # (bits 8 and up: the site that set the flag)
    assert said(8, POOL | RNG | PIPE | REROOT) == {POOL, RNG, REROOT}
    for (tree, word), msg in text.items():
        if word:
            assert msg.startswith(f"tree {tree}: ") and f"0x{word:x}" in msg
    assert text[(7, 0)] == ""                                          # nothing set: nothing to say
