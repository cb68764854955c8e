"""Grouped ranks on the CPU: csrc/group_rank.h - the rule group_rank_kernel compiles, the per-group carry between
chunks included - built alone into tests/group_rank_driver.cpp with the host compiler and held to a numpy stable argsort; the
proof that the corpus tells the right rule from five wrong ones; the same driver once more under the address and undefined
behaviour sanitizers (a stand-alone program, no Python in the process).  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "tamago_amd", "csrc")

RIGHT, INCLUSIVE_OFFSET, COUNTS_ITSELF, DROPPED_CARRY, ALL_GROUPS_CARRY, DESCENDING = range(6)
GROUP_COUNTS = (1, 2, 3, 64)


def chunk_size():
    return int(re.search(r"constexpr int kChunk = (\d+);", open(os.path.join(CSRC, "live_rank.h")).read()).group(1))


def tree_counts():
    chunk = chunk_size()
    sizes = {1, 63, 64, 65, 1024, 1025, 2049}
    if chunk != 1024:
        sizes |= {chunk - 1, chunk, chunk + 1, 2 * chunk + 1}
    return sorted(sizes)


def compiler():
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    return cxx


def runner(exe):
    def run(rows, rule=RIGHT):
        """rows: (err [T], halt [T], num_nodes [T], group [T], G) -> (count [G], offset [G], rank [T]) per row"""
        text = "".join("%d %d %d %s\n" % (rule, len(err), G, " ".join("%d %d %d %d" % w for w in zip(err, halt, nodes, group)))
                       for err, halt, nodes, group, G in rows)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        out = [np.array(line.split(), dtype=np.int64) for line in res.stdout.splitlines()]
        assert len(out) == len(rows)
        return [(o[:row[4]], o[row[4]:2 * row[4]], o[2 * row[4]:]) for o, row in zip(out, rows)]
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("group_rank") / "driver")
    subprocess.check_call([compiler(), "-std=c++17", "-O1", os.path.join(HERE, "group_rank_driver.cpp"), "-o", exe])
    return runner(exe)


def expected(err, halt, nodes, group, G):
    """The issue's words: count[g] the live trees of group g, offset[g] the counts of the groups before g, a live tree's rank
    its place in a STABLE sort of the live trees by group, -1 for a tree that is not live."""
    live = (np.asarray(err) == 0) & (np.asarray(halt) == 0) & (np.asarray(nodes) > 0)
    group = np.asarray(group)
    trees = np.flatnonzero(live)
    order = trees[np.argsort(group[trees], kind="stable")]
    rank = np.full(len(group), -1, dtype=np.int64)
    rank[order] = np.arange(len(order))
    count = np.bincount(group[trees], minlength=G)[:G]
    return count, np.cumsum(count) - count, rank


def masks(T, rnd):
    """Halt masks: none halted, all halted, alternating, only the first tree live, only the last tree live, random."""
    only_first, only_last = np.ones(T, int), np.ones(T, int)
    only_first[0] = 0
    only_last[-1] = 0
    return [np.zeros(T, int), np.ones(T, int), np.arange(T) % 2, only_first, only_last, (rnd.random_sample(T) < 0.4).astype(int)]


def patterns(T, G, rnd):
    """Group ids: all one group (the last), round-robin, descending, random, one group empty in the middle, a group present
    only beyond the first chunk."""
    t = np.arange(T)
    middle = rnd.randint(0, G, T)
    if G >= 3:
        middle = np.where(middle == G // 2, G - 1, middle)
    beyond = rnd.randint(0, max(G - 1, 1), T)
    beyond[chunk_size():] = np.where(rnd.random_sample(max(T - chunk_size(), 0)) < 0.5, G - 1, beyond[chunk_size():])
    return [np.full(T, G - 1), t % G, (G - 1) - (t * G) // T, rnd.randint(0, G, T), middle, beyond]


def corpus():
    rows = []
    for T in tree_counts():
        for G in GROUP_COUNTS:
            rnd = np.random.RandomState(1000 * G + T)
            for group in patterns(T, G, rnd):
                for halt in masks(T, rnd):
                    rows.append((np.zeros(T, int), halt, np.ones(T, int), group, G))
                # ... mixed with sticky error words (any non-zero word), halt words of any value and rootless trees
                err = np.where(rnd.random_sample(T) < 0.2, rnd.choice([1, 2, 4, 8, -1], T), 0)
                nodes = np.where(rnd.random_sample(T) < 0.2, 0, rnd.randint(1, 500, T))
                rows.append((err, rnd.choice([0, 0, 0, 1, 7, -3], T), nodes, group, G))
    return rows


@pytest.fixture(scope="module")
def rows():
    return corpus()


def mismatches(rows, got):
    bad = []
    for row, (count, offset, rank) in zip(rows, got):
        want = expected(*row)
        if not all(np.array_equal(a, b) for a, b in zip((count, offset, rank), want)):
            bad.append((len(row[0]), row[4]))
    return bad


def test_the_header_against_a_stable_argsort(driver, rows):
    assert mismatches(rows, driver(rows)) == []


@pytest.mark.parametrize("rule", [INCLUSIVE_OFFSET, COUNTS_ITSELF, DROPPED_CARRY, ALL_GROUPS_CARRY, DESCENDING],
                         ids=["inclusive_offsets", "counts_itself", "dropped_carry", "carry_over_all_groups", "descending_groups"])
def test_the_corpus_tells_the_rule_from_the_wrong_ones(driver, rows, rule):
    """Inclusive offsets and a position that counts the tree itself show with a single tree; a carry dropped between chunks
    only beyond one chunk; a carry over all groups only beyond one chunk AND with more than one group; descending groups only
    with more than one group."""
    chunk = chunk_size()
    wrong = mismatches(rows, driver(rows, rule))
    assert wrong, rule
    sizes, groups = {T for T, _ in wrong}, {G for _, G in wrong}
    if rule in (INCLUSIVE_OFFSET, COUNTS_ITSELF):
        assert (1, 1) in wrong and 65 in sizes
    elif rule == DROPPED_CARRY:
        assert min(sizes) > chunk and {chunk + 1, 2 * chunk + 1} <= sizes and 1 in groups
    elif rule == ALL_GROUPS_CARRY:
        assert min(sizes) > chunk and 2 * chunk + 1 in sizes and 1 not in groups and {2, 3, 64} <= groups
    else:
        assert 1 not in groups and {2, 3, 64} <= groups and 63 in sizes


def test_the_driver_under_the_sanitizers(tmp_path, rows):
    """The same program built with -fsanitize=address,undefined over a slice of the corpus that has every tree count and
    every group count: a report ends the program with a non-zero status."""
    exe = str(tmp_path / "driver_san")
    subprocess.check_call([compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "group_rank_driver.cpp"), "-o", exe])
    part = rows[::7]
    assert {len(r[0]) for r in part} == set(tree_counts()) and {r[4] for r in part} == set(GROUP_COUNTS)
    run = runner(exe)
    for rule in range(6):
        got = run(part, rule)
        if rule == RIGHT:
            assert mismatches(part, got) == []
