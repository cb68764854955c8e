"""The visit-budget rules on the CPU: csrc/visit_budget.h - the descents a tree makes in a mini-batch and the test that its
budget is spent, which the four PUCT selectors and budget_rule_kernel compile - built alone into tests/visit_budget_driver.cpp
with the host compiler (address and undefined-behaviour sanitizers where the compiler has them) and held to a Python
restatement over an exhaustive small grid; and the proof on the oracle that a search cut into mini-batches by the per-batch
rule is the search MCTSTree runs.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def descents(total, visits, max_leaves):
    return max(0, min(total - visits, max_leaves))


def spent(total, visits):
    return total - visits <= 0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("visit_budget") / "driver")
    base = [cxx, "-std=c++17", "-O1", os.path.join(HERE, "visit_budget_driver.cpp"), "-o", exe]
    # a stand-alone program with its own main: the sanitizers' runtimes are linked in, nothing is preloaded
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    probe = sanitized.returncode == 0 and subprocess.run([exe], input="1 0 1\n", capture_output=True, text=True)
    if not probe or probe.returncode != 0 or probe.stdout.split() != ["1", "0"]:
        subprocess.check_call(base)                    # (a compiler or a host without the sanitizer runtimes)

    def run(rows):
        text = "".join("%d %d %d\n" % row for row in rows)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        out = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
        assert len(out) == len(rows)
        return out
    return run


def test_rules_against_python_over_the_grid(driver):
    rows = [(total, visits, k) for total in range(1, 41) for visits in range(0, 46) for k in range(0, 10)]
    got = driver(rows)
    for row, (n, done) in zip(rows, got):
        assert n == descents(*row), row
        assert bool(done) == spent(row[0], row[1]), row
        assert 0 <= n <= row[2]
        assert (n == 0) == (done or row[2] == 0), row     # a tree is passed by exactly when nothing is owed (or no slot given)


def test_int32_edges(driver):
    big = 2 ** 31 - 1
    rows = [(big, 0, 8), (big, big, 8), (big, big - 3, 8), (1, big, 8), (1, 0, big), (big, 0, big)]
    assert driver(rows) == [(8, 0), (0, 1), (3, 0), (0, 1), (1, 0), (big, 0)]


def _batches_of_a_search(kept_plies, total, batch):
    """An oracle tree searched to `total` visits, its root advanced by its best moves `kept_plies` times (the subtree
    kept, as tree reuse keeps it), then searched to `total` again: the root's visits before each mini-batch of the second
    search and the leaves it evaluated."""
    from oracle.board import GoBoard
    from oracle.stubnet import StubNet
    from oracle.tree import MCTSTree, TimeControl, TimeManager
    from tests._tree_reuse import emulate_search, oracle_child
    tm = TimeManager(TimeControl.STRICT_PLAYOUT, total)
    tree = MCTSTree(StubNet(7), 9, tree_size=total + 16, batch_size=batch)
    board, color = GoBoard(9, 7.0, False), 1
    saved = np.random.get_state()
    np.random.seed(11)
    try:
        emulate_search(tree, board, color, tm)
        node = 0
        for _ in range(kept_plies):
            root = tree.node[node]
            move = root.action[root.best_move_index()]
            node = oracle_child(tree, node, move)
            assert node >= 0
            board.put_stone(move, color)
            color = 3 - color
        kept = tree.node[node].node_visits
        seen = []
        inner = tree.process_mini_batch

        def tap(*args, **kwargs):
            seen.append((int(tree.node[0].node_visits), len(tree.batch_queue.node_index)))
            return inner(*args, **kwargs)
        tree.process_mini_batch = tap
        emulate_search(tree, board, color, tm, reuse_root=node)
        return int(kept), seen
    finally:
        np.random.set_state(saved)


@pytest.mark.parametrize("kept_plies,total,batch", [(1, 60, 8), (2, 60, 8), (1, 45, 6), (1, 26, 8)])
def test_per_batch_recomputation_is_the_search(kept_plies, total, batch):
    """The mini-batches of a reused search - [K] * (n // K) + [n % K] for n = total - kept visits - are what the selectors'
    rule gives batch by batch: min(K, total - the root's visits before the batch), until nothing is owed."""
    kept, seen = _batches_of_a_search(kept_plies, total, batch)
    owed = total - kept
    assert 0 < kept < total
    want = [batch] * (owed // batch) + ([owed % batch] if owed % batch else [])
    assert [n for _, n in seen] == want
    assert [descents(total, visits, batch) for visits, _ in seen] == want
    assert seen[0][0] == kept and seen[-1][0] + seen[-1][1] == total
    assert not spent(total, seen[-1][0]) and spent(total, seen[-1][0] + seen[-1][1])
