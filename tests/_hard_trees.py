"""Helper of test_hard_trees_host.py and test_gpu_hard_trees.py: the searches recorded in tests/golden/trees_hard_s{9,19}.json
(tools/gen_golden_hard_trees.py: the reference's own MCTSTree under oracle/hardnets.py's LineNet, FlatNet and SpikyNet) run again
on the oracle tree and on the device tree, and the comparison of what they leave behind.

As a script it is the child process of the kernel-variant tests (the selection kernel is chosen from the environment once per
process, as in _select_rcp_digest.py):  argv = case names; one line "name digest nodes" per case, the digest over the WHOLE tree
as the fixtures record it.

What a record pins besides gen_golden.py's root record: `leaves`, the queued leaves in order as (node index, depth) - the first
pair that differs names the descent that went elsewhere, and the level it ended on."""
import functools
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.hardnets import LeafLog, make_net  # noqa: E402
from tests.helpers import load_json, load_npz, unhex  # noqa: E402

PATH_CAP = 48           # csrc/leaf_queue.h kPathCap: a leaf below this level has no recorded path


@functools.lru_cache(maxsize=None)
def records():
    """name -> record, in the fixtures' order (9x9 first)."""
    out = {}
    for size in (9, 19):
        for rec in load_json(f"trees_hard_s{size}.json"):
            out[rec["name"]] = dict(rec, size=size)
    return out


def names(kind=None, evaluators=None, size=None):
    return [n for n, r in records().items()
            if (kind is None or r["kind"] == kind) and (evaluators is None or r["evaluator"] in evaluators)
            and (size is None or r["size"] == size)]


LINE = names(evaluators=("line_half", "line_win"))
TIES = names(kind="puct", evaluators=("flat", "spiky"))
GUMBEL = names(kind="gumbel")


def tree_digest(tree, num_nodes):
    """The fixtures' digest: tests/test_oracle_tree.py tree_digest, tests/test_gpu_search.py product_digest."""
    h = hashlib.sha256()
    for i in range(num_nodes):
        nd = tree.node[i]
        n = nd.num_children
        h.update(np.array(nd.action[:n], dtype=np.int32).tobytes())
        h.update(nd.children_index[:n].astype(np.int32).tobytes())
        h.update(nd.children_visits[:n].astype(np.int32).tobytes())
        h.update(nd.children_virtual_loss[:n].astype(np.int32).tobytes())
        h.update(nd.children_value_sum[:n].astype(np.float64).tobytes())
        h.update(nd.children_policy[:n].astype(np.float64).tobytes())
        h.update(np.array([nd.node_visits, nd.virtual_loss], dtype=np.int64).tobytes())
    return h.hexdigest()


def first_difference(got, want):
    """Where two leaf sequences part, as text for an assertion message."""
    for i, (a, b) in enumerate(zip(got, want)):
        if list(a) != list(b):
            return f"leaf {i}: (node, depth) {tuple(a)} instead of {tuple(b)}"
    if len(got) != len(want):
        return f"{len(got)} leaves instead of {len(want)}"
    return ""


def flat_leaves(log: LeafLog):
    return [[int(node), int(depth)] for batch in log.leaves for node, depth in batch]


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def oracle_search(rec, tree_cls=None):
    """(tree, move, LeafLog) of the oracle's run of a record; tree_cls: an oracle.tree.MCTSTree subclass (the mutants)."""
    from oracle.tree import MCTSTree, TimeControl, TimeManager
    from tests.helpers import oracle_replay
    size = rec["size"]
    brd = load_npz(f"board_s{size}.npz")
    board = oracle_replay(size, brd["g0_move"], brd["g0_color"], rec["ply"], rec["superko"])
    net = LeafLog(make_net(rec["evaluator"], rec["seed"]))
    np.random.seed(rec["seed"])
    if rec["kind"] == "puct":
        tree = (tree_cls or MCTSTree)(net, size, tree_size=2048, batch_size=rec["batch"])
        net.watch(tree)
        mv = tree.search_best_move(board, rec["color"], TimeManager(TimeControl.STRICT_PLAYOUT, rec["visits"]))
    else:
        tree = (tree_cls or MCTSTree)(net, size, tree_size=2048)
        net.watch(tree)
        mv = tree.generate_move_with_sequential_halving(board, rec["color"],
                                                        TimeManager(TimeControl.CONSTANT_PLAYOUT, rec["visits"]), True)
    return tree, mv, net


def check_oracle(rec, tree, mv, net):
    """Everything a record holds, exactly (tests/test_oracle_tree.py check_root and what its tests add)."""
    from tests.test_oracle_tree import check_root
    assert net.calls == rec["batches"]
    got = flat_leaves(net)
    assert got == rec["leaves"], first_difference(got, rec["leaves"])
    check_root(tree, mv, rec)
    if rec["kind"] == "gumbel":
        root = tree.get_root()
        assert np.array_equal(root.noise, unhex(rec["noise"]))
        assert np.array_equal(root.improved_policy(), unhex(rec["improved"]))
    assert float(np.random.random_sample()) == float.fromhex(rec["rng_after"])


# ---- the device tree --------------------------------------------------------------------------------------------------------
def queued_leaves(engine, tree_index: int = 0):
    """(node index, depth) of the leaves in the device queue of one tree: the queue's node numbers, and the length of each
    leaf's path as the parent pointers give it (tg_search_read_path: not the recorded path, which ends at level 48)."""
    import ctypes
    from tamago_amd import lib as _lib
    idx = np.zeros(engine.K, dtype=np.int32)
    n = ctypes.c_int32(0)
    _lib.check(engine.lib.tg_search_read_queue(engine.handle, tree_index, idx.ctypes.data, engine.K, ctypes.byref(n)),
               "tg_search_read_queue")
    return [(int(idx[k]), len(engine.read_path(tree_index, k))) for k in range(n.value)]


def product_search(rec, with_leaves=True):
    """(tree, move, LeafLog) of the device tree's run of a record."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    size = rec["size"]
    brd = load_npz(f"board_s{size}.npz")
    board = GoBoard(size, 7.0, rec["superko"])
    for mv, c in zip(brd["g0_move"][:rec["ply"]], brd["g0_color"][:rec["ply"]]):
        board.put_stone(int(mv), int(c))
    net = LeafLog(make_net(rec["evaluator"], rec["seed"]))
    np.random.seed(rec["seed"])
    if rec["kind"] == "puct":
        tree = MCTSTree(net, tree_size=2048, batch_size=rec["batch"])
        net.watch(probe=(lambda: queued_leaves(tree._engine)) if with_leaves else (lambda: []))
        mv = tree.search_best_move(board, rec["color"], TimeManager(TimeControl.STRICT_PLAYOUT, rec["visits"]), {})
    else:
        tree = MCTSTree(net, tree_size=2048)
        net.watch(probe=(lambda: queued_leaves(tree._engine)) if with_leaves else (lambda: []))
        mv = tree.generate_move_with_sequential_halving(board, rec["color"],
                                                        TimeManager(TimeControl.CONSTANT_PLAYOUT, rec["visits"]), True)
    return tree, mv, net


def check_product(rec, tree, mv, net):
    """Exact equality with the record: the root arrays, the move, the node count and the whole-tree digest (check_root), the
    mini-batch sizes, the leaf sequence, the stream position and, for a Gumbel case, the noise and the improved policy."""
    from tests.test_gpu_search import check_root
    assert net.calls == rec["batches"]
    got = flat_leaves(net)
    assert got == rec["leaves"], first_difference(got, rec["leaves"])
    check_root(tree, mv, rec)
    if rec["kind"] == "gumbel":
        root = tree.get_root()
        assert np.array_equal(root.noise, unhex(rec["noise"]))
        assert np.array_equal(root.calculate_improved_policy(), unhex(rec["improved"]))
    assert float(np.random.random_sample()) == float.fromhex(rec["rng_after"])


class ChildFailed(AssertionError):
    pass


class ChildRuns:
    """Child processes of a test module, each started at most once: run(key, launch) calls launch() -> a
    subprocess.CompletedProcess the first time a key is asked for and remembers what became of it - the result, or the
    failure, which every later call for the key raises again without starting anything.  (functools.lru_cache remembers no
    exception: the next test that shares the key would start the failed child again.)  A child that ran into its timeout has
    hung, one that ended on a signal or on 134 / 139 / 124 / 137 has faulted: from then on no child is started for ANY key,
    the device is left alone."""
    FAULT_STATUS = (134, 139, 124, 137)

    def __init__(self):
        self.outcome = {}           # key -> CompletedProcess | ChildFailed
        self.stopped = None         # why nothing is started any more

    def run(self, key, launch):
        import subprocess
        if key not in self.outcome:
            if self.stopped:
                self.outcome[key] = ChildFailed(f"{key}: not started - {self.stopped}")
            else:
                try:
                    res = launch()
                except subprocess.TimeoutExpired as exc:
                    self.stopped = f"the child of {key} ran into its timeout of {exc.timeout} s (a hang: not run again)"
                    self.outcome[key] = ChildFailed(self.stopped)
                else:
                    if res.returncode == 0:
                        self.outcome[key] = res
                    else:
                        text = f"the child of {key} ended with status {res.returncode}"
                        if res.returncode < 0 or res.returncode in self.FAULT_STATUS:
                            self.stopped = text + " (a fault: nothing more is started)"
                        self.outcome[key] = ChildFailed(text + ": " + (res.stdout or "")[-1000:] + (res.stderr or "")[-2000:])
        got = self.outcome[key]
        if isinstance(got, ChildFailed):
            raise got
        return got


def main(argv):
    for name in argv:
        tree, _, _ = product_search(records()[name], with_leaves=False)
        print(name, tree_digest(tree, tree.num_nodes), tree.num_nodes, flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
