"""The device search (csrc/search.hip) vs the reference-generated hard-tree fixtures (needs a GPU).

tests/test_gpu_search.py holds the kernels to the reference under StubNet, whose searches stay shallow (26 levels at most),
tie rarely and never see an exact 0, 0.5 or 1.  The fixtures here (tests/golden/trees_hard_s{9,19}.json,
tools/gen_golden_hard_trees.py, evaluators in oracle/hardnets.py) reach what that leaves out:

  line_*    leaves far below the 48 recorded path levels (csrc/leaf_queue.h kPathCap): backup_kernel drops its partitioned
            walk and follows the parent pointers, in mini-batches that mix both kinds of leaf; finished games queued again and
            again inside one mini-batch (the stale-statistics forwarding of the backup); values exactly 0.5 and 1.
  flat_*, spiky_* (PUCT)   one selection in ten or more decided among exactly equal maxima, many of them past child 64 - the
            lowest lane + 64 r must win, not the lowest lane; zero priors; exact sums with inexact quotients.
  *_g*      sequential halving under zero logit spread (flat) and logits in [-32, 32) (spiky).

Exact equality is the only criterion: root arrays, move, node count, mini-batch sizes, whole-tree digest, stream position,
noise and improved policy, and the queued leaves as (node index, depth) - the first pair that differs names the descent that
went elsewhere.  tests/test_hard_trees_host.py shows on the CPU that a wrong tie-break or a backup cut short at level 48 would
change every case of its kind."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._hard_trees import GUMBEL, PATH_CAP, ChildRuns, check_product, names, product_search, records, tree_digest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# selection kernel -> environment, as tests/test_gpu_select_rcp.py VARIANTS
VARIANTS = {
    "pipe": {"TG_SELECT_MPIPE_TREES": "0"},
    "mpipe": {},
    "serial": {"TG_SELECT_SERIAL": "1"},
    "split": {"TG_SELECT_SPLIT": "1"},
}
# seconds a child process may take: twenty times what it was measured to take (run_variant), for a machine that loads the
# interpreter and the library cold
CHILD_TIMEOUT = {9: 60, 19: 60}


@pytest.mark.parametrize("name", list(records()))
def test_single_tree_equals_the_reference(name):
    rec = records()[name]
    tree, mv, net = product_search(rec)
    check_product(rec, tree, mv, net)


@pytest.mark.parametrize("name", GUMBEL)
def test_gumbel_one_by_one_equals_the_reference(name, monkeypatch):
    """The halving phases with node numbers handed out one by one through the job ring (TG_GUMBEL_ONE_BY_ONE, read at every
    launch: tests/test_gpu_search.py test_gumbel_phase_reports_a_full_node_pool)."""
    monkeypatch.setenv("TG_GUMBEL_ONE_BY_ONE", "1")
    rec = records()[name]
    tree, mv, net = product_search(rec)
    check_product(rec, tree, mv, net)


CHILDREN = ChildRuns()


def run_variant(variant, size):
    """name -> (digest, nodes) of every PUCT case of a board size, searched by ONE child process (the selection kernel is
    read from the environment once per process) under TG_DEBUG_KNOBS=1.  CHILDREN remembers what became of that child, its
    failure included: the other tests of the same (variant, size) fail on the remembered outcome and start nothing.  A child
    that runs into its timeout has hung, one that ends on a signal or an abort has faulted: neither is run again, and no
    child of ANY variant is started after it (tests/_hard_trees.py ChildRuns; tests/test_hard_trees_host.py shows it).
    Measured on an MI355X, start of the interpreter and of the library included: 9x9 (six cases) 2.8 s split, 3.0 s pipe,
    2.8 s mpipe, 2.9 s serial; 19x19 (three cases) 2.9 s split, 2.8 s pipe."""
    cases = names(kind="puct", size=size)

    def launch():
        env = dict(os.environ, TG_DEBUG_KNOBS="1", TG_SELECT_SPLIT="0")
        for key in ("TG_SELECT_SERIAL", "TG_SELECT_MPIPE_TREES", "TG_SPLIT_CFG", "TG_GUMBEL_ONE_BY_ONE"):
            env.pop(key, None)
        env.update(VARIANTS[variant])
        return subprocess.run([sys.executable, os.path.join(HERE, "_hard_trees.py")] + cases, env=env, capture_output=True,
                              text=True, timeout=CHILD_TIMEOUT[size])

    res = CHILDREN.run((variant, size), launch)
    out = {}
    for line in res.stdout.strip().splitlines()[-len(cases):]:
        name, digest, nodes = line.split()
        out[name] = (digest, int(nodes))
    return out


@pytest.mark.parametrize("variant", ["split", "pipe", "mpipe", "serial"])
@pytest.mark.parametrize("name", names(kind="puct", size=9))
def test_every_selection_kernel_builds_the_reference_tree_9x9(name, variant):
    rec = records()[name]
    assert run_variant(variant, 9)[name] == (rec["digest"], rec["num_nodes"]), (name, variant)


@pytest.mark.parametrize("variant", ["split", "pipe"])
@pytest.mark.parametrize("name", names(kind="puct", size=19))
def test_every_selection_kernel_builds_the_reference_tree_19x19(name, variant):
    rec = records()[name]
    assert run_variant(variant, 19)[name] == (rec["digest"], rec["num_nodes"]), (name, variant)


def test_lockstep_one_deep_tree_among_shallow_neighbours():
    """Five trees in one SearchEngine, mini-batches of 8, 400 visits, one HostEvaluator: tree 0 walks LineNet("half")'s line
    from the empty board - its leaves pass level 48, so its share of a backup launch falls to the one-wave walk - while trees
    1-4, on the ragged openings of tests/_select_rcp_digest.py (tree 1 on a superko position of the rule corpus) under StubNet,
    stay shallow and keep the partitioned one.  The trees are independent given their streams: each must equal its own
    single-tree oracle search, node for node."""
    import torch
    from oracle.board import GoBoard as OBoard
    from oracle.hardnets import LeafLog, LineNet, line_outputs
    from oracle.stubnet import StubNet, stub_outputs
    from oracle.tree import MCTSTree as OTree, TimeControl, TimeManager
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    from tests import _rule_corpus

    size, T, K, visits, salt = 9, 5, 8, 400, 3

    class Mixed:
        """rows of tree 0 (the first of T equal shares of a mini-batch) from LineNet, the others from StubNet"""

        def inference(self, planes):
            x = planes.numpy()
            per = x.shape[0] // T
            assert per * T == x.shape[0]
            lp, _, lv = line_outputs(x[:per], "half")
            sp, _, sv = stub_outputs(x[per:], salt)
            return torch.from_numpy(np.concatenate([lp, sp])), torch.from_numpy(np.concatenate([lv, sv]))

    eng = SearchEngine(size, T, visits + 16, K, HostEvaluator(Mixed(), torch.device("cuda:0")), check_superko=True)
    superko = next(e for e in _rule_corpus.load_fixture(size).entries if e.name.startswith("ko_expired:"))
    rs = np.random.RandomState(5)
    roots = []
    for t in range(T):
        b, ob, c = GoBoard(size, 7.0, True), OBoard(size, 7.0, True), 1
        stones = [int(p) for p in superko.moves] if t == 1 else []
        for pos in stones:
            b.put_stone(pos, c)
            ob.put_stone(pos, c)
            c = 3 - c
        for _ in range(0 if t == 1 else t % 9):
            while True:
                pos = b.onboard_pos[rs.randint(len(b.onboard_pos))]
                if b.is_legal(pos, c):
                    break
            b.put_stone(pos, c)
            ob.put_stone(pos, c)
            c = 3 - c
        eng.set_root(t, b, c, np.random.RandomState(100 + t).get_state())
        roots.append((ob, c))
    eng.root_eval(False)
    for _ in range(visits // K):
        eng.puct_batch(K)
    nodes = eng.num_nodes()

    class View:
        """tree t of the engine as tree_digest reads a tree"""

        def __init__(self, t):
            self.t = t

        @property
        def node(self):
            return self

        def __getitem__(self, i):
            return eng.read_node(self.t, i)

    for t, (oboard, color) in enumerate(roots):
        net = LeafLog(LineNet("half") if t == 0 else StubNet(salt))
        otree = OTree(net, size, tree_size=visits + 16, batch_size=K)
        net.watch(otree)
        np.random.set_state(np.random.RandomState(100 + t).get_state())
        otree.search_best_move(oboard, color, TimeManager(TimeControl.STRICT_PLAYOUT, visits))
        depths = [[d for _, d in batch] for batch in net.leaves]
        deep = sum(d > PATH_CAP for batch in depths for d in batch)
        if t == 0:        # the point of the case: leaves on both sides of the path cap, some within one mini-batch
            assert deep >= 50 and any(min(batch) <= PATH_CAP < max(batch) for batch in depths)
        else:
            assert deep == 0
        assert int(nodes[t]) == otree.num_nodes, t
        assert tree_digest(View(t), int(nodes[t])) == tree_digest(otree, otree.num_nodes), t
    eng.close()
