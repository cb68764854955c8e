"""Helper of test_gpu_board_rules.py (run as a script: the selection kernel variant is chosen from the environment once per
process).  argv = mode, size, output file.

puct:   the tree roots of the rule corpus (tests/_rule_corpus.py) in one engine, check_superko on, StubNet(3), batch 16:
        root_eval, then mini-batches of 16, 16 and 9 descents.  Written per tree t: n{t} nodes; a{t} / c{t} the action lists
        and children_index of its nodes back to back with o{t} their offsets; q{t} the node index of every evaluated leaf in
        evaluation order (tg_search_read_queue before each backup; the root first) and p{t} the planes the evaluator got.
gumbel: generate_move_with_sequential_halving from the first roots, 16 and 50 simulations, evaluated leaf by leaf and
        (u1) in the unique-leaf layout.  Written per search k = (root, simulations, unique): n{k}, a{k}, c{k}, o{k}."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import _rule_corpus as rc
from oracle.stubnet import StubNet
from tamago_amd import lib as _lib
from tamago_amd.board.go_board import GoBoard
from tamago_amd.mcts.engine import HostEvaluator, SearchEngine

BATCHES = (16, 16, 9)
GUMBEL_ROOTS = {9: 8, 19: 4}
GUMBEL_SIMS = (16, 50)


def host_board(entry, superko=True):
    board = GoBoard(entry.size, 7.0, superko)
    color = 1
    for pos in entry.moves:
        board.put_stone(pos, color)
        color = 3 - color
    return board


class KeepPlanes(HostEvaluator):
    def __init__(self, network, device):
        super().__init__(network, device)
        self.kept = []

    def __call__(self, planes, want_logits):
        self.kept.append(planes.cpu().numpy().copy())
        return super().__call__(planes, want_logits)


def pack_nodes(out, key, nodes):
    off = np.zeros(len(nodes) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(a) for a, _ in nodes])
    out[f"n{key}"] = np.int32(len(nodes))
    out[f"o{key}"] = off
    out[f"a{key}"] = np.concatenate([np.asarray(a, dtype=np.int32) for a, _ in nodes])
    out[f"c{key}"] = np.concatenate([np.asarray(c, dtype=np.int32) for _, c in nodes])


def read_nodes(read_node, count):
    nodes = []
    for index in range(count):
        view = read_node(index)
        n = view.num_children
        nodes.append((list(view.action[:n]), [int(c) for c in view.children_index[:n]]))
    return nodes


def run_puct(size, path):
    fx = rc.load_fixture(size)
    roots = [fx.entries[i] for i in fx.tree_roots]
    T = len(roots)
    evaluator = KeepPlanes(StubNet(3), torch.device("cuda:0"))
    eng = SearchEngine(size, T, 64, 16, evaluator, check_superko=True)
    for t, entry in enumerate(roots):
        eng.set_root(t, host_board(entry), entry.to_move, np.random.RandomState(100 + t).get_state())
    eng.root_eval(False)
    queue = [[0] for _ in range(T)]
    planes = [[evaluator.kept[0][t]] for t in range(T)]
    for leaves in BATCHES:
        eng.puct_select(leaves)
        counts = []
        for t in range(T):
            idx = np.zeros(eng.K, dtype=np.int32)
            n = ctypes.c_int32(0)
            _lib.check(eng.lib.tg_search_read_queue(eng.handle, t, idx.ctypes.data, eng.K, ctypes.byref(n)),
                       "tg_search_read_queue")
            queue[t] += [int(v) for v in idx[:n.value]]
            counts.append(n.value)
        eng.puct_flush()
        got = evaluator.kept[-1]
        assert got.shape[0] == T * leaves
        for t in range(T):
            planes[t] += list(got[t * leaves:t * leaves + counts[t]])
    torch.cuda.synchronize()
    out = {}
    nn = eng.num_nodes()
    for t in range(T):
        pack_nodes(out, t, read_nodes(lambda i, t=t: eng.read_node(t, i), int(nn[t])))
        out[f"q{t}"] = np.asarray(queue[t], dtype=np.int32)
        out[f"p{t}"] = np.stack(planes[t]).astype(np.float32)
    np.savez(path, **out)
    print("puct", size, T, int(nn.sum()))


def run_gumbel(size, path):
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    fx = rc.load_fixture(size)
    roots = [fx.entries[i] for i in fx.tree_roots[:GUMBEL_ROOTS[size]]]
    out = {}
    total = 0
    for r, entry in enumerate(roots):
        board = host_board(entry)
        for sims in GUMBEL_SIMS:
            for unique in (0, 1):
                np.random.seed(1000 + 10 * r + sims)
                tree = MCTSTree(StubNet(3), tree_size=256, batch_size=16, unique_leaves=bool(unique))
                manager = TimeManager(TimeControl.CONSTANT_PLAYOUT, constant_visits=sims)
                tree.generate_move_with_sequential_halving(board, entry.to_move, manager, True)
                pack_nodes(out, f"_{r}_{sims}_u{unique}", read_nodes(lambda i: tree.node[i], tree.num_nodes))
                total += tree.num_nodes
                tree._engine.close()
    np.savez(path, **out)
    print("gumbel", size, len(roots), total)


if __name__ == "__main__":
    mode, size, path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    {"puct": run_puct, "gumbel": run_gumbel}[mode](size, path)
