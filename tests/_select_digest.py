"""Helper of test_gpu_search.py::test_pipelined_selection_equals_serial (run as a script: the
selection kernel variant is chosen from the environment once per process).  Prints a digest of
the trees after a few PUCT mini-batches: argv = size, trees, batch, mini-batches [, "corpus": the roots are the dense tree roots
of the rule corpus (tests/_rule_corpus.py: fights with captures, kos, eyes and large strings) instead of a few random stones]."""
import os, sys, hashlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from oracle.stubnet import StubNet
from tamago_amd.board.go_board import GoBoard
from tamago_amd.mcts.engine import SearchEngine, HostEvaluator
size = int(sys.argv[1]); T = int(sys.argv[2]); batch = int(sys.argv[3]); nb = int(sys.argv[4])
eng = SearchEngine(size, T, batch * nb + 16, batch, HostEvaluator(StubNet(3), torch.device("cuda:0")), check_superko=True)
rs = np.random.RandomState(5)
dense = None
if len(sys.argv) > 5 and sys.argv[5] == "corpus":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _rule_corpus
    fx = _rule_corpus.load_fixture(size)
    dense = [fx.entries[i] for i in fx.tree_roots]
    assert T == len(dense)
for t in range(T):
    b = GoBoard(size, 7.0, True); c = 1
    for pos in (dense[t].moves if dense else ()):
        b.put_stone(pos, c); c = 3 - c
    for _ in range(0 if dense else t % 9):
        while True:
            pos = b.onboard_pos[rs.randint(len(b.onboard_pos))]
            if b.is_legal(pos, c): break
        b.put_stone(pos, c); c = 3 - c
    eng.set_root(t, b, c, np.random.RandomState(100 + t).get_state())
eng.root_eval(False)
for i in range(nb):
    eng.puct_batch(batch if i < nb - 1 else batch - 7)
h = hashlib.sha256()
st = eng.read_root_stats()
for k in sorted(st): h.update(np.ascontiguousarray(st[k]).tobytes())
nn = eng.num_nodes(); h.update(nn.tobytes())
for t in range(0, T, max(1, T // 8)):
    for node in range(0, int(nn[t]), 7):
        nd = eng.read_node(t, node)
        n = nd.num_children
        for arr in (nd.children_index[:n], nd.children_visits[:n], nd.children_virtual_loss[:n], nd.children_value_sum[:n], nd.children_policy[:n]):
            h.update(np.ascontiguousarray(arr).tobytes())
print(h.hexdigest()[:16], int(nn.sum()))
