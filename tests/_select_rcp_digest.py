"""Helper of test_gpu_select_rcp.py and tools/gen_golden_select_rcp.py (run as a script, like _select_digest.py: the selection
kernel variant is chosen from the environment once per process).  Prints a digest of the WHOLE trees (every node, node scalars
included) after a few PUCT mini-batches:  argv = size, trees, comma-separated mini-batch sizes.

Roots: tree t gets t % 9 seeded random opening stones (ragged roots), except tree 1, which stands on a superko position of the
rule corpus (the first "ko_expired" entry of tests/golden/rule_corpus_s<size>.npz: the retake is forbidden by superko alone).
Evaluator: the stub network of _select_digest.py.  CASES names the configurations whose digests, built by the one-wavefront
kernel (IEEE divisions and __dsqrt_rn, every node loaded from the pool at every step), are recorded in
tests/golden/select_rcp_digests.json."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

K_RCP_N = 2048          # csrc/search.hip kRcpN: the length of the split selector's reciprocal table

# name -> argv.  "boundary": the root's count passes kRcpN inside the search (where a reciprocal table gives way to the
# division sequence), in more mini-batches than any other case: 33 launches that each start from the root's stored statistics.
CASES = {
    "9x9_96": "9 5 32,32,32",
    "9x9_100_short_last": "9 5 32,32,32,4",
    "19x19_48": "19 2 16,16,16",
    "9x9_boundary": "9 2 " + ",".join(["64"] * ((K_RCP_N + 64) // 64)),
}


def main(argv):
    import numpy as np
    import torch
    import _rule_corpus
    from oracle.stubnet import StubNet
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import SearchEngine, HostEvaluator
    size, T = int(argv[0]), int(argv[1])
    batches = [int(v) for v in argv[2].split(",")]
    eng = SearchEngine(size, T, sum(batches) + 16, max(batches), HostEvaluator(StubNet(3), torch.device("cuda:0")),
                       check_superko=True)
    fx = _rule_corpus.load_fixture(size)
    superko = next(e for e in fx.entries if e.name.startswith("ko_expired:"))
    rs = np.random.RandomState(5)
    for t in range(T):
        b = GoBoard(size, 7.0, True)
        c = 1
        if t == 1:
            for pos in superko.moves:
                b.put_stone(int(pos), c)
                c = 3 - c
        for _ in range(0 if t == 1 else t % 9):
            while True:
                pos = b.onboard_pos[rs.randint(len(b.onboard_pos))]
                if b.is_legal(pos, c):
                    break
            b.put_stone(pos, c)
            c = 3 - c
        eng.set_root(t, b, c, np.random.RandomState(100 + t).get_state())
    eng.root_eval(False)
    for leaves in batches:
        eng.puct_batch(leaves)
    h = hashlib.sha256()
    st = eng.read_root_stats()
    for k in sorted(st):
        h.update(np.ascontiguousarray(st[k]).tobytes())
    nn = eng.num_nodes()
    h.update(nn.tobytes())
    for t in range(T):
        for node in range(int(nn[t])):
            nd = eng.read_node(t, node)
            n = nd.num_children
            h.update(np.array([n, nd.node_visits, nd.virtual_loss], dtype=np.int32).tobytes())
            for arr in (nd.children_index[:n], nd.children_visits[:n], nd.children_virtual_loss[:n], nd.children_value_sum[:n],
                        nd.children_policy[:n]):
                h.update(np.ascontiguousarray(arr).tobytes())
    print(h.hexdigest()[:16], int(nn.sum()), int(st["node_visits"].max()))


if __name__ == "__main__":
    main(sys.argv[1:])
