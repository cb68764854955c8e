"""Helper of test_gpu_leaf_queue.py (run as a script, like _select_digest.py: the selection kernel variant is chosen from the
environment once per process).  9x9, 2 trees, tree_size 80, batch 24: root_eval, then two PUCT selection launches of 24 descents
with a backup between them.  Prints "QUEUE <kernel of the launch plan> <digest>": the digest is over the device leaf queue after
each selection - per tree the count and node indices of tg_search_read_queue and tg_search_read_path of every slot."""
import ctypes, os, sys, hashlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from oracle.stubnet import StubNet
from tamago_amd import lib as tl
from tamago_amd.board.go_board import GoBoard
from tamago_amd.mcts.engine import SearchEngine, HostEvaluator
SIZE, TREES, TREE_SIZE, BATCH = 9, 2, 80, 24
eng = SearchEngine(SIZE, TREES, TREE_SIZE, BATCH, HostEvaluator(StubNet(3), torch.device("cuda:0")), check_superko=True)
rs = np.random.RandomState(5)
for t in range(TREES):
    b = GoBoard(SIZE, 7.0, True); c = 1
    for _ in range(3 * t):
        while True:
            pos = b.onboard_pos[rs.randint(len(b.onboard_pos))]
            if b.is_legal(pos, c): break
        b.put_stone(pos, c); c = 3 - c
    eng.set_root(t, b, c, np.random.RandomState(100 + t).get_state())
buf = ctypes.create_string_buffer(160)
tl.check(eng.lib.tg_search_launch_name(eng.handle, 0, BATCH, 0, buf, len(buf)), "tg_search_launch_name")
h = hashlib.sha256()
eng.root_eval(False)
for i in range(2):
    if i: eng.puct_flush()
    eng.puct_select(BATCH)
    for t in range(TREES):
        idx = np.zeros(BATCH, dtype=np.int32)
        n = ctypes.c_int32(0)
        tl.check(eng.lib.tg_search_read_queue(eng.handle, t, idx.ctypes.data, BATCH, ctypes.byref(n)), "tg_search_read_queue")
        assert n.value == BATCH, n.value
        h.update(np.int32(n.value).tobytes() + idx[:n.value].tobytes())
        for k in range(n.value):
            path = eng.read_path(t, k)
            assert path and path[0][0] == 0, path                       # every path starts at the root
            h.update(np.asarray(path, dtype=np.int32).tobytes() + b"|")
print("QUEUE", buf.value.decode().split(" grid=")[0].replace(" ", ""), h.hexdigest()[:16])
