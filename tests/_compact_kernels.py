"""Helper of test_gpu_compact_idle.py (run as a script: the selection knobs are read once per process).  Three trees under the
bit-exact host StubNet, the middle one halted from the host after one mini-batch; three more mini-batches in the strided or the
COMPACT layout (argv[1]: "strided" / "compact") by whatever PUCT selection kernel the environment names.  Prints, as one JSON
line, the kernel's name, every tree's state before the halt and at the end, and the positions the three mini-batches evaluated."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PLIES, SEED, TREE_SIZE, BATCH = (0, 10, 20), 9, 80, 4


def main():
    import numpy as np
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd import lib as tl
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    from tests import _early_stop_cases as cases
    from tests.test_gpu_early_stop import _tree_state
    compact = sys.argv[1] == "compact"
    eng = SearchEngine(9, len(PLIES), TREE_SIZE, BATCH, HostEvaluator(StubNet(salt=SEED), torch.device("cuda", 0)))
    for t, ply in enumerate(PLIES):
        eng.set_root(t, cases.product_board(ply), 1, np.random.RandomState(SEED).get_state())
    eng.root_eval(False)
    eng.puct_batch(BATCH)
    before = [_tree_state(eng, t) for t in range(len(PLIES))]
    eng.set_halt([0, 1, 0])
    buf = ctypes.create_string_buffer(160)
    tl.check(eng.lib.tg_search_launch_name(eng.handle, 0, BATCH, 0, buf, len(buf)), "tg_search_launch_name")
    launched = eng.forward_positions
    live = eng.compact_live() if compact else None
    for _ in range(3):
        eng.puct_batch(BATCH, compact=compact)
    positions = eng.forward_positions - launched
    after = [_tree_state(eng, t) for t in range(len(PLIES))]
    rank = eng.read_live_rank().tolist() if compact else None
    eng.close()
    print("COMPACT " + json.dumps({"kernel": buf.value.decode(), "before": before, "after": after, "positions": positions,
                                   "live": live, "rank": rank}))


if __name__ == "__main__":
    main()
