"""Helper of test_gpu_visit_budget.py (run as a script: the selection knobs are read once per process).  Six trees under the
bit-exact host StubNet, three plain mini-batches of 8, then two mini-batches under visit budgets whose caps are (8, 8, 3, 1,
0, 0) and (8, 4, 0, 0, 0, 0), then a plain one with the budgets off again - strided, or COMPACT behind the budget rule
(argv[1]: "strided" / "compact") - by whatever PUCT selection kernel the environment names; and every tree searched alone on
an engine of its own with puct_batch(cap).  Prints one JSON line: the kernel's name and, per stage, every tree's state in the
engine of six and alone, the leaves queued, whether the planes of leaf j of tree t sit at row t * 8 + j (its rank's rows
when compact), the positions evaluated, the live counts and ranks."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PLIES, SEED, TREE_SIZE, BATCH, WARM = (0, 4, 10, 20, 30, 10), 9, 128, 8, 3
TOTALS = (40, 36, 27, 25, 24, 10)                          # after WARM * BATCH = 24 visits: caps 8, 8, 3, 1, 0, 0 (10: below the visits)
CAPS = ((8, 8, 3, 1, 0, 0), (8, 4, 0, 0, 0, 0))


def main():
    import numpy as np
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd import lib as tl
    from tamago_amd.mcts.engine import HostEvaluator, SearchEngine
    from tests import _early_stop_cases as cases
    from tests.test_gpu_early_stop import _tree_state
    compact = sys.argv[1] == "compact"
    T = len(PLIES)
    device = torch.device("cuda", 0)

    def engine(plies, first):
        eng = SearchEngine(9, len(plies), TREE_SIZE, BATCH, HostEvaluator(StubNet(salt=SEED), device))
        for t, ply in enumerate(plies):
            eng.set_root(t, cases.product_board(ply), 1, np.random.RandomState(SEED + first + t).get_state())
        eng.root_eval(False)
        for _ in range(WARM):
            eng.puct_batch(BATCH)
        return eng

    counts = torch.full((T,), -1, dtype=torch.int32, device=device)

    eng = engine(PLIES, 0)
    alone = [engine(PLIES[t:t + 1], t) for t in range(T)]
    buf = ctypes.create_string_buffer(160)
    tl.check(eng.lib.tg_search_launch_name(eng.handle, 0, BATCH, 0, buf, len(buf)), "tg_search_launch_name")
    out = {"kernel": buf.value.decode(), "stages": [], "alone": [], "leaves": [], "planes_ok": [], "positions": [], "live": [],
           "rank": []}

    def snapshot():
        out["stages"].append([_tree_state(eng, t) for t in range(T)])
        out["alone"].append([_tree_state(alone[t], 0) for t in range(T)])
    snapshot()
    eng.set_budget(TOTALS)
    halted = [False] * T
    for caps in CAPS + (None,):
        if caps is None:
            eng.set_budget(None)                             # budgets off again: the plain mini-batch
            caps = tuple(0 if h else BATCH for h in halted)
        rank = list(range(T))
        if compact:
            if eng._budget is not None:
                eng.budget_rule()
            out["live"].append(eng.compact_live())
            rank = eng.read_live_rank().tolist()
            out["rank"].append(rank)
            halted = [r < 0 for r in rank]
        launched = eng.forward_positions
        eng.puct_batch(BATCH, compact=compact, n_leaves=counts)
        out["positions"].append(eng.forward_positions - launched)
        planes = eng.planes.cpu()
        ok = True
        for t in range(T):
            if caps[t]:
                alone[t].puct_batch(caps[t])
                want = alone[t].planes[:caps[t]].cpu()
                row = rank[t] * BATCH
                ok = ok and rank[t] >= 0 and bool(torch.equal(planes[row:row + caps[t]], want))
        out["planes_ok"].append(ok)
        out["leaves"].append(counts.cpu().tolist())
        snapshot()
    eng.close()
    for e in alone:
        e.close()
    print("BUDGET " + json.dumps(out))


if __name__ == "__main__":
    main()
