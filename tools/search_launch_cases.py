#!/usr/bin/env python3
"""Every family of search launches once, at tiny shapes - the workload under a kernel trace when two builds are to be shown
to launch the same kernels on the same grids (profiles/search_launch_plan.json).  One process = one knob setting (most
selection knobs are read once per process): set the knobs (and TG_DEBUG_KNOBS=1, TAMAGO_HIP_LIB) in the environment.
    python tools/search_launch_cases.py search S T          root, PUCT mini-batch, Gumbel phases (packed, unique, strided)
    python tools/search_launch_cases.py selfplay 0|1        8 boards in two sub-groups, 3 moves' worth of games (1: unique leaves)"""
import os, shutil, sys, tempfile
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")          # before torch loads the HIP runtime (tamago_amd/__init__.py)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from oracle.net import make_state_dict
from tamago_amd.board.go_board import GoBoard
from tamago_amd.mcts.engine import SearchEngine, DeviceEvaluator
from tamago_amd.nn.network.dual_net import DualNet
from tamago_amd.selfplay.worker import selfplay_shard


def search(size, trees, batch=8):
    net = DualNet(torch.device("cuda:0"), size)
    net.load_state_dict(make_state_dict(size, 3, 1.0))
    engine = SearchEngine(size, trees, 64, batch, DeviceEvaluator(net))
    board = GoBoard(size, 7.0, False)
    for t in range(trees):
        engine.set_root(t, board, 1, np.random.RandomState(7 + t).get_state())
    engine.root_eval(first_batch=batch)
    engine.puct_batch(batch)
    engine.set_gumbel_noise()
    nc, mc = np.full(trees, 4, dtype=np.int32), np.full(trees, 2, dtype=np.int32)
    engine.gumbel_phase(nc, mc, packed=True)
    engine.gumbel_phase(nc, mc, unique=True)
    engine.gumbel_phase(nc, mc, packed=False)
    torch.cuda.synchronize()
    print(f"search {size}x{size} T={trees}: nodes {engine.num_nodes().tolist()[:4]}")
    engine.close()


def selfplay(unique):
    torch.manual_seed(0)
    net = DualNet(torch.device("cuda:0"), 9)
    out = tempfile.mkdtemp(prefix="sp_")
    try:
        stats = selfplay_shard(out, net, list(range(1, 9)), 9, 16, boards=8, never_resign_flags=[False] * 8, lanes=1,
                               unique_leaves=bool(unique))
    finally:
        shutil.rmtree(out, ignore_errors=True)
    torch.cuda.synchronize()
    print(f"selfplay 8 boards unique={unique}: {stats}")


if __name__ == "__main__":
    if sys.argv[1] == "search":
        search(int(sys.argv[2]), int(sys.argv[3]))
    else:
        selfplay(int(sys.argv[2]))
