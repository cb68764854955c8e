"""Helper of test_gpu_unique_leaves.py (run as a script: TG_SELECT_SERIAL is read once per process).  Runs the 9x9 Gumbel
cases of tests/golden/trees_s9.json through MCTSTree(unique_leaves=True) with StubNet and prints, per case, the whole-tree
digest, the move, a digest of the improved policy, the next draw of numpy's stream and the positions handed to the network."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from oracle.stubnet import StubNet
from tamago_amd.mcts.time_manager import TimeManager, TimeControl
from tamago_amd.mcts.tree import MCTSTree
from tests.helpers import load_json, load_npz
from tests.test_gpu_search import product_digest, product_replay
brd = load_npz("board_s9.npz")
for rec in [r for r in load_json("trees_s9.json") if r["kind"] == "gumbel"]:
    board = product_replay(9, brd["g0_move"], brd["g0_color"], rec["ply"], rec["superko"])
    tree = MCTSTree(StubNet(salt=100 + rec["seed"]), tree_size=160 if rec["visits"] <= 100 else 2048, unique_leaves=True)
    np.random.seed(rec["seed"])
    mv = tree.generate_move_with_sequential_halving(board, rec["color"], TimeManager(TimeControl.CONSTANT_PLAYOUT, rec["visits"]), True)
    improved = hashlib.sha256(tree.get_root().calculate_improved_policy().tobytes()).hexdigest()[:16]
    print(product_digest(tree, tree.num_nodes), int(mv), improved, float(np.random.random_sample()).hex(),
          tree._engine.forward_positions)
