"""Shared by the reanalysis tests (tests/test_reanalyse_host.py, tests/test_gpu_reanalyse.py): the yardstick for an
improved-policy row - the oracle's calculate_improved_policy on a root, scattered into a dense row by a few lines of
numpy -, the bound a device row is held to, the positions the read-out kernel is tried on and the single-tree path of
the module's contract."""
import copy

import numpy as np

from tamago_amd.board.constant import PASS
from tamago_amd.board.go_board import BLACK, WHITE, GoBoard

FILL = np.float32(1e-18)                         # what an rl_data row holds where the root had no candidate
FLT_MIN = float(np.finfo(np.float32).tiny)


def slots_of(size: int, actions) -> np.ndarray:
    """Network output slot of padded coordinates: board points row-major, PASS last."""
    a = np.asarray(actions, dtype=np.int64)
    w = size + 2
    return np.where(a == PASS, size * size, (a // w - 1) * size + a % w - 1)


def oracle_policy(root) -> np.ndarray:
    """float64 [num_children]: oracle.node.Node.improved_policy (node.py:281-321) on a root view (MCTSNode)."""
    from oracle.node import Node
    node = Node(len(root.children_policy))
    node.num_children = int(root.num_children)
    node.node_visits = int(root.node_visits)
    node.raw_value = np.float32(root.raw_value)
    node.children_visits = np.array(root.children_visits, dtype=np.int32)
    node.children_value_sum = np.array(root.children_value_sum, dtype=np.float64)
    node.children_policy = np.array(root.children_policy, dtype=np.float64)
    return node.improved_policy()


def dense_row(root, size: int) -> np.ndarray:
    """The yardstick row: float32(oracle64) of child i at the slot of action[i], FILL everywhere else."""
    n = int(root.num_children)
    row = np.full(size * size + 1, FILL, dtype=np.float32)
    row[slots_of(size, root.action[:n])] = oracle_policy(root).astype(np.float32)
    return row


def assert_row_within_bound(got, root, size: int, what=""):
    """|row - float32(oracle64)| <= max(1 ulp_f32, FLT_MIN) at the children's slots (both sides compute in float64 and
    differ by ~1e-13 relative at most - a 362-term softmax, exponents up to a few hundred - so the float32 casts can
    differ at a rounding boundary only, by one ulp; below FLT_MIN the conversion may flush); the children's slots sum
    to 1 within 1e-6; every other slot is float32(1e-18) exactly."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == (size * size + 1,), what
    want = dense_row(root, size)
    n = int(root.num_children)
    child = np.zeros(len(want), dtype=bool)
    child[slots_of(size, root.action[:n])] = True
    assert int(child.sum()) == n, what
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = np.maximum(np.spacing(np.abs(want)).astype(np.float64), FLT_MIN)
    worst = int(np.argmax(np.where(child, diff - bound, -np.inf)))
    print(f"{what}: {n} children, max |row - oracle| {diff[child].max():.3e} (bound there {bound[worst]:.3e}), "
          f"sum {float(got[child].astype(np.float64).sum()):.9f}")
    assert np.all(diff[child] <= bound[child]), (what, worst, float(got[worst]), float(want[worst]))
    assert abs(float(got[child].astype(np.float64).sum()) - 1.0) <= 1e-6, what
    assert np.array_equal(got[~child].view(np.uint32), np.full(int((~child).sum()), FILL).view(np.uint32)), what


# ---- positions ---------------------------------------------------------------------------------------------------------
def played(size: int, moves, superko: bool = True):
    """(board, colour to move) after `moves` from the empty board, colours alternating from black."""
    board, color = GoBoard(size, check_superko=superko), BLACK
    for pos in moves:
        board.put_stone(int(pos), color)
        color = 3 - color
    return board, color


def walled(size: int, open_points, eyes, to_move=WHITE, superko: bool = True):
    """A board full of black stones except `eyes` (single points: no move for white) and `open_points`: the side to move
    has the open points it can legally enter, and PASS."""
    board = GoBoard(size, check_superko=superko)
    for p in board.onboard_pos:
        if p not in eyes and p not in open_points:
            board.cells[p] = BLACK
    board.moves = 5
    return board, to_move


def cases9():
    """name -> (board, colour): the 9x9 positions of the read-out test."""
    from tests._replay_records import random_record
    w = 11
    mid = random_record(9, 30, 21, pass_rate=0.0)
    after_pass = random_record(9, 11, 22, pass_rate=0.0) + [PASS]
    corner = [x + y * w for y in (7, 8, 9) for x in (7, 8, 9)]
    return {
        "empty": played(9, []),
        "midgame": played(9, mid),
        "after_pass": played(9, after_pass),
        "late": walled(9, corner, (12, 14)),
        "pass_only": walled(9, (), (12, 14)),
    }


def cases13():
    from tests._replay_records import random_record
    return {"empty": played(13, []), "midgame": played(13, random_record(13, 40, 23, pass_rate=0.0))}


def single_tree(network, board, color, seed: int, visits: int, unique_leaves: bool = False):
    """The contract's single-tree run: (tree, move, root).  The global generator is left where the run leaves it."""
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    np.random.set_state(np.random.RandomState(seed).get_state())
    tree = MCTSTree(network, tree_size=visits + 16, unique_leaves=unique_leaves)
    move = tree.generate_move_with_sequential_halving(copy.deepcopy(board), color,
                                                      TimeManager(TimeControl.STRICT_PLAYOUT, visits), True)
    return tree, move, tree.get_root()


def synthetic_root(size: int, actions, seed: int, visited: int):
    """An MCTSNode as a search leaves a root: logits, `visited` of the children with visits and value sums, the others
    untouched."""
    from tamago_amd.mcts.node import MCTSNode
    rs = np.random.RandomState(seed)
    n = len(actions)
    root = MCTSNode(size * size + 1)
    root.num_children = n
    root.action[:n] = [int(a) for a in actions]
    root.children_policy[:n] = rs.normal(0.0, 2.0, n)
    seen = rs.permutation(n)[:visited]
    root.children_visits[seen] = rs.randint(1, 12, size=len(seen))
    root.children_value_sum[seen] = root.children_visits[seen] * rs.random_sample(len(seen))
    root.node_visits = int(root.children_visits.sum())
    root.raw_value = np.float32(rs.random_sample())
    return root
