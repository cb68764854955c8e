"""The three packed read-outs of a root (csrc/readout.h) against each other: tg_search_read_root_stats, tg_search_read_node
of node 0 and tg_search_read_analysis pack the same device arrays into three records, so what they return must be the same
bits - at every board size, i.e. every layout (A = 82: one full 64-lane stride and a ragged one; 170; 362: six strides).
The self-play tail behind the root records is held to the host's decision, move by move and over whole games, by
tests/test_gpu_selfplay.py::test_one_call_per_move_path_equals_the_phase_by_phase_path (four 9x9 boards)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TREES, TREE_SIZE, BATCH = 3, 300, 8


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


@pytest.mark.parametrize("size", [9, 13, 19])
def test_three_readouts_agree_on_the_root(size):
    import torch
    from oracle.stubnet import StubNet
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import SearchEngine, HostEvaluator
    eng = SearchEngine(size, TREES, TREE_SIZE, BATCH, HostEvaluator(StubNet(3), torch.device("cuda:0")), check_superko=True)
    rs = np.random.RandomState(7)
    for t in range(TREES):                                   # 0, 3 and 6 random legal moves in: three different roots
        board, color = GoBoard(size, 7.0, True), 1
        for _ in range(3 * t):
            while True:
                pos = board.onboard_pos[rs.randint(len(board.onboard_pos))]
                if board.is_legal(pos, color):
                    break
            board.put_stone(pos, color)
            color = 3 - color
        eng.set_root(t, board, color, np.random.RandomState(100 + t).get_state())
    eng.root_eval(False)
    eng.puct_batch(BATCH)
    eng.puct_batch(BATCH)
    a = size * size + 1
    stats = eng.read_root_stats()
    analysis = eng.read_analysis(max_depth=2)
    num_nodes = eng.num_nodes()
    assert len(analysis) == TREES and stats["children_visits"].shape == (TREES, a)
    seen = set()
    for t in range(TREES):
        node = eng.read_node(t, 0)
        ana, _ = analysis[t]
        n = int(stats["num_children"][t])
        assert 0 < n <= a and stats["node_visits"][t] > 0 and stats["children_visits"][t, :n].sum() > 0
        seen.add(stats["children_visits"][t].tobytes() + stats["action"][t].tobytes())
        # the root record against the node record
        assert n == node.num_children
        assert int(stats["node_visits"][t]) == node.node_visits
        assert bits(stats["raw_value"][t:t + 1])[0] == bits(np.float32(node.raw_value).reshape(1))[0]
        assert np.array_equal(stats["action"][t], np.asarray(node.action, dtype=np.int32))
        assert np.array_equal(stats["children_visits"][t], node.children_visits)
        assert np.array_equal(stats["children_virtual_loss"][t], node.children_virtual_loss)
        assert np.array_equal(bits(stats["children_value_sum"][t]), bits(node.children_value_sum))
        assert np.array_equal(bits(stats["children_policy"][t]), bits(node.children_policy))
        # ... and both against the analysis record
        assert ana.num_children == n and ana.node_visits == node.node_visits
        assert bits(np.float32(ana.node_value_sum).reshape(1))[0] == bits(np.float32(node.node_value_sum).reshape(1))[0]
        assert np.array_equal(np.asarray(ana.action, dtype=np.int32), stats["action"][t])
        assert np.array_equal(ana.children_visits, stats["children_visits"][t])
        assert np.array_equal(bits(ana.children_value_sum), bits(stats["children_value_sum"][t]))
        assert np.array_equal(bits(ana.children_policy), bits(stats["children_policy"][t]))
        # num_nodes as it travels in the node record
        assert node.tree_num_nodes == int(num_nodes[t]) and 1 < node.tree_num_nodes <= TREE_SIZE
    assert len(seen) == TREES                                # three different roots were read, each as its own
    eng.close()
