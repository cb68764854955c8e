"""UNIQUE leaf layout (tg_search_select_gumbel with slots_per_tree -1), host side: the plane-range arithmetic
(mcts/sequential_halving.py unique_plane_caps = the library's) and the bound it rests on - one sequential-halving phase
enters at most E = 17 root children (node.py:324-346), so a phase's descents end on at most E distinct leaves - checked on
the oracle (= the reference's algorithm) with the network wrapped to hash every batch's planes."""
import numpy as np
import pytest

from oracle.halving import candidates_and_visit_pairs
from oracle.stubnet import StubNet, plane_hash
from oracle.tree import MCTSTree, TimeManager, TimeControl
from tamago_amd.mcts.sequential_halving import (UNIQUE_E, UNIQUE_PIPE_MAX, get_candidates_and_visit_pairs,
                                                unique_plane_caps)
from tests.helpers import load_json, load_npz, oracle_replay


def test_unique_plane_caps_hand_computed():
    assert UNIQUE_E == 17 and UNIQUE_PIPE_MAX == 512
    # 16 x 6 = 96 descents -> 17; 2 x 3 = 6 -> 6; idle tree -> 0; 1 x 400 -> 17; exactly 17 and 18 descents
    assert unique_plane_caps([16, 2, 0, 1, 17, 9], [6, 3, 0, 400, 1, 2]) == [17, 6, 0, 17, 17, 17]
    assert unique_plane_caps([16], [1]) == [16]
    assert unique_plane_caps([4, 2], [25, 54], E=5) == [5, 5]
    # a tree with more than 512 descents sends the whole launch to the one-wavefront kernel: nothing saved, for any tree
    assert unique_plane_caps([2, 16], [400, 6]) == [800, 96]
    assert unique_plane_caps([2, 16], [256, 6]) == [17, 17]                       # 512 descents: still the pipelined kernel
    assert unique_plane_caps([16, 8], [6, 12], pipelined=False) == [96, 96]       # TG_SELECT_SERIAL / pool beyond 2^21 nodes
    assert unique_plane_caps([], []) == []


class Hashing:
    """Evaluator wrapper: per forward call, how many positions and how many DISTINCT ones."""

    def __init__(self, net):
        self.net = net
        self.log = []

    def _note(self, planes):
        h = plane_hash(planes.numpy())
        self.log.append((int(planes.shape[0]), len(set(int(v) for v in h))))

    def inference(self, planes):
        self._note(planes)
        return self.net.inference(planes)

    def inference_with_policy_logits(self, planes):
        self._note(planes)
        return self.net.inference_with_policy_logits(planes)


def check_move(log, n_root, visits):
    """One Gumbel move's forward calls: the root, then one batch per phase with at most cap distinct positions."""
    pairs = list(candidates_and_visit_pairs(min(n_root, 16), visits).items())
    assert [n for n, _ in log] == [1] + [w * c for w, c in pairs]
    caps = unique_plane_caps([w for w, _ in pairs], [c for _, c in pairs], pipelined=True)
    for (n, distinct), cap, (w, c) in zip(log[1:], caps, pairs):
        assert distinct <= cap, (n_root, visits, w, c, distinct, cap)
    return sum(d for _, d in log[1:]), sum(n for n, _ in log[1:])


def oracle_net(kind, size, seed):
    if kind == "stub":
        return StubNet(salt=100 + seed)
    from oracle.net import OracleNet, make_state_dict
    return OracleNet(make_state_dict(size, seed, 1.0))


@pytest.mark.parametrize("kind", ["stub", "oracle"])
@pytest.mark.parametrize("size", [9, 13])
def test_a_phase_has_at_most_cap_distinct_leaves_on_the_tree_fixtures(size, kind):
    brd = load_npz(f"board_s{size}.npz")
    for rec in [r for r in load_json(f"trees_s{size}.json") if r["kind"] == "gumbel"]:
        board = oracle_replay(size, brd["g0_move"], brd["g0_color"], rec["ply"], rec["superko"])
        net = Hashing(oracle_net(kind, size, rec["seed"]))
        tree = MCTSTree(net, size, tree_size=160 if rec["visits"] <= 100 else 2048)
        np.random.seed(rec["seed"])
        tree.generate_move_with_sequential_halving(board, rec["color"],
                                                   TimeManager(TimeControl.CONSTANT_PLAYOUT, rec["visits"]), True)
        distinct, queued = check_move(net.log, tree.get_root().num_children, rec["visits"])
        if rec["visits"] >= 100 and tree.get_root().num_children >= 16:
            assert distinct < queued                     # (what the layout saves: repeats exist)


def test_a_phase_has_at_most_cap_distinct_leaves_through_a_400_simulation_game():
    from oracle.board import GoBoard, BLACK
    size, visits = 9, 400
    net = Hashing(StubNet(salt=7))
    tree = MCTSTree(net, size, tree_size=visits * 10, batch_size=10 ** 9)
    tm = TimeManager(TimeControl.CONSTANT_PLAYOUT, visits)
    np.random.seed(1)
    board = GoBoard(size, 7.0, True)
    color, passes, most = BLACK, 0, 0
    for _ in range(2 * size * size):
        net.log.clear()
        pos = tree.generate_move_with_sequential_halving(board, color, tm, True)
        check_move(net.log, tree.get_root().num_children, visits)
        most = max([most] + [d for _, d in net.log[1:]])
        board.put_stone(pos if pos > 0 else 0, color)
        passes = passes + 1 if pos == 0 else 0
        color = 3 - color
        if passes == 2:
            break
    assert 2 <= most <= UNIQUE_E


def phases_of(width, visits):
    return list(get_candidates_and_visit_pairs(min(width, 16), visits).items())


@pytest.mark.parametrize("visits", [16, 100, 400, 800])
def test_forwarded_and_queued_positions_of_a_move(visits):
    """Per move and board: queued = visits + 1 (the reference's count), forwarded = 1 + the phases' plane ranges."""
    for width in range(1, 83):
        pairs = phases_of(width, visits)
        queued = 1 + sum(w * c for w, c in pairs)
        assert queued == visits + 1
        forwarded = 1
        for w, c in pairs:                                # (one launch per phase: a lone board decides its kernel)
            cap, = unique_plane_caps([w], [c])
            assert cap == (min(w * c, UNIQUE_E) if w * c <= UNIQUE_PIPE_MAX else w * c)
            forwarded += cap
        assert forwarded <= queued
        if all(w * c <= UNIQUE_PIPE_MAX for w, c in pairs):
            assert forwarded <= 1 + len(pairs) * UNIQUE_E


def test_share_forwarded_at_400_simulations_is_bounded_by_the_schedule():
    visits = 400
    phases = max(len(phases_of(width, visits)) for width in range(1, 83))
    bound = (phases * UNIQUE_E + 1) / (visits + 1)
    assert phases <= 5 and bound <= 0.22
    for width in range(1, 83):
        pairs = phases_of(width, visits)
        forwarded = 1 + sum(unique_plane_caps([w for w, _ in pairs], [c for _, c in pairs], pipelined=True))
        assert forwarded / (visits + 1) <= bound
