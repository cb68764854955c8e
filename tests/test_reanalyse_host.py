"""CPU checks of the reanalysis path's host side (tamago_amd/mcts/reanalyse.py): the yardstick row of the GPU tests against
the text round trip it replaces, the symmetry mapping of a row, the per-tree schedules and the refusals."""
import numpy as np
import pytest
import torch

from tests import _reanalyse_cases as rc


@pytest.mark.parametrize("size,visited", [(9, 0), (9, 5), (9, 16), (19, 16)])
def test_dense_row_against_the_comment_round_trip(size, visited):
    """The helper's dense row (oracle improved policy, scattered) against what generate_rl_target_data makes of the
    comment SelfPlayRecord writes for the same root: the text keeps 4 significant digits ("%.3e"), so the two agree to
    5e-4 relative; a slot without a child holds 1e-18 on both sides."""
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.nn.feature import generate_rl_target_data
    from tamago_amd.sgf.selfplay_record import SelfPlayRecord
    board = GoBoard(size)
    rs = np.random.RandomState(size + visited)
    points = [board.onboard_pos[i] for i in rs.choice(size * size, size=40, replace=False)]
    root = rc.synthetic_root(size, points + [0], seed=visited, visited=visited)
    record = SelfPlayRecord("", Coordinate(size))
    record.save_record(root, points[0], 1)
    want = generate_rl_target_data(board, record.comments[0], 0)
    got = rc.dense_row(root, size).astype(np.float64)
    assert got.shape == want.shape == (size * size + 1,)
    child = np.zeros(len(got), dtype=bool)
    child[rc.slots_of(size, root.action[:root.num_children])] = True
    assert int(child.sum()) == 41 and child[-1]
    assert np.all(np.abs(got[child] - want[child]) <= 5.0e-4 * np.abs(want[child]) + 1e-45)
    assert np.all(want[~child] == 1e-18) and np.all(got[~child] == float(np.float32(1e-18)))
    assert abs(got[child].sum() - 1.0) < 1e-6
    # the host copy the product uses (MCTSNode.calculate_improved_policy) is the oracle's arithmetic
    assert np.array_equal(root.calculate_improved_policy(), rc.oracle_policy(root))


def test_symmetry_mapping_of_a_row():
    """symmetric_rows against generate_rl_target_data's own ordering (symmetry_pos_table) for all 8 symmetries of an
    asymmetric position: a row whose every slot is different."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.reanalyse import symmetric_rows
    from tamago_amd.nn.feature import generate_rl_target_data, symmetry_pos_table
    for size in (9, 13):
        board = GoBoard(size)
        a = size * size + 1
        values = (np.arange(a, dtype=np.float64) + 1.0) / 1024.0            # exact in float32, all different
        names = [board.coordinate.convert_to_gtp_format(p) for p in board.onboard_pos] + ["PASS"]
        text = " ".join([str(a)] + [f"{n}:{float(v)!r}" for n, v in zip(names, values)])
        rows = torch.from_numpy(np.tile(values.astype(np.float32), (8, 1)))
        got = symmetric_rows(size, rows, np.arange(8)).numpy()
        table = symmetry_pos_table(size)
        for sym in range(8):
            want = generate_rl_target_data(board, text, sym)
            assert np.array_equal(got[sym].astype(np.float64), want), (size, sym)
            assert np.array_equal(got[sym], rows[0].numpy()[rc.slots_of(size, table[sym])])
        assert len({got[sym].tobytes() for sym in range(8)}) == 8


@pytest.mark.parametrize("visits", [2, 16, 50])
def test_per_tree_schedules(visits):
    """Tree t follows the single-tree schedule of its own child count; a shorter schedule is padded with (0, 0)."""
    from tamago_amd.mcts.constant import MAX_CONSIDERED_NODES
    from tamago_amd.mcts.reanalyse import tree_schedules
    from tamago_amd.mcts.sequential_halving import get_candidates_and_visit_pairs
    children = [1, 2, 5, 16, 82]
    considered, counts = tree_schedules(children, visits)
    assert len(considered) == len(counts) and all(len(row) == len(children) for row in considered + counts)
    longest = 0
    for t, c in enumerate(children):
        want = list(get_candidates_and_visit_pairs(min(c, MAX_CONSIDERED_NODES), visits).items())
        got = [(considered[ph][t], counts[ph][t]) for ph in range(len(considered))]
        assert got[:len(want)] == want and all(pair == (0, 0) for pair in got[len(want):]), (c, got)
        assert sum(a * b for a, b in got) == visits                   # every simulation is spent, in every tree
        assert all(a * b <= visits for a, b in got)                   # a phase fits the engine's batch (= visits)
        longest = max(longest, len(want))
    assert len(considered) == longest
    assert [considered[0][t] for t in range(5)] == [min(c, 16, visits) for c in children]
    assert tree_schedules([], visits) == ([], [])


def test_refusals():
    """Refused before anything touches the device."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.reanalyse import reanalyse_positions

    class Net:
        board_size = 9

    nine, thirteen = (GoBoard(9), 1), (GoBoard(13), 1)
    with pytest.raises(ValueError, match="several board sizes"):
        reanalyse_positions(Net(), [nine, thirteen], 16)
    with pytest.raises(ValueError, match="network is built for 9x9"):
        reanalyse_positions(Net(), [thirteen], 16)
    with pytest.raises(ValueError, match="visits"):
        reanalyse_positions(Net(), [nine], 0)
    with pytest.raises(ValueError, match="one seed per position"):
        reanalyse_positions(Net(), [nine, nine], 16, seeds=[1])
