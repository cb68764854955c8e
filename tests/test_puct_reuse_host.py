"""The tree-reuse match game on the CPU oracle (tests/_puct_reuse_cases.py): deterministic and restartable, with searches that
reuse a subtree and searches that fall back to a fresh root among the games the GPU test plays, told apart from two wrong
oracles; and the ABI of the entry points tree reuse in lock-step matches is built from.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import _puct_reuse_cases as cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("tg_search_advance", "tg_search_root_planes_fresh", "tg_search_set_budget", "tg_search_budget_rule",
                    "tg_search_puct_chain_budget")


def test_games_are_deterministic_and_restartable():
    np.random.seed(12345)
    before = np.random.get_state()
    first = cases.oracle_reuse_match_game(1, cases.make_net(cases.S301), cases.make_net(cases.S302))
    after = np.random.get_state()
    assert before[2] == after[2] and np.array_equal(before[1], after[1])          # the caller's stream is not touched
    np.random.seed(999)                                                         # ... and does not matter
    second = cases.oracle_reuse_match_game(1, cases.make_net(cases.S301), cases.make_net(cases.S302))
    assert first[0] == second[0] and first[1] == second[1] and first[3] == second[3]
    for a, b in zip(first[2], second[2]):
        assert a[2] == b[2] and np.array_equal(a[1], b[1])
    assert first[0] == cases.oracle_reuse_game(1)[0]


def test_the_gpu_seeds_reuse_and_fall_back():
    reused = fresh_again = 0
    for seed in cases.GPU_SEEDS:
        text, (moves, ending), _, searches = cases.oracle_reuse_game(seed)
        assert len(re.findall(r";[BW]\[", text)) == moves and ending in ("resign", "passes", "limit")
        first = {}
        for ply, (color, kept) in enumerate(searches):
            assert color == 1 + ply % 2
            if color not in first:
                first[color] = ply
                assert kept is None                                             # a colour's first search is always fresh
            elif kept is None:
                fresh_again += 1
            else:
                assert kept >= 0
                reused += 1
    assert reused > 0 and fresh_again > 0, (reused, fresh_again)


def test_kept_visits_shorten_the_search():
    """Some reused search of the GPU seeds keeps visits (so it owes fewer descents than a fresh one): without one the budget
    would never bind and the wrong budget below could not show."""
    kept = [k for seed in cases.GPU_SEEDS for _, k in cases.oracle_reuse_game(seed)[3] if k]
    assert kept and max(kept) >= 1


@pytest.mark.parametrize("rule", cases.RULES[1:])
def test_wrong_oracles_change_the_games(rule):
    changed = [seed for seed in cases.GPU_SEEDS
               if cases.oracle_reuse_game(seed, rule=rule)[0] != cases.oracle_reuse_game(seed)[0]
               or any(a[2] != b[2] or not np.array_equal(a[1], b[1])
                      for a, b in zip(cases.oracle_reuse_game(seed, rule=rule)[2], cases.oracle_reuse_game(seed)[2]))]
    assert changed, rule


def test_reuse_differs_from_rebuilding():
    from tests._puct_match_cases import oracle_puct_game
    assert any(cases.oracle_reuse_game(seed)[0] != oracle_puct_game(seed, cases.S301, cases.S302)[0] for seed in cases.GPU_SEEDS)


def test_reuse_best_move_is_emulate_search():
    """reuse_best_move restates _tree_reuse.emulate_search with the resign threshold as an argument: same moves, trees and
    draws over a line of play, fresh and reused."""
    from oracle.board import GoBoard
    from oracle.tree import MCTSTree, TimeControl, TimeManager
    from tests._tree_reuse import emulate_search
    net = cases.make_net(cases.S301)
    saved = np.random.get_state()
    try:
        runs = []
        for which in (0, 1):
            np.random.seed(4)
            tree = MCTSTree(net, 9, tree_size=60, batch_size=8)
            board, color, pending, line = GoBoard(9, 7.0, False), 1, None, []
            for _ in range(6):
                root = cases.reuse_root_of(tree, pending)
                if which == 0:
                    move = emulate_search(tree, board, color, TimeManager(TimeControl.STRICT_PLAYOUT, 40), reuse_root=root)
                else:
                    move, _ = cases.reuse_best_move(tree, board, color, 40, root)
                assert move >= 0
                board.put_stone(move, color)
                line.append((move, int(tree.node[0].node_visits), tree.num_nodes))
                pending, color = [move], 3 - color
            runs.append((line, np.random.get_state()[2], np.random.get_state()[1].tobytes()))
        assert runs[0] == runs[1]
        assert len(runs[0][0]) == 6 and all(visits >= 40 for _, visits, _ in runs[0][0])
    finally:
        np.random.set_state(saved)


def test_header_declares_and_lib_binds_the_entry_points():
    from tamago_amd import lib as tl
    with open(os.path.join(REPO, "include", "tamago_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*tg_search\s*\*" % name, header), name
        assert name in tl.exported_symbols(), name
    assert re.search(r"typedef\s+struct\s+tg_advance_record\s*\{[^}]*kept_visits[^}]*kept_nodes[^}]*num_children[^}]*status[^}]*\}", header)
    with open(os.path.join(REPO, "tamago_amd", "csrc", "visit_budget.h"), encoding="utf-8") as f:
        rules = f.read()
    assert "descents(" in rules and "spent(" in rules and "hip_runtime" not in rules


def test_the_command_lines_take_reuse_tree():
    from tamago_amd.selfplay.match import parse_args
    base = ["--black", "a.bin", "--white", "b.bin", "--games", "8"]
    assert parse_args(base + ["--search", "puct"]).reuse_tree is False
    assert parse_args(base + ["--search", "puct", "--reuse-tree"]).reuse_tree is True
    with pytest.raises(SystemExit):
        parse_args(base + ["--reuse-tree"])                                     # only with --search puct


def test_reuse_needs_strict_setups():
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    with pytest.raises(ValueError, match="strict"):
        puct_match(EngineSetup(object(), 8, 4), EngineSetup(object(), 8, 4, strict=False), 1, reuse_tree=True)
