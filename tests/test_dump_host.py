"""Whole-tree dumps on the CPU (tamago_amd/mcts/dump.py) against what tools/gen_golden_tree_dump.py recorded from
the reference: enrich_mcts_dict on the recorded small dump gives the recorded fields; dump_mcts_to_json writes the recorded text
again; and oracle.tree's tree of every fixture case, put through the host half of tree_to_dict, has the recorded sha256 - so the
serialisation and the fixtures agree before any GPU is involved.  No GPU."""
import json

import numpy as np
import pytest

from tamago_amd.mcts import dump
from tests import _tree_dump_cases as cases


def test_enrich_mcts_dict_on_the_recorded_dump():
    small = cases.fixture(9)["small"]
    state = json.loads(small["json"])
    dump.enrich_mcts_dict(state)
    got = cases.tool().enriched_fields(state)
    assert got["sorted_indices_list"] == small["enriched"]["sorted_indices_list"]
    assert len(got["nodes"]) == small["num_nodes"] == len(small["enriched"]["nodes"])
    for i, (a, b) in enumerate(zip(got["nodes"], small["enriched"]["nodes"])):
        assert a == b, (i, {k for k in set(a) | set(b) if a.get(k) != b.get(k)})
    # (exact: the enriched floats are copies and one division of recorded float64 values)
    assert json.loads(json.dumps(got)) == small["enriched"]


def test_dump_mcts_to_json_round_trips():
    """The recorded tree dict and the position set up again on our board give the recorded text, byte for byte; and what
    json.loads makes of it sets the same position up again (enrich_mcts_dict's first lines)."""
    small = cases.fixture(9)["small"]
    state = json.loads(small["json"])
    board = cases.product_board(9, small["ply"], small["superko"])
    text = dump.dump_mcts_to_json(state["tree"], board, small["superko"])
    assert text == small["json"]
    assert "\n" not in text
    from tamago_amd.board.go_board import GoBoard
    again = GoBoard(state["board_size"], state["komi"], state["superko"])
    again.set_history([(dump._str_to_stone(c), p, None) for c, p in state["move_history"]], state["handicap_history"])
    assert np.array_equal(again.cells, board.cells) and again.moves == board.moves == small["ply"] + 1
    assert again.get_board_string() == board.get_board_string()


def test_the_empty_tree():
    empty = dump.empty_tree_dict(16, False)
    assert empty == {"node": [], "num_nodes": 0, "root": 0, "current_root": 0, "batch_size": 16, "cgos_mode": False, "to_move": "black"}
    assert dump.digest_of(empty).tolist() == dump.digest_of_packed(dump.pack_nodes([], 0)).tolist()


@pytest.mark.parametrize("size", cases.SIZES)
def test_the_oracles_trees_have_the_recorded_sha256(size):
    for case in cases.fixture(size)["cases"]:
        tree_dict = cases.oracle_tree_dict(size, case)
        assert tree_dict["num_nodes"] == case["num_nodes"]
        assert cases.tool().canonical_sha256(tree_dict) == case["sha256"], case["index"]


def test_the_oracles_small_tree_is_the_recorded_dump():
    """Element for element, not only by hash: every key of the reference's to_dict, arrays of full length with their tails."""
    case = cases.small_case()
    tree_dict = cases.oracle_tree_dict(9, case)
    want = json.loads(cases.fixture(9)["small"]["json"])["tree"]
    assert list(tree_dict) == list(want) and list(tree_dict["node"][0]) == list(want["node"][0])
    assert tree_dict == want
    assert cases.tool().canonical_sha256(tree_dict) == case["sha256"]
    assert all(len(node[k]) == 82 for node in tree_dict["node"] for k in ("action", "children_index", "children_policy", "noise"))
