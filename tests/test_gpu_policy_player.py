"""Policy-only play on the device (tg_policy_*: policy_planes_kernel / policy_move_kernel of csrc/search.hip) against the
reference's recorded moves, and whole games against a host replay of the policies the device itself produced."""
import random

import numpy as np
import pytest
import torch

from _policy_cases import digest, load, prepared_rng, replay

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _net(size, seed):
    from tamago_amd.nn.network.dual_net import DualNet
    torch.manual_seed(seed)
    return DualNet(DEV, size)


@pytest.fixture(scope="module")
def nets9():
    return _net(9, 21), _net(9, 22)


def _run_cases(size, cases, policies, play):
    """The cases as ONE batch (T = len(cases)): moves, stream states after, and the boards read back."""
    from tamago_amd.nn.policy_player import PolicyBoards
    boards = PolicyBoards(size, len(cases), True)
    try:
        for t, case in enumerate(cases):
            board, color = replay(size, case)
            boards.set_root(t, board, color)
            boards.seed(t, prepared_rng(case).getstate())
        moves = boards.moves(torch.as_tensor(np.ascontiguousarray(policies)).to(DEV), play=play)
        states = [boards.state(t) for t in range(len(cases))]
        return moves, states, boards.read_positions()
    finally:
        boards.close()


@pytest.mark.parametrize("size", [9, 13, 19])
def test_move_kernel_reproduces_the_reference(size):
    labels, arrays = load(size)
    cases, policies = labels["cases"], arrays["policy"]
    for picked, play in ((slice(None), False), (slice(None), True), (slice(0, 1), False), (slice(0, 1), True)):
        sub, pol = cases[picked], policies[picked]
        moves, states, (cells, n_moves, to_move) = _run_cases(size, sub, pol, play)
        for t, case in enumerate(sub):
            assert int(moves[t]) == case["move"], (case["name"], play)
            assert digest(states[t]) == (case["state_pos"], case["state_sha256"]), (case["name"], play)
            board, color = replay(size, case)
            if play:
                board.put_stone(case["move"], color)
                color = 3 - color
            assert np.array_equal(cells[t], board.cells), (case["name"], play)
            assert (int(n_moves[t]), int(to_move[t])) == (board.moves, color), (case["name"], play)


def test_planes_kernel_matches_the_featurizer():
    """tg_policy_planes against generate_input_planes (the featurise kernel) for every recorded 9x9 position."""
    from tamago_amd.nn.feature import generate_input_planes
    from tamago_amd.nn.policy_player import PolicyBoards
    cases = load(9)[0]["cases"]
    boards = PolicyBoards(9, len(cases), True)
    try:
        want = []
        for t, case in enumerate(cases):
            board, color = replay(9, case)
            boards.set_root(t, board, color)
            want.append(generate_input_planes(board, color))
        assert np.array_equal(boards.write_planes().cpu().numpy(), np.stack(want))
    finally:
        boards.close()


def test_public_function_is_the_host_rule_on_the_networks_own_output():
    """generate_move_from_policy(DualNet): three consecutive moves on a mid-game board equal choose_from_policy on the
    network's own inference output, and the global generator ends in the same state."""
    from tamago_amd.nn.feature import generate_input_planes
    from tamago_amd.nn.policy_player import choose_from_policy, generate_move_from_policy
    net = _net(9, 23)
    case = next(c for c in load(9)[0]["cases"] if c["name"] == "random_play_3")
    for seed in (5, 6):
        dev_board, color = replay(9, case)
        host_board, _ = replay(9, case)
        random.seed(seed)
        got = []
        for _ in range(3):
            got.append(generate_move_from_policy(net, dev_board, color))
            dev_board.put_stone(got[-1], color)
            color = 3 - color
        state_dev = random.getstate()
        random.seed(seed)
        color = case["color"]
        want = []
        for _ in range(3):
            planes = torch.tensor(generate_input_planes(host_board, color).reshape(1, 6, 9, 9))
            policy, _ = net.inference(planes)
            want.append(choose_from_policy(policy[0].numpy().tolist(), host_board, color))
            host_board.put_stone(want[-1], color)
            color = 3 - color
        assert got == want
        assert random.getstate() == state_dev


def _replay_games(result, games, seeds, size, komi, max_moves, boards, superko, answer_pass):
    """Every game again on the host: GoBoard, choose_from_policy on the policies the device recorded, random.Random(seed)."""
    from tamago_amd.board.constant import PASS
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.nn.policy_player import choose_from_policy
    policies = result["policies"]
    next_free = [0] * boards                       # first ply at which a slot may start a game
    for g in range(games):
        slot = g % boards
        start = next_free[slot] + (next_free[slot] & 1)          # a slot takes a game at an even ply only
        board, rng = GoBoard(size, komi, superko), random.Random(seeds[g])
        color, passes, moves, end = 1, 0, [], "max_moves"
        for k in range(max_moves):
            assert (start + k) % 2 == color - 1    # black moves at even plies, white at odd ones
            pos = choose_from_policy(policies[start + k, slot], board, color, rng)
            if answer_pass and board.moves > 1 and board.prev_move(1) == PASS:
                pos = PASS
            board.put_stone(pos, color)
            moves.append(pos)
            passes = passes + 1 if pos == PASS else 0
            color = 3 - color
            if passes == 2:
                end = "two_passes"
                break
        next_free[slot] = start + len(moves)
        got = result["games"][g]
        assert got["moves"] == moves, g
        assert (got["length"], got["end"]) == (len(moves), end), g
        if end == "two_passes":
            score = board.count_score() - komi
            winner = "black" if score > 0.1 else "white" if score < -0.1 else "draw"
            assert (got["score"], got["winner"]) == (score, winner), g
        else:
            assert (got["score"], got["winner"]) == (0.0, None), g
    return [r["length"] for r in result["games"]]


def _games(nets, games, boards, max_moves, answer_pass=True, size=9, keep_policy=True):
    from tamago_amd.nn.policy_player import policy_games
    seeds = [300 + g for g in range(games)]
    result = policy_games(nets[0], nets[1], games, size=size, komi=7.0, seeds=seeds, max_moves=max_moves, boards=boards,
                          superko=True, answer_pass=answer_pass, keep_policy=keep_policy)
    return result, seeds


@pytest.fixture(scope="module")
def games_on_8_boards(nets9):
    return _games(nets9, 20, 8, 30)


def test_games_equal_their_host_replay(games_on_8_boards):
    result, seeds = games_on_8_boards
    lengths = _replay_games(result, 20, seeds, 9, 7.0, 30, 8, True, True)
    assert result["positions"] == result["plies"] * 8
    # slots are refilled, and after games of odd and of even length
    refilled_after = [lengths[g] % 2 for g in range(20 - 8)]
    assert 0 in refilled_after and 1 in refilled_after, lengths


def test_games_without_the_pass_rule(nets9):
    result, seeds = _games(nets9, 6, 8, 30, answer_pass=False)
    _replay_games(result, 6, seeds, 9, 7.0, 30, 8, True, False)


def test_games_19x19():
    nets = _net(19, 31), _net(19, 32)
    result, seeds = _games(nets, 3, 2, 8, size=19)
    _replay_games(result, 3, seeds, 19, 7.0, 8, 2, True, True)


def test_games_do_not_depend_on_the_number_of_boards(nets9, games_on_8_boards):
    on3, _ = _games(nets9, 20, 3, 30, keep_policy=False)
    assert on3["games"] == games_on_8_boards[0]["games"]


def test_handle_lifetime_and_a_search_afterwards(nets9):
    """Create, run, destroy twice; the search handle goes after the player.  A following MCTSTree search is the search done
    before the player existed."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    from tamago_amd.nn.policy_player import PolicyBoards

    def search():
        np.random.seed(9)
        tree = MCTSTree(nets9[0], tree_size=512, batch_size=8)
        board = GoBoard(9, 7.0, True)
        board.put_stone(board.onboard_pos[40], 1)
        move = tree.search_best_move(board, 2, TimeManager(TimeControl.STRICT_PLAYOUT, 64), {})
        root = tree.get_root()
        return move, [int(v) for v in root.children_visits[:root.num_children]], float(np.random.random_sample())

    before = search()
    for life in range(2):
        boards = PolicyBoards(9, 4, True)
        for t in range(4):
            boards.set_root(t, GoBoard(9, 7.0, True), 1)
            boards.seed(t, random.Random(life * 10 + t).getstate())
        first = boards.moves_with(nets9[0], play=True)
        second = boards.moves_with(nets9[1], play=True, answer_pass=True)
        assert (first >= 0).all() and (second >= 0).all() and (boards.read_positions()[1] == 3).all()
        boards.close()                                   # tg_policy_destroy, then tg_search_destroy
        result, seeds = _games(nets9, 5, 4, 12, keep_policy=False)
        assert len(result["games"]) == 5
    assert search() == before


def test_match_plays_both_colour_assignments(nets9):
    from tamago_amd.policy_games import match
    one = match(nets9[0], nets9[1], 6, boards=4, max_moves=20)
    both = match(nets9[0], nets9[1], 6, boards=4, max_moves=20, swap=True)
    for res, games in ((one, 6), (both, 12)):
        assert res["games"] == games == res["wins_a"] + res["wins_b"] + res["draws"] + res["unfinished"]
        assert res["positions"] > 0 and 2 <= res["mean_length"] <= 20
    # the first leg of the swapped match is the plain match: the second leg accounts for the difference
    for key in ("wins_a", "wins_b", "draws", "unfinished"):
        assert both[key] >= one[key]


def test_rl_loop_gate_logs_new_against_previous(tmp_path, monkeypatch):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import rl_loop
    import tamago_amd.nn.data_generator as dg
    monkeypatch.setattr(dg, "BATCH_SIZE", 32)
    torch.manual_seed(12)
    np.random.seed(12)
    lines = []
    rl_loop.run_generation(str(tmp_path), 0, 24, 16, 16, 32, log=lines.append, gate_games=6)
    assert len(lines) == 2 and "new against previous over 12 policy games" in lines[0]
    plain = []
    rl_loop.run_generation(str(tmp_path), 1, 24, 16, 16, 32, log=plain.append)
    assert len(plain) == 1


def test_policy_moves_of_mixed_positions(nets9):
    """policy_moves: positions of both colours, with and without the superko check, one stream each, in one launch set - each
    the host rule on the network's own output for that position, each stream advanced by its one draw."""
    from tamago_amd.nn.feature import generate_input_planes
    from tamago_amd.nn.policy_player import choose_from_policy, policy_moves
    cases = load(9)[0]["cases"]
    assert {c["color"] for c in cases} == {1, 2} and {c["superko"] for c in cases} == {True, False}
    positions = [replay(9, case) for case in cases]
    states = [prepared_rng(case).getstate() for case in cases]
    moves, after = policy_moves(nets9[0], positions, states)
    for k, (case, (board, color)) in enumerate(zip(cases, positions)):
        rng = prepared_rng(case)
        policy, _ = nets9[0].inference(torch.tensor(generate_input_planes(board, color).reshape(1, 6, 9, 9)))
        assert int(moves[k]) == choose_from_policy(policy[0].numpy().tolist(), board, color, rng), case["name"]
        assert after[k] == rng.getstate()[1], case["name"]


def test_command_line_match(nets9, tmp_path, capsys):
    import json
    from tamago_amd import policy_games
    files = []
    for k, net in enumerate(nets9):
        files.append(str(tmp_path / f"net{k}.bin"))
        torch.save(net.state_dict(), files[-1])
    grad = torch.is_grad_enabled()
    try:
        policy_games.main(["--black", files[0], "--white", files[1], "--games", "6", "--boards", "4", "--max-moves", "20",
                           "--swap", "true"])
    finally:
        torch.set_grad_enabled(grad)                  # (load_network switches it off for the process, like the reference)
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["games"] == 12 == summary["wins_a"] + summary["wins_b"] + summary["draws"] + summary["unfinished"]
    assert summary["games_per_second"] > 0 and 2 <= summary["mean_length"] <= 20
    direct = policy_games.match(nets9[0], nets9[1], 6, boards=4, max_moves=20, swap=True)
    for key in ("wins_a", "wins_b", "draws", "unfinished", "mean_length", "positions"):
        assert summary[key] == direct[key], key
