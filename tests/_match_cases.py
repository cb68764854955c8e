"""Shared cases of the match tests (test_match_host.py, test_gpu_match.py): the match game on the CPU oracle and a crafted
evaluator that makes its user resign."""
import functools
import random
import re

import numpy as np
import torch

from oracle.stubnet import StubNet

SIZE, VISITS = 9, 16


def reference_never_resign(k: int) -> bool:
    """never_resign as the reference worker draws it after random.seed(k) (worker.py:39,53; test_gpu_selfplay.py)."""
    random.seed(k)
    random.choice([k])
    return random.randint(1, 10) == 1


class Despair(StubNet):
    """StubNet(salt) whose value output is [0, 0, 1] - "the side to move wins" - for every position with fewer than `empty`
    empty points (input plane 0): every move its user looks at then hands the opponent a won position, its root's best child
    evaluates to 0 and falls under the resign threshold."""

    def __init__(self, salt: int, empty: int):
        super().__init__(salt)
        self.empty = empty

    def _value(self, planes, value):
        lost = planes[:, 0].reshape(planes.shape[0], -1).sum(dim=1) < self.empty
        value = value.clone()
        value[lost] = torch.tensor([0.0, 0.0, 1.0])
        return value

    def inference(self, planes):
        policy, value = super().inference(planes)
        return policy, self._value(planes, value)

    def inference_with_policy_logits(self, planes):
        logits, value = super().inference_with_policy_logits(planes)
        return logits, self._value(planes, value)


class _RootView:
    """What SelfPlayRecord.save_record reads of a root, off an oracle node: child count, child moves, improved_policy()."""

    def __init__(self, node):
        self.node = node

    def get_num_children(self):
        return int(self.node.num_children)

    def get_child_move(self, i):
        return int(self.node.action[i])

    def calculate_improved_policy(self):
        return self.node.improved_policy()


def oracle_match_game(seed, net_black, net_white, visits, size, never_resign, names=None):
    """The reference's selfplay_worker loop (selfplay/worker.py:44-90) after np.random.seed(seed) on oracle.tree.MCTSTree, with
    tree.network = net_black for every black move and net_white for every white move.  Returns the SGF text (PB / PW = names,
    None: the self-play defaults) and (moves played, ending): ending is "resign", "passes" or "limit"."""
    from oracle.board import GoBoard, BLACK, PASS, RESIGN
    from oracle.tree import MCTSTree, TimeManager, TimeControl
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.board.stone import Stone
    from tamago_amd.sgf.selfplay_record import SelfPlayRecord
    nets = {1: net_black, 2: net_white}
    tree = MCTSTree(net_black, size, tree_size=max(160, visits + 8), batch_size=10 ** 9)
    tm = TimeManager(TimeControl.CONSTANT_PLAYOUT, visits)
    record = SelfPlayRecord("", Coordinate(size), players=names)
    saved = np.random.get_state()
    np.random.seed(seed)                                                      # worker.py:38
    try:
        board = GoBoard(size, 7.0, True)
        color, passes, moves = BLACK, 0, 0
        winner, is_resign, score, ending = Stone.EMPTY, False, 0.0, "limit"
        for _ in range(size * size * 2):                                      # worker.py:44
            tree.network = nets[color]
            pos = tree.generate_move_with_sequential_halving(board, color, tm, never_resign)
            if pos == RESIGN:
                winner, is_resign, ending = (Stone.WHITE if color == BLACK else Stone.BLACK), True, "resign"
                break
            board.put_stone(pos, color)
            passes = passes + 1 if pos == PASS else 0
            record.save_record(_RootView(tree.get_root()), pos, color)
            color = 3 - color
            moves += 1
            if passes == 2:
                score = board.count_score() - board.get_komi()
                winner = Stone.BLACK if score > 0.1 else (Stone.WHITE if score < -0.1 else Stone.OUT_OF_BOARD)
                ending = "passes"
                break
        return record.to_sgf(winner, board.get_komi(), is_resign, score), (moves, ending)
    finally:
        np.random.set_state(saved)


def oracle_result(text: str, moves: int, ending: str, a_is_black: bool = True) -> dict:
    """The per-game result search_match reports (winner, is_resign, moves, a_is_black), read off an oracle game."""
    result = re.search(r"RE\[([^\]]*)\]", text).group(1)
    winner = {"B": "black", "W": "white"}.get(result[0]) if result != "0" else ("draw" if ending == "passes" else None)
    return {"winner": winner, "is_resign": ending == "resign", "moves": moves, "a_is_black": a_is_black}


def make_net(spec):
    """("stub", salt) / ("despair", salt, empty) -> a fresh evaluator (a spec is hashable: the oracle games are cached by it)."""
    return StubNet(spec[1]) if spec[0] == "stub" else Despair(spec[1], spec[2])


@functools.lru_cache(maxsize=None)
def oracle_game(seed, black, white, never_resign=False, visits=VISITS, size=SIZE, names=("A", "B")):
    """oracle_match_game for evaluator specs, computed once per process and shared by the tests."""
    return oracle_match_game(seed, make_net(black), make_net(white), visits, size, never_resign, names)


S301, S302 = ("stub", 301), ("stub", 302)
