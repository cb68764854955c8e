"""Batch analysis on the GPU (tamago_amd/mcts/analysis.py, tg_search_read_analysis): against the reference's recorded
analysis, against the single-tree path at every size and with the device network, the read-out kernel against the host
PV walk, edge cases and the command line."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def _games():
    return json.load(open(os.path.join(GOLDEN, "selfplay_games.json")))


def _game_positions(key, superko=True):
    from tamago_amd.mcts.analysis import game_positions
    from tamago_amd.sgf.reader import SGFReader
    return game_positions(SGFReader(_games()[key], 9, literal=True), superko, key)


def _single(network, board, color, seed, visits, batch, cgos_mode=False):
    """The contract's single-tree run: (best, lz, cgos or None)."""
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    np.random.seed(seed)
    tree = MCTSTree(network, tree_size=visits + 16, batch_size=batch, cgos_mode=cgos_mode)
    best = tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, visits), {})
    root = tree.get_root()
    lz = root.get_analysis(board, "lz", tree.get_pv_lists)
    cg = root.get_analysis(board, "cgos", tree.get_pv_lists) if root.node_visits else None
    return best, lz, cg


def _strings(results):
    return [(a.best_move, a.lz(), a.cgos() if a.visits else None) for a in results]


def _playout_positions(size, count, seed):
    """Plies of a seeded random play-out (legal moves, no passes), the side to move alternating."""
    from tamago_amd.board.go_board import GoBoard
    import copy
    rs = np.random.RandomState(seed)
    board, color, out = GoBoard(size), 1, []
    for ply in range(count * 3):
        if ply % 3 == 0:
            out.append((copy.deepcopy(board), color))
        legal = [p for p in board.get_all_legal_pos(color)]
        board.put_stone(int(legal[rs.randint(len(legal))]), color)
        color = 3 - color
    return out[:count]


def test_against_the_reference_recording():
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.analysis import analyze_positions
    gold = json.load(open(os.path.join(GOLDEN, "analysis_s9.json")))
    pos = _game_positions(gold["game"], gold["superko"])
    res = analyze_positions(StubNet(8), [(p.board, p.color) for p in pos], gold["visits"], batch_size=gold["batch_size"],
                            check_superko=True, seeds=[gold["seed0"] + k for k in range(len(pos))])
    assert len(res) == len(pos)
    for rec in gold["positions"]:
        a = res[rec["k"]]
        assert a.best_move == rec["best"], rec["k"]
        assert a.lz() == rec["lz"], rec["k"]
        if "cgos" in rec:
            assert a.cgos() == rec["cgos"], rec["k"]


def test_tree_count_does_not_change_the_results():
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.analysis import analyze_positions
    pos = _game_positions("2,16")[::4]
    args = ([(p.board, p.color) for p in pos], 60)
    kw = dict(batch_size=16, check_superko=True, seeds=[11 + k for k in range(len(pos))])
    runs = [_strings(analyze_positions(StubNet(8), *args, max_trees=m, **kw)) for m in (1, 7, None)]
    assert runs[0] == runs[1] == runs[2]


@pytest.mark.parametrize("size", [13, 19])
def test_against_the_single_tree_path_at_every_size(size):
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.analysis import analyze_positions
    pos = _playout_positions(size, 6, size)
    seeds = [100 + k for k in range(len(pos))]
    res = analyze_positions(StubNet(5), pos, 48, batch_size=8, seeds=seeds, pv_depth=4)
    for (board, color), seed, got in zip(pos, seeds, _strings(res)):
        assert got == _single(StubNet(5), board, color, seed, 48, 8)


def test_real_network_against_the_single_tree_path():
    from oracle.net import make_state_dict
    from tamago_amd.mcts.analysis import analyze_positions
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), 9)
    net.load_state_dict(make_state_dict(9, 11, 1.4))
    pos = [(p.board, p.color) for key in ("1,16", "2,16", "3,50") for p in _game_positions(key, False)[::5]][:64]
    assert len(pos) == 64
    seeds = [1000 + k for k in range(len(pos))]
    res = analyze_positions(net, pos, 200, batch_size=16, max_trees=40, seeds=seeds)
    for (board, color), seed, got in zip(pos, seeds, _strings(res)):
        assert got == _single(net, board, color, seed, 200, 16)


def _host_pv_lists(engine, tree, root, coord):
    """mcts/tree.py:432-473 over read_node (node[-1] is the pool's last slot)."""
    from tamago_amd.mcts.engine import continue_pv
    out = {}
    full = engine.read_node(tree, 0)
    for i in range(root.num_children):
        if root.children_visits[i] > 0:
            start = int(full.children_index[i])
            seq = continue_pv([root.action[i]], start if start != -1 else engine.N - 1,
                              lambda n: engine.read_node(tree, n))
            out[coord.convert_to_gtp_format(root.action[i])] = [coord.convert_to_gtp_format(p) for p in seq]
    return out


@pytest.mark.parametrize("batch", [1, 16])
def test_read_out_kernel_against_the_host_walk(batch):
    from oracle.stubnet import StubNet
    from tamago_amd.board.coordinate import Coordinate
    from tamago_amd.mcts.engine import SearchEngine, HostEvaluator
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    pos = _game_positions("1,16", False)
    coord = Coordinate(9)
    # one tree through MCTSTree: the kernel's PVs are MCTSTree.get_pv_lists's
    board, color = pos[10].board, pos[10].color
    np.random.seed(3)
    tree = MCTSTree(StubNet(8), tree_size=1100, batch_size=batch)
    tree.search_best_move(board, color, TimeManager(TimeControl.STRICT_PLAYOUT, 1000), {})
    want = tree.get_pv_lists(tree.get_root(), coord)
    assert max(len(v) for v in want.values()) > 2
    for depth in (32, 2):
        root, pv_lists = tree._engine.read_analysis(depth)[0]
        assert pv_lists(root, coord) == want
    # several trees at once: every tree's PVs against the host walk
    engine = SearchEngine(9, 4, 1100, batch, HostEvaluator(StubNet(8), torch.device("cuda:0")))
    for k in range(4):
        engine.set_root(k, pos[20 * k].board, pos[20 * k].color, np.random.RandomState(k).get_state())
    engine.root_eval()
    for _ in range(1000 // batch):
        engine.ensure_capacity(batch)
        engine.puct_batch(batch)
    for depth in (32, 2):
        for k, (root, pv_lists) in enumerate(engine.read_analysis(depth)):
            assert pv_lists(root, coord) == _host_pv_lists(engine, k, root, coord)
    engine.close()


class _LosingNet:
    """StubNet policy; the value says the side to move at the leaf wins (plane 5: the colour plane), so every root child
    of a Black (White) root looks lost (won)."""

    def __init__(self):
        from oracle.stubnet import StubNet
        self.stub = StubNet(1)

    def inference(self, x):
        policy, _ = self.stub.inference(x)
        black = (x[:, 5].reshape(x.shape[0], -1).mean(dim=1) > 0).float()
        value = torch.stack([1.0 - black, torch.zeros_like(black), black], dim=1)
        return policy, value


def test_edge_cases():
    from oracle.stubnet import StubNet
    from tamago_amd.board.constant import PASS, RESIGN
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.lib import TamagoHipError
    from tamago_amd.mcts.analysis import analyze_positions
    from tamago_amd.mcts.engine import SearchEngine, HostEvaluator
    # a pass-only root answers PASS without a search, in a batch with ordinary positions
    full = GoBoard(9)
    for p in full.onboard_pos:
        if p not in (12, 14):
            full.cells[p] = 1
    full.moves = 5
    pos = [(GoBoard(9), 1), (full, 2), (GoBoard(9), 2)]
    res = analyze_positions(StubNet(3), pos, 40, batch_size=8, seeds=[1, 2, 3])
    assert res[1].best_move == PASS and res[1].status == [] and res[1].lz() == "\n"
    for (board, color), seed, a in zip(pos, [1, 2, 3], res):
        best, lz, _ = _single(StubNet(3), board, color, seed, 40, 8)
        assert (a.best_move, a.lz()) == (best, lz)
    # resigning positions
    net = _LosingNet()
    pos = [(p.board, p.color) for p in _game_positions("3,50", False)[10:14]]
    res = analyze_positions(net, pos, 40, batch_size=8, seeds=[7, 8, 9, 10])
    assert RESIGN in [a.best_move for a in res]
    for (board, color), seed, got in zip(pos, [7, 8, 9, 10], _strings(res)):
        assert got == _single(net, board, color, seed, 40, 8)
    # the kernel looks an unexpanded root child up as node N - 1 (the host's node[-1]); a search never leaves a visited
    # root child unexpanded, so this checks the walks against the host's with the pool's last slot in use
    engine = SearchEngine(9, 2, 24, 8, HostEvaluator(StubNet(3), torch.device("cuda:0")))
    for k in range(2):
        engine.set_root(k, GoBoard(9), 1, np.random.RandomState(k).get_state())
    engine.root_eval()
    for _ in range(64):                               # one descent at a time until the pool's last slot holds a node
        if int(engine.num_nodes().min()) == 24:
            break
        engine.puct_batch(1)
    assert list(engine.num_nodes()) == [24, 24]
    from tamago_amd.board.coordinate import Coordinate
    coord = Coordinate(9)
    for k, (root, pv_lists) in enumerate(engine.read_analysis(32)):
        assert pv_lists(root, coord) == _host_pv_lists(engine, k, root, coord)
    # a tree with its error flag set raises
    engine.puct_batch(8)                              # the pool is full: sticky error
    with pytest.raises(TamagoHipError, match="node pool full"):
        engine.read_analysis(32)
    engine.close()


def test_command_line(tmp_path):
    from oracle.stubnet import StubNet
    from tamago_amd import analyze
    from tamago_amd.mcts.analysis import analyze_positions, game_seeds
    from tamago_amd.board.stone import color_value
    from tamago_amd.sgf.reader import SGFReader
    games = _games()
    paths = []
    for key, cut in (("1,16", 12), ("2,16", 9)):
        sgf = SGFReader(games[key], 9, literal=True)
        moves = "".join(f";{'B' if color_value(sgf.get_color(i)) == 1 else 'W'}[{_sgf_coord(sgf.get_move_data(i))}]"
                        for i in range(cut))
        path = tmp_path / f"g{key[0]}.sgf"
        path.write_text(f"(;GM[1]SZ[9]KM[7.0]{moves})")
        paths.append(str(path))
    out_dir = tmp_path / "out"
    common = paths + ["--visits", "30", "--batch-size", "8", "--trees", "5", "--seed", "4", "--sgf-out", str(out_dir)]
    jsonl = tmp_path / "a.jsonl"
    with open(jsonl, "w") as f:
        analyze.run(analyze.parser().parse_args(common), out=f, network_for=lambda size: StubNet(2))
    lines = [json.loads(x) for x in open(jsonl)]
    assert len(lines) == 13 + 10
    lz = tmp_path / "a.lz"
    with open(lz, "w") as f:
        analyze.run(analyze.parser().parse_args(common + ["--format", "lz"]), out=f, network_for=lambda size: StubNet(2))
    got = open(lz).read().splitlines(keepends=True)
    want = []
    for path in paths:
        positions = analyze.load_games([path], False)[path][1]
        res = analyze_positions(StubNet(2), [(p.board, p.color) for p in positions], 30, batch_size=8,
                                seeds=game_seeds(4, len(positions)))
        want += [a.lz() for a in res]
    assert got == want
    for path in paths:
        back = SGFReader(str(out_dir / os.path.basename(path)), 9)
        orig = SGFReader(path, 9)
        assert back.get_n_moves() == orig.get_n_moves()
        assert [back.get_move_data(i) for i in range(back.get_n_moves())] == list(orig.get_moves())
        assert back.get_comment(0).startswith("B to move, winrate ")


def _sgf_coord(pos):
    if pos == 0:
        return ""
    from tamago_amd.board.coordinate import Coordinate
    return Coordinate(9).convert_to_sgf_format(pos)
