"""Many networks in one lock-step engine (csrc/search.hip: group_rank_kernel, rows_by_rank_kernel, tg_search_puct_chain_groups;
SearchEngine.group_live / root_eval_groups / puct_chain_groups; selfplay/tournament.py) against numpy, the same
trees searched on one-network engines, the CPU oracle's games and puct_match.  Every comparison is exact; comparisons between
DualNet launches of different shapes count only while no f16 range fallback was taken - asserted, not skipped."""
import ctypes
import os

import numpy as np
import pytest

from tests import _early_stop_cases as cases
from tests import _puct_match_cases as pc
from tests._match_cases import make_net

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
SPECS = (("stub", 301), ("stub", 302), ("stub", 303))
NAMES = ("s301", "s302", "s303")


def _three_nets(size=9):
    import torch
    from tamago_amd.nn.network.dual_net import DualNet
    nets = []
    for seed in (21, 22, 23):
        torch.manual_seed(seed)
        nets.append(DualNet(torch.device("cuda:0"), size))
    return nets


def _small_engine(trees):
    """`trees` empty 9x9 boards on a minimal pool, roots expanded."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    from tests.test_gpu_early_stop import _dualnet
    eng = SearchEngine(9, trees, 4, 1, DeviceEvaluator(_dualnet(9)))
    board = GoBoard(9)
    for t in range(trees):
        eng.set_root(t, board, 1)
    eng.seed_trees(range(trees))
    eng.root_eval(False)
    return eng


def _expected(live, group, G):
    trees = np.flatnonzero(live)
    order = trees[np.argsort(group[trees], kind="stable")]
    rank = np.full(len(group), -1, dtype=np.int64)
    rank[order] = np.arange(len(order))
    count = np.bincount(group[trees], minlength=G)[:G]
    return count, np.cumsum(count) - count, rank


# ---- ranks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [3, 64])
@pytest.mark.parametrize("trees", [65, 1025])
def test_grouped_ranks_against_numpy(trees, groups):
    """T = 65 (a second wavefront of one tree) and 1025 (a second chunk of one tree: the per-group carry), G = 3 and 64, a
    third of the trees halted: ranks, counts and offsets are a stable sort's."""
    eng = _small_engine(trees)
    try:
        rnd = np.random.RandomState(trees + groups)
        halted = np.arange(trees) % 3 == 1
        eng.set_halt(halted)
        for group in (rnd.randint(0, groups, trees), np.arange(trees) % groups, np.full(trees, groups - 1)):
            count = eng.group_live((group, groups))
            want_count, want_offset, want_rank = _expected(~halted, group, groups)
            assert np.array_equal(count, want_count) and np.array_equal(eng.group_offsets, want_offset)
            assert np.array_equal(eng.read_live_rank(), want_rank)
        # plain live ranks replace the table, and the other way round
        assert eng.compact_live() == int((~halted).sum())
        assert np.array_equal(eng.read_live_rank(), _expected(~halted, np.zeros(trees, dtype=np.int64), 1)[2])
    finally:
        eng.close()


# ---- rows by rank ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trees", [1, 63, 65])
def test_gather_then_scatter_is_the_identity_on_ranked_trees(trees):
    """Rows of 3, 82, 170, 362, 6 x 81 floats (none a multiple of 16 bytes) and of 324 (one that is), from buffers aligned to
    16 bytes and from buffers one float off: gathered rows lie at their ranks, rows without a tree keep what they held, the
    scatter brings every ranked tree's row back and leaves the others alone."""
    import torch
    eng = _small_engine(trees)
    try:
        rnd = np.random.RandomState(trees)
        halted = (np.arange(trees) % 3 == 1) & (trees > 1)
        eng.set_halt(halted)
        group = rnd.randint(0, 3, trees)
        eng.group_live((group, 3))
        rank = eng.read_live_rank()
        ranked = np.flatnonzero(rank >= 0)
        assert len(ranked) == int((~halted).sum())
        dev = eng.device
        for row in (3, 82, 170, 362, 6 * 81, 324):
            for shift in (0, 1):
                def buffer(fill):
                    flat = torch.full((trees * row + shift,), float(fill), dtype=torch.float32, device=dev)
                    return flat[shift:].view(trees, row)
                src = buffer(0.0)
                src.copy_(torch.from_numpy(rnd.standard_normal((trees, row)).astype(np.float32)))
                packed, back = buffer(-7.0), buffer(5.0)
                eng.gather_rows_by_rank(src, packed)
                eng.scatter_rows_by_rank(packed, back)
                host, got, again = src.cpu().numpy(), packed.cpu().numpy(), back.cpu().numpy()
                assert np.array_equal(got[rank[ranked]], host[ranked]), (row, shift)
                assert (got[len(ranked):] == -7.0).all(), (row, shift)
                assert np.array_equal(again[ranked], host[ranked]) and (again[rank < 0] == 5.0).all(), (row, shift)
    finally:
        eng.close()


# ---- the chain ------------------------------------------------------------------------------------------------------------
PLIES, GROUPS, VISITS, BATCH = (0, 4, 10, 20, 30, 40), (0, 1, 2, 2, 1, 0), 48, 16


def _roots(eng):
    for t, ply in enumerate(PLIES):
        eng.set_root(t, cases.product_board(ply), 1, np.random.RandomState(100 + t).get_state())


def _states(eng):
    digests = eng.tree_digests()
    return [(tuple(int(x) for x in digests[t]), eng.streams[t].final_state()) for t in range(len(PLIES))]


@pytest.fixture(scope="module")
def chain_case():
    """Three random-init DualNets and, per network, the six trees searched by puct_chain on a one-network engine."""
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    nets = _three_nets()
    batches = [BATCH] * (VISITS // BATCH)
    alone = []
    for net in nets:
        eng = SearchEngine(9, len(PLIES), VISITS + 16, BATCH, DeviceEvaluator(net))
        try:
            _roots(eng)
            eng.root_eval(False)
            assert eng.can_chain(VISITS)
            eng.puct_chain(batches)
            alone.append(_states(eng))
        finally:
            eng.close()
    return nets, batches, alone


@pytest.mark.parametrize("halted", [None, 2], ids=["all_live", "one_halted"])
def test_the_grouped_chain_equals_one_network_chains(chain_case, halted):
    """Six trees on distinct real positions, groups [0, 1, 2, 2, 1, 0], 48 visits in mini-batches of 16 through the library's
    grouped chain: every tree's digest and stream are those of the same root and seed on a one-network engine.  With tree 2
    halted the same holds for the others; with trees 2 and 3 halted group 2 is empty and its network gets nothing."""
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    nets, batches, alone = chain_case
    fallbacks0 = sum(n.range_fallbacks() for n in nets)
    for halt in ([None] if halted is None else [[0, 0, 1, 0, 0, 0], [0, 0, 1, 1, 0, 0]]):
        evaluators = [DeviceEvaluator(n) for n in nets]
        eng = SearchEngine(9, len(PLIES), VISITS + 16, BATCH, evaluators[0])
        try:
            _roots(eng)
            eng.root_eval_groups(evaluators, np.array(GROUPS), halt=None if halt is None else np.array(halt, dtype=bool))
            live = np.ones(len(PLIES), dtype=bool) if halt is None else ~np.array(halt, dtype=bool)
            count = np.bincount(np.array(GROUPS)[live], minlength=3)
            assert eng.group_counts.tolist() == count.tolist()
            assert [e.batches for e in evaluators] == [[int(c)] if c else [] for c in count]          # the roots: one call per segment
            assert eng.can_chain_groups(VISITS, evaluators)
            before = dict(eng.forward_positions_by_group)
            assert eng.puct_chain_groups(batches, evaluators) == len(batches)
            by_group = [eng.forward_positions_by_group.get(g, 0) - before.get(g, 0) for g in range(3)]
            assert by_group == [int(c) * VISITS for c in count]
            got = _states(eng)
            visits = eng.read_root_stats()["node_visits"]
            for t in np.flatnonzero(live):
                want = alone[GROUPS[t]][t]
                assert got[t][0] == want[0], t
                assert pc.same_stream((got[t][1][1], got[t][1][2]), want[1]), t
                assert int(visits[t]) == VISITS
            for t in np.flatnonzero(~live):
                assert int(visits[t]) == 0                                                        # a halted tree never searched
        finally:
            eng.close()
    assert sum(n.range_fallbacks() for n in nets) == fallbacks0, "an f16 range fallback was taken: the comparison does not count"


# ---- tournaments ----------------------------------------------------------------------------------------------------------
def _read(d, index):
    return open(os.path.join(d, f"{index}.sgf"), encoding="utf-8").read()


@pytest.mark.parametrize("boards", [1, 2, 4])
def test_the_tournament_under_host_stubnets_equals_the_oracle_games(boards, tmp_path):
    """Three StubNets, 26 visits x batch 8, one game per ordered pair: the one-by-one path (host evaluators) - records, results
    and final streams are the oracle's on 1, 2 and 4 boards."""
    from tamago_amd.selfplay.tournament import puct_tournament, schedule
    games = [pc.oracle_puct_game(index, SPECS[b], SPECS[w], black_search=(26, 8), white_search=(26, 8), names=(NAMES[b], NAMES[w]))
             for index, (b, w) in enumerate(schedule(3, 1))]
    out = puct_tournament([(name, make_net(spec)) for name, spec in zip(NAMES, SPECS)], 26, 8, boards=boards, save_dir=str(tmp_path))
    for i, (text, end, state) in enumerate(games):
        assert _read(tmp_path, i) == text, i
        want = pc.oracle_result(text, *end)
        assert {k: out["results"][i][k] for k in ("winner", "is_resign", "moves")} == {k: want[k] for k in ("winner", "is_resign", "moves")}
        assert pc.same_stream(out["results"][i]["stream"], state), i
    assert sum(sum(c.values()) for row in out["crosstable"] for c in row if c is not None) == 6
    assert sum(out["forward_positions_by_entrant"]) == out["forward_positions"] >= out["leaf_evals"]


def _against_puct_match(nets, names, visits, batch, size, boards, tmp_path):
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    from tamago_amd.selfplay.tournament import puct_tournament, schedule
    d = tmp_path / "tournament"
    out = puct_tournament(list(zip(names, nets)), visits, batch, size=size, boards=boards, save_dir=str(d))
    fallbacks = out["range_fallbacks"]
    per_game = []
    for index, (b, w) in enumerate(schedule(len(nets), 1)):
        duel = tmp_path / f"duel{index}"
        ref = puct_match(EngineSetup(nets[b], visits, batch), EngineSetup(nets[w], visits, batch), 1, size=size, boards=1, seeds=[index],
                         save_dir=str(duel), names=(names[b], names[w]))
        fallbacks += ref["range_fallbacks"]
        assert _read(d, index) == _read(duel, 0), index
        a, r = out["results"][index], ref["results"][0]
        assert {k: a[k] for k in ("winner", "is_resign", "moves", "score", "seed")} == {k: r[k] for k in ("winner", "is_resign", "moves", "score", "seed")}
        assert pc.same_stream(a["stream"], ("MT19937", r["stream"][0], r["stream"][1], 0, 0.0)), index
        per_game.append(a["moves"] + (1 if a["is_resign"] else 0))
    assert fallbacks == 0, "an f16 range fallback was taken: the comparison does not count"
    return out, per_game


def test_the_tournament_under_dualnets_equals_puct_match_game_by_game(tmp_path):
    """Three random-init DualNets, 48 visits x batch 16, 4 boards, the library's grouped chain: every game is the puct_match
    game of its ordered pair and seed.  No parking: every live game moves in every call, so the calls are bounded as a greedy
    schedule of the games on 4 slots is - the games' calls over the slots, plus the longest game."""
    nets = _three_nets()
    out, per_game = _against_puct_match(nets, ("a", "b", "c"), 48, 16, 9, 4, tmp_path)
    assert all(n >= 10 for n in per_game)
    assert max(per_game) <= out["calls"] <= sum(per_game) / 4 + max(per_game)
    assert out["restarts"] == 2
    assert sum(out["forward_positions_by_entrant"]) == out["forward_positions"]
    assert out["leaf_evals"] <= out["forward_positions"] <= out["leaf_evals"] + out["one_child_roots"] * 48


def test_a_13x13_game_pair_equals_puct_match(tmp_path):
    """Nothing is hard-wired to 9: two entrants, both colours, 16 visits x batch 8 on 13x13."""
    from tests import _match_games as mg
    out, per_game = _against_puct_match(list(mg.two_nets(13)), ("a", "b"), 16, 8, 13, 2, tmp_path)
    assert out["calls"] == max(per_game) and out["restarts"] == 0


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_abi():
    from tamago_amd import lib as tl
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    nets = _three_nets()
    eng = SearchEngine(9, 3, 64, 4, DeviceEvaluator(nets[0]))
    try:
        for t, ply in enumerate((0, 10, 20)):
            eng.set_root(t, cases.product_board(ply), 1, np.random.RandomState(9).get_state())
        eng.root_eval(False)
        lib, count = eng.lib, np.zeros(64, dtype=np.int32)

        def group_live(group, n):
            arr = np.ascontiguousarray(group, dtype=np.int32)
            return lib.tg_search_group_live(eng.handle, arr.ctypes.data, n, count.ctypes.data, eng._stream())

        import torch
        policy = torch.zeros((3 * 4, eng.A), dtype=torch.float32, device=eng.device)
        value = torch.zeros((3 * 4, 3), dtype=torch.float32, device=eng.device)
        leaves = np.array([4, 4], dtype=np.int32)

        def chain(handles, n=None):
            arr = (ctypes.c_void_p * len(handles))(*handles)
            return lib.tg_search_puct_chain_groups(eng.handle, arr, len(handles) if n is None else n, leaves.ctypes.data, 2, 1,
                                                   eng.planes.data_ptr(), policy.data_ptr(), value.data_ptr(), eng._stream(), None)
        handles = [n.handle for n in nets]
        assert chain(handles) == ERR_STATE                                # never computed
        assert group_live([0, 0, 0], 0) == ERR_ARG and group_live([0, 0, 0], 65) == ERR_ARG
        assert group_live([0, 3, 1], 3) == ERR_ARG and group_live([0, -1, 1], 3) == ERR_ARG
        assert "group" in tl.load().tg_last_error().decode()
        assert group_live([0, 2, 2], 3) == 0 and count[:3].tolist() == [1, 0, 2]
        assert chain(handles, 0) == ERR_ARG and chain(handles * 22, 65) == ERR_ARG and chain(handles[:2]) == ERR_ARG
        assert chain([handles[0], handles[1], None]) == ERR_ARG           # a null network for a group that has live trees
        eng.root_eval(False)
        assert chain(handles) == ERR_STATE                                # stale after root_eval
        assert "reset a root" in tl.load().tg_last_error().decode()
        assert eng.compact_live() == 3
        assert chain(handles) == ERR_STATE                                # plain live ranks are in force
        assert "plain live ranks" in tl.load().tg_last_error().decode()
        assert group_live([0, 2, 2], 3) == 0
        eng.set_halt([0, 0, 1])
        assert chain(handles) == ERR_STATE                                # halt words written since
        assert eng.num_nodes().tolist() == [1, 1, 1]                      # nothing was launched by a refused call
        # ... and a null network for an EMPTY group is accepted
        assert group_live([0, 2, 2], 3) == 0 and count[:3].tolist() == [1, 0, 1]
        eng.node_bound += 8
        assert chain([handles[0], None, handles[2]]) == 0
        eng._collect_rng()
        assert eng.read_root_stats()["node_visits"].tolist() == [8, 8, 0]
    finally:
        eng.close()
