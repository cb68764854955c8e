"""Idle trees compacted out of the forward passes of lock-step PUCT (csrc/search.hip: live_rank_kernel, the COMPACT leaf layout of
the four PUCT selectors and the backup, tg_search_puct_chain_compact) against numpy, the CPU oracle's searches and
games (tests/_early_stop_cases.py, tests/_puct_match_cases.py) and the same calls without compaction.  Every comparison is
exact; the positions a call may evaluate are worked out on the CPU (tests/test_live_rank_host.py)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _early_stop_cases as cases
from tests.test_live_rank_host import compact_positions, lockstep_expected

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ERR_ARG, ERR_STATE = -1, -3


def _stub_evaluator(seed):
    import torch
    from tamago_amd.mcts.engine import HostEvaluator
    return HostEvaluator(cases.make_evaluator("stub", seed), torch.device("cuda", 0))


def _dualnet(size=9):
    from tests.test_gpu_early_stop import _dualnet as make
    return make(size)


def _expected_ranks(live):
    live = np.asarray(live, dtype=bool)
    return int(live.sum()), np.where(live, np.cumsum(live) - live, -1)


# ---- ranks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trees", [65, 1025])
def test_live_ranks_against_numpy(trees):
    """T = 65 (a second wavefront of one tree) and 1025 (a second chunk of one tree: the carry) on engines with a minimal
    pool: the ranks behind set_halt are numpy's, for a random mask, for the ends and for no live tree at all; rootless trees
    are not live."""
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    eng = SearchEngine(9, trees, 4, 1, DeviceEvaluator(_dualnet()))
    try:
        rank = np.zeros(trees, dtype=np.int32)
        assert eng.lib.tg_search_read_live_rank(eng.handle, rank.ctypes.data) == ERR_STATE        # nothing computed, nothing allocated
        assert eng.compact_live() == 0 and (eng.read_live_rank() == -1).all()                     # no tree has a root yet
        board = GoBoard(9)
        for t in range(trees):
            eng.set_root(t, board, 1)
        eng.seed_trees(range(trees))
        eng.root_eval(False)
        assert eng.compact_live() == trees and eng.read_live_rank().tolist() == list(range(trees))
        rnd = np.random.RandomState(trees)
        halted = np.zeros(trees, dtype=bool)
        for mask in (rnd.random_sample(trees) < 0.4, np.arange(trees) == 0, np.arange(trees) == trees - 1,
                     np.arange(trees) % 2 == 1, np.ones(trees, dtype=bool)):
            eng.set_halt(mask)                                           # (words are only ever set: the masks add up)
            halted |= mask
            count, want = _expected_ranks(~halted)
            assert eng.compact_live() == count
            assert np.array_equal(eng.read_live_rank(), want)
        assert halted.all() and (eng.read_live_rank() == -1).all()
    finally:
        eng.close()


def test_stale_ranks_are_refused_before_anything_is_launched():
    """After set_halt, after stop_rule and after root_eval the compact selection is refused with TG_ERR_STATE and no tree
    moves; ranks that only lost trees are taken where the caller says so, ranks from before a root reset never."""
    from tamago_amd.mcts.engine import SearchEngine
    eng = SearchEngine(9, 3, 80, 4, _stub_evaluator(9))
    try:
        for t, ply in enumerate((0, 10, 20)):
            eng.set_root(t, cases.product_board(ply), 1, np.random.RandomState(9).get_state())
        eng.root_eval(False)

        def select(shrunk_ok=0):
            return eng.lib.tg_search_select_puct_compact(eng.handle, 4, shrunk_ok, eng.planes.data_ptr(), None, eng._stream())
        assert select() == ERR_STATE and select(1) == ERR_STATE          # never computed
        assert eng.compact_live() == 3
        eng.set_halt([0, 1, 0])
        assert select() == ERR_STATE
        assert eng.compact_live() == 2
        eng.stop_rule(1000, wait=True)
        assert select() == ERR_STATE
        assert eng.compact_live() == 2
        eng.root_eval(False)
        assert select() == ERR_STATE and select(1) == ERR_STATE
        assert eng.num_nodes().tolist() == [1, 1, 1]                     # nothing was launched by a refused call
        # ... and with fresh ranks, or ranks that only lost trees, the mini-batch runs
        assert eng.compact_live() == 3
        eng.puct_batch(4, compact=True)
        eng.set_halt([0, 0, 1])
        eng.puct_batch(4, compact=True, shrunk_ok=True)
        assert eng.read_root_stats()["node_visits"].tolist() == [8, 8, 4]
    finally:
        eng.close()


# ---- lock-step trees against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [(0, 4, 10, 20, 30), (30, 4, 0, 10, 20)], ids=["corpus_order", "first_tree_halts"])
@pytest.mark.parametrize("poll_every", [1, 2, 0], ids=["poll1", "poll2", "poll_never"])
def test_lockstep_trees_equal_their_oracle_searches(poll_every, order):
    """tests/_early_stop_cases.py LOCKSTEP under the host StubNet, mini-batches one by one in the compact layout: every tree -
    pool digest, root, node count, next stream draw, halt word, stopped_at - is its single oracle search, and the positions
    evaluated are the CPU's figures (134 / 136 / 150; without compaction: 150 whatever the polls).  In the second order
    the first tree halts, which shifts every later tree's rank."""
    from tests.test_gpu_early_stop import _lockstep_engine, _tree_state
    kind, seed, visits, batch, plies = cases.LOCKSTEP
    by_ply = {c[3]: cases.oracle_result(c[0]) for c in cases.lockstep_cases()}
    want = [by_ply[p] for p in order]
    eng = _lockstep_engine(_stub_evaluator(seed), order, seed, visits, batch)
    try:
        launched, calls = eng.forward_positions, len(eng.evaluator.batches)
        run = eng.puct_chain([batch] * (visits // batch) + [visits % batch], early_total=visits, poll_every=poll_every, compact=True)
        assert run == 8
        for t, w in enumerate(want):
            assert _tree_state(eng, t) == (w["num_nodes"], w["node_visits"], w["child_visits"], w["digest"], w["rng_after"]), t
        halted, stopped_at = eng.read_halt()
        assert halted.tolist() == [w["halted"] for w in want] and stopped_at.tolist() == [w["stopped_at"] for w in want]
        positions = eng.forward_positions - launched
        print(f"positions evaluated: {positions} (poll_every {poll_every})")
        assert positions == lockstep_expected(poll_every, order) == {1: 134, 2: 136, 0: 150}[poll_every]
        assert sum(eng.evaluator.batches[calls:]) == positions and sum(eng.evaluator.network.calls[1:]) == positions
    finally:
        eng.close()


# ---- each selection kernel ------------------------------------------------------------------------------------------------
KERNELS = {
    "serial": ({"TG_SELECT_SERIAL": "1"}, "select_puct_kernel<"),
    "pipe": ({"TG_SELECT_MPIPE_TREES": "0"}, "select_puct_pipe_kernel<"),
    "mpipe": ({}, "select_puct_mpipe_kernel<"),
    "split": ({"TG_SELECT_SPLIT": "1"}, "select_puct_split_kernel<"),
}


@functools.lru_cache(maxsize=None)
def _kernel_run(kernel, layout):
    env = dict(os.environ, TG_DEBUG_KNOBS="1", TG_SELECT_SPLIT="0")
    for name in ("TG_SELECT_SERIAL", "TG_SELECT_MPIPE_TREES", "TG_SPLIT_CFG", "TG_MPIPE_CFG", "TG_SPLIT_TEST_MUTE", "TG_SHARED_DEVICE"):
        env.pop(name, None)
    env.update(KERNELS[kernel][0])
    res = subprocess.run([sys.executable, os.path.join(HERE, "_compact_kernels.py"), layout], env=env, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(next(line for line in res.stdout.splitlines() if line.startswith("COMPACT "))[len("COMPACT "):])


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_each_selection_kernel_in_the_compact_layout(kernel):
    """Three trees, the middle one halted from the host: under each of the four PUCT selection kernels the neighbours are,
    after three compact mini-batches, what they are after three strided ones - the last tree's leaves one tree's rows lower -,
    the halted tree is what it was, and the forward passes cover two trees, not three."""
    compact, strided = _kernel_run(kernel, "compact"), _kernel_run(kernel, "strided")
    assert KERNELS[kernel][1] in compact["kernel"] and compact["kernel"] == strided["kernel"]
    assert (compact["live"], compact["rank"]) == (2, [0, -1, 1])
    assert compact["before"] == strided["before"]
    assert compact["after"] == strided["after"]
    assert compact["after"][1] == compact["before"][1]
    assert compact["after"][0] != compact["before"][0] and compact["after"][2] != compact["before"][2]
    assert (compact["positions"], strided["positions"]) == (2 * 4 * 3, 3 * 4 * 3)


# ---- the chained path under a DualNet -------------------------------------------------------------------------------------
def test_chained_compaction_equals_the_chain_without_it():
    """Five trees, 120 visits, batch 4, the library's own chain: tree states and halt words with compaction are those
    without, polled after every mini-batch and never; strictly fewer positions where a tree halts and the host looks, exactly
    the figure the halts allow; a call whose every tree is halted queues no forward pass; no range fallback."""
    from tamago_amd.mcts.engine import DeviceEvaluator
    from tests.test_gpu_early_stop import _lockstep_engine, _tree_state
    net = _dualnet()
    plies, visits, batch = (0, 4, 10, 20, 30), 120, 4
    batches = [batch] * (visits // batch)

    def run(poll_every, compact):
        eng = _lockstep_engine(DeviceEvaluator(net), plies, 77, visits, batch)
        try:
            assert eng.can_chain(visits)
            launched = len(eng.evaluator.batches)
            ran = eng.puct_chain(batches, early_total=visits, poll_every=poll_every, compact=compact)
            positions = sum(eng.evaluator.batches[launched:])
            halted, stopped_at = eng.read_halt()
            states = [_tree_state(eng, t) + (bool(halted[t]), int(stopped_at[t])) for t in range(len(plies))]
            if compact:
                # every tree halted (by the rule or, now, by the host): the call looks once and launches no forward pass
                eng.set_halt([1] * len(plies))
                before = eng.forward_positions
                assert eng.puct_chain(batches[:3], early_total=visits, poll_every=1, compact=True) == 0
                assert eng.forward_positions == before and eng.evaluator.batches[-1] == 0
                assert [_tree_state(eng, t) for t in range(len(plies))] == [s[:5] for s in states]
            return ran, states, positions
        finally:
            eng.close()
    for poll_every in (1, 0):
        ran, states, positions = run(poll_every, False)
        ran_c, states_c, positions_c = run(poll_every, True)
        assert (ran_c, states_c) == (ran, states)
        assert positions == len(plies) * batch * ran
        # a tree the rule halted ran stopped_at / batch mini-batches (the rule follows full mini-batches only)
        tree_ran = [s[6] // batch if s[5] else len(batches) for s in states]
        halts_seen = any(s[5] and s[6] // batch < ran for s in states)
        print(f"poll_every {poll_every}: {positions_c} positions compacted, {positions} not; mini-batches per tree {tree_ran}")
        assert positions_c == compact_positions(tree_ran, batches[:ran], poll_every)
        if poll_every == 1:
            assert halts_seen and positions_c < positions             # (the corpus has a tree that halts before the last one)
        else:
            assert positions_c == positions                            # never looked: every slot stays
    assert net.range_fallbacks() == 0


# ---- matches and analysis -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _match_games(strict):
    from tests import _puct_match_cases as pc
    from tests.test_gpu_early_stop import MATCH_SEARCH, MATCH_SEEDS
    from tests.test_gpu_puct_match import SEEDS
    if strict == (True, True):
        return SEEDS, (pc.BLACK_SEARCH, pc.WHITE_SEARCH), [pc.oracle_puct_game(seed, pc.S301, pc.S302) for seed in SEEDS]
    return MATCH_SEEDS, MATCH_SEARCH, [cases.oracle_early_game(seed, pc.S301, pc.S302, *MATCH_SEARCH, strict) for seed in MATCH_SEEDS]


@pytest.mark.parametrize("boards", [2, 3])
@pytest.mark.parametrize("strict", [(False, False), (True, False), (True, True)], ids=["not_strict", "mixed", "strict"])
def test_matches_with_compaction_equal_the_oracle_games(strict, boards, tmp_path):
    """Four games on 2 and 3 boards, byte for byte the oracle's: records, results, final streams, with the idle slots of
    every call left out of its forward passes - so forward_positions lies below the figure of the same match without
    compaction (which the games' own idle slot-calls show must differ)."""
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    from tests._match_cases import make_net
    from tests._puct_match_cases import S301, S302
    from tests.test_gpu_puct_match import _check_games, _check_tally
    seeds, search, games = _match_games(strict)

    def match(d, **kwargs):
        a = EngineSetup(make_net(S301), *search[0], strict=strict[0])
        b = EngineSetup(make_net(S302), *search[1], strict=strict[1])
        return puct_match(a, b, len(seeds), boards=boards, seeds=list(seeds), save_dir=str(d), poll_every=1, **kwargs)
    out = match(tmp_path / "compact", compact_idle=True)
    _check_tally(out, _check_games(out, games, tmp_path / "compact"))
    plain = match(tmp_path / "plain")
    idle_slot_calls = out["slot_calls"] - out["moves"] - out["resignations"]
    assert idle_slot_calls > 0                                         # a slot without a game in some call: games differ in length
    for key in ("calls", "slot_calls", "moves", "leaf_evals", "one_child_roots"):
        assert out[key] == plain[key], key
    print(f"forward positions: {out['forward_positions']} compacted, {plain['forward_positions']} not; leaf evaluations {out['leaf_evals']}")
    assert out["leaf_evals"] <= out["forward_positions"] < plain["forward_positions"]
    assert out["range_fallbacks"] == 0


def test_batch_analysis_in_constant_mode_with_compaction():
    """Four positions, one engine, CONSTANT_PLAYOUT with compact_idle: lz and cgos bytes, best move and visits of
    MCTSTree.search_best_move under TimeManager(CONSTANT_PLAYOUT); and the strict mode with spare trees (5 positions in chunks
    of 4) equals itself without compaction."""
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.analysis import analyze_positions
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    from tamago_amd.mcts.tree import MCTSTree
    kind, seed, visits, batch, plies = cases.LOCKSTEP
    positions = [(cases.product_board(ply), 1) for ply in plies[1:]]
    seeds = [seed] * len(positions)
    res = analyze_positions(StubNet(seed), positions, visits, batch_size=batch, seeds=seeds, mode=TimeControl.CONSTANT_PLAYOUT,
                            compact_idle=True)
    for k, (board, color) in enumerate(positions):
        tree = MCTSTree(StubNet(seed), tree_size=visits + 16, batch_size=batch)
        np.random.seed(seeds[k])
        best = tree.search_best_move(board, color, TimeManager(TimeControl.CONSTANT_PLAYOUT, visits), {})
        root = tree.get_root()
        assert res[k].lz() == root.get_analysis(board, "lz", tree.get_pv_lists)
        assert res[k].cgos() == root.get_analysis(board, "cgos", tree.get_pv_lists)
        assert (res[k].best_move, res[k].visits) == (int(best), int(root.node_visits))
    assert [r.visits for r in res] == [28, 30, 30, 16]
    five = [(cases.product_board(ply), 1) for ply in plies]
    net_c, net_p = StubNet(seed), StubNet(seed)
    strict_c = analyze_positions(net_c, five, visits, batch_size=batch, seeds=[seed] * 5, max_trees=4, compact_idle=True)
    strict_p = analyze_positions(net_p, five, visits, batch_size=batch, seeds=[seed] * 5, max_trees=4)
    assert [(r.lz(), r.cgos(), r.best_move, r.visits) for r in strict_c] == [(r.lz(), r.cgos(), r.best_move, r.visits) for r in strict_p]
    assert sum(net_c.calls) < sum(net_p.calls)                         # the second chunk's three spare trees are not evaluated


# ---- misuse ---------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused():
    """A compact backup after a strided selection and a strided backup after a compact one; compaction with a Gumbel
    selection; compaction with the UNIQUE (and the packed) layout: TG_ERR_ARG, and no tree moves."""
    import torch
    from tamago_amd.mcts.engine import SearchEngine
    eng = SearchEngine(9, 3, 80, 4, _stub_evaluator(9))
    try:
        for t, ply in enumerate((0, 10, 20)):
            eng.set_root(t, cases.product_board(ply), 1, np.random.RandomState(9).get_state())
        eng.root_eval(False)
        lib, st = eng.lib, eng._stream()
        policy = torch.full((12, eng.A), 1.0 / eng.A, dtype=torch.float32, device=eng.device)
        value = torch.full((12, 3), 1.0 / 3, dtype=torch.float32, device=eng.device)

        def backup(compact, slots=4):
            fn = lib.tg_search_backup_compact if compact else lib.tg_search_backup
            return fn(eng.handle, policy.data_ptr(), value.data_ptr(), slots, 0, st)
        assert backup(True) == ERR_ARG                                   # the root launch is no compact selection
        eng.puct_select(4)                                               # strided
        assert backup(True) == ERR_ARG
        assert backup(False) == 0
        assert eng.compact_live() == 3
        eng._feed_rng(4 * eng.A)
        assert lib.tg_search_select_puct_compact(eng.handle, 4, 0, eng.planes.data_ptr(), None, st) == 0
        eng._collect_rng()
        assert backup(False) == ERR_ARG                                  # compact selection, strided backup
        assert backup(True, -1) == ERR_ARG and backup(True, 0) == ERR_ARG and backup(True, 5) == ERR_ARG      # unique, packed, beyond K
        assert backup(True) == 0
        visited = eng.read_root_stats()["node_visits"].tolist()
        assert visited == [8, 8, 8]
        # a Gumbel selection takes the record: no compact backup behind it
        eng.set_gumbel_noise()
        nc, mc = np.array([2, 2, 2], dtype=np.int32), np.array([1, 1, 1], dtype=np.int32)
        eng._feed_rng(2 * eng.A)
        assert lib.tg_search_select_gumbel(eng.handle, nc.ctypes.data, mc.ctypes.data, 2, eng.planes.data_ptr(), st) == 0
        eng._collect_rng()
        assert backup(True, 2) == ERR_ARG
        assert lib.tg_search_backup(eng.handle, policy.data_ptr(), value.data_ptr(), 2, 1, st) == 0
        assert eng.read_root_stats()["node_visits"].tolist() == [10, 10, 10]
        assert lib.tg_search_compact_live(None, None, None) == ERR_ARG and lib.tg_search_read_live_rank(eng.handle, None) == ERR_ARG
    finally:
        eng.close()
