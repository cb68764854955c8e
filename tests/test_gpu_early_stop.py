"""Early stops of CONSTANT_PLAYOUT searches on the device (csrc/search.hip: halt words, stop_rule_kernel,
tg_search_puct_chain_early) against the reference's recorded trees, the CPU oracle's searches and games
(tests/_early_stop_cases.py) and the host loop the option replaces.  Every comparison is exact.

The oracle cases run under the bit-exact host evaluators (StubNet, FlatNet, SpikyNet): an engine with a host evaluator
sends its mini-batches one by one and asks the device rule in between.  The chained path - the library queues the forward
passes itself - needs a DualNet, which has no bit-exact CPU counterpart: there the yardstick is the same search with the
option off, the host loop over read_node and TimeManager.is_move_decided."""
import numpy as np
import pytest

from tests import _early_stop_cases as cases
from tests._hard_trees import tree_digest
from tests.helpers import load_json, load_npz

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3


def _constant(visits):
    from tamago_amd.mcts.time_manager import TimeControl, TimeManager
    return TimeManager(TimeControl.CONSTANT_PLAYOUT, visits)


def _next_draw(state):
    g = np.random.RandomState()
    g.set_state(state)
    return float(g.random_sample())


# ---- the reference's own records ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [9, 13, 19])
def test_golden_constant_records_with_the_device_rule(size):
    """The CONSTANT_PLAYOUT records of tests/golden/trees_s{9,13,19}.json (19x19: A = 362, six passes per lane): tree digest,
    move, node count, mini-batches and stream position, with the option on and off."""
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.tree import MCTSTree
    from tests.test_gpu_search import check_root, product_replay
    brd = load_npz(f"board_s{size}.npz")
    recs = [r for r in load_json(f"trees_s{size}.json") if r["kind"] == "puct" and r["mode"] == "CONSTANT"]
    assert recs
    for rec in recs:
        for option in (True, False):
            board = product_replay(size, brd["g0_move"], brd["g0_color"], rec["ply"], rec["superko"])
            net = StubNet(salt=rec["seed"])
            tree = MCTSTree(net, tree_size=2048, batch_size=rec["batch"], cgos_mode=rec["cgos"], device_early_stop=option, poll_every=1)
            np.random.seed(rec["seed"])
            mv = tree.search_best_move(board, rec["color"], _constant(rec["visits"]), {})
            assert net.calls == rec["batches"], (rec["ply"], option)
            check_root(tree, mv, rec)
            assert float(np.random.random_sample()) == float.fromhex(rec["rng_after"])
            halted, stopped_at = tree._engine.read_halt()
            early = rec["node_visits"] < rec["visits"]
            assert bool(halted[0]) == (option and early) and int(stopped_at[0]) == (rec["node_visits"] if option and early else 0)


# ---- the oracle's cases: when the rule fires ------------------------------------------------------------------------------
def _product_case(case, poll_every, device_early_stop=True):
    from tamago_amd.mcts.tree import MCTSTree
    name, kind, seed, ply, color, visits, batch = case
    net = cases.make_evaluator(kind, seed)
    tree = MCTSTree(net, tree_size=visits + 16, batch_size=batch, device_early_stop=device_early_stop, poll_every=poll_every)
    np.random.seed(seed)
    mv = tree.search_best_move(cases.product_board(ply), color, _constant(visits), {})
    rng_after = float(np.random.random_sample())
    return tree, int(mv), rng_after, net


@pytest.mark.parametrize("poll_every", [1, 0], ids=["poll1", "poll_all"])
@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_the_rule_fires_where_the_oracle_stops(case, poll_every):
    """First test, last test, in between, never; remaining == cutoff and tied leaders go on; no test behind the partial last
    mini-batch.  poll_every 1: the mini-batches launched are the oracle's; 0 (never polled): all of them are launched, and
    the halted tree is what it was when it halted - digest, node count, stream."""
    want = cases.oracle_result(case[0])
    visits, batch = case[5], case[6]
    tree, mv, rng_after, net = _product_case(case, poll_every)
    root = tree.get_root()
    assert [int(v) for v in root.children_visits[:root.num_children]] == want["child_visits"]
    assert (mv, tree.num_nodes, int(root.node_visits)) == (want["move"], want["num_nodes"], want["node_visits"])
    assert tree_digest(tree, tree.num_nodes) == want["digest"]
    assert rng_after == want["rng_after"]
    halted, stopped_at = tree._engine.read_halt()
    assert (bool(halted[0]), int(stopped_at[0])) == (want["halted"], want["stopped_at"])
    every = [batch] * (visits // batch) + ([visits % batch] if visits % batch else [])
    assert net.calls[1:] == (want["batches"] if poll_every == 1 else every)


# ---- the chained path (a DualNet) against the host loop -------------------------------------------------------------------
def _dualnet(size):
    import torch
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    net = DualNet(torch.device("cuda:0"), size)
    net.load_state_dict(make_state_dict(size, 3, 1.3))
    return net


@pytest.mark.parametrize("size,visits,batch,ply", [(9, 120, 4, 30), (9, 100, 16, 0), (9, 40, 1, 20), (13, 60, 4, 100), (19, 60, 4, 100)])
def test_chained_early_stop_equals_the_host_loop(size, visits, batch, ply):
    """MCTSTree(device_early_stop=True) under a DualNet takes tg_search_puct_chain_early: the same tree, move, node count,
    mini-batches (poll_every 1) and numpy position as the host loop; with everything queued (poll_every 0) the same tree."""
    from tamago_amd.mcts.tree import MCTSTree
    net = _dualnet(size)
    runs = {}
    for key, kwargs in (("off", {}), ("on", dict(device_early_stop=True, poll_every=1)), ("all", dict(device_early_stop=True, poll_every=0))):
        tree = MCTSTree(net, tree_size=visits + 16, batch_size=batch, **kwargs)
        np.random.seed(40 + ply)
        mv = tree.search_best_move(cases.product_board(ply, size), 1, _constant(visits), {})
        assert tree._engine.can_chain(1)
        root = tree.get_root()
        runs[key] = (int(mv), tree.num_nodes, int(root.node_visits), tree_digest(tree, tree.num_nodes), float(np.random.random_sample()),
                     list(tree._engine.evaluator.batches), tuple(int(x[0]) for x in tree._engine.read_halt()))
    off, on, queued = runs["off"], runs["on"], runs["all"]
    assert on[:6] == off[:6]
    assert queued[:5] == off[:5] and sum(queued[5]) == 1 + visits
    early = off[2] < visits
    assert on[6] == queued[6] == ((1, off[2]) if early else (0, 0)) and off[6] == (0, 0)


def test_misuse_is_refused():
    """NULL totals, poll_every < 1, a total < 1: TG_ERR_ARG; an unexpanded root: TG_ERR_STATE; nothing is launched."""
    import torch
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import DeviceEvaluator, SearchEngine
    net = _dualnet(9)
    eng = SearchEngine(9, 2, 64, 4, DeviceEvaluator(net))
    try:
        lib = eng.lib
        leaves = np.array([4, 4, 2], dtype=np.int32)
        totals = np.array([1000, 1000], dtype=np.int32)
        policy = torch.empty((8, 82), dtype=torch.float32, device=eng.device)
        value = torch.empty((8, 3), dtype=torch.float32, device=eng.device)

        def chain(tot=totals, poll=1, n=3):
            return lib.tg_search_puct_chain_early(eng.handle, net.handle, leaves.ctypes.data, n, None if tot is None else tot.ctypes.data,
                                                  poll, 1, eng.planes.data_ptr(), policy.data_ptr(), value.data_ptr(), eng._stream(), None)
        for t in range(2):
            eng.set_root(t, GoBoard(9), 1, np.random.RandomState(5 + t).get_state())
        assert chain() == ERR_STATE                                      # staged roots, never expanded
        eng.root_eval(False)
        assert chain(tot=None) == ERR_ARG and chain(poll=0) == ERR_ARG and chain(poll=-3) == ERR_ARG and chain(n=0) == ERR_ARG
        assert chain(tot=np.array([10, 0], dtype=np.int32)) == ERR_ARG
        assert lib.tg_search_stop_rule(eng.handle, None, None, eng._stream()) == ERR_ARG
        assert lib.tg_search_stop_rule(eng.handle, np.array([0, 5], dtype=np.int32).ctypes.data, None, eng._stream()) == ERR_ARG
        assert lib.tg_search_set_halt(eng.handle, None, eng._stream()) == ERR_ARG
        assert lib.tg_search_set_halt(None, None, None) == ERR_ARG and lib.tg_search_read_halt(None, None, None) == ERR_ARG
        assert eng.num_nodes().tolist() == [1, 1] and not eng.read_halt()[0].any()
        assert chain() == 0                                              # ... and the same call with good arguments runs
        eng._collect_rng()
        assert eng.num_nodes().tolist() == [11, 11]
        eng.set_root(0, GoBoard(9), 1)
        assert chain() == ERR_STATE                                      # a root was replaced since
    finally:
        eng.close()


# ---- lock-step ------------------------------------------------------------------------------------------------------------
def _lockstep_engine(evaluator, plies, seed, visits, batch, size=9):
    from tamago_amd.mcts.engine import SearchEngine
    eng = SearchEngine(size, len(plies), visits + 16, batch, evaluator)
    for t, ply in enumerate(plies):
        eng.set_root(t, cases.product_board(ply, size), 1, np.random.RandomState(seed).get_state())
    eng.root_eval(False)
    return eng


def _tree_state(eng, t):
    n = int(eng.num_nodes()[t])

    class View:
        node = [eng.read_node(t, i) for i in range(n)]
    root = View.node[0]
    return (n, int(root.node_visits), [int(v) for v in root.children_visits[:root.num_children]], tree_digest(View, n),
            _next_draw(eng.streams[t].final_state()))


@pytest.mark.parametrize("poll_every", [1, 0], ids=["poll1", "poll_all"])
def test_lockstep_trees_equal_their_oracle_searches(poll_every):
    """Five positions in one engine, three that never halt, one that halts at its last test and one after 4 of 8 mini-batches:
    every tree - pool digest, root, node count, stream - is the oracle's single search, whatever shares the launches and
    however many launches follow its halt."""
    from tamago_amd.mcts.engine import HostEvaluator
    import torch
    kind, seed, visits, batch, plies = cases.LOCKSTEP
    want = [cases.oracle_result(c[0]) for c in cases.lockstep_cases()]
    eng = _lockstep_engine(HostEvaluator(cases.make_evaluator(kind, seed), torch.device("cuda", 0)), plies, seed, visits, batch)
    try:
        run = eng.puct_chain([batch] * (visits // batch) + [visits % batch], early_total=visits, poll_every=poll_every)
        assert run == 8                                              # (three trees never halt)
        for t, w in enumerate(want):
            n, node_visits, child_visits, digest, draw = _tree_state(eng, t)
            assert (n, node_visits, child_visits, digest, draw) == (w["num_nodes"], w["node_visits"], w["child_visits"], w["digest"], w["rng_after"]), t
        halted, stopped_at = eng.read_halt()
        assert halted.tolist() == [w["halted"] for w in want] and stopped_at.tolist() == [w["stopped_at"] for w in want]
        assert stopped_at.tolist() == [0, 28, 0, 0, 16]
    finally:
        eng.close()


def test_lockstep_chain_equals_single_trees_under_a_dualnet():
    """The chained call on five trees against the same call on each tree alone, poll_every 1 and never: root statistics,
    node counts, streams, halt words; the call returns once the last live tree has halted."""
    from tamago_amd.mcts.engine import DeviceEvaluator
    net = _dualnet(9)
    plies, visits, batch = (0, 4, 10, 20, 30), 120, 4
    batches = [batch] * (visits // batch)

    def run(which, poll_every):
        eng = _lockstep_engine(DeviceEvaluator(net), which, 77, visits, batch)
        try:
            assert eng.can_chain(visits)
            ran = eng.puct_chain(batches, early_total=visits, poll_every=poll_every)
            halted, stopped_at = eng.read_halt()
            return ran, [_tree_state(eng, t) + (bool(halted[t]), int(stopped_at[t])) for t in range(len(which))]
        finally:
            eng.close()
    alone = [run((ply,), 1) for ply in plies]
    for poll_every in (1, 0):
        ran, together = run(plies, poll_every)
        assert together == [a[1][0] for a in alone]
        assert ran == (max(a[0] for a in alone) if poll_every == 1 else len(batches))
    assert net.range_fallbacks() == 0


def test_host_set_halt_words():
    """A tree halted from the host is untouched by three further mini-batches - pool digest, cursor, no leaf queued - while its
    neighbours are what they are without it; root_eval clears the word; the Gumbel selection ignores it."""
    from tamago_amd.mcts.engine import DeviceEvaluator
    net = _dualnet(9)

    def run(halt):
        eng = _lockstep_engine(DeviceEvaluator(net), (0, 10, 20), 9, 64, 4)
        try:
            eng.puct_batch(4)
            before = _tree_state(eng, 1)
            if halt:
                eng.set_halt([0, 1, 0])
                assert eng.read_halt()[0].tolist() == [False, True, False] and eng.read_halt()[1].tolist() == [0, 0, 0]
                eng.set_halt([0, 0, 0])                              # (zero entries leave a word alone)
                assert eng.read_halt()[0].tolist() == [False, True, False]
            for _ in range(2):
                eng.puct_batch(4)
            eng.puct_select(3)
            queued = [len(eng.read_queue(t).node_index) for t in range(3)]
            eng.puct_flush()
            states = [_tree_state(eng, t) for t in range(3)]
            if halt:
                assert queued == [3, 0, 3] and states[1] == before
                # the Gumbel selection is not a PUCT search: it runs the halted tree like the others
                visited = eng.read_root_stats()["node_visits"].copy()
                eng.gumbel_phase([2, 2, 2], [1, 1, 1])
                assert eng.read_halt()[0].tolist() == [False, True, False]
                assert (eng.read_root_stats()["node_visits"] - visited).tolist() == [2, 2, 2] and int(visited[1]) == before[1]
                eng.root_eval(False)                                 # the root expansion clears every word
                assert not eng.read_halt()[0].any()
                eng.puct_batch(4)
                assert eng.read_root_stats()["node_visits"].tolist() == [4, 4, 4]
            else:
                assert queued == [3, 3, 3]
            return states
        finally:
            eng.close()
    with_halt, without = run(True), run(False)
    assert with_halt[0] == without[0] and with_halt[2] == without[2] and with_halt[1] != without[1]
    assert net.range_fallbacks() == 0


def test_clears_reset_stopped_at_and_touch_only_the_trees_they_reset():
    """A tree the rule halted (stopped_at = its visits) and the host halts after the next root expansion reads stopped_at 0,
    not the earlier search's figure.  A reroot of one tree, and a staged root of one tree going up, clear that tree's word
    and leave a neighbour halted; the root expansion clears every word."""
    import torch
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import HostEvaluator
    kind, seed, visits, batch, plies = cases.LOCKSTEP
    eng = _lockstep_engine(HostEvaluator(cases.make_evaluator(kind, seed), torch.device("cuda", 0)), plies[3:], seed, visits, batch)
    try:
        eng.puct_chain([batch] * (visits // batch) + [visits % batch], early_total=visits, poll_every=1)
        assert [a.tolist() for a in eng.read_halt()] == [[False, True], [0, 16]]          # (plies 20 and 30 of the oracle's five)
        eng.root_eval(False)
        assert [a.tolist() for a in eng.read_halt()] == [[False, False], [0, 0]]
        eng.set_halt([1, 1])
        assert [a.tolist() for a in eng.read_halt()] == [[True, True], [0, 0]]
        # the same searches again: the rule halts tree 1 again, the host adds tree 0 - the rule's figure stays with tree 1 alone
        for t in range(2):
            eng.set_stream(t, np.random.RandomState(seed).get_state())
        eng.root_eval(False)
        eng.puct_chain([batch] * (visits // batch) + [visits % batch], early_total=visits, poll_every=0)
        eng.set_halt([1, 1])
        assert [a.tolist() for a in eng.read_halt()] == [[True, True], [0, 16]]
        eng.reroot([-1, 1])                                            # tree 1 restarts below its root: its word and figure go
        assert [a.tolist() for a in eng.read_halt()] == [[True, False], [0, 0]]
        eng.set_halt([0, 1])
        eng.set_root(1, GoBoard(9), 1)
        eng.play([-1, -1])                                             # (plays nothing; the staged root of tree 1 goes up)
        assert [a.tolist() for a in eng.read_halt()] == [[True, False], [0, 0]]
    finally:
        eng.close()


# ---- batch analysis -------------------------------------------------------------------------------------------------------
def test_batch_analysis_in_constant_mode_equals_the_single_tree_path():
    """Four positions, one engine: lz and cgos bytes, best move and visits of MCTSTree.search_best_move under
    TimeManager(CONSTANT_PLAYOUT) with the option off."""
    from oracle.stubnet import StubNet
    from tamago_amd.mcts.analysis import analyze_positions
    from tamago_amd.mcts.time_manager import TimeControl
    from tamago_amd.mcts.tree import MCTSTree
    kind, seed, visits, batch, plies = cases.LOCKSTEP
    plies = plies[1:]
    positions = [(cases.product_board(ply), 1) for ply in plies]
    seeds = [seed] * len(plies)
    res = analyze_positions(StubNet(seed), positions, visits, batch_size=batch, seeds=seeds, mode=TimeControl.CONSTANT_PLAYOUT)
    strict = analyze_positions(StubNet(seed), positions, visits, batch_size=batch, seeds=seeds)
    for k, (board, color) in enumerate(positions):
        tree = MCTSTree(StubNet(seed), tree_size=visits + 16, batch_size=batch)
        np.random.seed(seeds[k])
        best = tree.search_best_move(board, color, _constant(visits), {})
        root = tree.get_root()
        assert res[k].lz() == root.get_analysis(board, "lz", tree.get_pv_lists)
        assert res[k].cgos() == root.get_analysis(board, "cgos", tree.get_pv_lists)
        assert (res[k].best_move, res[k].visits) == (int(best), int(root.node_visits))
        assert strict[k].visits == visits
    assert [r.visits for r in res] == [28, 30, 30, 16]


# ---- PUCT matches ---------------------------------------------------------------------------------------------------------
MATCH_SEEDS = (3, 4, 6, 8)
MATCH_SEARCH = ((30, 4), (20, 1))


ONE_CHILD_PLIES = {(False, False): {4: [90, 92, 96], 8: [102, 104, 105]}, (True, False): {3: [98, 99]}}       # by seed, of the oracle's games


def _match(strict, tmp_path, boards, poll_every=None):
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    from tests._match_cases import make_net
    from tests._puct_match_cases import S301, S302
    a = EngineSetup(make_net(S301), *MATCH_SEARCH[0], strict=strict[0])
    b = EngineSetup(make_net(S302), *MATCH_SEARCH[1], strict=strict[1])
    return puct_match(a, b, len(MATCH_SEEDS), boards=boards, seeds=list(MATCH_SEEDS), save_dir=str(tmp_path), poll_every=poll_every)


@pytest.mark.parametrize("strict,boards,poll_every", [((False, False), 4, 1), ((False, False), 3, None), ((True, False), 4, 0)],
                         ids=["both", "refill", "mixed"])
def test_matches_with_setups_that_are_not_strict_equal_the_oracle_games(strict, boards, poll_every, tmp_path):
    """Four games, 30 visits x 4 against 20 x 1, byte for byte the oracle's loop under TimeManager(CONSTANT_PLAYOUT) for the
    colours that are not strict: records, results, final streams - with one-child roots inside the games (halted: no draw, no
    put-back), games that end while others run (their slots halted) and, mixed, black strict and white not; polled after
    every mini-batch, at the default interval and never."""
    from tests._puct_match_cases import S301, S302
    from tests.test_gpu_puct_match import _check_games, _check_tally
    games = [cases.oracle_early_game(seed, S301, S302, *MATCH_SEARCH, strict) for seed in MATCH_SEEDS]
    plies = {seed: cases.one_child_plies_of(text) for seed, (text, _, _) in zip(MATCH_SEEDS, games)}
    assert {seed: p for seed, p in plies.items() if p} == ONE_CHILD_PLIES[strict]          # one-child roots followed by searched moves
    lengths = [end[0] for _, end, _ in games]
    assert max(lengths) - min(lengths) >= 15                          # a game ends while the others run on
    out = _match(strict, tmp_path, boards, poll_every)
    _check_tally(out, _check_games(out, games, tmp_path))
    assert out["one_child_roots"] == sum(len(p) for p in plies.values())
    assert out["range_fallbacks"] == 0
    assert 0 < out["leaf_evals"] < out["forward_positions"]                   # (idle slots are still part of a launch)


def test_dualnet_match_with_early_stops_does_not_depend_on_the_boards(tmp_path):
    """DualNets take the chained call: the games on 4 boards are the games on 1 board, and no launch with idle slots falls
    back from the f16 kernels (range fallbacks 0)."""
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    net = _dualnet(9)
    a, b = EngineSetup(net, 30, 4, strict=False), EngineSetup(net, 20, 1, strict=False)
    outs = []
    for boards in (4, 1):
        d = tmp_path / str(boards)
        out = puct_match(a, b, 3, boards=boards, seeds=[11, 12, 13], save_dir=str(d))
        outs.append([open(d / f"{i}.sgf").read() for i in range(3)] + [[(r["winner"], r["moves"], r["stream"][1], r["stream"][0].tobytes()) for r in out["results"]]])
        assert out["range_fallbacks"] == 0
    assert outs[0] == outs[1]
