"""The code paths bench.py TIMES, at BASELINE.json's full sizes, against the CPU oracle.

1. cfg-3 / cfg-4-shard self-play through ``tg_selfplay_play_move`` (DualNet evaluator: ONE library
   call per lock-step move, one random window for all phases of a move) - 16 and 64 boards x 400
   simulations, games to completion:
   * byte-identical SGF files to the phase-by-phase host-driven path on the same network;
   * every mini-batch the one-call path evaluated is tapped (tg_selfplay_set_observer) and the
     slices of four boards are replayed, in order, into the CPU oracle's Gumbel tree
     (mcts/tree.py:318-422, selfplay/worker.py:46-90 restated in oracle/): the oracle must ask for
     bit-identical leaf planes in the same order, its own CPU network must agree with the recorded
     GPU outputs within 1e-4, and after every move the root's actions, visit vector, value sums
     and the move played must equal what the library decided.
2. ``select_puct_pipe_kernel`` (the selector above 256 trees, i.e. of the 2 048-tree headline):
   a 512-tree lock-step PUCT search on the DeviceEvaluator path, every 16th tree replayed into its
   own oracle tree.
"""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VISITS = 400
TOL = 1e-4          # north_star tolerance on policy / value outputs (fp32)


class HostOnly:
    """The same network, not recognisable as a DualNet: selfplay_shard then drives every phase
    from Python through the host evaluator API (worker.py's phase-by-phase branch)."""

    def __init__(self, net):
        self.net = net

    def inference(self, planes):
        return self.net.inference(planes)

    def inference_with_policy_logits(self, planes):
        return self.net.inference_with_policy_logits(planes)


class Tap:
    """Observer of tg_selfplay_play_move: keeps, for the watched slots only, the leaf planes (int8:
    plane values are -1 / 0 / 1), logits and value rows of every mini-batch and the root statistics
    behind every decided move."""

    def __init__(self, watch, size):
        self.watch = list(watch)
        self.P = size * size
        self.A = self.P + 1
        self.batches = {t: [] for t in self.watch}       # per slot: (planes i8, policy, value)
        self.moves = {t: [] for t in self.watch}         # per slot: dict per decided move
        self.closed = set()
        self.errors = []
        self.phase_sizes = []

    def __call__(self, engine, ev):
        try:
            self._on(engine, ev)
        except BaseException as exc:      # an exception cannot cross the C frame: keep it for the test
            self.errors.append(repr(exc))

    def _on(self, engine, ev):
        T = ev.trees
        if ev.kind == 0:
            torch.cuda.synchronize()
            policy, value = engine.sp_outputs
            if ev.phase < 0:
                offs = np.arange(T + 1)
            else:
                nc = np.ctypeslib.as_array(ev.num_considered, shape=(T,)).astype(np.int64)
                mc = np.ctypeslib.as_array(ev.max_count, shape=(T,)).astype(np.int64)
                offs = np.concatenate([[0], np.cumsum(nc * mc)])
            assert offs[-1] == ev.positions
            self.phase_sizes.append(int(ev.positions))
            for t in self.watch:
                lo, hi = int(offs[t]), int(offs[t + 1])
                if t in self.closed or hi == lo:
                    continue
                pl = engine.planes[lo:hi].cpu()
                assert float((pl - pl.round()).abs().max()) == 0.0 and float(pl.abs().max()) <= 1.0
                self.batches[t].append((pl.to(torch.int8), policy[lo:hi].cpu().clone(), value[lo:hi].cpu().clone()))
        else:
            A = self.A
            nch = np.ctypeslib.as_array(ev.num_children, shape=(T,))
            act = np.ctypeslib.as_array(ev.action, shape=(T, A))
            vis = np.ctypeslib.as_array(ev.children_visits, shape=(T, A))
            vsum = np.ctypeslib.as_array(ev.children_value_sum, shape=(T, A))
            mv = np.ctypeslib.as_array(ev.moves, shape=(T,))
            fin = np.ctypeslib.as_array(ev.finished, shape=(T,))
            for t in self.watch:
                if t in self.closed:
                    continue
                n = int(nch[t])
                self.moves[t].append(dict(n=n, action=act[t, :n].copy(), visits=vis[t, :n].copy(),
                                          vsum=vsum[t, :n].copy(), move=int(mv[t]), finished=int(fin[t])))
                if fin[t]:
                    self.closed.add(t)


class SliceNet:
    """Oracle-side network of ONE board: hands out that board's recorded GPU outputs mini-batch by
    mini-batch, checks the oracle's planes against the recorded ones and the CPU network against
    the GPU outputs."""

    def __init__(self, batches, cpu_net):
        self.batches = batches
        self.cpu_net = cpu_net
        self.i = 0
        self.max_err = 0.0

    def inference_with_policy_logits(self, planes):
        rec_planes, policy, value = self.batches[self.i]
        self.i += 1
        assert planes.shape[0] == rec_planes.shape[0], f"mini-batch {self.i - 1}: {planes.shape[0]} leaves vs {rec_planes.shape[0]} recorded"
        assert torch.equal(planes, rec_planes.to(torch.float32)), f"leaf planes differ in mini-batch {self.i - 1}"
        ref_p, ref_v = self.cpu_net.inference_with_policy_logits(planes)
        self.max_err = max(self.max_err, float(((ref_p - policy).abs() / (1.0 + ref_p.abs())).max()),
                           float((ref_v - value).abs().max()))
        return policy, value

    def inference(self, planes):
        raise AssertionError("Gumbel search evaluates logits only (tree.py:283)")


def _sgf_moves(text):
    return re.findall(r";([BW])\[([a-z]{2})\]", text)


def _replay_game(tap, slot, seed, never_resign, state_dict, sgf_text, max_moves=None):
    """selfplay/worker.py:46-90 on the oracle with the recorded outputs of `slot` (the whole game, or its
    first `max_moves` moves: the oracle runs at ~0.3 s per move)."""
    from oracle.board import GoBoard as OBoard, BLACK, PASS, RESIGN
    from oracle.net import OracleNet
    from oracle.tree import MCTSTree as OTree, TimeManager as OTM, TimeControl as OTC
    net = SliceNet(tap.batches[slot], OracleNet(state_dict))
    otree = OTree(net, 9, tree_size=max(160, VISITS + 8))
    tm = OTM(OTC.CONSTANT_PLAYOUT, VISITS)
    oboard = OBoard(9, 7.0, True)
    color = BLACK
    saved = np.random.get_state()
    np.random.set_state(np.random.RandomState(seed).get_state())
    try:
        for k, rec in enumerate(tap.moves[slot]):
            if max_moves is not None and k >= max_moves:
                return k, net.max_err
            omv = otree.generate_move_with_sequential_halving(oboard, color, tm, never_resign)
            root = otree.get_root()
            n = root.num_children
            assert n == rec["n"], (slot, k)
            assert list(root.action[:n]) == list(rec["action"]), (slot, k)
            assert np.array_equal(root.children_visits[:n], rec["visits"]), (slot, k)
            assert np.array_equal(root.children_value_sum[:n], rec["vsum"]), (slot, k)
            if rec["finished"]:
                assert k == len(tap.moves[slot]) - 1
                if omv != RESIGN:                      # two passes / move limit: the SGF holds the move
                    assert omv == PASS or len(_sgf_moves(sgf_text)) == 2 * 81
                else:
                    assert "+R]" in sgf_text
                break
            assert omv == rec["move"], (slot, k, omv, rec["move"])
            oboard.put_stone(omv, color)
            color = 3 - color
    finally:
        np.random.set_state(saved)
    assert net.i == len(net.batches), "the oracle evaluated fewer mini-batches than the library"
    assert tap.moves[slot][-1]["finished"] == 1
    return len(tap.moves[slot]), net.max_err


def _fast_vs_slow(tmp_path, boards, first_index, watch, replay_moves_at_least, caps):
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    from tamago_amd.selfplay.worker import selfplay_shard
    sd = make_state_dict(9, 23, 1.5)                      # seeded synthetic weights, non-trivial BN statistics
    net = DualNet(torch.device("cuda:0"), 9)
    net.load_state_dict(sd)
    idx = list(range(first_index, first_index + boards))
    flags = [i % 5 != 0 for i in idx]                     # most games never resign (worker.py:53 draws 1 in 10)
    fast, slow = tmp_path / "fast", tmp_path / "slow"
    fast.mkdir(), slow.mkdir()
    tap = Tap(watch, 9)
    a = selfplay_shard(str(fast), net, idx, 9, VISITS, boards=boards, never_resign_flags=flags, observer=tap)
    assert not tap.errors, tap.errors[:3]
    b = selfplay_shard(str(slow), HostOnly(net), idx, 9, VISITS, boards=boards, never_resign_flags=flags)
    assert a == b and a["games"] == boards
    assert a["leaf_evals"] == a["moves"] * (VISITS + 1)
    texts = {}
    for i in idx:
        texts[i] = open(fast / f"{i}.sgf").read()
        assert texts[i] == open(slow / f"{i}.sgf").read(), i
    # the first lock-step move: every board has the full 1 + 96 + 96 + 100 + 108 schedule
    assert tap.phase_sizes[:5] == [boards, 96 * boards, 96 * boards, 100 * boards, 108 * boards]
    total_moves = 0
    worst = 0.0
    for t, cap in zip(watch, caps):
        n_moves, err = _replay_game(tap, t, idx[t], flags[t], sd, texts[idx[t]], cap)
        total_moves += n_moves
        worst = max(worst, err)
    assert worst < TOL, worst
    assert total_moves >= replay_moves_at_least
    return a


def test_selfplay_move_schemes_play_the_same_games(tmp_path, monkeypatch):
    """tg_selfplay_play_move's schemes - move decided on the host with three round trips (TG_SP_CHAIN=0), decided on the
    device with the next root chained behind it (default), the same with the boards of a lock-step move in 2 / 3 / 4
    staggered sub-groups on their own streams (default below 29 boards) - and the phase-by-phase host path: same SGF files
    byte for byte, same counters.  (The chained scheme itself is replayed against the oracle by the two tests below: the
    observer they attach keeps the boards in one group.)"""
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    from tamago_amd.selfplay.worker import selfplay_shard
    net = DualNet(torch.device("cuda:0"), 9)
    net.load_state_dict(make_state_dict(9, 23, 1.5))
    idx = list(range(301, 301 + 44))
    flags = [i % 5 != 0 for i in idx]
    results = {}
    # round 6: lanes - the boards as independent engines on their own streams, driven by one host thread through
    # tg_selfplay_move_begin / _end, each lane on a move of its own (an option; one lock-step group is the default)
    for name, chain, sub, lanes in (("host decision", "0", None, 1), ("chained", "1", "1", 1), ("2 sub-groups", "1", "2", 1),
                                    ("default", None, None, 0), ("4 sub-groups", "1", "4", 1), ("3 lanes", None, None, 3),
                                    ("8 lanes of one group", "1", "1", 8)):
        for key, val in (("TG_SP_CHAIN", chain), ("TG_SP_SUBGROUPS", sub)):
            if val is None:
                monkeypatch.delenv(key, raising=False)
            else:
                monkeypatch.setenv(key, val)
        d = tmp_path / name.replace(" ", "_")
        d.mkdir()
        stats = selfplay_shard(str(d), net, idx, 9, VISITS, boards=16, never_resign_flags=flags, lanes=lanes)
        results[name] = (stats, [open(d / f"{i}.sgf").read() for i in idx])
    monkeypatch.delenv("TG_SP_CHAIN", raising=False)
    monkeypatch.delenv("TG_SP_SUBGROUPS", raising=False)
    d = tmp_path / "phases"
    d.mkdir()
    stats = selfplay_shard(str(d), HostOnly(net), idx[:16], 9, VISITS, boards=16, never_resign_flags=flags[:16])
    ref = results["host decision"]
    assert ref[0]["games"] == len(idx) and ref[0]["leaf_evals"] == ref[0]["moves"] * (VISITS + 1)
    for name, got in results.items():
        assert got[0] == ref[0], name
        assert got[1] == ref[1], name
    assert [open(d / f"{i}.sgf").read() for i in idx[:16]] == ref[1][:16]
    # 40 boards at a time: two halves with the forward launches kept off 32 CUs (the default from 29 boards on) - the same
    # games once more, whatever the grouping
    d = tmp_path / "forty"
    d.mkdir()
    stats = selfplay_shard(str(d), net, idx, 9, VISITS, boards=40, never_resign_flags=flags)
    assert stats == ref[0]
    assert [open(d / f"{i}.sgf").read() for i in idx] == ref[1]


class Ledger:
    """Observer that keeps the host-side arguments of every event only (no device read): the positions of every forward
    pass, per board the phase sizes of every move it took part in, and per board the moves of the first game in its slot."""

    def __init__(self, boards):
        self.T = boards
        self.errors = []
        self.phase_positions = 0                          # kind 0, phase >= 0
        self.root_positions = []                          # kind 0, phase -1: one entry per event
        self.decisions = 0                                # (board, move) pairs decided
        self.open_phases = [[] for _ in range(boards)]    # phase sizes since the board's last decided move
        self.move_shapes = [[] for _ in range(boards)]    # per board: one tuple of phase sizes per decided move
        self.first_game = [[] for _ in range(boards)]     # per board: moves up to the first finished game
        self.closed = [False] * boards

    def __call__(self, engine, ev):
        try:
            self._on(ev)
        except BaseException as exc:      # an exception cannot cross the C frame: keep it for the test
            self.errors.append(repr(exc))

    def _on(self, ev):
        T = ev.trees
        assert T == self.T
        if ev.kind == 0 and ev.phase < 0:
            self.root_positions.append(int(ev.positions))
        elif ev.kind == 0:
            nc = np.ctypeslib.as_array(ev.num_considered, shape=(T,)).astype(np.int64)
            mc = np.ctypeslib.as_array(ev.max_count, shape=(T,)).astype(np.int64)
            assert int((nc * mc).sum()) == ev.positions
            self.phase_positions += int(ev.positions)
            for t in range(T):
                if nc[t] * mc[t] > 0:
                    self.open_phases[t].append(int(nc[t] * mc[t]))
        else:
            mv = np.ctypeslib.as_array(ev.moves, shape=(T,))
            fin = np.ctypeslib.as_array(ev.finished, shape=(T,))
            for t in range(T):
                took_part = mv[t] >= 0 or fin[t] != 0
                assert took_part == bool(self.open_phases[t]), (t, int(mv[t]), int(fin[t]), self.open_phases[t])
                if not took_part:
                    continue
                self.decisions += 1
                self.move_shapes[t].append(tuple(self.open_phases[t]))
                self.open_phases[t] = []
                if not self.closed[t]:
                    if mv[t] >= 0:
                        self.first_game[t].append(int(mv[t]))
                    self.closed[t] = bool(fin[t])


def test_observer_sees_the_same_moves_under_the_round_trip_and_the_chained_scheme(tmp_path, monkeypatch):
    """The observer of tg_selfplay_play_move under the round-trip scheme (TG_SP_CHAIN=0), which no other test attaches there:
    4 boards, 6 games (slots are refilled, then parked), 16 visits, resigning and never-resigning games mixed.  (a) round trip
    with an observer, (b) round trip without, (c) chained with an observer: same SGF bytes and counters; in (a) and (c) the
    events account for every position the network was given and for every move of the first game in each slot, and a board's
    moves have the same phase sizes under both schemes.

    Positions: stats["forward_positions"] counts, per move, the phases' positions and ONE root evaluation per board that takes
    part in the move, while a root evaluation is launched - and reported, event.positions == boards - for the whole group,
    parked and just-started slots included (the chained scheme's first call evaluates roots only).  So the events are held to
    the counter as: phase events' positions + boards that took part in a decided move == forward_positions, and every root
    event reports the whole group.  (Here: forward_positions 9 843 = 9 264 in phase events + 579 decided moves under both
    schemes; the root events add up to 190 x 4 in (a) and 192 x 4 in (c), so a plain sum over all kind-0 events gives
    10 024 / 10 032 and cannot equal the counter under either scheme.)"""
    from collections import Counter
    from oracle.net import make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    from tamago_amd.selfplay.worker import selfplay_shard
    S, boards, visits = 9, 4, 16
    net = DualNet(torch.device("cuda:0"), S)
    net.load_state_dict(make_state_dict(S, 23, 1.5))
    idx = list(range(401, 407))
    flags = [i % 2 == 0 for i in idx]
    runs = {}
    try:
        for name, chain, watched in (("a", "0", True), ("b", "0", False), ("c", None, True)):
            if chain is None:
                monkeypatch.delenv("TG_SP_CHAIN", raising=False)
            else:
                monkeypatch.setenv("TG_SP_CHAIN", chain)
            d = tmp_path / name
            d.mkdir()
            ledger = Ledger(boards) if watched else None
            stats = selfplay_shard(str(d), net, idx, S, visits, boards=boards, never_resign_flags=flags, observer=ledger)
            runs[name] = (stats, [open(d / f"{i}.sgf").read() for i in idx], ledger)
    finally:
        monkeypatch.delenv("TG_SP_CHAIN", raising=False)
    stats, texts, _ = runs["a"]
    assert stats["games"] == len(idx) and stats["leaf_evals"] == stats["moves"] * (visits + 1)
    for name in ("b", "c"):
        assert runs[name][0] == stats, name
        assert runs[name][1] == texts, name
    W = S + 2
    for name in ("a", "c"):
        ledger = runs[name][2]
        assert not ledger.errors, (name, ledger.errors[:3])
        print(f"[{name}] forward_positions {stats['forward_positions']}, phase events {ledger.phase_positions}, "
              f"root events {len(ledger.root_positions)} x {boards}, decisions {ledger.decisions}, moves {stats['moves']}")
        assert ledger.root_positions and set(ledger.root_positions) == {boards}, name
        assert ledger.decisions == stats["moves"], name
        assert ledger.phase_positions + ledger.decisions == stats["forward_positions"], name
        for t in range(boards):                       # slot t starts with game idx[t]
            assert ledger.closed[t], (name, t)
            sgf = [0 if xy == "tt" else (ord(xy[1]) - 96) * W + (ord(xy[0]) - 96) for _, xy in _sgf_moves(texts[t])]
            assert [c for c, _ in _sgf_moves(texts[t])] == ["B", "W"] * (len(sgf) // 2) + ["B"] * (len(sgf) % 2)
            if "+R]" not in texts[t]:                   # two passes / move limit: the SGF holds the last move, the event -1
                assert sgf[-1] == 0 or len(sgf) == 2 * S * S, (name, t)
                sgf = sgf[:-1]
            assert ledger.first_game[t] == sgf, (name, t)
    for t in range(boards):
        assert Counter(runs["a"][2].move_shapes[t]) == Counter(runs["c"][2].move_shapes[t]), t


def test_cfg3_one_call_path_16_boards_400_sims_vs_phase_path_and_oracle(tmp_path):
    # two games replayed move for move to their end, two for their first 50 moves
    _fast_vs_slow(tmp_path, 16, 101, watch=(0, 5, 10, 15), replay_moves_at_least=160, caps=(None, 50, None, 50))


def test_cfg4_shard_one_call_path_64_boards_400_sims_vs_phase_path_and_oracle(tmp_path):
    _fast_vs_slow(tmp_path, 64, 201, watch=(1, 22, 43, 63), replay_moves_at_least=160, caps=(40, 40, 40, 40))


def test_512_tree_puct_pipe_kernel_device_evaluator_replay():
    """512 trees > 256: tg_search_select_puct launches select_puct_pipe_kernel (1 selector + 2 worker
    waves per tree), the selector of bench.py's 2 048-tree headline.  Every 16th tree's slice of every
    recorded mini-batch is replayed into its own CPU oracle tree: identical leaf planes in order,
    identical visit counts / value sums / policies / node counts."""
    from oracle.board import GoBoard as OBoard
    from oracle.net import OracleNet, make_state_dict
    from oracle.tree import MCTSTree as OTree, TimeManager as OTM, TimeControl as OTC
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import SearchEngine, DeviceEvaluator
    from tamago_amd.nn.network.dual_net import DualNet
    from tests.helpers import load_npz
    from tests.test_gpu_end_to_end import Recorder

    for knob in ("TG_SELECT_SERIAL", "TG_SELECT_MPIPE_TREES", "TG_MPIPE_PROF"):
        assert not os.environ.get(knob), "the kernel choice must be the library's default"
    size, T, K, visits = 9, 512, 64, 200
    sd = make_state_dict(size, 7, 1.5)
    net = DualNet(torch.device("cuda:0"), size)
    net.load_state_dict(sd)
    rec = Recorder(DeviceEvaluator(net))
    engine = SearchEngine(size, T, visits + 16, K, rec)
    brd = load_npz("board_s9.npz")
    roots = []
    for t in range(T):
        game, plies = t % 4, 2 + (t * 5) % 40
        board, oboard = GoBoard(size, 7.0, False), OBoard(size, 7.0, False)
        mv, col = brd[f"g{game}_move"], brd[f"g{game}_color"]
        plies = min(plies, len(mv) - 1)
        for m, c in zip(mv[:plies], col[:plies]):
            board.put_stone(int(m), int(c))
            oboard.put_stone(int(m), int(c))
        color = 3 - int(col[plies - 1])
        engine.set_root(t, board, color, np.random.RandomState(5000 + t).get_state())
        roots.append((oboard, color))
    engine.root_eval(False)
    done = 0
    while done < visits:
        k = min(K, visits - done)
        engine.puct_batch(k)
        done += k
    stats = engine.read_root_stats()
    nodes = engine.num_nodes()
    assert [b[0].shape[0] for b in rec.log] == [T, T * 64, T * 64, T * 64, T * 8]
    cpu = OracleNet(sd)
    for planes, policy, value, _ in rec.log[:2]:
        ref_p, ref_v = cpu.inference(planes[:4096])
        assert float((ref_p - policy[:4096]).abs().max()) < TOL and float((ref_v - value[:4096]).abs().max()) < TOL

    class Slice:
        def __init__(self, t):
            self.t, self.i = t, 0

        def inference(self, planes):
            rp, pol, val, _ = rec.log[self.i]
            per = rp.shape[0] // T
            self.i += 1
            lo = self.t * per
            assert torch.equal(planes, rp[lo:lo + planes.shape[0]]), (self.t, self.i - 1)
            return pol[lo:lo + planes.shape[0]], val[lo:lo + planes.shape[0]]

    for t in range(0, T, 16):
        oboard, color = roots[t]
        sl = Slice(t)
        otree = OTree(sl, size, tree_size=visits + 16, batch_size=K)
        np.random.set_state(np.random.RandomState(5000 + t).get_state())
        otree.search_best_move(oboard, color, OTM(OTC.STRICT_PLAYOUT, visits))
        oroot = otree.get_root()
        n = oroot.num_children
        assert sl.i == len(rec.log) and int(stats["num_children"][t]) == n and int(nodes[t]) == otree.num_nodes
        assert np.array_equal(stats["children_visits"][t][:n], oroot.children_visits[:n]), t
        assert np.array_equal(stats["children_value_sum"][t][:n], oroot.children_value_sum[:n]), t
        assert np.array_equal(stats["children_policy"][t][:n], oroot.children_policy[:n]), t
    engine.close()


def test_headline_launch_shape_pipe_kernel_batch_256_1000_visits_replay():
    """The headline's exact launch shape: more than 256 trees -> select_puct_pipe_kernel + backup_kernel<9, 8>,
    NN batch 256 per tree, 1000 strict visits (mini-batches 1 + 256 + 256 + 256 + 232).  Four of the 320 trees - first, two
    inside, last - are replayed into CPU oracle trees from their slices of the recorded mini-batches: identical leaf planes in
    order, identical visit counts / value sums / policies / node counts."""
    from oracle.board import GoBoard as OBoard
    from oracle.net import make_state_dict
    from oracle.tree import MCTSTree as OTree, TimeManager as OTM, TimeControl as OTC
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.mcts.engine import SearchEngine, DeviceEvaluator
    from tamago_amd.nn.network.dual_net import DualNet
    from tests.helpers import load_npz

    for knob in ("TG_SELECT_SERIAL", "TG_SELECT_MPIPE_TREES", "TG_MPIPE_PROF"):
        assert not os.environ.get(knob), "the kernel choice must be the library's default"
    size, T, K, visits = 9, 320, 256, 1000
    watch = (0, 107, 213, 319)
    net = DualNet(torch.device("cuda:0"), size)
    net.load_state_dict(make_state_dict(size, 7, 1.5))
    inner = DeviceEvaluator(net)
    log = []                                                # per mini-batch: the watched trees' slices only (host copies)

    def evaluator(planes, want_logits):
        policy, value = inner(planes, want_logits)
        per = planes.shape[0] // T
        log.append((per, [(planes[t * per:(t + 1) * per].cpu(), policy[t * per:(t + 1) * per].cpu(),
                           value[t * per:(t + 1) * per].cpu()) for t in watch]))
        return policy, value

    engine = SearchEngine(size, T, visits + 16, K, evaluator)
    brd = load_npz("board_s9.npz")
    roots = {}
    for t in range(T):
        game, plies = t % 4, 2 + (t * 7) % 40
        board, oboard = GoBoard(size, 7.0, False), OBoard(size, 7.0, False)
        mv, col = brd[f"g{game}_move"], brd[f"g{game}_color"]
        plies = min(plies, len(mv) - 1)
        for m, c in zip(mv[:plies], col[:plies]):
            board.put_stone(int(m), int(c))
            oboard.put_stone(int(m), int(c))
        color = 3 - int(col[plies - 1])
        engine.set_root(t, board, color, np.random.RandomState(7000 + t).get_state())
        roots[t] = (oboard, color)
    engine.root_eval(False)
    done = 0
    while done < visits:
        k = min(K, visits - done)
        engine.puct_batch(k)
        done += k
    stats = engine.read_root_stats()
    nodes = engine.num_nodes()
    assert [per for per, _ in log] == [1, 256, 256, 256, 232]

    class Slice:
        def __init__(self, w):
            self.w, self.i = w, 0

        def inference(self, planes):
            rp, pol, val = log[self.i][1][self.w]
            self.i += 1
            assert torch.equal(planes, rp[:planes.shape[0]]), (watch[self.w], self.i - 1)
            return pol[:planes.shape[0]], val[:planes.shape[0]]

    for w, t in enumerate(watch):
        oboard, color = roots[t]
        sl = Slice(w)
        otree = OTree(sl, size, tree_size=visits + 16, batch_size=K)
        np.random.set_state(np.random.RandomState(7000 + t).get_state())
        otree.search_best_move(oboard, color, OTM(OTC.STRICT_PLAYOUT, visits))
        oroot = otree.get_root()
        n = oroot.num_children
        assert sl.i == len(log) and int(stats["num_children"][t]) == n and int(nodes[t]) == otree.num_nodes
        assert np.array_equal(stats["children_visits"][t][:n], oroot.children_visits[:n]), t
        assert np.array_equal(stats["children_value_sum"][t][:n], oroot.children_value_sum[:n]), t
        assert np.array_equal(stats["children_policy"][t][:n], oroot.children_policy[:n]), t
    engine.close()


def test_forward_launch_of_524288_positions_first_middle_last_vs_oracle():
    """The headline's forward launch is 2 048 trees x 256 leaves = 524 288 positions; the net tests stop at a few thousand.
    One launch of that size on random planes: the first, a middle and the last 4 096 positions against the CPU oracle."""
    from oracle.net import OracleNet, make_state_dict
    from tamago_amd.nn.network.dual_net import DualNet
    sd = make_state_dict(9, 7, 1.5)
    net = DualNet(torch.device("cuda:0"), 9)
    net.load_state_dict(sd)
    n, w = 524288, 4096
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    x = torch.randint(-1, 2, (n, 6, 9, 9), device="cuda", generator=g).float()
    pol, val = net.forward_device(x)
    torch.cuda.synchronize()
    ora = OracleNet(sd)
    for lo in (0, (n // 2 // 768) * 768 + 5, n - w):          # (the middle window straddles workgroup-round boundaries)
        rp, rv = ora.inference(x[lo:lo + w].cpu())
        assert float((pol[lo:lo + w].cpu() - rp).abs().max()) < TOL, lo
        assert float((val[lo:lo + w].cpu() - rv).abs().max()) < TOL, lo
    assert net.range_fallbacks() == 0
