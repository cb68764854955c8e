"""Live ranks on the CPU: csrc/live_rank.h - the predicate and the scan rule live_rank_kernel compiles, the carry
between chunks included - built alone into tests/live_rank_driver.cpp with the host compiler and held to numpy.cumsum; the
proof that the corpus tells the right rule from two wrong ones; the positions a compacted lock-step search evaluates, from the
oracle's own mini-batch logs; the switches of the command lines.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _early_stop_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "tamago_amd", "csrc", "live_rank.h")

RIGHT, INCLUSIVE, DROPPED_CARRY = 0, 1, 2


def chunk_size():
    return int(re.search(r"constexpr int kChunk = (\d+);", open(HEADER).read()).group(1))


def tree_counts():
    chunk = chunk_size()
    sizes = {1, 63, 64, 65, 1024, 1025, 2049}
    if chunk != 1024:
        sizes |= {chunk - 1, chunk, chunk + 1}
    return sorted(sizes)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("live_rank") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", os.path.join(HERE, "live_rank_driver.cpp"), "-o", exe])

    def run(rows, rule=RIGHT):
        """rows: (err [T], halt [T], num_nodes [T]) -> (count, rank [T]) per row"""
        text = "".join("%d %d %s\n" % (rule, len(err), " ".join("%d %d %d" % w for w in zip(err, halt, nodes)))
                       for err, halt, nodes in rows)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        out = [[int(x) for x in line.split()] for line in res.stdout.splitlines()]
        assert len(out) == len(rows)
        return [(o[0], np.array(o[1:], dtype=np.int64)) for o in out]
    return run


def expected(err, halt, nodes):
    """The issue's words: a live tree's rank is the count of live trees before it, a tree that is not live gets -1, the
    live count is the total."""
    live = (np.asarray(err) == 0) & (np.asarray(halt) == 0) & (np.asarray(nodes) > 0)
    before = np.cumsum(live) - live
    return int(live.sum()), np.where(live, before, -1)


def masks(T, rnd):
    """Halt masks: none halted, all halted, alternating (both phases), only the first tree live, only the last tree live,
    random at three densities."""
    out = [np.zeros(T, int), np.ones(T, int), np.arange(T) % 2, (np.arange(T) + 1) % 2]
    only_first, only_last = np.ones(T, int), np.ones(T, int)
    only_first[0] = 0
    only_last[-1] = 0
    out += [only_first, only_last]
    out += [(rnd.random_sample(T) < p).astype(int) for p in (0.1, 0.5, 0.9)]
    return out


def corpus():
    rows = []
    for T in tree_counts():
        rnd = np.random.RandomState(T)
        for halt in masks(T, rnd):
            rows.append((np.zeros(T, int), halt, np.ones(T, int)))                       # halt words alone
            # ... mixed with sticky error words (any non-zero word) and rootless trees (num_nodes 0)
            err = np.where(rnd.random_sample(T) < 0.2, rnd.choice([1, 2, 4, 8, -1], T), 0)
            nodes = np.where(rnd.random_sample(T) < 0.2, 0, rnd.randint(1, 500, T))
            rows.append((err, halt, nodes))
        # a halt word is any non-zero value; a live tree needs all three
        rows.append((np.zeros(T, int), rnd.choice([0, 1, 7, -3], T), np.ones(T, int)))
        rows.append((np.ones(T, int), np.zeros(T, int), np.ones(T, int)))                # every tree in error
        rows.append((np.zeros(T, int), np.zeros(T, int), np.zeros(T, int)))              # no tree has a root
    return rows


def test_the_header_against_cumsum(driver):
    rows = corpus()
    for row, (count, rank) in zip(rows, driver(rows)):
        want_count, want_rank = expected(*row)
        assert count == want_count and np.array_equal(rank, want_rank), (len(row[0]), count, want_count)


@pytest.mark.parametrize("rule", [INCLUSIVE, DROPPED_CARRY], ids=["inclusive_scan", "dropped_carry"])
def test_the_corpus_tells_the_rule_from_two_wrong_ones(driver, rule):
    """An inclusive scan ranks every live tree one too high; a carry dropped between chunks restarts the ranks at the second
    chunk, so only tree counts beyond one chunk can show it."""
    rows = corpus()
    wrong = [len(row[0]) for row, (count, rank) in zip(rows, driver(rows, rule))
             if (count, rank.tolist()) != (expected(*row)[0], expected(*row)[1].tolist())]
    assert wrong, rule
    if rule == DROPPED_CARRY:
        assert min(wrong) > chunk_size() and {chunk_size() + 1, 2 * chunk_size() + 1} <= set(wrong)
    else:
        assert 1 in wrong and 65 in wrong


# ---- the positions a compacted lock-step search evaluates -----------------------------------------------------------------
def compact_positions(ran, ks, poll_every):
    """ran[t]: the mini-batches tree t's oracle search ran; ks: the call's mini-batch sizes.  A forward pass covers k leaves
    of every tree that was live at the host's last look: before the first mini-batch, and after every poll_every-th one
    (0: never again) where a rule launch precedes it - a full mini-batch with descents to follow."""
    n = len(ks)
    live = sum(1 for r in ran if r > 0)
    total = 0
    for b, k in enumerate(ks):
        if live == 0:
            break
        total += k * live
        ruled = k == ks[0] and b + 1 < n
        if poll_every and (b + 1) % poll_every == 0 and ruled:
            live = sum(1 for r in ran if r > b + 1)
    return total


def lockstep_expected(poll_every, order=None):
    kind, seed, visits, batch, plies = cases.LOCKSTEP
    results = [cases.oracle_result(c[0]) for c in cases.lockstep_cases()]
    if order is not None:
        results = [results[plies.index(p)] for p in order]
    ks = [batch] * (visits // batch) + ([visits % batch] if visits % batch else [])
    for r in results:
        assert r["batches"] == ks[:len(r["batches"])]
    return compact_positions([len(r["batches"]) for r in results], ks, poll_every)


def test_expected_positions_of_the_lockstep_corpus():
    """From the oracle's own batches logs: sum over mini-batches b of k_b x (trees whose oracle search ran more than b
    mini-batches as of the last poll).  Plies 0, 10 and 20 never halt, ply 4 halts after 7 of 8 mini-batches, ply 30 after 4."""
    every, two, never = lockstep_expected(1), lockstep_expected(2), lockstep_expected(0)
    assert (every, two, never) == (134, 136, 150)
    assert len({every, two, never}) == 3
    # the order of the trees moves ranks, not counts
    assert lockstep_expected(1, (30, 4, 0, 10, 20)) == every and lockstep_expected(2, (30, 4, 0, 10, 20)) == two
    # the figure is the sum over the trees of what each was evaluated for
    ran = [len(cases.oracle_result(c[0])["batches"]) for c in cases.lockstep_cases()]
    assert ran == [8, 7, 8, 8, 4]


# ---- command lines --------------------------------------------------------------------------------------------------------
def test_the_command_lines_take_the_switch():
    from tamago_amd.analyze import parser as analyze_parser
    from tamago_amd.selfplay.match import parse_args
    assert analyze_parser().parse_args(["g.sgf"]).compact_idle is False
    assert analyze_parser().parse_args(["g.sgf", "--compact-idle"]).compact_idle is True
    base = ["--black", "a.bin", "--white", "b.bin", "--games", "8"]
    assert parse_args(base + ["--search", "puct"]).compact_idle is False
    assert parse_args(base + ["--search", "puct", "--compact-idle"]).compact_idle is True
    with pytest.raises(SystemExit):
        parse_args(base + ["--compact-idle"])                          # only with --search puct


def test_the_switches_reach_the_drivers(tmp_path, capsys, monkeypatch):
    """python -m tamago_amd.match --search puct --compact-idle: puct_match gets compact_idle and its legs ask the engine for
    compact chains - strict calls after halting the slots without a game - while the games stay the fake engine's oracle games;
    without the switch no call names the option.  python -m tamago_amd.analyze --compact-idle: analyze_positions gets it."""
    import tamago_amd.selfplay.match as match
    import tamago_amd.selfplay.puct_match as pm
    from tests import _puct_match_cases as pc
    from tests._match_cases import make_net
    from tests.test_puct_match_host import FakeEngine

    class CompactFake(FakeEngine):
        forward_positions = 0

        def puct_chain(self, batches, early_total=None, poll_every=None, compact=False):
            self.log.append(("chain", tuple(batches), early_total, compact))
            for leaves in batches:
                self.puct_batch(leaves)
            self.forward_positions += self.T * sum(batches)
            return len(batches)

        def set_halt(self, halt):
            self.log.append(("halt", tuple(bool(h) for h in halt)))

    def run(extra):
        engines, seen = [], {}
        real = pm.puct_match

        def spy(a, b, games, **kwargs):
            seen.update(kwargs)
            return real(pm.EngineSetup(make_net(pc.S301), *pc.BLACK_SEARCH), pm.EngineSetup(make_net(pc.S302), *pc.WHITE_SEARCH), games,
                        **dict(kwargs, seeds=[6, 1, 6], _make_engine=lambda leg: engines.append(CompactFake(leg)) or engines[-1]))
        monkeypatch.setattr(pm, "puct_match", spy)
        import tamago_amd.nn.utility as utility
        monkeypatch.setattr(utility, "load_network", lambda *a, **k: object())
        match.main(["--black", "a.bin", "--white", "b.bin", "--games", "3", "--boards", "2", "--search", "puct",
                    "--save-dir", str(tmp_path / ("on" if extra else "off"))] + extra)
        monkeypatch.setattr(pm, "puct_match", real)
        return seen, engines[0].log, capsys.readouterr().out

    seen, log, out_on = run(["--compact-idle"])
    assert seen["compact_idle"] is True
    chains = [e for e in log if e[0] == "chain"]
    assert chains and all(e[3] is True and e[2] is None for e in chains)        # (both setups are strict)
    halts = [e for e in log if e[0] == "halt"]
    assert halts and all(any(h) and not all(h) for _, h in halts)              # a game ended while the other ran: its slot halted
    seen, log, out_off = run([])
    assert "compact_idle" not in seen and not [e for e in log if e[0] in ("chain", "halt")]
    for i in range(3):                                                         # the same games either way
        assert open(tmp_path / "on" / f"{i}.sgf").read() == open(tmp_path / "off" / f"{i}.sgf").read()

    # analyze: a fake analyze_positions
    import io
    import tamago_amd.analyze as analyze
    import tamago_amd.mcts.analysis as analysis
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.board.stone import Stone
    got = []

    def fake_positions(network, positions, visits, **kwargs):
        got.append(kwargs)
        raise KeyboardInterrupt                                               # (what follows the call is not of interest here)
    monkeypatch.setattr(analysis, "analyze_positions", fake_positions)
    games = {"g.sgf": (type("Record", (), {"board_size": 9})(), [analysis.GamePosition("g.sgf", 1, Stone.BLACK, None, GoBoard(9))])}
    for argv, want in ((["g.sgf", "--compact-idle"], True), (["g.sgf"], False)):
        args = analyze.parser().parse_args(argv)
        with pytest.raises(KeyboardInterrupt):
            analyze.run(args, games=games, network_for=lambda size: object(), out=io.StringIO())
        assert got[-1].get("compact_idle", False) is want
