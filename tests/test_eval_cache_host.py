"""The evaluation cache on the CPU: csrc/eval_cache.h - the key, the hash, the hit and insert rules, the miss ranks,
the kernels' order of operations - built alone into tests/eval_cache_driver.cpp with the host compiler and held to numpy and
Python restatements and to a dict model; the proof that the corpus tells the right rules from wrong ones; the driver once
more under the address and undefined-behaviour sanitizers; the oracle's evaluated-row counts of the games the GPU tests
play; the switches of the command lines.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _eval_cache_cases as ec

HERE = os.path.dirname(os.path.abspath(__file__))
RIGHT, ONE_BUCKET, TAG_IS_HIT, EVICT_ANY = 0, 1, 2, 3
RANK_RIGHT, RANK_INCLUSIVE, RANK_DROPPED_CARRY = 0, 1, 2


def _compiler():
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    return cxx


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "driver")
    subprocess.check_call([_compiler(), "-std=c++17"] + flags + [os.path.join(HERE, "eval_cache_driver.cpp"), "-o", exe])
    return exe


def _run(exe, lines):
    res = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    out = res.stdout.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "eval_cache", ["-O1"])


def hexes(a) -> str:
    return " ".join("%x" % int(w) for w in np.ascontiguousarray(a).reshape(-1).view(np.uint32))


def outputs_of(rows, want_logits):
    """The stand-in network of the replays: A + 3 words a row that depend on every float of the row and on want_logits."""
    n, A = rows.shape[0], rows.shape[2] * rows.shape[3] + 1
    flat = rows.reshape(n, -1).view(np.uint32).astype(np.uint64)
    seed = (flat * (np.arange(flat.shape[1], dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345))).sum(axis=1)
    out = (seed[:, None] * np.uint64(6364136223846793005) + np.arange(A + 3, dtype=np.uint64)[None, :] * np.uint64(1442695040888963407)
           + np.uint64(7 if want_logits else 0)) >> np.uint64(32)
    return out.astype(np.uint32)


class Session:
    """One table of the driver: calls are collected and run in one process at the end (run())."""

    def __init__(self, exe, variant, S, entries, ways):
        self.exe, self.S = exe, S
        self.lines = ["new %d %d %d %d" % (variant, S, entries, ways)]
        self.calls = []

    def run_calls(self, calls):
        """calls: (rows float32 [n,6,S,S], want_logits) or "clear"; the probe's answer decides the commit's input, so the
        driver is run once per prefix - cheap at these sizes.  -> per call (n_miss, flags, miss_row, outputs [n, A+3])."""
        results = []
        script = list(self.lines)
        for call in calls:
            if isinstance(call, str):
                script.append(call)
                results.append(None)
                continue
            rows, want_logits = call
            probe = "probe %d %d %s" % (int(want_logits), len(rows), hexes(rows))
            out = _run(self.exe, script + [probe])[-1].split()
            n_miss = int(out[0])
            flags = np.array([int(x) for x in out[1:1 + len(rows)]])
            miss_row = [int(x) for x in out[1 + len(rows):]]
            assert len(miss_row) == min(max(n_miss, 0), len(rows))
            safe = [r if 0 <= r < len(rows) else 0 for r in miss_row]
            commit = "commit " + hexes(outputs_of(rows[safe], want_logits)) if safe else "commit"
            script += [probe, commit]
            final = _run(self.exe, script)[-1].split()
            A = self.S * self.S + 1
            results.append((n_miss, flags, miss_row, np.array([int(x, 16) for x in final], dtype=np.uint32).reshape(len(rows), A + 3)))
        self.script = script
        return results

    def stats(self):
        return [int(x) for x in _run(self.exe, self.script + ["stats"])[-1].split()]

    def table(self):
        text = _run(self.exe, self.script + ["table"])[-1]
        return [[int(x, 16) if i else int(x) for i, x in enumerate(e.split())] for e in text.split(";") if e.strip()]


# ---- key and canonical test -----------------------------------------------------------------------------------------------
def key_lines(S, cases, nb=64, ways=4):
    return ["key %d %d %d %d %s" % (S, int(lg), nb, ways, hexes(row)) for row, lg in cases]


@pytest.mark.parametrize("S", [9, 13, 19])
def test_the_key_against_numpy(exe, S):
    rnd = np.random.RandomState(S)
    P = S * S
    assert ec.key_words(P) == {9: 16, 13: 31, 19: 61}[S]            # 15 / 30 / 60 plane words and the meta word
    rows = ec.random_rows(rnd, S, 12)
    cases = [(row, bool(i % 2)) for i, row in enumerate(rows)]
    out = _run(exe, key_lines(S, cases))
    keys = []
    for (row, lg), line in zip(cases, out):
        f = line.split()
        key = np.array([int(x, 16) for x in f[5:]], dtype=np.uint32)
        want = ec.pack(row.reshape(6, P), lg)
        assert f[0] == "1" and np.array_equal(key, want)
        wpp = ec.words_per_plane(P)
        tail = (1 << (P % 32)) - 1                                  # (all three sizes have a partial last word)
        assert all(int(key[pl * wpp + wpp - 1]) & ~tail == 0 for pl in range(5))
        # hash, bucket, tag and victim against the Python restatement
        h = ec.hash_key(want)
        assert int(f[1], 16) == h and (int(f[2]), int(f[3], 16), int(f[4])) == ec.placement(h, 64, 4)
        keys.append(key)
    # unpack(pack(row)) == row
    back = _run(exe, ["unpack %d %s" % (S, " ".join("%x" % int(w) for w in key)) for key in keys])
    for (row, lg), line in zip(cases, back):
        f = line.split()
        assert int(f[0]) == int(lg)
        assert np.array_equal(np.array([int(x, 16) for x in f[1:]], dtype=np.uint32), row.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("S", [9, 13, 19])
def test_one_flip_changes_the_key(exe, S):
    rnd = np.random.RandomState(100 + S)
    P = S * S
    base = ec.random_rows(rnd, S, 1)[0]
    cases = [(base, False), (base, True)]
    flipped = base.copy()
    flipped[5] = -flipped[5]
    cases.append((flipped, False))
    for pl in range(5):
        for p in sorted({0, 31, 32, 63, 64, P - 1, int(rnd.randint(P))}):      # (word borders, the tail word, anywhere)
            row = base.copy().reshape(6, P)
            row[pl, p] = 1.0 - row[pl, p]
            cases.append((row.reshape(6, S, S), False))
    out = _run(exe, key_lines(S, cases))
    keys = [tuple(line.split()[5:]) for line in out]
    assert all(line.split()[0] == "1" for line in out)
    assert len(set(keys)) == len(keys)                               # every single flip is another key
    for (row, lg), key in zip(cases, keys):
        assert np.array_equal(np.array([int(x, 16) for x in key], dtype=np.uint32), ec.pack(row.reshape(6, P), lg))


@pytest.mark.parametrize("S", [9, 13, 19])
def test_rows_that_are_not_canonical(exe, S):
    rnd = np.random.RandomState(200 + S)
    P = S * S
    base = ec.random_rows(rnd, S, 1)[0]
    cases = []
    for bad in (0.5, 2.0, -1.0, float("nan"), -0.0):
        for pl, p in ((0, 0), (2, P - 1), (4, 40)):
            row = base.copy().reshape(6, P)
            row[pl, p] = bad
            cases.append(row)
    mixed = base.copy().reshape(6, P)
    mixed[5, P - 1] = -mixed[5, P - 1]                               # a mixed plane 5
    cases += [mixed, np.zeros((6, P), dtype=np.float32)]             # ... and the zero row of a compacted launch
    half = base.copy().reshape(6, P)
    half[5] = 0.5
    cases.append(half)
    out = _run(exe, key_lines(S, [(row.reshape(6, S, S), False) for row in cases]))
    assert [line.split()[0] for line in out] == ["0"] * len(cases)
    assert not any(ec.canonical(row) for row in cases) and ec.canonical(base)


# ---- miss ranks -------------------------------------------------------------------------------------------------------------
RANK_SIZES = (1, 63, 64, 65, 1024, 1025, 2049, 65537)


def rank_corpus():
    out = []
    for n in RANK_SIZES:
        rnd = np.random.RandomState(n)
        first, last = np.zeros(n, int), np.zeros(n, int)
        first[0] = 1
        last[-1] = 1
        masks = [np.zeros(n, int), np.ones(n, int), np.arange(n) % 2, (np.arange(n) + 1) % 2, first, last,
                 (rnd.random_sample(n) < 0.5).astype(int), (rnd.random_sample(n) < 0.1).astype(int)]
        for m in masks:
            out.append(m)
            out.append(np.where(m == 1, rnd.choice([ec.MISS, ec.UNCACHED], n), ec.HIT))      # (uncacheable rows need the network too)
    return out


def rank_expected(flags):
    need = (np.asarray(flags) != ec.HIT).astype(np.int64)
    return int(need.sum()), np.where(need == 1, np.cumsum(need) - need, -1)


def run_ranks(exe, corpus, rule):
    out = _run(exe, ["rank %d %s" % (rule, "".join(str(int(f)) for f in flags)) for flags in corpus])
    return [(int(line.split()[0]), np.array(line.split()[1:], dtype=np.int64)) for line in out]


def test_the_miss_ranks_against_cumsum(exe):
    corpus = rank_corpus()
    for flags, (count, rank) in zip(corpus, run_ranks(exe, corpus, RANK_RIGHT)):
        want_count, want_rank = rank_expected(flags)
        assert count == want_count and np.array_equal(rank, want_rank), len(flags)


@pytest.mark.parametrize("rule", [RANK_INCLUSIVE, RANK_DROPPED_CARRY], ids=["inclusive_scan", "dropped_carry"])
def test_the_rank_corpus_tells_the_rule_from_two_wrong_ones(exe, rule):
    corpus = rank_corpus()
    wrong = {len(flags) for flags, (count, rank) in zip(corpus, run_ranks(exe, corpus, rule))
             if (count, rank.tolist()) != (rank_expected(flags)[0], rank_expected(flags)[1].tolist())}
    if rule == RANK_DROPPED_CARRY:
        assert wrong and min(wrong) > 1024 and {1025, 2049, 65537} <= wrong
    else:
        assert {1, 65, 65537} <= wrong


# ---- sequential replay of probe and commit against a dict model ---------------------------------------------------------------
def replay_calls(S, rnd):
    """Calls over a pool of rows: old rows, new rows, in-call twins, rows that are not canonical, both want_logits, a clear."""
    pool = ec.random_rows(rnd, S, 40)
    odd = pool[:4].copy()
    odd[0, 1, 2, 3] = 0.5
    odd[1, 5] = 0.0
    odd[2] = 0.0
    odd[3, 5, 0, 0] = -odd[3, 5, 0, 0]

    def take(idx, extra=()):
        rows = [pool[i] for i in idx] + [odd[i] for i in extra]
        order = rnd.permutation(len(rows))
        return np.stack([rows[i] for i in order])
    return [(take(range(0, 10)), False),
            (take([0, 1, 2, 10, 11, 11, 11, 12, 3], extra=[0, 1]), False),       # old, new, twins, uncacheable
            (take([0, 1, 10, 13]), True),                                         # the other outputs: nothing is known yet
            (take([0, 1, 10, 13, 14, 14], extra=[2, 3, 0]), True),
            (take(range(0, 20)), False),
            "clear",
            (take(range(0, 20), extra=[1]), False),
            (take(range(15, 40)), False)]


@pytest.mark.parametrize("S", [9, 13])
def test_replay_against_the_dict_model(exe, S):
    rnd = np.random.RandomState(300 + S)
    calls = replay_calls(S, rnd)
    session = Session(exe, RIGHT, S, 4096, 8)
    model = ec.DictModel()
    for call, result in zip(calls, session.run_calls(calls)):
        if isinstance(call, str):
            model.clear()
            continue
        rows, want_logits = call
        n_miss, flags, miss_row, outputs = result
        want_flags = model.call(rows, want_logits)
        assert np.array_equal(flags, want_flags)
        assert n_miss == int((want_flags != ec.HIT).sum()) and miss_row == [int(r) for r in np.nonzero(want_flags != ec.HIT)[0]]
        assert np.array_equal(outputs, outputs_of(rows, want_logits))          # hits return what was committed for the equal row
    stats = session.stats()
    # the inputs show no overflow themselves: nothing was evicted or dropped, no tag matched with another key
    assert stats[5] == stats[6] == stats[7] == 0
    assert stats[:5] == [model.stats[k] for k in ("lookups", "hits", "uncacheable", "inserts", "twin_skips")]
    assert stats[1] > 0 and stats[2] > 0 and stats[4] > 0
    # every resident key is the key of a row that was committed since the clear, once
    resident = [tuple(e[2:]) for e in session.table()]
    assert len(resident) == len(set(resident)) == len(model.known)


# ---- wrong rules --------------------------------------------------------------------------------------------------------------
def test_a_tag_match_alone_is_not_a_hit(exe):
    """Under a hash that sends every row to one bucket with one tag, the right hit rule still tells the rows apart by their
    keys (the second row is never served the first row's outputs; it is not cached either: its tag is taken); the wrong rule
    "a tag match is a hit" returns another row's outputs - so the corpus would catch it."""
    rnd = np.random.RandomState(5)
    rows = ec.random_rows(rnd, 9, 3)
    calls = [(rows[:1], False), (rows[1:2], False), (rows, False)]
    right = Session(exe, ONE_BUCKET, 9, 64, 4)
    results = right.run_calls(calls)
    for (r, lg), (n_miss, flags, _, outputs) in zip(calls, results):
        assert np.array_equal(outputs, outputs_of(r, lg))
    assert results[2][1].tolist() == [ec.HIT, ec.MISS, ec.MISS]
    stats = right.stats()
    assert stats[7] >= 3 and stats[3] == 1 and stats[4] == 3          # tag-only matches; one insert; the others skipped as twins
    wrong = Session(exe, TAG_IS_HIT, 9, 64, 4)
    results = wrong.run_calls(calls)
    assert results[1][1].tolist() == [ec.HIT]                         # served ...
    assert not np.array_equal(results[1][3], outputs_of(rows[1:2], False))
    assert np.array_equal(results[1][3], outputs_of(rows[:1], False))  # ... the other row's outputs


def test_a_way_is_evicted_at_most_once_a_call(exe):
    """One bucket of 2 ways, 12 distinct rows in each of three calls.  The right rule: a way written in this call carries its
    epoch and is not evicted again, so a call evicts at most `ways` entries and drops the rest; "evict regardless of epoch"
    lets row after row claim the same way within one call."""
    rnd = np.random.RandomState(6)
    rows = ec.random_rows(rnd, 9, 36)
    calls = [(rows[0:12], False), (rows[12:24], False), (rows[24:36], False)]
    for variant in (RIGHT, EVICT_ANY):
        session = Session(exe, variant, 9, 2, 2)
        per_call = []
        before = [0] * 8
        for k in range(3):
            results = session.run_calls(calls[:k + 1])
            for (r, lg), res in zip(calls[:k + 1], results):
                assert np.array_equal(res[3], outputs_of(r, lg))      # the outputs are right whatever the table keeps
            stats = session.stats()
            per_call.append([a - b for a, b in zip(stats, before)])
            before = stats
        total = session.stats()
        assert total[3] + total[4] + total[6] == 36 - total[1]        # inserts + twin skips + dropped == cacheable misses
        evictions = [c[5] for c in per_call]
        if variant == RIGHT:
            assert evictions[0] == 0 and all(e <= 2 for e in evictions) and sum(evictions) > 0
            assert per_call[0][6] == 10                               # 2 ways claimed, 10 inserts dropped
        else:
            assert evictions[0] > 2                                   # two rows claimed one way in one call
        assert len(session.table()) == 2


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------
def test_the_driver_under_sanitizers(tmp_path_factory):
    """The driver as a stand-alone program with -fsanitize=address,undefined: keys, ranks at the chunk borders, and a replay
    with twins, uncacheable rows, evictions and a clear."""
    cxx = _compiler()
    probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path_factory.mktemp("san") / "t")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    assert probe.returncode == 0, "the host compiler cannot link -fsanitize=address,undefined: " + probe.stderr[-500:]
    san = _build(tmp_path_factory, "eval_cache_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    rnd = np.random.RandomState(8)
    for S in (9, 19):
        rows = ec.random_rows(rnd, S, 4)
        _run(san, key_lines(S, [(row, True) for row in rows]))
    corpus = [f for f in rank_corpus() if len(f) in (1, 65, 1025, 2049)]
    run_ranks(san, corpus, RANK_RIGHT)
    calls = replay_calls(9, np.random.RandomState(9))
    for variant, entries, ways in ((RIGHT, 4096, 8), (RIGHT, 4, 2), (EVICT_ANY, 2, 2), (TAG_IS_HIT, 8, 4)):
        Session(san, variant, 9, entries, ways).run_calls(calls)


# ---- the oracle's counts of the games the GPU tests play ------------------------------------------------------------------------
def test_oracle_counts_of_the_match_game():
    """Oracle game 1 of tests/_puct_match_cases (black 26 x 8, white 20 x 6) - what puct_match plays on ONE board, call for
    call: the rows its networks are handed and how many a cache per network serves; with one network on both sides one
    cache sees both colours' searches and serves more."""
    two, one = ec.oracle_match_counts(False), ec.oracle_match_counts(True)
    assert two == EXPECTED_MATCH[False] and one == EXPECTED_MATCH[True]
    assert 0 < two[1] < two[0] and 0 < one[1] < one[0]
    assert one[1] / one[0] > two[1] / two[0]


def test_oracle_counts_of_two_consecutive_searches():
    first, second, counts = ec.oracle_two_moves()
    assert (first, second, counts) == EXPECTED_TWO_MOVES
    (rows1, served1), (rows2, served2) = counts
    assert served2 - served1 > 0                                      # the second search meets positions of the first


# (rows handed to the networks, rows a cache per network serves) of oracle game 1: StubNet(301) against StubNet(302), and
# StubNet(301) on both sides; the two moves and the cumulative (rows, served) of the two consecutive searches
EXPECTED_MATCH = {False: (2264, 89), True: (2667, 476)}
EXPECTED_TWO_MOVES = (57, 29, [(61, 0), (122, 12)])


# ---- command lines ------------------------------------------------------------------------------------------------------------
def test_the_command_lines_take_the_switch():
    from tamago_amd.analyze import parser as analyze_parser
    from tamago_amd.gtp.__main__ import parser as gtp_parser
    from tamago_amd.selfplay.match import parse_args
    assert analyze_parser().parse_args(["g.sgf"]).eval_cache is None
    assert analyze_parser().parse_args(["g.sgf", "--eval-cache", "4096"]).eval_cache == 4096
    assert gtp_parser().parse_args([]).eval_cache is None
    assert gtp_parser().parse_args(["--eval-cache", "65536"]).eval_cache == 65536
    base = ["--black", "a.bin", "--white", "b.bin", "--games", "8"]
    assert parse_args(base + ["--search", "puct"]).eval_cache is None
    assert parse_args(base + ["--search", "puct", "--eval-cache", "1024"]).eval_cache == 1024
    for bad in (base + ["--eval-cache", "1024"],                      # only with --search puct
                base + ["--search", "puct", "--eval-cache", "0"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    for p in (analyze_parser(), gtp_parser()):
        with pytest.raises(SystemExit):
            p.parse_args((["g.sgf"] if p.prog.endswith("analyze") else []) + ["--eval-cache", "0"])


def test_the_switches_reach_the_drivers(monkeypatch):
    """python -m tamago_amd.analyze --eval-cache N: analyze_positions gets eval_cache=N, and does not hear of it without the
    switch; python -m tamago_amd.match --search puct --eval-cache N: puct_match gets it; MCTSTree keeps what GtpClient hands it."""
    import io
    import tamago_amd.analyze as analyze
    import tamago_amd.mcts.analysis as analysis
    import tamago_amd.selfplay.match as match
    import tamago_amd.selfplay.puct_match as pm
    from tamago_amd.board.go_board import GoBoard
    from tamago_amd.board.stone import Stone
    got = []

    def fake_positions(network, positions, visits, **kwargs):
        got.append(kwargs)
        raise KeyboardInterrupt
    monkeypatch.setattr(analysis, "analyze_positions", fake_positions)
    games = {"g.sgf": (type("Record", (), {"board_size": 9})(), [analysis.GamePosition("g.sgf", 1, Stone.BLACK, None, GoBoard(9))])}
    for argv, want in ((["g.sgf", "--eval-cache", "512"], 512), (["g.sgf"], None)):
        with pytest.raises(KeyboardInterrupt):
            analyze.run(analyze.parser().parse_args(argv), games=games, network_for=lambda size: object(), out=io.StringIO())
        assert got[-1].get("eval_cache") == want and (want is not None or "eval_cache" not in got[-1])

    seen = []

    def fake_match(a, b, games, **kwargs):
        seen.append(kwargs)
        raise KeyboardInterrupt
    monkeypatch.setattr(pm, "puct_match", fake_match)
    import tamago_amd.nn.utility as utility
    monkeypatch.setattr(utility, "load_network", lambda *a, **k: object())
    base = ["--black", "a.bin", "--white", "b.bin", "--games", "3", "--search", "puct"]
    for argv, want in ((base + ["--eval-cache", "2048"], 2048), (base, None)):
        with pytest.raises(KeyboardInterrupt):
            match.main(argv)
        assert seen[-1].get("eval_cache") == want and (want is not None or "eval_cache" not in seen[-1])

    from tamago_amd.mcts.tree import MCTSTree
    assert MCTSTree(object()).eval_cache == 0 and MCTSTree(object(), eval_cache=4096).eval_cache == 4096
    evaluator = object()
    assert MCTSTree(object())._cached(evaluator, 9) is evaluator      # off: the evaluator as it is
