"""The early-stop rule on the CPU: csrc/stop_rule.h - the pair merge and the predicate stop_rule_kernel compiles - built alone
into tests/stop_rule_driver.cpp with the host compiler and held to Python's sorted(); the proof that the corpus of
tests/_early_stop_cases.py tells the right rule from three wrong ones; the switches of the command lines and EngineSetup's
defaults.  No GPU."""
import os
import random
import shutil
import subprocess

import pytest

from tests import _early_stop_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("stop_rule") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", os.path.join(HERE, "stop_rule_driver.cpp"), "-o", exe])

    def run(rows):
        """rows: (total, node_visits, [visits per slot]) -> (first, second, decided) per row"""
        text = "".join("%d %d %d %s\n" % (len(v), total, nv, " ".join(str(x) for x in v)) for total, nv, v in rows)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        out = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
        assert len(out) == len(rows) and all(o[3] == 1 for o in out), "the lanes of a butterfly disagree"
        return [(o[0], o[1], bool(o[2])) for o in out]
    return run


def expected(total, node_visits, visits):
    ordered = sorted(visits)
    return ordered[-1], ordered[-2], total - node_visits < ordered[-1] - ordered[-2]


def crafted_rows(A):
    rows = []
    for slot in (0, 63, 64, A - 1):                                  # the maximum in the first lane, across a stripe, in the tail
        v = [1] * A
        v[slot] = 9
        rows.append((20, 12, v))
        v = [0] * A                                                   # all zeros but one
        v[slot] = 5
        rows += [(9, 5, v), (10, 5, v), (11, 5, v)]                  # remaining 4, 5 (== cutoff: not decided), 6
    for a, b in ((3, 3 + 64), (0, A - 1), (63, 64), (5, 5 + 64 * ((A - 6) // 64))):
        v = [2] * A                                                   # two equal maxima in different 64-stripes: cutoff 0
        v[a] = v[b] = 40
        rows += [(100, 99, v), (100, 100, v), (100, 101, v)]         # (a remaining of -1 is below a cutoff of 0)
        v = list(v)
        v[a] = 41                                                     # ... and one visit apart
        rows += [(100, 99, v), (100, 100, v)]
    v = [0] * A
    rows += [(1, 0, v), (1, 1, v), (1, 2, v)]                        # an unvisited root
    v = [7] * A                                                       # every slot equal
    rows += [(7 * A + 3, 7 * A, v)]
    v = list(range(A))                                                # increasing, decreasing: second = first - 1
    rows += [(A + 5, A + 4, v), (A + 5, A + 5, v), (A + 5, A + 4, v[::-1])]
    return rows


@pytest.mark.parametrize("A", [82, 170, 362])
def test_pair_merge_and_predicate_against_sorted(driver, A):
    rnd = random.Random(A)
    rows = crafted_rows(A)
    for _ in range(300):
        children = rnd.randint(1, A)
        top = rnd.choice((1, 2, 3, 50, 100000))
        v = [rnd.randint(0, top) for _ in range(children)] + [0] * (A - children)
        nv = sum(v)
        ordered = sorted(v)
        cutoff = ordered[-1] - ordered[-2]
        rows.append((nv + cutoff + rnd.choice((-1, 0, 1)), nv, v))   # around remaining == cutoff
        rows.append((nv + rnd.randint(0, 3 * top), nv, v))
    got = driver(rows)
    for row, g in zip(rows, got):
        assert g == expected(*row), row


def test_int32_arithmetic_at_the_largest_counts(driver):
    big = 2 ** 31 - 1
    v = [0] * 82
    v[81], v[0] = big, 1
    assert driver([(big, big, v), (big, 1, v), (big, 2, v)]) == [(big, 1, True), (big, 1, False), (big, 1, True)]


def test_the_corpus_tells_the_rule_from_three_wrong_ones():
    """Every wrong rule - <= for <, the second largest taken as the second DISTINCT value, the rule applied after the last
    mini-batch as well - changes what at least one case leaves behind, so the exact comparisons of test_gpu_early_stop.py are
    not vacuous.  And the corpus holds what its docstring says."""
    right = {c[0]: cases.oracle_result(c[0]) for c in cases.CASES}
    for rule in cases.RULES[1:]:
        changed = [c[0] for c in cases.CASES if cases.search_oracle(c, rule) != right[c[0]]]
        assert changed, rule
    ran = {name: len(r["batches"]) for name, r in right.items()}
    assert right["first_test"]["halted"] and ran["first_test"] == 1 and right["first_test"]["batches"] == [16]
    assert right["last_full"]["halted"] and ran["last_full"] == 7
    assert right["mid_batch4"]["halted"] and ran["mid_batch4"] == 4 and right["mid_batch4"]["stopped_at"] == 16
    assert right["mid_batch1"]["halted"] and ran["mid_batch1"] == 11
    for name in ("never", "never_120", "equality", "equality_white", "tied_leaders"):
        assert not right[name]["halted"] and right[name]["stopped_at"] == 0 and sum(right[name]["batches"]) == right[name]["node_visits"]
    by_name = {c[0]: c for c in cases.CASES}
    assert any(rem == first - second for name in ("equality", "equality_white") for rem, first, second, _ in cases.rule_tests(by_name[name]))
    assert any(first == second and rem < first - distinct for rem, first, second, distinct in cases.rule_tests(by_name["tied_leaders"]))
    lock = [cases.oracle_result(c[0]) for c in cases.lockstep_cases()]
    assert [len(r["batches"]) for r in lock] == [8, 7, 8, 8, 4] and [r["halted"] for r in lock] == [False, True, False, False, True]


def test_the_command_lines_take_the_new_switches():
    from tamago_amd.analyze import parser as analyze_parser
    from tamago_amd.gtp.__main__ import parser as gtp_parser
    from tamago_amd.selfplay.match import parse_args, puct_setups
    assert gtp_parser().parse_args([]).device_early_stop is False
    assert gtp_parser().parse_args(["--device-early-stop"]).device_early_stop is True
    assert gtp_parser().parse_args(["--device-early-stop", "false"]).device_early_stop is False
    assert analyze_parser().parse_args(["g.sgf"]).strict_visits is True
    assert analyze_parser().parse_args(["g.sgf", "--strict-visits", "false"]).strict_visits is False
    base = ["--black", "a.bin", "--white", "b.bin", "--games", "8"]
    args = parse_args(base + ["--search", "puct"])
    assert args.strict_visits is None and args.white_strict_visits is None
    assert [s.strict for s in puct_setups(args, "A", "B")] == [True, True]
    args = parse_args(base + ["--search", "puct", "--strict-visits", "false"])
    assert [s.strict for s in puct_setups(args, "A", "B")] == [False, False]
    args = parse_args(base + ["--search", "puct", "--white-strict-visits", "false", "--visits", "50"])
    assert [s.strict for s in puct_setups(args, "A", "B")] == [True, False]
    assert puct_setups(args, "A", "B") == (("A", 50, 16), ("B", 50, 16))
    args = parse_args(base + ["--search", "puct", "--strict-visits", "false", "--white-strict-visits", "true"])
    assert [s.strict for s in puct_setups(args, "A", "B")] == [False, True]
    assert args.poll_every is None and parse_args(base + ["--search", "puct", "--poll-every", "1"]).poll_every == 1
    for bad in (["--strict-visits", "false"], ["--white-strict-visits", "true"], ["--poll-every", "2"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)                                    # only with --search puct


def test_engine_setup_defaults_and_identity():
    from tamago_amd.mcts.constant import NN_BATCH_SIZE, PLAYOUTS
    from tamago_amd.selfplay.puct_match import EngineSetup, puct_match
    s = EngineSetup("net")
    assert (s.network, s.visits, s.batch_size, s.strict) == ("net", PLAYOUTS, NN_BATCH_SIZE, True)
    network, visits, batch = s                                        # (a setup still unpacks as the triple it was)
    assert (network, visits, batch) == ("net", PLAYOUTS, NN_BATCH_SIZE)
    loose = EngineSetup("net", 30, 4, strict=False)
    assert loose.strict is False and loose == ("net", 30, 4) and loose != EngineSetup("net", 30, 4) and loose == EngineSetup("net", 30, 4, False)
    assert "strict=False" in repr(loose)
    # the tuple's own constructors keep the flag
    assert loose._replace(visits=40) == EngineSetup("net", 40, 4, False) and loose._replace(strict=True).strict is True
    assert EngineSetup._make(("net", 30, 4)).strict is True and EngineSetup._make(("net", 30, 4, False)) == loose
    assert loose._asdict() == {"network": "net", "visits": 30, "batch_size": 4, "strict": False}
    with pytest.raises(ValueError, match="strict"):
        puct_match(EngineSetup(object(), 8, 4), EngineSetup(object(), 8, 4, strict="no"), 1)


def test_analyze_positions_refuses_other_modes():
    from tamago_amd.mcts.analysis import analyze_positions
    from tamago_amd.mcts.time_manager import TimeControl
    from tamago_amd.board.go_board import GoBoard
    with pytest.raises(ValueError, match="mode"):
        analyze_positions(object(), [(GoBoard(9), 1)], 10, mode=TimeControl.CONSTANT_TIME)
