"""Row scoring on the CPU: csrc/row_score.h - the rank rule, the value hit, the invalid rows, the candidate mass,
the bucket rule and the table's order of summation, as the kernels of csrc/row_score.hip compile them - built alone into
tests/row_score_driver.cpp with the host compiler and held to the numpy / Python restatement of tests/_row_score_cases.py
(stable argsort, math.fsum); the proof that the corpus tells the right rules from two wrong ones; the same driver once more
under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _row_score_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
RIGHT, TIES_GREATER, LAST_MAXIMUM = 0, 1, 2
BW, NB = 10, 32


def _compiler():
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and (os.path.sep not in c or os.path.exists(c))), None)
    assert cxx, "no host C++ compiler"
    return cxx


def _input_text(arrays, rule, bucket_width, n_buckets, with_mask):
    policy, value, mask, move, cls, ply = arrays
    lines = ["%d %d %d %d %d %d" % (rule, policy.shape[1], len(move), bucket_width, n_buckets, int(with_mask))]
    pol_bits, val_bits = policy.view(np.uint32), value.view(np.uint32)
    for i in range(len(move)):
        lines.append("%d %d %d %s %s %s" % (move[i], cls[i], ply[i], " ".join(map(str, pol_bits[i])), " ".join(map(str, val_bits[i])),
                                            " ".join(map(str, mask[i]))))
    return "\n".join(lines) + "\n"


def _parse(stdout, n, n_buckets):
    lines = stdout.splitlines()
    assert len(lines) == n + n_buckets
    rows = np.zeros(n, dtype=cases.ROW_DTYPE)
    for i, line in enumerate(lines[:n]):
        p_move, rank, v_label, flags, bucket, mass, brier = (int(x) for x in line.split())
        rows[i] = (0.0, 0.0, p_move, rank, v_label, flags, bucket, 0)
        rows["cand_mass"][i:i + 1].view(np.uint64)[0] = mass
        rows["brier"][i:i + 1].view(np.uint64)[0] = brier
    table = np.zeros(n_buckets, dtype=cases.BUCKET_DTYPE)
    for b, line in enumerate(lines[n:]):
        words = [int(x) for x in line.split()]
        table["count"][b] = words[:6]
        table["sum"][b].view(np.uint64)[:] = words[6:]
    return rows, table


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "driver")
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-ffp-contract=off"] + extra +
                          [os.path.join(HERE, "row_score_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = _build(tmp_path_factory, "row_score", [])

    def run(arrays, rule=RIGHT, bucket_width=BW, n_buckets=NB, with_mask=True):
        res = subprocess.run([exe], input=_input_text(arrays, rule, bucket_width, n_buckets, with_mask), capture_output=True,
                             text=True, check=True)
        return _parse(res.stdout, len(arrays[3]), n_buckets)
    run.exe = exe
    return run


@pytest.fixture(scope="module")
def corpora():
    return {A: cases.corpus(A, bucket_width=BW, n_buckets=NB).arrays() for A in cases.ACTIONS}


@pytest.mark.parametrize("with_mask", [True, False], ids=["masks", "no_masks"])
@pytest.mark.parametrize("A", cases.ACTIONS)
def test_the_header_against_the_restatement(driver, corpora, A, with_mask):
    arrays = corpora[A]
    assert len(arrays[3]) > 257
    rows, table = driver(arrays, with_mask=with_mask)
    want = cases.restate(arrays, BW, NB, with_mask)
    cases.check_records(rows, want)
    cases.check_table(table, want, NB, rows["cand_mass"])
    # the corpus has what it says: invalid rows, ties, moves outside the mask, hits and misses
    flags = np.array([w["flags"] for w in want])
    assert (flags & cases.INVALID).sum() >= 8 and ((flags & cases.VALUE_HIT) != 0).sum() > 50
    if with_mask:
        valid = (flags & cases.INVALID) == 0
        assert ((flags & cases.MOVE_IS_CANDIDATE) == 0)[valid].sum() > 10 and ((flags & cases.MOVE_IS_CANDIDATE) != 0).sum() > 50
    else:
        assert not (flags & (cases.MOVE_IS_CANDIDATE | cases.HAS_MASK)).any()
        assert not rows["cand_mass"].any() and not table["count"][:, 3].any() and not table["sum"][:, 1].any()
    assert table["count"][:, 5].sum() == (flags & cases.INVALID != 0).sum()


@pytest.mark.parametrize("rule", [TIES_GREATER, LAST_MAXIMUM], ids=["ties_count_as_greater", "last_maximum_wins"])
@pytest.mark.parametrize("A", cases.ACTIONS)
def test_the_corpus_tells_the_rules_from_two_wrong_ones(driver, corpora, A, rule):
    """Ties counted as greater push a move behind every action tied with it, those after it included; the last maximum of the
    three values gives another hit flag wherever two values tie for the maximum."""
    arrays = corpora[A]
    rows, table = driver(arrays, rule=rule)
    want = cases.restate(arrays, BW, NB)
    valid = [i for i, w in enumerate(want) if not w["flags"] & cases.INVALID]
    wrong_rank = [i for i in valid if int(rows["rank"][i]) != want[i]["rank"]]
    wrong_hit = [i for i in valid if (int(rows["flags"][i]) ^ want[i]["flags"]) & cases.VALUE_HIT]
    if rule == TIES_GREATER:
        assert wrong_rank and not wrong_hit
        assert not np.array_equal(table["count"][:, 1:3], cases.restate_table(want, NB)[0][:, 1:3])     # top-1 / top-5 move with it
    else:
        assert wrong_hit and not wrong_rank
        assert not np.array_equal(table["count"][:, 4], cases.restate_table(want, NB)[0][:, 4])


def test_the_bucket_rule_at_the_last_bucket(driver):
    """min(ply / bucket_width, n_buckets - 1): the last ply of the last regular bucket, the first ply beyond, far beyond - and
    with one bucket everything falls into it."""
    A = 82
    rnd = np.random.RandomState(3)
    for bw, nb in ((10, 32), (7, 5), (1, 1), (3, 1)):
        edge = bw * nb
        plies = [max(p, 0) for p in (0, bw - 1, bw, edge - bw - 1, edge - bw, edge - 1, edge, edge + 1, edge + bw, 2 ** 31 - 1)]
        rows = cases.Rows(A)
        for ply in plies:
            rows.add(cases.softmax32(rnd.standard_normal(A)), cases.softmax32(rnd.standard_normal(3)), 3, 1, ply)
        got, table = driver(rows.arrays(), bucket_width=bw, n_buckets=nb)
        assert got["bucket"].tolist() == [min(p // bw, nb - 1) for p in plies]
        assert got["bucket"][5] == nb - 1 and got["bucket"][6] == nb - 1 and got["bucket"][9] == nb - 1
        if nb > 1:
            assert got["bucket"][3] == nb - 2 and got["bucket"][4] == nb - 1
        assert table["count"][:, 0].tolist() == np.bincount(got["bucket"], minlength=nb).tolist()


def test_the_driver_under_the_sanitizers(driver, corpora, tmp_path_factory):
    """The same text, built with -fsanitize=address,undefined as a stand-alone program: no report (a report ends the run with a
    non-zero status) and the same output, on rows that end at the last action of a partial lane pass and masks whose last word
    is partial."""
    exe = _build(tmp_path_factory, "row_score_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for A in cases.ACTIONS:
        text = _input_text(corpora[A], RIGHT, BW, NB, True)
        plain = subprocess.run([driver.exe], input=text, capture_output=True, text=True, check=True)
        checked = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert checked.returncode == 0, checked.stderr[-2000:]
        assert checked.stdout == plain.stdout


def test_the_header_and_the_abi_agree():
    """include/tamago_hip.h's tg_score_row / tg_score_bucket are csrc/row_score.h's records (row_score.hip asserts the sizes): the
    member order the tests' dtypes read them by, and the flag values."""
    import re
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "tamago_amd", "csrc", "row_score.h")).read()
    abi = open(os.path.join(root, "include", "tamago_hip.h")).read()
    members = re.findall(r"^\s+(?:double|uint32_t|int32_t)\s+(\w+);", re.search(r"struct RowRecord \{(.*?)\n\};", header, re.S).group(1), re.M)
    assert members == list(cases.ROW_DTYPE.names)
    abi_members = re.findall(r"^\s+(?:double|uint32_t|int32_t)\s+(\w+);", re.search(r"typedef struct tg_score_row \{(.*?)\n\}", abi, re.S).group(1), re.M)
    assert abi_members == members
    for name, value in (("kMoveIsCandidate", cases.MOVE_IS_CANDIDATE), ("kValueHit", cases.VALUE_HIT), ("kInvalid", cases.INVALID),
                        ("kHasMask", cases.HAS_MASK)):
        assert int(re.search(r"constexpr uint32_t %s = (\d+)u;" % name, header).group(1)) == value
    for name, value in (("TG_SCORE_MOVE_IS_CANDIDATE", 1), ("TG_SCORE_VALUE_HIT", 2), ("TG_SCORE_INVALID", 4), ("TG_SCORE_HAS_MASK", 8)):
        assert int(re.search(r"#define %s (\d+)u" % name, abi).group(1)) == value
