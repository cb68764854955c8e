"""tg_score_rows (csrc/row_score.hip) against the numpy / Python restatement of tests/_row_score_cases.py on the
crafted and random rows the CPU test holds the header to: row records bit for bit, table counts exactly, every logarithm the
bits of tg_glibc_log, every fp64 sum within the summation bound of its own addends; equal calls give equal table bits; chunks add
up; the refusals of the C ABI."""
import ctypes
import functools

import numpy as np
import pytest

from tests import _row_score_cases as cases

pytestmark = pytest.mark.gpu

BW, NB = 10, 32
SIZES = (1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def _corpus(A):
    return cases.corpus(A, bucket_width=BW, n_buckets=NB)


@functools.lru_cache(maxsize=None)
def _restated(A, n, with_mask=True):
    return cases.restate(_corpus(A).arrays(n), BW, NB, with_mask)


def _score(arrays, table=None, clear=1, with_mask=True, bucket_width=BW, n_buckets=NB):
    """-> (rows structured [n], table structured [n_buckets], the device table)"""
    import torch
    from tamago_amd import lib as tl
    lib = tl.load()
    policy, value, mask, move, cls, ply = arrays
    n, A = policy.shape
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(x).to(dev) for x in (policy, value, mask.view(np.int32), move, cls, ply)]
    rows = torch.zeros(max(n, 1) * cases.ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    if table is None:
        table = torch.full((n_buckets * cases.BUCKET_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)   # (clear must clear it)
    tl.check(lib.tg_score_rows(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr() if with_mask else None, t[3].data_ptr(),
                               t[4].data_ptr(), t[5].data_ptr(), n, A, bucket_width, n_buckets, rows.data_ptr(), table.data_ptr(),
                               clear, torch.cuda.current_stream().cuda_stream), "tg_score_rows")
    torch.cuda.synchronize()
    return (rows.cpu().numpy().view(cases.ROW_DTYPE)[:n], table.cpu().numpy().view(cases.BUCKET_DTYPE), table)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("A", cases.ACTIONS)
def test_rows_and_table_against_the_restatement(A, n):
    arrays = _corpus(A).arrays(n)
    rows, table, _ = _score(arrays)
    want = _restated(A, n)
    cases.check_records(rows, want)
    cases.check_table(table, want, NB, rows["cand_mass"])
    # two calls on the same rows: the same table bits, the same records
    rows2, table2, _ = _score(arrays)
    assert rows.tobytes() == rows2.tobytes() and table.tobytes() == table2.tobytes()


@pytest.mark.parametrize("A", cases.ACTIONS)
def test_every_log_term_is_tg_glibc_log(A):
    """One row per call and one bucket: the table's policy and value sums ARE the row's terms, 0 + term, and must be the bits of
    -tg_glibc_log((double)p + 1e-8)."""
    from tamago_amd import lib as tl
    lib = tl.load()
    policy, value, mask, move, cls, ply = _corpus(A).arrays(65)
    want = _restated(A, 65)
    checked = 0
    for i in range(0, 65, 2):
        if want[i]["flags"] & cases.INVALID:
            continue
        one = tuple(x[i:i + 1] for x in (policy, value, mask, move, cls, ply))
        rows, table, _ = _score(one, bucket_width=1, n_buckets=1)
        x = np.array([float(policy[i, move[i]]) + 1e-8, float(value[i, cls[i]]) + 1e-8], dtype=np.float64)
        out = np.zeros(2, dtype=np.float64)
        tl.check(lib.tg_glibc_log(x.ctypes.data, 2, out.ctypes.data), "tg_glibc_log")
        got = table["sum"][0]
        assert got[0:1].tobytes() == (-out[0:1]).tobytes() and got[2:3].tobytes() == (-out[1:2]).tobytes(), i
        assert got[1] == rows["cand_mass"][0] and got[3] == rows["brier"][0]
        checked += 1
    assert checked > 20


@pytest.mark.parametrize("A", cases.ACTIONS)
def test_without_masks(A):
    arrays = _corpus(A).arrays(65)
    rows, table, _ = _score(arrays, with_mask=False)
    want = _restated(A, 65, False)
    cases.check_records(rows, want)
    cases.check_table(table, want, NB, rows["cand_mass"])
    assert not rows["cand_mass"].any() and not (rows["flags"] & (cases.HAS_MASK | cases.MOVE_IS_CANDIDATE)).any()
    assert not table["count"][:, 3].any() and not table["sum"][:, 1].any()


@pytest.mark.parametrize("A", cases.ACTIONS)
def test_chunks_add_up(A):
    """Two calls of 100 and 157 rows into one table (clear on the first only): the counts of one call of 257, the sums within
    the bound; a third call of no rows changes nothing, and clear with no rows clears."""
    arrays = _corpus(A).arrays(257)
    whole_rows, whole, _ = _score(arrays)
    head = tuple(x[:100] for x in arrays)
    tail = tuple(np.ascontiguousarray(x[100:]) for x in arrays)
    rows_a, _, dev_table = _score(head)
    rows_b, both, dev_table = _score(tail, table=dev_table, clear=0)
    assert np.array_equal(both["count"], whole["count"])
    assert rows_a.tobytes() + rows_b.tobytes() == whole_rows.tobytes()
    cases.check_table(both, _restated(A, 257), NB, whole_rows["cand_mass"])
    empty = tuple(x[:0] for x in arrays)
    _, same, dev_table = _score(empty, table=dev_table, clear=0)
    assert same.tobytes() == both.tobytes()
    _, cleared, _ = _score(empty, table=dev_table, clear=1)
    assert not cleared.tobytes().strip(b"\0")


def test_other_bucket_shapes():
    """One bucket; a width beyond every ply; more buckets than plies."""
    arrays = _corpus(82).arrays(130)
    for bw, nb in ((1, 1), (1000000, 3), (3, 200)):
        rows, table, _ = _score(arrays, bucket_width=bw, n_buckets=nb)
        want = cases.restate(arrays, bw, nb)
        cases.check_records(rows, want)
        cases.check_table(table, want, nb, rows["cand_mass"])


def test_refusals():
    import torch
    from tamago_amd import lib as tl
    lib = tl.load()
    policy, value, mask, move, cls, ply = _corpus(82).arrays(4)
    dev = torch.device("cuda", 0)
    inputs = [torch.from_numpy(x).to(dev) for x in (policy, value, mask.view(np.int32), move, cls, ply)]      # (kept alive)
    t = [x.data_ptr() for x in inputs]
    keep = [torch.zeros(4 * 40, dtype=torch.uint8, device=dev), torch.zeros(32 * 80, dtype=torch.uint8, device=dev)]
    good = t + [4, 82, BW, NB, keep[0].data_ptr(), keep[1].data_ptr(), 1, None]
    for index in (0, 1, 3, 4, 5, 10, 11):                                   # every pointer but the masks
        bad = list(good)
        bad[index] = None
        assert lib.tg_score_rows(*bad) == -1 and b"null" in lib.tg_last_error(), index
    for index, value_, word in ((9, 0, b"n_buckets"), (9, -1, b"n_buckets"), (8, 0, b"bucket_width"), (8, -5, b"bucket_width"),
                                (6, -1, b"negative"), (7, 1, b"actions")):
        bad = list(good)
        bad[index] = value_
        assert lib.tg_score_rows(*bad) == -1 and word in lib.tg_last_error(), (index, value_)
    torch.cuda.synchronize()
    assert not keep[1].cpu().numpy().any()                                  # a refused call touched nothing
    assert lib.tg_score_rows(*good) == 0
    torch.cuda.synchronize()
    assert int(keep[1].cpu().numpy().view(cases.BUCKET_DTYPE)["count"][:, [0, 5]].sum()) == 4
