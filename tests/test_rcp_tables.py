"""The four-instruction quotient of the PUCT selectors (csrc/search.hip div_by_count: a / n from a table entry y = RN(1 / n))
against exact arithmetic - CPU only, no library needed.

The split selector fills its LDS table with the device's IEEE division; Python's `/` on two doubles is correctly rounded too,
so 1.0 / n here is the same table.  The quotient is evaluated with exact rationals (fractions.Fraction) and one rounding to
nearest even per operation, which is what v_mul_f64 / v_fma_f64 do, and compared with the correctly rounded a / n - the bits
of the division sequence it replaces.  The check beside the kernel covers integer a; here a is what the selectors divide: value
sums and prior-times-square-root products."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _select_rcp_digest import K_RCP_N  # noqa: E402


@pytest.fixture(scope="module")
def tables():
    """(n, rcp, sq): rcp[i] = RN(1 / i) as select_puct_split_kernel fills it (rcp[0] = 1, never read), sq[i] = RN(sqrt i)."""
    rcp = np.array([1.0] + [1.0 / i for i in range(1, K_RCP_N)])
    sq = np.array([math.sqrt(i) for i in range(K_RCP_N)])
    return K_RCP_N, rcp, sq


def rn(x: Fraction) -> float:
    """Round to nearest even: int / int is correctly rounded in CPython."""
    return x.numerator / x.denominator


def fma(a: float, b: float, c: float) -> float:
    return rn(Fraction(a) * Fraction(b) + Fraction(c))


def div_by_count(a: float, n: int, y: float) -> float:
    """csrc/search.hip div_by_count, operation by operation."""
    q0 = a * y
    r = fma(-q0, float(n), a)
    return fma(r, y, q0)


def test_table_entries_are_correctly_rounded(tables):
    n, rcp, sq = tables
    for i in range(1, n):
        assert Fraction(rcp[i]) == Fraction(rn(Fraction(1, i))), i
    for i in range(n):                         # RN(sqrt i): the nearest double, by comparing squares of the neighbours' midpoints
        lo = (Fraction(sq[i]) + Fraction(np.nextafter(sq[i], -1.0))) / 2 if i else Fraction(0)
        hi = (Fraction(sq[i]) + Fraction(np.nextafter(sq[i], np.inf))) / 2
        assert lo * lo <= i <= hi * hi, i


def test_quotient_of_value_sums_is_the_ieee_quotient(tables):
    """a = a value sum: a multiple of 2^-24 (sums of float32 values in [-1, 1]) of magnitude up to n."""
    n, rcp, _ = tables
    rs = np.random.RandomState(11)
    for b in range(1, n):
        ks = [1, b << 24, (b << 24) - 1, -(b << 24)] + [int(k) for k in rs.randint(-(b << 24), (b << 24) + 1, size=8)]
        for k in ks:
            a = k / float(1 << 24)              # exact: |k| < 2^35
            assert div_by_count(a, b, rcp[b]) == rn(Fraction(a) / b), (a, b)


def test_quotient_of_prior_times_sqrt_is_the_ieee_quotient(tables):
    """a = RN(p sqrt(N)), p a random double in (0, 1] (the child's prior), N = the node's count + 1: inside the table's
    range and far beyond it (the root's square root then comes from __dsqrt_rn, the children's reciprocals still from the table)."""
    n, rcp, sq = tables
    rs = np.random.RandomState(12)
    for b in range(1, n):
        ps = [1.0, 2.0 ** -40] + [1.0 - float(p) for p in rs.random_sample(6)]          # random_sample: [0, 1)
        for p in ps:
            big = int(rs.randint(1, 1 << 22))
            for root in (sq[int(rs.randint(1, n))], math.sqrt(big)):
                a = p * root
                assert div_by_count(a, b, rcp[b]) == rn(Fraction(a) / b), (p, root, b)
