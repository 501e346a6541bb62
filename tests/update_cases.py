"""Same-pattern value updates (sluamd_[dz]UpdateValues) -- test helper for test_gpu_update_values.py and test_update_values_cpu.py; not a conftest.

Exact part: the sweep cases of sweep_cases.py / trans_cases.py.  `csr_case(name)` gives the CSR of B = L0 U0 on the case's pattern (the values the exact
factors belong to) and `wrong_values(...)`, OTHER values on the same pattern: 3 v with the diagonal doubled again (6 v there) -- every entry differs from v,
so an entry the update left stale anywhere changes the factors, and the ratio of diagonal to off-diagonal entries differs too, so a handle that kept the
wrong values does not even solve a multiple of the system.

Floating-point part: `scaled_values` is the numpy restatement of what an equilibrated handle stores for new values, (a r[i]) c[j] in exactly that order
(include/superlu_dist_amd.h); `second_values` the new values of those tests, v (1 + k / 8) with k in {0, 1, 2, 3} by position: exact products for the case
matrices (mantissas of 53 bits times 9/8 .. 11/8 round, which is fine: the test compares against the same numpy product), and no two neighbouring entries
share a factor."""
import functools
import numpy as np
import equil_cases as ec
import trans_cases as tc

EQUIL_CASE = "dense65_B"      # the smallest equed = B case of equil_cases whose R and C are reciprocals of random mantissas, not powers of two


@functools.lru_cache(maxsize=None)
def csr_case(name):
    """(case, n, rowptr, colind, values of B in CSR order) of a sweep case, built once"""
    c = tc.prepared(name)[0]
    n, rp, ci = c.pattern_csr()
    rows = ec.rows_of(n, rp)
    v = c.B[rows, ci].copy()
    assert np.count_nonzero(c.B) == np.count_nonzero(v)          # the pattern holds all of B
    v.setflags(write=False)
    return c, n, rp, ci, v


def wrong_values(n, rp, ci, v):
    rows = ec.rows_of(n, rp)
    return np.where(rows == ci, 6, 3) * v


def second_values(n, rp, ci, v):
    rows = ec.rows_of(n, rp)
    return v * (1.0 + ((3 * rows + 5 * np.asarray(ci)) % 4) / 8.0)


def scaled_values(n, rp, ci, v, R, C):
    """(a r[i]) c[j]; R / C all ones where that side is not scaled (what LUHandle.scalings returns): a product with 1.0 is exact"""
    rows = ec.rows_of(n, rp)
    with np.errstate(over="ignore", under="ignore"):
        return (np.asarray(v) * R[rows]) * C[np.asarray(ci)]
