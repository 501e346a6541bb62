"""k_xrfs_residual through sluamd_[dz]Residual_dev, one pass at a time, bitwise: tests/xrefine_cases.py restates the doubled accumulation in the kernel's
order (the product errors from fractions.Fraction, the sums in IEEE doubles) on data where that restatement is the exact residual (checked on the CPU:
test_xrefine_cases_cpu.py and `check_case` below).  Orders at the edges of the 256-thread workgroup; rows of 0, 1, 3 and 70 entries; a row whose fp64 sum
loses the answer (2^60, 1, -2^60); rows whose one product is not a double, wrong by a factor 2 if s - a x is contracted into one multiply-add; the maximum q
at every position of MAXPOS; trans N / T (double) and N / T / C (complex16), the latter two through the transposed index.  Every comparison is on bit
patterns."""
import numpy as np
import pytest
import xrefine_cases as xc

pytestmark = pytest.mark.gpu
KEYS = [(n, z) for z in (False, True) for n in xc.ORDERS]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("key", KEYS, ids=lambda k: "n%d-%s" % (k[0], "z" if k[1] else "d"))
def test_residual_dev_is_the_restatement_bitwise(key):
    n, z = key
    h = xc.factored("diag", n, z)
    dt = np.complex128 if z else np.float64
    pc = xc.rx.perm(n)
    for nn, m in xc.xcase_list():
        if nn != n:
            continue
        c = xc.xcase(n, z, m)
        for trans in xc.TRANS[z]:
            xc.check_case(c, trans)
            e = c.expected(trans)
            h.attach_matrix(n, *c.attached(trans), pc)
            # ldb = n + 3, ldx = n + 5, ldr = n + 2: the padding rows of R must come back untouched
            B = np.zeros((n + 3, 1), dtype=dt, order="F"); B[:n, 0] = c.b
            X = np.zeros((n + 5, 1), dtype=dt, order="F"); X[:n, 0] = c.x
            got = {}
            for extra in (1, 0):
                R0 = np.full((n + 2, 1), np.nan, dtype=dt, order="F")
                dB, dX, dR = xc.Dev(B), xc.Dev(X), xc.Dev(R0)
                berr = h.residual_dev(dB.ptr.value, n + 3, dX.ptr.value, n + 5, 1, dR.ptr.value, n + 2, trans=trans, extra=bool(extra))
                R = dR.host()
                assert np.array_equal(_bits(dB.host()), _bits(B)) and np.array_equal(_bits(dX.host()), _bits(X))
                for d in (dB, dX, dR):
                    d.free()
                assert np.array_equal(_bits(R[n:]), _bits(R0[n:])), (n, m, trans, extra)
                got[extra] = (R[:n, 0], berr[0])
            what = (n, m, trans)
            bad = np.flatnonzero(_bits(got[1][0]) != _bits(e["extra"]))
            assert bad.size == 0, (what, "extra differs at rows", bad[:8].tolist(), got[1][0][bad[:4]], e["extra"][bad[:4]])
            bad = np.flatnonzero(_bits(got[0][0]) != _bits(e["plain"]))
            assert bad.size == 0, (what, "plain differs at rows", bad[:8].tolist())
            assert got[1][1] == e["berr_extra"] and got[0][1] == e["berr_plain"], (what, got[1][1], e["berr_extra"], got[0][1], e["berr_plain"])
            assert not np.array_equal(_bits(got[0][0]), _bits(got[1][0]))
    h.destroy()


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_host_form_columns_and_null_berr(z):
    """sluamd_[dz]Residual on host arrays: two columns (the case and the case with x = 0: r = b), LUHandle.residual's return value"""
    n = 257
    c = xc.xcase(n, z, 137)
    h = xc.factored("diag", n, z)
    h.attach_matrix(n, *c.attached("N"), xc.rx.perm(n))
    e = c.expected("N")
    B = np.stack([c.b, c.b], axis=1)
    X = np.stack([c.x, np.zeros_like(c.x)], axis=1)
    r, berr = h.residual(B, X, extra=True)
    assert np.array_equal(_bits(r[:, 0]), _bits(e["extra"])) and np.array_equal(_bits(r[:, 1]), _bits(c.b)) and berr[0] == e["berr_extra"]
    r1, berr1 = h.residual(c.b, c.x)
    assert r1.shape == (n,) and np.array_equal(_bits(r1), _bits(e["plain"])) and berr1[0] == e["berr_plain"]
    h.destroy()
