"""CPU checks behind tests/test_gpu_trans_solve.py: the exactness bounds of the transposed right-hand sides (trans_cases.rhs_t) hold for every case and
nrhs the GPU file runs, an independent solver recovers x from them, and a build of the library without the transposed sweeps (the CPU test build of the
host sources) says so by name instead of solving something else."""
import os, subprocess, sys
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import trans_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, r, False) for n in tc.D_CASES for r in tc.NRHS] + [(n, r, cj) for n in tc.Z_CASES for r in tc.Z_NRHS for cj in (False, True)] \
    + [("groups", r, False) for r in tc.GROUPS_NRHS]


def test_no_case_needed_a_narrowed_x():
    assert not tc.NARROW


@pytest.mark.parametrize("name", sorted({c[0] for c in CASES}))
def test_bounds_of_the_transposed_sweeps_hold(name):
    """every (nrhs, conj) the GPU tests run on this case: both sweep bounds below 2^53 with the margin of 64 (rhs_t asserts; the margin left is reported)"""
    c = tc.prepared(name)[0]
    worst = 0
    for n_, nrhs, conj in CASES:
        if n_ != name:
            continue
        x, b = tc.rhs_t(c, nrhs, conj)
        assert x.shape == b.shape == (c.n, nrhs)
        worst = max(worst, *tc.bounds_t(c, nrhs, conj))
    assert 0 < worst < tc.LIMIT
    print(f"{name}: largest scaled bound 2^{np.log2(worst):.1f} of 2^53")


@pytest.mark.parametrize("name", ["widths", "narrow", "levels", "z_wide", "z_levels"])
def test_independent_solvers_recover_x(name):
    """b_t really is the right-hand side of the transposed system with solution x, by routes that share nothing with rhs_t's integer products:
    (1) B^T x == b_t exactly with the dense B of fill() (every operand a small multiple of 2^-4: the float product is exact);
    (2) scipy.linalg.solve_triangular on U0^T, then on L0^T (unit), returns x EXACTLY (substitution on the bidiagonal / scaled-ones blocks is exact);
    (3) scipy.sparse.linalg.spsolve(B^T, b_t), a pivoting LU that knows nothing of L0 and U0.  These matrices are built for exact UNPIVOTED elimination,
        not for conditioning, and spsolve's own error on them is large: on the UNTRANSPOSED system B x = b it misses x by 1.6e3 (widths), 5.8e1 (narrow),
        1.2e6 (levels), 2.3e-5 (z_wide), 9.7e-6 (z_levels).  Its error on B x = b of the same case is therefore the yardstick: the transposed solve may
        miss x by at most ten times that (floor n eps |x|) -- asserted where spsolve's untransposed error leaves a meaningful statement (z_wide, z_levels,
        levels); for widths and narrow (transposed error 2.3e4 and 8.8e2, 14 and 15 times the untransposed one) the figures are printed only."""
    import scipy.linalg as la
    c = tc.prepared(name)[0]
    for conj in ((False, True) if c.z else (False,)):
        x, b = tc.rhs_t(c, 3, conj)
        Bt = c.B.conj().T if conj else c.B.T
        assert np.array_equal(Bt @ x, b), (name, conj)
        U0t, L0t = (c.U0.conj().T, c.L0.conj().T) if conj else (c.U0.T, c.L0.T)
        y = la.solve_triangular(U0t, b, lower=True)
        assert np.array_equal(la.solve_triangular(L0t, y, lower=False, unit_diagonal=True), x), (name, conj)
        x0, b0 = c.rhs(3)
        e_n = float(np.abs(spla.spsolve(sp.csc_matrix(c.B), b0) - x0).max())
        e_t = float(np.abs(spla.spsolve(sp.csc_matrix(Bt), b) - x).max())
        print(f"{name} conj={conj}: spsolve misses x by {e_t:.3g} (transposed), {e_n:.3g} (untransposed)")
        if name in ("levels", "z_wide", "z_levels"):
            assert e_t <= 10 * max(e_n, c.n * np.finfo(float).eps * np.abs(x).max()), (name, conj, e_t, e_n)
    if c.z:                                                                                # the Gaussian-integer phases make T and C different systems
        assert not np.array_equal(tc.rhs_t(c, 3, False)[1], tc.rhs_t(c, 3, True)[1])


CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
from superlu_dist_amd import _lib, driver, matgen
assert "emul" in _lib.load()._name
n, rp, ci, v = matgen.poisson3d(4)
symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=4, maxsup=16)
h = driver.LUHandle.from_symbolic(symb, v)
assert h.pdgstrf3d(0.0) == 0
b = np.ones((n, 1))
x = h.pdgstrs3d(b)                                   # the default, trans = "N", solves here
A = np.zeros((n, n)); A[np.repeat(np.arange(n), np.diff(rp)), ci] = v
assert np.abs(A @ x - b).max() < 1e-12
assert np.array_equal(h.pdgstrs3d(b, trans="N"), x)
try:
    h.pdgstrs3d(b, trans="T")
    print("RESULT solved")
except RuntimeError as e:
    print("RESULT " + str(e))
"""


def test_a_library_without_the_transposed_sweeps_names_the_missing_entry_point(emul):
    so = os.path.join(ROOT, "oracle", "libsluamd_emul.so")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=dict(os.environ, SLUAMD_LIB=so), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1500:]
    res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    assert "sluamd_pdgstrs3d_trans" in res and "missing" in res, res


def test_trans_argument_is_validated():
    from superlu_dist_amd import driver
    with pytest.raises(ValueError):
        driver._trans_code("X")
    assert [driver._trans_code(t) for t in ("N", "t", "C")] == [0, 1, 2]
