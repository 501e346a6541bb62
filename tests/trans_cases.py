"""Right-hand sides of the TRANSPOSED and CONJUGATE-TRANSPOSED systems of the exact sweep cases (test helper for test_gpu_trans_solve.py and
test_trans_cases_cpu.py; not a conftest).

sweep_cases.SweepCase.fill() leaves exact L0, U0, B = L0 U0 and the scaled integer images L4 = 4 L0, U4 = 4 U0 with their absolute values aL, aU and
those of the diagonal-block inverses, aLi (scaled by 4) and aUi (scaled by 16).  The transposed solve (L0 U0)^T x = b_t runs U0^T y_t = b_t forward and
L0^T x = y_t backward, so with the integer x of SweepCase.rhs():
    y_t = op(L0)^T x,   b_t = op(U0)^T y_t          (op = identity, or the conjugate for the conjugate transpose)
are formed from the integer images, y4 = op(L4)^T x and b16 = op(U4)^T y4.

Bounds (the transposes of those of SweepCase.rhs, in Python integers): every partial sum of the transposed sweeps is bounded, entry by entry, by
    forward:   aUi^T (|b_t| + aU^T |y_t|)           (diagonal step Uinv^T applied to the right-hand side minus the updates, each bounded by absolute values)
    backward:  aLi^T (|y_t| + aL^T |x|)
With the operands scaled to integers -- 16 |b_t| = |b16|, 4 |y_t| = |y4| -- the forward bound carries a factor 16 * 16 and the backward one 4 * 4.  The
values of the forward sweep are multiples of 2^-8 (U0 and y_t in 2^-2, Uinv in 2^-4) and those of the backward sweep of 2^-4 (L0, Linv in 2^-2), so the
scaled bounds ARE the bounds in units of the last place: below 2^53 every partial sum of ANY summation order (lanes, waves, atomics) is an exact double
and the device must return x itself.  The helper asserts them with the further factor 64 that SweepCase.rhs keeps as a margin.
The complex16 cases substitute on the factored blocks instead of multiplying with inverses; the intermediate values of a substitution on a bidiagonal
inverse's dense triangle are the partial sums of the same products, covered by the same bound through aUi / aLi (|re| + |im| bounds both parts).

Should a case miss a bound, `narrow=True` restricts x to {-1, 0, 1}; no case of the GPU tests needs it (NARROW is empty, asserted by the CPU tests)."""
import functools
import numpy as np
import sweep_cases as sw

LIMIT = sw.LIMIT
NARROW = set()                                     # names of cases whose x had to be narrowed to {-1, 0, 1}: none

# what tests/test_gpu_trans_solve.py runs (the CPU tests evaluate the bounds for exactly these)
D_CASES = ("widths", "narrow", "wide_launch", "levels")
Z_CASES = ("z_narrow", "z_wide", "z_levels")
NRHS = (1, 2, 3, 4, 5, 17, 97)
Z_NRHS = (1, 2, 5)
GROUPS_NRHS = (1, 3, 5)


def _abs(v, z):
    return np.abs(v.real).astype(np.int64) + (np.abs(v.imag).astype(np.int64) if z else 0)


def _system(case, nrhs, conj, narrow):
    """integer x, b16 = 16 b_t and the two scaled sweep bounds (Python integers, the margin factor 64 included)"""
    z = case.z
    x = case.rhs(nrhs)[0]
    x = np.rint(x.real).astype(np.int64) + (1j * np.rint(x.imag) if z else 0)
    if narrow:
        x = np.sign(x.real).astype(np.int64) + (1j * np.sign(x.imag) if z else 0)
        assert np.unique(x, axis=1).shape[1] == nrhs
    op = (lambda M: M.conj()) if (z and conj) else (lambda M: M)
    y4 = op(case.L4).T.tocsr() @ x
    b16 = op(case.U4).T.tocsr() @ y4
    ax, ay, ab = _abs(x, z), _abs(y4, z), _abs(b16, z)
    fwd = case.aUi.T.tocsr() @ (ab + case.aU.T.tocsr() @ ay)          # 16 * 16 * aUi^T (|b_t| + aU^T |y_t|)
    bwd = case.aLi.T.tocsr() @ (ay + case.aL.T.tocsr() @ ax)          # 4 * 4 * aLi^T (|y_t| + aL^T |x|)
    return x, b16, (int(fwd.max()) * 64, int(bwd.max()) * 64)


def bounds_t(case, nrhs, conj=False, narrow=None):
    """the two bounds of rhs_t as Python integers (for reporting the margin)"""
    return _system(case, nrhs, conj, (case.name in NARROW) if narrow is None else narrow)[2]


def rhs_t(case, nrhs, conj=False, narrow=None):
    """(x, b_t) of a filled SweepCase: the integer x of case.rhs(nrhs) and b_t = op(U0)^T op(L0)^T x; the bounds of the transposed sweeps asserted"""
    x, b16, bounds = _system(case, nrhs, conj, (case.name in NARROW) if narrow is None else narrow)
    assert bounds[0] < LIMIT and bounds[1] < LIMIT, (case.name, nrhs, conj, bounds)
    vt = np.complex128 if case.z else np.float64
    return np.asfortranarray(x.astype(vt)), np.asfortranarray(b16.astype(vt) / 16)


@functools.lru_cache(maxsize=None)
def prepared(name):
    """(case, flat store holding B, expected Lnzval, expected Unzval, DAG level sizes) of a sweep case: built once, host code only"""
    import schur_cases as sc
    from superlu_dist_amd import driver
    c = sw.CASES[name]()
    n, rp, ci = c.pattern_csr()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    assert symb.xsup().tolist() == c.xsup.tolist()
    fs = symb.flat_store(values=False)
    symb.free()
    expL, expU = c.fill(fs)
    return c, fs, expL, expU, sw.level_sizes(sw.levels_of(sc.sources(fs)))


def predicted_launches_t(sizes, nrhs, chunk):
    """stats()["solve_launches"] of a transposed solve (sluamd_tsolve.cpp): per chunk of right-hand sides one diagonal and one update launch per DAG
    level and sweep.  stats() reports the launches of all chunks of the last solve."""
    return 4 * len(sizes) * -(-nrhs // chunk)


def max_rhs_chunk(max_width, z=False):
    """max_rhs_chunk (sluamd_factor.cpp): x_k of the widest supernode in 96 KiB of LDS"""
    return max(1, (96 * 1024) // (max_width * (16 if z else 8)))
