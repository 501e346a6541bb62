"""Complex16 batches on the device (sluamd_zBatch*, driver.ZBatchHandle): the exact cases of zbatch_cases.py bit for bit for A, A^T and A^H, strides, float
cases against the single-matrix driver, isolation of a singular matrix, value updates (host and device form), per-matrix equilibration and refinement
against a complex16 handle on each matrix alone, refusals (d / z mismatch both ways, the argument checks of the z entry points)."""
import ctypes as C
import functools
import numpy as np
import pytest
import batch_cases as bc
import zbatch_cases as zc
from superlu_dist_amd import _lib, driver

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


def _symb(c):
    return driver.Symbolic(c.m, c.rp, c.ci, None, relax=8, maxsup=c.maxsup)


def _pv(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _factored(name):
    """one factored batch per exact shape, shared by the solves below (never modified)"""
    c = zc.exact_case(name)
    s = _symb(c)
    bh = driver.ZBatchHandle.create(s, c.values)
    info = bh.factor()
    s.free()
    return c, bh, info


@pytest.mark.parametrize("name", list(zc.SHAPES))
def test_exact_cases_solve_bit_for_bit(name):
    c, bh, info = _factored(name)
    assert np.array_equal(info, np.zeros(c.count, dtype=np.int32))
    for nrhs in zc.NRHS:
        x, b, bt, bhh = c.rhs(nrhs)
        for trans, rhs in (("N", b), ("T", bt), ("C", bhh)):
            got, berr, steps = bh.solve(rhs, trans=trans)
            assert got.dtype == np.complex128 and np.array_equal(got, x), (name, nrhs, trans)
            assert berr is None and not steps.any()
    got, _, _ = bh.solve(c.rhs(1)[1][:, :, 0])                    # [count, n]
    assert np.array_equal(got, c.rhs(1)[0][:, :, 0])


def test_strides_larger_than_the_blocks():
    """stride > nnz at creation, ldb > m, strideB > ldb nrhs, strideX another one (all in values); the gaps of X come back untouched"""
    c = zc.exact_case("m100x5")
    L = _lib.load()
    s = _symb(c)
    stride = c.nnz + 7
    nz = np.full((c.count, stride), 99.0 - 98.0j); nz[:, :c.nnz] = c.values
    b = C.c_void_p()
    _lib.check(L.sluamd_zBatchCreate(C.byref(b), s._h, c.count, s.rowptr.ctypes.data_as(_lib.P_int), s.colind.ctypes.data_as(_lib.P_int), _pv(nz), stride,
                                     s.perm_c.ctypes.data_as(_lib.P_int), None), "sluamd_zBatchCreate")
    info = np.ones(c.count, dtype=np.int32)
    _lib.check(L.sluamd_zBatchFactor(b, info.ctypes.data_as(_lib.P_int)), "sluamd_zBatchFactor")
    assert not info.any()
    nrhs, ldb, ldx = 3, c.m + 3, c.m + 1
    sB, sX = ldb * nrhs + 5, ldx * nrhs + 2
    x, _, _, rhs = c.rhs(nrhs)                                   # A^H x = bh
    gap = -5.0 + 6.0j
    B = np.full(c.count * sB, -7.0 + 1.0j); X = np.full(c.count * sX, gap)
    for k in range(c.count):
        for j in range(nrhs):
            B[k * sB + j * ldb:k * sB + j * ldb + c.m] = rhs[k, :, j]
    _lib.check(L.sluamd_zBatchSolve(b, 2, _pv(B), ldb, sB, _pv(X), ldx, sX, nrhs, 0, None, None), "sluamd_zBatchSolve")
    seen = np.zeros(len(X), dtype=bool)
    for k in range(c.count):
        for j in range(nrhs):
            o = k * sX + j * ldx
            assert np.array_equal(X[o:o + c.m], x[k, :, j])
            seen[o:o + c.m] = True
    assert np.all(X[~seen] == gap)
    L.sluamd_BatchDestroy(b); s.free()


@pytest.mark.parametrize("name", ["m100x5", "m300x2"])
def test_float_cases_match_the_single_matrix_driver(name):
    c = zc.float_case(name)
    rng = np.random.default_rng(3)
    b = rng.uniform(-1, 1, size=(c.count, c.m, 3)) + 1j * rng.uniform(-1, 1, size=(c.count, c.m, 3))
    s = _symb(c)
    perm = s.perm_c.copy()
    bh = driver.ZBatchHandle.create(s, c.values)
    assert not bh.factor().any()
    x, _, _ = bh.solve(b)
    xc, _, _ = bh.solve(b, trans="C")
    bh.destroy(); s.free()
    for k in range(c.count):
        ref, info, _ = driver.pzgssvx3d(c.m, c.rp, c.ci, c.values[k], np.asfortranarray(b[k]), perm, relax=8, maxsup=c.maxsup)
        assert info == 0
        err = np.abs(x[k] - ref).max() / np.abs(ref).max()
        print(f"{name} matrix {k}: relative difference to the single-matrix driver {err:.3e}")
        assert err <= 1e-10
        rc = np.abs(c.dense[k].conj().T @ xc[k] - b[k]).max() / (np.abs(c.dense[k]).sum(axis=0).max() * np.abs(xc[k]).max())
        print(f"{name} matrix {k}: residual of the A^H solve {rc:.3e}")
        assert rc <= 1e-14


def test_singular_matrix_is_isolated():
    name, k, c0 = "m100x5", 2, 37
    c = zc.exact_case(name, singular=(k, c0))
    reg, bh_reg, _ = _factored(name)
    s = _symb(c)
    col = int(s.perm_c[c0])
    assert zc.first_zero_pivot(c.dense[k], s.perm_c) == col
    bh = driver.ZBatchHandle.create(s, c.values)
    info = bh.factor()
    expect = np.zeros(c.count, dtype=np.int32); expect[k] = col + 1
    assert np.array_equal(info, expect)
    # A_k alone gives the same info
    h = driver.LUHandle.from_symbolic(s, c.values[k])
    assert h.z and h.pdgstrf3d() == col + 1
    h.destroy()
    x, b, _, _ = reg.rhs(3)
    got, _, _ = bh.solve(b)
    same, _, _ = bh_reg.solve(b)
    for q in range(c.count):
        if q != k:
            assert np.array_equal(got[q], same[q]) and np.array_equal(got[q], x[q])
    bh.destroy(); s.free()


def _update_roundtrip(device):
    """a batch of other values, updated (host array / torch device tensor), refactored: bitwise the solutions of a fresh batch of the new values"""
    name = "m257x3"
    c0, c1 = zc.exact_case(name, seed=1), zc.exact_case(name)
    assert not np.array_equal(c0.values, c1.values)
    s = _symb(c0)
    bh = driver.ZBatchHandle.create(s, c0.values)
    assert not bh.factor().any()
    x, b, bt, bhh = c1.rhs(3)
    if device:
        import torch
        t = torch.from_numpy(c1.values.copy()).cuda()
        assert t.dtype == torch.complex128
        torch.cuda.synchronize()
        bh.update_values(t)
    else:
        bh.update_values(c1.values)
    with pytest.raises(RuntimeError, match="holds no factors"):        # a solve between update and factor is refused
        bh.solve(b)
    assert not bh.factor().any()
    fresh = _factored(name)[1]
    for trans, rhs in (("N", b), ("T", bt), ("C", bhh)):
        got = bh.solve(rhs, trans=trans)[0]
        assert np.array_equal(got, fresh.solve(rhs, trans=trans)[0]) and np.array_equal(got, x)
    bh.destroy(); s.free()
    return True


def test_update_values_host_form_equals_a_fresh_batch():
    assert _update_roundtrip(False)


_DEV_CHILD = r"""
import os, sys
import torch                                   # first: torch's HIP context must exist before the library initialises the runtime
assert torch.cuda.is_available(), "torch sees no HIP device"
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_zbatch as t
print("RESULT", t._update_roundtrip(True))
"""


def test_update_values_device_form_equals_a_fresh_batch():
    """the _dev form through a complex128 torch device tensor, in a fresh child process that initialises torch first (as test_gpu_batch.py)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _DEV_CHILD, root], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "RESULT True" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


# ---- equilibration per matrix: the recipe of test_gpu_batch._equil_values with the modulus |re| + |im| the complex equilibration takes its maxima of ----
def _equil_values(c):
    """values [count, nnz] of the complex float case with matrix 1's rows, matrix 2's columns and matrix 3's rows and columns scaled by powers of two (exact)"""
    rng = np.random.default_rng(8)
    v = c.values.copy()

    def balance(vk):                                         # row maxima of |re| + |im| into [1, 2) by exact power-of-two row scalings: rowcnd >= 1/2; and
        rowmax = np.zeros(c.m); np.maximum.at(rowmax, c.rows, zc.abs1(vk))       # colcnd >= 1/2: the real diagonal 2 sum |a| + 1 exceeds sqrt(2) |a| >= abs1(a)
        return vk * 2.0 ** -np.floor(np.log2(rowmax))[c.rows]                    # of every entry of its row, so it is the largest entry of its column too
    for k in range(c.count):
        v[k] = balance(v[k])
    pr = 2.0 ** rng.choice([-20, 0, 20], size=c.m); pcs = 2.0 ** rng.choice([-20, 0, 20], size=c.m)
    v[1] *= pr[c.rows]
    v[2] = balance(v[2] * pcs[c.ci])                         # rows balanced again, so only the columns are left to scale -> C
    v[3] = (v[3] * pr[c.rows]) * pcs[c.ci]
    return v


def _alone(c, s, vals):
    h = driver.LUHandle.from_symbolic(s, vals)
    e = h.equilibrate(c.m, c.rp, c.ci, vals, s.perm_c)
    R, Cs = h.scalings()
    h.destroy()
    return e, R, Cs


def test_equilibration_per_matrix_equals_each_matrix_alone():
    c = zc.float_case("m100x5")
    v = _equil_values(c)
    s = _symb(c)
    bh = driver.ZBatchHandle.create(s, v)
    eq = bh.equilibrate()
    R, Cs = bh.scalings()
    kinds = [e["equed"] for e in eq]
    print("equed per matrix:", kinds)
    assert kinds[0] == "N" and kinds[1] in "RB" and kinds[2] == "C" and kinds[3] in "RB" and kinds[4] == "N"
    assert R.dtype == np.float64 and Cs.dtype == np.float64
    # anorm = max column sum of the moduli hypot(re, im) of the scaled values, summed with fp64 atomics: batch and handle add the SAME terms (the same device
    # hypot of the same scaled values) in another order, each within k 2^-52 (relative) of the exact sum of those terms for a longest column of k entries
    # (sluamd_zEquilibrate): they differ by at most twice that.  numpy's terms are its own rounded moduli: the device's hypot and numpy's are each within one
    # ulp (2^-52 relative) of the true modulus, so every term, and with it any sum of them, differs by at most 2 2^-52 relative on top; the scalings are powers
    # of two and change no significand.
    col_len = np.bincount(c.ci, minlength=c.m).max()
    for k in range(c.count):
        e, Rk, Ck = _alone(c, s, v[k])
        for key in ("equed", "info", "rowcnd", "colcnd", "amax"):
            assert eq[k][key] == e[key], (k, key, eq[k][key], e[key])
        assert np.array_equal(R[k], Rk) and np.array_equal(Cs[k], Ck), k
        print(f"matrix {k}: anorm batch {eq[k]['anorm']!r} alone {e['anorm']!r}")
        assert abs(eq[k]["anorm"] - e["anorm"]) <= 2 * col_len * 2.0 ** -52 * e["anorm"], (k, eq[k]["anorm"], e["anorm"])
        A = np.zeros((c.m, c.m), dtype=np.complex128); A[c.rows, c.ci] = v[k]
        exact = np.abs((A * Rk[:, None]) * Ck[None, :]).sum(axis=0).max()
        assert abs(eq[k]["anorm"] - exact) <= (2 * col_len + 2) * 2.0 ** -52 * exact, (k, eq[k]["anorm"], exact)
    with pytest.raises(RuntimeError, match="already"):
        bh.equilibrate()
    # the solves in the caller's scaling, against each matrix alone
    assert not bh.factor().any()
    rng = np.random.default_rng(6)
    b = rng.uniform(-1, 1, size=(c.count, c.m, 3)) + 1j * rng.uniform(-1, 1, size=(c.count, c.m, 3))
    x, _, _ = bh.solve(b)
    xc, _, _ = bh.solve(b, trans="C")
    xr, berr, steps = bh.solve(b, refine=True)
    for k in range(c.count):
        ref, info, _ = driver.pzgssvx3d(c.m, c.rp, c.ci, v[k], np.asfortranarray(b[k]), s.perm_c, relax=8, maxsup=c.maxsup, equil=True)
        assert info == 0
        for got in (x[k], xr[k]):
            assert np.abs(got - ref).max() / np.abs(ref).max() <= 1e-10
        refc, info, _ = driver.pzgssvx3d(c.m, c.rp, c.ci, v[k], np.asfortranarray(b[k]), s.perm_c, relax=8, maxsup=c.maxsup, equil=True, trans="C")
        assert np.abs(xc[k] - refc).max() / np.abs(refc).max() <= 1e-10
    bh.destroy(); s.free()


# ---- refinement per matrix: the exact trajectories of zbatch_cases.refine_case against a complex16 handle on each matrix alone ----
@pytest.mark.parametrize("trans", ["N", "C"])
def test_refinement_per_matrix_equals_each_matrix_alone(trans):
    m, count, d, A, N, b = zc.refine_case(True)
    drp, dci = np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32)
    s = driver.Symbolic(m, drp, dci, None, relax=8, maxsup=64)
    perm = s.perm_c.copy()
    bh = driver.ZBatchHandle.create(s, d)
    assert not bh.factor().any()
    rp, ci, v = zc.csr(zc.block_diag(A))                    # diag(A'_0, A'_1, A'_2) attached to the batch's handle
    driver._attach_matrix(bh.handle(), True, count * m, rp, ci, v, np.concatenate([perm + k * m for k in range(count)]))
    x, berr, steps = bh.solve(b, trans=trans, refine=True)
    print(f"trans {trans}: steps", steps, "berr", berr)
    for k in range(count):
        h = driver.LUHandle.from_symbolic(s, d[k])
        assert h.pdgstrf3d() == 0
        xp = np.zeros((m, 2), dtype=np.complex128, order="F"); xp[perm, :] = b[k]
        x0 = np.asfortranarray(h.pdgstrs3d(xp, trans=trans)[perm, :])
        rpk, cik, vk = zc.csr(A[k])
        h.attach_matrix(m, rpk, cik, vk, perm)
        xs, bes, st = h.pdgsrfs3d(np.asfortranarray(b[k]), x0, trans=trans)
        h.destroy()
        assert st == steps[k]
        assert np.array_equal(bes, berr[k]) and np.array_equal(xs, x[k]), k
        for j in range(2):                                          # and both are the replay's
            xe, be, se, _ = zc.replay(d[k], A[k], b[k][:, j], trans, m)
            assert np.array_equal(x[k][:, j], xe) and berr[k, j] == be and (j == 0 or se == steps[k])
        assert np.array_equal(zc.op(A[k], trans) @ x[k], b[k])       # the nilpotent iterations ended at the exact solution
    bh.destroy(); s.free()


def test_refusals():
    L = _lib.load()
    c, cd = zc.exact_case("m40x7"), bc.exact_case("m40x7")
    s = _symb(c)
    pi = lambda a: a.ctypes.data_as(_lib.P_int)
    b, bd = C.c_void_p(), C.c_void_p()

    def create(count=c.count, stride=c.nnz, opt=None):
        return L.sluamd_zBatchCreate(C.byref(b), s._h, count, pi(s.rowptr), pi(s.colind), _pv(c.values), stride, pi(s.perm_c), opt)

    def refused(rc, word):
        assert rc == -1 and word in L.sluamd_last_error().decode(), (rc, L.sluamd_last_error())

    refused(create(count=0), "count")
    refused(create(count=-2), "count")
    refused(create(stride=c.nnz - 1), "stride")
    o = driver.LUHandle._opts(replace_tiny=True)
    refused(create(opt=C.byref(o)), "replace_tiny_pivot")
    assert not b.value
    assert create() == 0
    x, rhs, _, _ = c.rhs(1)
    B = np.ascontiguousarray(rhs[:, :, 0]); X = np.zeros_like(B)
    args = lambda h=b, ldb=c.m, ldx=c.m, trans=0, refine=0, berr=None: (h, trans, _pv(B), ldb, c.m, _pv(X), ldx, c.m, 1, refine, berr, None)
    refused(L.sluamd_zBatchSolve(*args()), "no factors")
    info = np.zeros(c.count, dtype=np.int32)
    assert L.sluamd_zBatchFactor(b, pi(info)) == 0
    refused(L.sluamd_zBatchSolve(*args(ldb=c.m - 1)), "ldb")
    refused(L.sluamd_zBatchSolve(*args(ldx=c.m - 1)), "ldx")
    refused(L.sluamd_zBatchSolve(*args(trans=3)), "trans")
    refused(L.sluamd_zBatchSolve(*args(refine=1)), "berr")
    refused(L.sluamd_zBatchUpdateValues(b, _pv(c.values), c.nnz - 1), "stride")
    # the borrowed handle is a complex16 handle: the double entry points refuse it
    assert L.sluamd_pdgstrf3d(L.sluamd_BatchHandle(b), 0.0, pi(info)) == -1
    # a d call on the complex16 batch names the z call ...
    e = (_lib.Equil * c.count)()
    Bd = np.zeros((c.count, c.m)); Xd = np.zeros_like(Bd)
    dargs = (b, 0, _pv(Bd), c.m, c.m, _pv(Xd), c.m, c.m, 1, 0, None, None)
    refused(L.sluamd_dBatchFactor(b, pi(info)), "sluamd_zBatchFactor")
    refused(L.sluamd_dBatchSolve(*dargs), "sluamd_zBatchSolve")
    refused(L.sluamd_dBatchSolve_dev(*dargs), "sluamd_zBatchSolve_dev")
    refused(L.sluamd_dBatchUpdateValues(b, _pv(cd.values), c.nnz), "sluamd_zBatchUpdateValues")
    refused(L.sluamd_dBatchUpdateValues_dev(b, _pv(cd.values), c.nnz), "sluamd_zBatchUpdateValues_dev")
    refused(L.sluamd_dBatchEquilibrate(b, e), "sluamd_zBatchEquilibrate")
    # ... and a z call on a double batch the d call
    assert L.sluamd_dBatchCreate(C.byref(bd), s._h, cd.count, pi(s.rowptr), pi(s.colind), cd.values.ctypes.data_as(_lib.P_dbl), cd.nnz, pi(s.perm_c), None) == 0
    refused(L.sluamd_zBatchFactor(bd, pi(info)), "sluamd_dBatchFactor")
    refused(L.sluamd_zBatchSolve(*args(h=bd)), "sluamd_dBatchSolve")
    refused(L.sluamd_zBatchSolve_dev(*args(h=bd)), "sluamd_dBatchSolve_dev")
    refused(L.sluamd_zBatchUpdateValues(bd, _pv(c.values), c.nnz), "sluamd_dBatchUpdateValues")
    refused(L.sluamd_zBatchUpdateValues_dev(bd, _pv(c.values), c.nnz), "sluamd_dBatchUpdateValues_dev")
    refused(L.sluamd_zBatchEquilibrate(bd, e), "sluamd_dBatchEquilibrate")
    # neither refusal disturbed the batches
    assert L.sluamd_dBatchFactor(bd, pi(info)) == 0 and not info.any()
    assert L.sluamd_zBatchSolve(*args()) == 0 and np.array_equal(X, x[:, :, 0])
    L.sluamd_BatchDestroy(b); L.sluamd_BatchDestroy(bd); s.free()
    # the Python classes: BatchHandle refuses complex values and points to ZBatchHandle; ZBatchHandle takes real values as complex ones
    s = _symb(c)
    with pytest.raises(ValueError, match="complex16"):
        driver.BatchHandle.create(s, c.values)
    zb = driver.ZBatchHandle.create(s, cd.values)
    assert not zb.factor().any()
    xr, br, _ = cd.rhs(2)
    got, _, _ = zb.solve(br)
    assert got.dtype == np.complex128 and np.array_equal(got, xr)
    zb.destroy(); s.free()


def test_python_driver():
    """pzgssvx3d_batch with equil, refine and trans = C: residuals of A^H x = b and the shapes of the per-matrix statistics"""
    c = zc.float_case("m100x5")
    rng = np.random.default_rng(4)
    b = rng.uniform(-1, 1, size=(c.count, c.m, 2)) + 1j * rng.uniform(-1, 1, size=(c.count, c.m, 2))
    x, info, st = driver.pzgssvx3d_batch(c.m, c.rp, c.ci, c.values, b, relax=8, maxsup=64, equil=True, refine=True, trans="C")
    assert not info.any() and st["berr"].shape == (c.count, 2) and st["refine_steps"].shape == (c.count,)
    assert len(st["equed"]) == c.count and not st["equil_info"].any() and st["amax"].shape == (c.count,)
    for k in range(c.count):
        A = c.dense[k].conj().T
        res = np.abs(A @ x[k] - b[k]).max() / (np.abs(A).sum(axis=1).max() * np.abs(x[k]).max())
        print(f"matrix {k}: residual {res:.3e}, berr {st['berr'][k]}")
        assert res <= 1e-14
    assert st["berr"].dtype == np.float64 and np.all(st["berr"] >= 0.0) and np.all(st["berr"] < 1.0)
