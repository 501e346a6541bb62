"""Batches of same-pattern systems on the device (sluamd_dBatch*), through the C ABI: exact cases (batch_cases.py) bit for bit, float cases against the
single-matrix driver, isolation of a singular matrix, value updates, per-matrix refinement against sluamd_pdgsrfs3d on each matrix alone, refusals, and the
Python driver, per-matrix equilibration against LUHandle.equilibrate on each matrix alone."""
import ctypes as C
import functools
import numpy as np
import pytest
import batch_cases as bc
from superlu_dist_amd import _lib, driver

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


def _symb(c):
    return driver.Symbolic(c.m, c.rp, c.ci, None, relax=8, maxsup=c.maxsup)


@functools.lru_cache(maxsize=None)
def _factored(name):
    """one factored batch per exact shape, shared by the solves below (never modified)"""
    c = bc.exact_case(name)
    s = _symb(c)
    bh = driver.BatchHandle.create(s, c.values)
    info = bh.factor()
    s.free()
    return c, bh, info


@pytest.mark.parametrize("name", list(bc.SHAPES))
def test_exact_cases_solve_bit_for_bit(name):
    c, bh, info = _factored(name)
    assert np.array_equal(info, np.zeros(c.count, dtype=np.int32))
    for nrhs in bc.NRHS:
        x, b, bt = c.rhs(nrhs)
        for trans, rhs in (("N", b), ("T", bt)):
            got, berr, steps = bh.solve(rhs, trans=trans)
            assert np.array_equal(got, x), (name, nrhs, trans)
            assert berr is None and not steps.any()
    got, _, _ = bh.solve(c.rhs(1)[1][:, :, 0])                    # [count, n]
    assert np.array_equal(got, c.rhs(1)[0][:, :, 0])


def test_strides_larger_than_the_blocks():
    """stride > nnz at creation, ldb > m, strideB > ldb nrhs, strideX another one; the gaps of X come back untouched"""
    c = bc.exact_case("m100x5")
    L = _lib.load()
    s = _symb(c)
    stride = c.nnz + 7
    nz = np.full((c.count, stride), 99.0); nz[:, :c.nnz] = c.values
    b = C.c_void_p()
    _lib.check(L.sluamd_dBatchCreate(C.byref(b), s._h, c.count, s.rowptr.ctypes.data_as(_lib.P_int), s.colind.ctypes.data_as(_lib.P_int),
                                     nz.ctypes.data_as(_lib.P_dbl), stride, s.perm_c.ctypes.data_as(_lib.P_int), None), "sluamd_dBatchCreate")
    info = np.ones(c.count, dtype=np.int32)
    _lib.check(L.sluamd_dBatchFactor(b, info.ctypes.data_as(_lib.P_int)), "sluamd_dBatchFactor")
    assert not info.any()
    nrhs, ldb, ldx = 3, c.m + 3, c.m + 1
    sB, sX = ldb * nrhs + 5, ldx * nrhs + 2
    x, rhs, _ = c.rhs(nrhs)
    B = np.full(c.count * sB, -7.0); X = np.full(c.count * sX, -5.0)
    for k in range(c.count):
        for j in range(nrhs):
            B[k * sB + j * ldb:k * sB + j * ldb + c.m] = rhs[k, :, j]
    _lib.check(L.sluamd_dBatchSolve(b, 0, B.ctypes.data_as(C.c_void_p), ldb, sB, X.ctypes.data_as(C.c_void_p), ldx, sX, nrhs, 0, None, None), "sluamd_dBatchSolve")
    seen = np.zeros(len(X), dtype=bool)
    for k in range(c.count):
        for j in range(nrhs):
            o = k * sX + j * ldx
            assert np.array_equal(X[o:o + c.m], x[k, :, j])
            seen[o:o + c.m] = True
    assert np.all(X[~seen] == -5.0)
    L.sluamd_BatchDestroy(b); s.free()


@pytest.mark.parametrize("name", ["m100x5", "m300x2"])
def test_float_cases_match_the_single_matrix_driver(name):
    c = bc.float_case(name)
    rng = np.random.default_rng(3)
    b = rng.uniform(-1, 1, size=(c.count, c.m, 3))
    s = _symb(c)
    perm = s.perm_c.copy()
    bh = driver.BatchHandle.create(s, c.values)
    assert not bh.factor().any()
    x, _, _ = bh.solve(b)
    xt, _, _ = bh.solve(b, trans="T")
    bh.destroy(); s.free()
    for k in range(c.count):
        ref, info, _ = driver.pdgssvx3d(c.m, c.rp, c.ci, c.values[k], np.asfortranarray(b[k]), perm, relax=8, maxsup=c.maxsup)
        assert info == 0
        err = np.abs(x[k] - ref).max() / np.abs(ref).max()
        print(f"{name} matrix {k}: relative difference to the single-matrix driver {err:.3e}")
        assert err <= 1e-10
        rt = np.abs(c.dense[k].T @ xt[k] - b[k]).max() / (np.abs(c.dense[k]).sum(axis=0).max() * np.abs(xt[k]).max())
        assert rt <= 1e-14


def test_singular_matrix_is_isolated():
    name, k, c0 = "m100x5", 2, 37
    c = bc.exact_case(name, singular=(k, c0))
    reg, bh_reg, _ = _factored(name)
    s = _symb(c)
    col = int(s.perm_c[c0])
    assert bc.first_zero_pivot(c.dense[k], s.perm_c) == col
    bh = driver.BatchHandle.create(s, c.values)
    info = bh.factor()
    expect = np.zeros(c.count, dtype=np.int32); expect[k] = col + 1
    assert np.array_equal(info, expect)
    # A_k alone gives the same info
    h = driver.LUHandle.from_symbolic(s, c.values[k])
    assert h.pdgstrf3d() == col + 1
    h.destroy()
    x, b, _ = reg.rhs(3)
    got, _, _ = bh.solve(b)
    same, _, _ = bh_reg.solve(b)
    for q in range(c.count):
        if q != k:
            assert np.array_equal(got[q], same[q]) and np.array_equal(got[q], x[q])
    bh.destroy(); s.free()


def _update_roundtrip(device):
    """a batch of other values, updated (host array / torch device tensor), refactored: bitwise the solutions of a fresh batch of the new values"""
    name = "m257x3"
    c0, c1 = bc.exact_case(name, seed=1), bc.exact_case(name)
    assert not np.array_equal(c0.values, c1.values)
    s = _symb(c0)
    bh = driver.BatchHandle.create(s, c0.values)
    assert not bh.factor().any()
    x, b, bt = c1.rhs(3)
    if device:
        import torch
        t = torch.from_numpy(c1.values.copy()).cuda()
        torch.cuda.synchronize()
        bh.update_values(t)
    else:
        bh.update_values(c1.values)
    with pytest.raises(RuntimeError, match="holds no factors"):        # a solve between update and factor is refused
        bh.solve(b)
    assert not bh.factor().any()
    fresh = _factored(name)[1]
    for trans, rhs in (("N", b), ("T", bt)):
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
import test_gpu_batch as t
print("RESULT", t._update_roundtrip(True))
"""


def test_update_values_device_form_equals_a_fresh_batch():
    """the _dev form through a torch device tensor, in a child process that initialises torch first (torch.cuda reports no device once the library has
    initialised the HIP runtime in the process: test_gpu_update_values.py)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _DEV_CHILD, root], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "RESULT True" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


# ---- refinement: the attached matrix differs from the factored one (the construction of refine_exact_cases.py), so the trajectory is known exactly ----
# Factored: F_k = diag(d_k), signed powers of two.  Attached: A'_k = F_k (I + E_k), E_k = 2^-8 N_k with N_k nilpotent: the iteration
# x <- x + F^-1 (b - A' x) started from x0 = F^-1 b reaches the solution after p - 1 steps when N^p = 0, every iterate a dyadic number of a few bits.
#   matrix 0: E = 0: berr = 0 at once, 0 steps.
#   matrix 1: N^4 = 0 != N^3 (links i -> i + 1 inside groups of four): berr 2^-8-ish, 2^-16-ish, 2^-24-ish, 0: 3 steps.
#   matrix 2: N^2 = 0 and b of the order 2^-1000, below SAFE2: every row takes the (SAFE1 + |r|) / t branch.  After one step r = 0 and berr = SAFE1 / t,
#             which still exceeds eps and is less than half the previous one: a second step, then the same berr: stop after 2 steps.  SAFE1 = (m + 1) safmin:
#             taken from count m it changes berr of both later sweeps.
RM = 100


def _refine_case():
    m, count = RM, 3
    rng = np.random.default_rng(9)
    d = rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], size=(count, m))
    N = np.zeros((count, m, m))
    i = np.arange(m - 1)
    chain = i[(i % 4) != 3]
    N[1, chain, chain + 1] = rng.choice([-1.0, 1.0], size=len(chain))
    ev = i[(i % 2) == 0]
    N[2, ev, ev + 1] = rng.choice([-1.0, 1.0], size=len(ev))
    A = np.stack([np.diag(d[k]) @ (np.eye(m) + N[k] / 256.0) for k in range(count)])
    b = rng.integers(1, 8, size=(count, m, 2)).astype(np.float64)
    b[:, :, 0] *= 2.0
    b[2] *= 2.0 ** -1000
    return m, count, d, A, b


def _csr(A):
    rows, cols = np.nonzero(A)
    rp = np.zeros(A.shape[0] + 1, dtype=np.int32); np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp).astype(np.int32), cols.astype(np.int32), A[rows, cols]


def test_refinement_per_matrix_equals_each_matrix_alone():
    m, count, d, A, b = _refine_case()
    drp, dci = np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32)
    s = driver.Symbolic(m, drp, dci, None, relax=8, maxsup=64)
    perm = s.perm_c.copy()
    bh = driver.BatchHandle.create(s, d)
    assert not bh.factor().any()
    # attach diag(A'_0, A'_1, A'_2) to the batch's handle
    big = np.zeros((count * m, count * m))
    for k in range(count):
        big[k * m:(k + 1) * m, k * m:(k + 1) * m] = A[k]
    rp, ci, v = _csr(big)
    driver._attach_matrix(bh.handle(), False, count * m, rp, ci, v, np.concatenate([perm + k * m for k in range(count)]))
    x, berr, steps = bh.solve(b, refine=True)
    print("batch refinement: steps", steps, "berr", berr)
    assert list(steps) == [0, 3, 2]
    assert berr[0, 1] == 0.0
    for k in range(count):
        h = driver.LUHandle.from_symbolic(s, d[k])
        assert h.pdgstrf3d() == 0
        xp = np.zeros((m, 2), order="F"); xp[perm, :] = b[k]
        x0 = h.pdgstrs3d(xp)[perm, :]
        rpk, cik, vk = _csr(A[k])
        h.attach_matrix(m, rpk, cik, vk, perm)
        xs, bes, st = h.pdgsrfs3d(np.asfortranarray(b[k]), x0)
        h.destroy()
        assert st == steps[k]
        assert np.array_equal(bes, berr[k]) and np.array_equal(xs, x[k]), k
        assert np.array_equal(A[k] @ x[k], b[k])                     # the nilpotent iterations ended at the exact solution
    # SAFE1 from m, not from count m
    safe1 = (m + 1) * 2.0 ** -1022
    t = np.abs(A[2]) @ np.abs(x[2][:, 1]) + np.abs(b[2][:, 1])
    assert berr[2, 1] == (safe1 / t).max() and berr[2, 1] != ((count * m + 1) * 2.0 ** -1022 / t).max()
    bh.destroy(); s.free()


def test_refusals():
    L = _lib.load()
    c = bc.exact_case("m40x7")
    s = _symb(c)
    pi = lambda a: a.ctypes.data_as(_lib.P_int)
    b = C.c_void_p()

    def create(count=c.count, stride=c.nnz, opt=None):
        return L.sluamd_dBatchCreate(C.byref(b), s._h, count, pi(s.rowptr), pi(s.colind), c.values.ctypes.data_as(_lib.P_dbl), stride, pi(s.perm_c), opt)

    def refused(rc, word):
        assert rc == -1 and word in L.sluamd_last_error().decode(), (rc, L.sluamd_last_error())

    refused(create(count=0), "count")
    refused(create(count=-2), "count")
    refused(create(stride=c.nnz - 1), "stride")
    o = driver.LUHandle._opts(replace_tiny=True)
    refused(create(opt=C.byref(o)), "replace_tiny_pivot")
    assert not b.value
    assert create() == 0
    x, rhs, _ = c.rhs(1)
    B = np.ascontiguousarray(rhs[:, :, 0]); X = np.zeros_like(B)
    args = lambda ldb=c.m, ldx=c.m, trans=0, refine=0, berr=None: (b, trans, B.ctypes.data_as(C.c_void_p), ldb, c.m, X.ctypes.data_as(C.c_void_p), ldx, c.m, 1, refine, berr, None)
    refused(L.sluamd_dBatchSolve(*args()), "no factors")
    info = np.zeros(c.count, dtype=np.int32)
    assert L.sluamd_dBatchFactor(b, pi(info)) == 0
    refused(L.sluamd_dBatchSolve(*args(ldb=c.m - 1)), "ldb")
    refused(L.sluamd_dBatchSolve(*args(ldx=c.m - 1)), "ldx")
    refused(L.sluamd_dBatchSolve(*args(trans=3)), "trans")
    refused(L.sluamd_dBatchSolve(*args(refine=1)), "berr")
    refused(L.sluamd_dBatchUpdateValues(b, c.values.ctypes.data_as(C.c_void_p), c.nnz - 1), "stride")
    # the borrowed handle is a double handle: the complex16 entry points refuse it
    assert L.sluamd_pzgstrf3d(L.sluamd_BatchHandle(b), 0.0, pi(info)) == -1
    assert L.sluamd_dBatchSolve(*args()) == 0 and np.array_equal(X, x[:, :, 0])
    L.sluamd_BatchDestroy(b); s.free()


def test_python_driver_with_refinement():
    c = bc.float_case("m100x5")
    rng = np.random.default_rng(4)
    b = rng.uniform(-1, 1, size=(c.count, c.m, 2))
    x, info, st = driver.pdgssvx3d_batch(c.m, c.rp, c.ci, c.values, b, relax=8, maxsup=64, equil=True, refine=True)
    assert not info.any() and st["berr"].shape == (c.count, 2) and st["refine_steps"].shape == (c.count,)
    assert len(st["equed"]) == c.count and not st["equil_info"].any() and st["amax"].shape == (c.count,)
    for k in range(c.count):
        A = c.dense[k]
        res = np.abs(A @ x[k] - b[k]).max() / (np.abs(A).sum(axis=1).max() * np.abs(x[k]).max())
        print(f"matrix {k}: residual {res:.3e}, berr {st['berr'][k]}")
        assert res <= 1e-14
    assert np.all(st["berr"] <= 4 * EPS)


# ---- equilibration per matrix: rows scaled by 2^+-20 (-> R or B), columns scaled (-> C), untouched (-> N), one matrix with a zero row ----
def _equil_values(c):
    """values [count, nnz] of the float case with matrix 1's rows, matrix 2's columns and matrix 3's rows and columns scaled by powers of two (exact)"""
    rng = np.random.default_rng(8)
    v = c.values.copy()
    for k in range(c.count):                                 # every matrix starts with row maxima in [1, 2) (exact power-of-two row scalings): rowcnd and
        rowmax = np.zeros(c.m); np.maximum.at(rowmax, c.rows, np.abs(v[k]))      # colcnd >= 1/2 (the diagonal is each column's largest entry), equed = N
        v[k] *= 2.0 ** -np.floor(np.log2(rowmax))[c.rows]
    pr = 2.0 ** rng.choice([-20, 0, 20], size=c.m); pcs = 2.0 ** rng.choice([-20, 0, 20], size=c.m)
    v[1] *= pr[c.rows]
    v[2] *= pcs[c.ci]
    rowmax = np.zeros(c.m); np.maximum.at(rowmax, c.rows, np.abs(v[2]))
    v[2] *= 2.0 ** -np.floor(np.log2(rowmax))[c.rows]        # rows balanced to maxima in [1, 2): rowcnd >= 1/2, so only the columns are left to scale -> C
    v[3] = (v[3] * pr[c.rows]) * pcs[c.ci]
    return v


def _alone(c, s, vals):
    h = driver.LUHandle.from_symbolic(s, vals)
    e = h.equilibrate(c.m, c.rp, c.ci, vals, s.perm_c)
    R, Cs = h.scalings()
    h.destroy()
    return e, R, Cs


def test_equilibration_per_matrix_equals_each_matrix_alone():
    c = bc.float_case("m100x5")
    v = _equil_values(c)
    s = _symb(c)
    bh = driver.BatchHandle.create(s, v)
    eq = bh.equilibrate()
    R, Cs = bh.scalings()
    kinds = [e["equed"] for e in eq]
    print("equed per matrix:", kinds)
    assert kinds[0] == "N" and kinds[1] in "RB" and kinds[2] == "C" and kinds[3] in "RB" and kinds[4] == "N"
    # anorm is summed with fp64 atomics: each result is within k 2^-52 (relative) of the exact sum for a longest column of k entries (sluamd_dEquilibrate), so
    # two such results, or one and numpy's own rounded sum, differ by at most twice that
    col_len = np.bincount(c.ci, minlength=c.m).max()
    for k in range(c.count):
        e, Rk, Ck = _alone(c, s, v[k])
        for key in ("equed", "info", "rowcnd", "colcnd", "amax"):
            assert eq[k][key] == e[key], (k, key, eq[k][key], e[key])
        assert np.array_equal(R[k], Rk) and np.array_equal(Cs[k], Ck), k
        # anorm: fp64 atomic sums, relative error <= k 2^-52 for a longest column of k entries on either side (sluamd_dEquilibrate)
        assert abs(eq[k]["anorm"] - e["anorm"]) <= 2 * col_len * 2.0 ** -52 * e["anorm"], (k, eq[k]["anorm"], e["anorm"])
        exact = np.abs((c_dense(c, v[k]) * Rk[:, None]) * Ck[None, :]).sum(axis=0).max()
        assert abs(eq[k]["anorm"] - exact) <= 2 * col_len * 2.0 ** -52 * exact
    with pytest.raises(RuntimeError, match="already"):
        bh.equilibrate()
    # the solve in the caller's scaling, against each matrix alone
    assert not bh.factor().any()
    rng = np.random.default_rng(6)
    b = rng.uniform(-1, 1, size=(c.count, c.m, 3))
    x, _, _ = bh.solve(b)
    xt, _, _ = bh.solve(b, trans="T")
    xr, berr, steps = bh.solve(b, refine=True)
    for k in range(c.count):
        ref, info, _ = driver.pdgssvx3d(c.m, c.rp, c.ci, v[k], np.asfortranarray(b[k]), s.perm_c, relax=8, maxsup=c.maxsup, equil=True)
        assert info == 0
        for got in (x[k], xr[k]):
            assert np.abs(got - ref).max() / np.abs(ref).max() <= 1e-10
        reft, info, _ = driver.pdgssvx3d(c.m, c.rp, c.ci, v[k], np.asfortranarray(b[k]), s.perm_c, relax=8, maxsup=c.maxsup, equil=True, trans="T")
        assert np.abs(xt[k] - reft).max() / np.abs(reft).max() <= 1e-10
    # new values of the same pattern re-apply the stored R / C: bitwise a fresh equilibrated batch would not be (R, C are kept), so against numpy's (a r) c
    v2 = v * 1.25
    bh.update_values(v2)
    assert not bh.factor().any()
    x2, _, _ = bh.solve(b)
    assert np.abs(x2 * 1.25 - x).max() <= 1e-10 * np.abs(x).max()
    bh.destroy(); s.free()


def c_dense(c, vals):
    A = np.zeros((c.m, c.m)); A[c.rows, c.ci] = vals
    return A


def test_equilibration_zero_row_in_one_matrix():
    c = bc.float_case("m100x5")
    v = _equil_values(c)
    row = 41
    v[2, c.rows == row] = 0.0
    s = _symb(c)
    bh = driver.BatchHandle.create(s, v)
    eq = bh.equilibrate()
    R, Cs = bh.scalings()
    assert eq[2]["info"] == row + 1 and eq[2]["equed"] == "N" and eq[2]["rowcnd"] == 0.0 and eq[2]["colcnd"] == 0.0
    assert np.all(R[2] == 1.0) and np.all(Cs[2] == 1.0)
    e2, _, _ = _alone(c, s, v[2])
    assert (e2["info"], e2["equed"], e2["amax"]) == (eq[2]["info"], eq[2]["equed"], eq[2]["amax"])
    for k in (0, 1, 3, 4):                                  # the others are scaled as they would be alone
        e, Rk, Ck = _alone(c, s, v[k])
        assert eq[k]["info"] == 0 and eq[k]["equed"] == e["equed"] and np.array_equal(R[k], Rk) and np.array_equal(Cs[k], Ck)
    assert eq[1]["equed"] in "RB" and eq[3]["equed"] in "RB"
    bh.destroy(); s.free()


def test_complex_values_and_foreign_handle_state_are_refused():
    c = bc.exact_case("m40x7")
    s = _symb(c)
    with pytest.raises(ValueError, match="complex16"):
        driver.BatchHandle.create(s, c.values.astype(np.complex128))
    # an equilibration made through the borrowed handle would be ignored by the batch's pack / unpack: every batch call refuses the handle from then on
    bh = driver.BatchHandle.create(s, c.values)
    n, rp, ci, v = bc.block_diag_csr(c)
    L = _lib.load()
    e = _lib.Equil()
    pc = np.concatenate([s.perm_c + k * c.m for k in range(c.count)]).astype(np.int32)
    rc = L.sluamd_dEquilibrate(bh.handle(), n, rp.ctypes.data_as(_lib.P_int), ci.ctypes.data_as(_lib.P_int), v.ctypes.data_as(C.c_void_p),
                               pc.ctypes.data_as(_lib.P_int), C.byref(e))
    assert rc == -1                                         # the structure-only handle keeps no entry map: the single-matrix call refuses by itself
    assert not bh.factor().any()
    bh.destroy(); s.free()
