"""Equil = YES on the device (sluamd_[dz]Equilibrate, sluamd_GetScalings, sluamd_p[dz]gssvx3d_solve[_dev]) against the numpy restatement of
pdgsequ + pdlaqgs in equil_cases.py: bit-exact scalings and store values, the 1-norm within its documented bound, the solve wrapper against the
parent path, end-to-end systems that the unequilibrated static-pivoting LU cannot solve, grids and error codes.
Bars: residual max|A'x' - b'| <= 1e-10 max|b'| (the project's residual bar), berr <= 4 * 2^-53 (the refinement tests' bar), repeated solves
1e-13 max|x| (test_gpu_edge_cases.py)."""
import ctypes as C
import functools
import numpy as np
import pytest
import equil_cases as ec
from superlu_dist_amd import _lib, driver, grid3d, matgen

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


def _create(n, rp, ci, v, perm=None, **kw):
    symb = driver.Symbolic(n, rp, ci, perm, relax=8, maxsup=64)
    return symb, driver.LUHandle.from_symbolic(symb, v, **kw)


@functools.lru_cache(maxsize=None)
def _restated(name):
    n, rp, ci, v = ec.case(name)
    return n, rp, ci, v, ec.equilibrate(n, rp, ci, v)


# ---- bit-exact scalings ----

@pytest.mark.parametrize("name", sorted(ec.EXPECT))
def test_scalings_bit_exact(name):
    n, rp, ci, v, e = _restated(name)
    symb, h = _create(n, rp, ci, v)
    try:
        d = h.equilibrate(n, rp, ci, v, symb.perm_c)
        R, Cs = h.scalings()
    finally:
        h.destroy(); symb.free()
    print(name, d)
    assert (d["equed"], d["info"]) == (e["equed"], e["info"]) == ec.EXPECT[name]
    assert d["rowcnd"] == e["rowcnd"] and d["colcnd"] == e["colcnd"] and d["amax"] == e["amax"]
    assert np.array_equal(R, e["R"]) and np.array_equal(Cs, e["C"])
    # 1-norm of the matrix the handle holds: fp64 atomic column sums, relative error <= k 2^-52 for a longest column of k entries
    ref, k = ec.anorm_exact(n, ci, e["vals"])
    print("anorm", d["anorm"], ref, "k", k)
    assert abs(d["anorm"] - ref) <= k * 2.0 ** -52 * ref


# ---- bit-exact values in the store ----

def _store_of(symb, vals):
    """the store symb.distribute_host builds from `vals` (complex: real and imaginary parts distributed one after the other)"""
    symb.distribute_host(np.ascontiguousarray(vals.real))
    fs = symb.flat_store()
    if not np.iscomplexobj(vals):
        return fs.Lnzval.copy(), fs.Unzval.copy()
    symb.distribute_host(np.ascontiguousarray(vals.imag))
    fi = symb.flat_store()
    return fs.Lnzval + 1j * fi.Lnzval, fs.Unzval + 1j * fi.Unzval


def _device_store(symb, h):
    fs = symb.flat_store(values=False)
    if h.z:
        fs = driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind, fs.Lnzval_off, fs.Lnzval.astype(np.complex128), fs.Ufstnz_off, fs.Ufstnz,
                              fs.Unzval_off, fs.Unzval.astype(np.complex128))
    h.copy_to_host(fs)
    return fs.Lnzval, fs.Unzval


@pytest.mark.parametrize("name", ["diag63_R", "neg257_C", "dense65_B", "z_rows1_R", "z_dense64_C", "z_abs1"])
def test_store_values_bit_exact(name):
    n, rp, ci, v, e = _restated(name)
    symb, h = _create(n, rp, ci, v)
    try:
        expL, expU = _store_of(symb, e["vals"])
        d = h.equilibrate(n, rp, ci, v, symb.perm_c)
        assert d["equed"] == e["equed"] != "N"
        L1, U1 = _device_store(symb, h)
        assert np.array_equal(L1, expL) and np.array_equal(U1, expU)
        h.pdgstrf3d(0.0)                                   # (random values: the factors themselves are of no interest here)
        h.reset_values()                                   # restores the SCALED values
        L2, U2 = _device_store(symb, h)
        assert np.array_equal(L2, expL) and np.array_equal(U2, expU)
    finally:
        h.destroy(); symb.free()


# ---- the solve wrapper against the parent path ----

@pytest.fixture(scope="module")
def plain():
    """a factored, NOT equilibrated handle with its matrix attached"""
    n, rp, ci, v = matgen.stencil3d_unsym(5, seed=3)
    perm = matgen.nd_perm_grid3d(5, 5, 5, leaf=27)
    symb, h = _create(n, rp, ci, v, perm)
    assert h.pdgstrf3d(driver.pivot_thresh(n, rp, ci, v)) == 0
    h.attach_matrix(n, rp, ci, v, symb.perm_c)
    yield n, rp, ci, v, symb, h
    h.destroy(); symb.free()


def _parent_solve(h, symb, b, trans="N"):
    xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b
    return np.asfortranarray(h.pdgstrs3d(xp, trans=trans)[symb.perm_c, :])


@pytest.mark.parametrize("nrhs", [1, 3, 16, 17])
def test_wrapper_equals_parent_path(plain, nrhs):
    n, rp, ci, v, symb, h = plain
    b = np.asfortranarray(np.random.default_rng(nrhs).standard_normal((n, nrhs)))
    b0 = b.copy()
    x0 = _parent_solve(h, symb, b)
    x1 = h.gssvx_solve(b)
    assert np.array_equal(b, b0)
    assert np.array_equal(h.scalings()[0], np.ones(n))
    if nrhs == 1:
        assert np.array_equal(x1, x0)
    else:
        assert np.abs(x1 - x0).max() <= 1e-13 * np.abs(x0).max()      # atomics reorder: the bar of repeated solves


def test_wrapper_leading_dimensions_and_sentinels(plain):
    n, rp, ci, v, symb, h = plain
    nrhs, pad = 3, 5
    rng = np.random.default_rng(7)
    B = np.full((n + pad, nrhs), np.nan, order="F"); B[:n] = rng.standard_normal((n, nrhs))
    X = np.full((n + pad + 2, nrhs), np.nan, order="F")
    B0 = B.copy()
    berr = np.zeros(nrhs); steps = C.c_int32(0)
    _lib.check(_lib.entry("sluamd_pdgssvx3d_solve")(h._h, 0, B.ctypes.data_as(C.c_void_p), n + pad, X.ctypes.data_as(C.c_void_p), n + pad + 2, nrhs, 0,
                                                    berr.ctypes.data_as(_lib.P_dbl), C.byref(steps)), "sluamd_pdgssvx3d_solve")
    assert np.array_equal(B, B0, equal_nan=True)
    assert np.all(np.isnan(X[n:])) and np.all(np.isfinite(X[:n]))
    x0 = _parent_solve(h, symb, np.asfortranarray(B[:n]))
    assert np.abs(X[:n] - x0).max() <= 1e-13 * np.abs(x0).max()


class _DevBuf:
    """device memory through the HIP runtime itself (the library has initialised it; no second framework in the process)"""
    hip = None

    def __init__(self, a):
        import os
        if _DevBuf.hip is None:
            _DevBuf.hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.a = np.asfortranarray(a)
        self.ptr = C.c_void_p()
        assert _DevBuf.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.a.nbytes)) == 0
        assert _DevBuf.hip.hipMemcpy(self.ptr, self.a.ctypes.data_as(C.c_void_p), C.c_size_t(self.a.nbytes), 1) == 0      # hipMemcpyHostToDevice

    def host(self):
        out = np.empty_like(self.a, order="F")
        assert _DevBuf.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes), 2) == 0          # hipMemcpyDeviceToHost
        return out

    def free(self):
        _DevBuf.hip.hipFree(self.ptr)


def test_wrapper_on_device_pointers(plain):
    n, rp, ci, v, symb, h = plain
    nrhs, ldb, ldx = 3, n + 4, n + 1
    rng = np.random.default_rng(9)
    B = np.full((ldb, nrhs), np.nan, order="F"); B[:n] = rng.standard_normal((n, nrhs))
    d_b, d_x = _DevBuf(B), _DevBuf(np.full((ldx, nrhs), np.nan, order="F"))
    try:
        h.gssvx_solve_dev(d_b.ptr.value, ldb, d_x.ptr.value, ldx, nrhs)
        assert np.array_equal(d_b.host(), B, equal_nan=True)
        X = d_x.host()
        x0 = _parent_solve(h, symb, np.asfortranarray(B[:n]))
        assert np.all(np.isnan(X[n:])) and np.abs(X[:n] - x0).max() <= 1e-13 * np.abs(x0).max()
        berr, steps = h.gssvx_solve_dev(d_b.ptr.value, ldb, d_x.ptr.value, ldx, nrhs, refine=True)
        X = d_x.host()
        assert np.all(berr <= 4 * EPS) and np.all(np.isnan(X[n:])) and np.abs(X[:n] - x0).max() <= 1e-12 * np.abs(x0).max()
        assert np.array_equal(d_b.host(), B, equal_nan=True)
    finally:
        d_b.free(); d_x.free()


# ---- end to end ----

def _resid_scaled(n, rp, ci, e, x, b):
    """max|A'x' - b'| / max|b'| on the scaled system: A' = the restated scaled values, x' = x / C, b' = R b"""
    xs, bs = x / e["C"][:, None], b * e["R"][:, None]
    return float(np.abs(matgen.csr_matvec(n, rp, ci, e["vals"], xs) - bs).max() / np.abs(bs).max())


def _rhs(n, rp, ci, v, nrhs=2, seed=0):
    rng = np.random.default_rng(seed)
    xt = rng.choice([-1.0, 1.0], (n, nrhs)) * (1.0 + 0.5j * rng.choice([-1.0, 1.0], (n, nrhs)) if np.iscomplexobj(v) else 1.0)
    return np.asfortranarray(matgen.csr_matvec(n, rp, ci, v, xt))


@pytest.mark.parametrize("z", [False, True], ids=["double", "complex16"])
def test_scaled_2pm40_needs_equilibration(z):
    """(a), (d): row and column scalings 2^+-40 of a diagonally dominant operator, ReplaceTinyPivot = YES"""
    n, rp, ci, v, perm, rs, cs = ec.scaled_operator(mode="a", z=z)
    b = _rhs(n, rp, ci, v)
    x0, info0, st0 = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=8, maxsup=64, replace_tiny=True)
    res0 = float(np.abs(matgen.csr_matvec(n, rp, ci, v, x0) - b).max() / np.abs(b).max()) if np.all(np.isfinite(x0)) else float("inf")
    print("plain path: tiny_pivots", st0["tiny_pivots"], "info", info0, "residual", res0)
    assert st0["tiny_pivots"] > 0 and not res0 <= 1e-3            # the precondition: without equilibration the threshold fires and the answer is garbage
    e = ec.equilibrate(n, rp, ci, v)
    x, info, st = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=8, maxsup=64, replace_tiny=True, equil=True)
    res = _resid_scaled(n, rp, ci, e, x, b)
    print("equil: equed", st["equed"], "tiny_pivots", st["tiny_pivots"], "scaled residual", res)
    assert info == 0 and st["equed"] == e["equed"] and st["rowcnd"] == e["rowcnd"] and st["colcnd"] == e["colcnd"] and st["amax"] == e["amax"]
    assert st["tiny_pivots"] == 0 and res <= 1e-10
    xr, info, st = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=8, maxsup=64, replace_tiny=True, equil=True, refine=True)
    print("refined: berr/eps", (st["berr"] / EPS).tolist(), "steps", st["refine_steps"])
    assert np.all(st["berr"] <= 4 * EPS) and _resid_scaled(n, rp, ci, e, xr, b) <= 1e-10


def test_rows_2pm520_need_equilibration():
    """(b): row scalings alternating 2^520 / 2^-520; A and b finite, amax inside [small, large]"""
    n, rp, ci, v, perm, rs, cs = ec.scaled_operator(mode="b")
    b = _rhs(n, rp, ci, v)
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(b))
    x0, info0, st0 = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=8, maxsup=64)
    print("plain path: info", info0, "finite", bool(np.all(np.isfinite(x0))))
    assert info0 != 0 or not np.all(np.isfinite(x0))              # the precondition
    e = ec.equilibrate(n, rp, ci, v)
    assert ec.SMALL <= e["amax"] <= ec.LARGE
    x, info, st = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=8, maxsup=64, equil=True)
    res = _resid_scaled(n, rp, ci, e, x, b)
    print("equil: equed", st["equed"], "tiny_pivots", st["tiny_pivots"], "scaled residual", res)
    assert info == 0 and st["tiny_pivots"] == 0 and res <= 1e-10
    xr, info, st = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=8, maxsup=64, equil=True, refine=True)
    print("refined: berr/eps", (st["berr"] / EPS).tolist())
    assert np.all(st["berr"] <= 4 * EPS) and _resid_scaled(n, rp, ci, e, xr, b) <= 1e-10


@pytest.mark.parametrize("z,trans", [(False, "T"), (True, "T"), (True, "C")])
def test_transposed_system_swaps_the_scalings(z, trans):
    """A^T x = b (A^H x = b) on the equilibrated factors: s_in = C, s_out = R.  Against the same steps by hand around pdgstrs3d(trans), and the residual
    of the transposed scaled system A'^T x' = b' with x' = x / R, b' = C b."""
    n, rp, ci, v, perm, rs, cs = ec.scaled_operator(mode="a", z=z, seed=1)
    e = ec.equilibrate(n, rp, ci, v)
    assert e["equed"] == "B"
    import scipy.sparse as sp
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    At = A.T.conj() if trans == "C" else A.T
    rng = np.random.default_rng(5)
    xt = rng.choice([-1.0, 1.0], (n, 2)).astype(v.dtype)
    b = np.asfortranarray(At @ xt)
    x, info, st, h, symb = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=8, maxsup=64, equil=True, trans=trans, keep=True)
    try:
        R, Cs = h.scalings()
        assert np.array_equal(R, e["R"]) and np.array_equal(Cs, e["C"]) and info == 0
        xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = Cs[:, None] * b
        y_hand = h.pdgstrs3d(xp, trans=trans)[symb.perm_c, :]
        # compared before the unscaling (x = R o y holds components 2^80 apart: a max-norm bar would see the largest ones only)
        assert np.abs(x / R[:, None] - y_hand).max() <= 1e-13 * np.abs(y_hand).max()
        with pytest.raises(RuntimeError, match="transposed"):
            h.gssvx_solve(b, trans=trans, refine=True)
    finally:
        h.destroy(); symb.free()
    As = sp.csr_matrix((e["vals"], ci, rp), shape=(n, n))
    Ast = As.T.conj() if trans == "C" else As.T
    bs = Cs[:, None] * b
    assert np.abs(Ast @ (x / R[:, None]) - bs).max() <= 1e-10 * np.abs(bs).max()


# ---- grids ----

@pytest.mark.parametrize("grid", [(1, 1, 2), (2, 2, 2)])
def test_grids_scale_and_solve_alike(grid):
    Pr, Pc, Pz = grid
    n, rp, ci, v, perm, rs, cs = ec.scaled_operator(mode="a")      # the system of case (a): its equilibrated form keeps a unit diagonal (test_equil_cases_cpu.py)
    e = ec.equilibrate(n, rp, ci, v)
    b = _rhs(n, rp, ci, v)
    symb = driver.Symbolic(n, rp, ci, perm, relax=8, maxsup=64)
    sn_tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], sn_tree)
        try:
            d = h.equilibrate(n, rp, ci, v, symb.perm_c)
            R, Cs = h.scalings()
            info = h.pdgstrf3d(0.5 * float(np.finfo(np.float32).eps) * d["anorm"])
            x = h.gssvx_solve(b)
            xr, berr, steps = h.gssvx_solve(b, refine=True)
            with pytest.raises(RuntimeError, match="1 x 1 x 1"):
                h.gssvx_solve(b, trans="T")
            return d["equed"], R, Cs, info, x, xr, berr, steps
        finally:
            h.destroy()

    out = grid3d.run_ranks(Pr * Pc * Pz, body)
    symb.free()
    eq0, R0, C0, info0, x0, xr0, berr0, steps0 = out[0]
    assert eq0 == e["equed"] and np.array_equal(R0, e["R"]) and np.array_equal(C0, e["C"]) and info0 == 0
    for eq, R, Cs, info, x, xr, berr, steps in out[1:]:
        assert eq == eq0 and np.array_equal(R, R0) and np.array_equal(Cs, C0) and info == 0
        assert np.array_equal(x, x0) and np.array_equal(xr, xr0) and np.array_equal(berr, berr0) and steps == steps0
    assert _resid_scaled(n, rp, ci, e, x0, b) <= 1e-10 and _resid_scaled(n, rp, ci, e, xr0, b) <= 1e-10
    assert np.all(berr0 <= 4 * EPS)


# ---- error codes ----

def test_error_codes(plain, golden):
    n, rp, ci, v, symb, h = plain
    b = np.ones((n, 1))
    # refine with trans; nrhs == 0
    with pytest.raises(RuntimeError, match="transposed"):
        h.gssvx_solve(b, trans="T", refine=True)
    assert h.gssvx_solve(np.zeros((n, 0))).shape == (n, 0)
    symb2, h2 = _create(n, rp, ci, v, symb.perm_c)
    try:
        # a wrong n / nnz, the wrong precision, no matrix attached
        with pytest.raises(RuntimeError, match="differs"):
            driver._equilibrate(h2._h, False, n - 1, rp[:n], ci[:rp[n - 1]], v[:rp[n - 1]], symb2.perm_c[:n - 1])
        rp2 = rp.copy(); rp2[n] -= 1
        with pytest.raises(RuntimeError, match="differs"):
            driver._equilibrate(h2._h, False, n, rp2, ci, v, symb2.perm_c)
        with pytest.raises(RuntimeError, match="double handle"):
            driver._equilibrate(h2._h, True, n, rp, ci, v.astype(np.complex128), symb2.perm_c)
        with pytest.raises(RuntimeError, match="no matrix attached"):
            h2.gssvx_solve(b)
        with pytest.raises(RuntimeError, match="double handle"):
            driver._gssvx_solve(h2._h, True, b.astype(np.complex128), "N", False)
        # a second call
        assert h2.equilibrate(n, rp, ci, v, symb2.perm_c)["info"] == 0
        with pytest.raises(RuntimeError, match="already"):
            h2.equilibrate(n, rp, ci, v, symb2.perm_c)
    finally:
        h2.destroy(); symb2.free()
    # a view-created handle
    g = golden("poisson8_nd")
    hv = driver.LUHandle.from_store(driver.FlatStore.from_golden(g, 0, "pre"))
    try:
        m = hv.n
        with pytest.raises(RuntimeError, match="not created from the symbolic structure"):
            hv.equilibrate(m, np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32), np.ones(m), np.arange(m, dtype=np.int32))
        assert np.array_equal(hv.scalings()[1], np.ones(m))
    finally:
        hv.destroy()


# ---- (e): the exact transposed systems of trans_cases.py under power-of-two scalings ----

@pytest.mark.parametrize("name,trans", [("narrow", "T"), ("z_narrow", "T"), ("z_narrow", "C")])
def test_exact_transposed_cases_under_power_of_two_scalings(name, trans):
    """A = Dr B Dc with B = L0 U0 of a sweep case and Dr, Dc powers of two (2^+-100, exact), the handle created from the symbolic structure, equil=True,
    gssvx_solve(Dc b_t, trans): the exact solution is x_int / Dr with the integer x_int and b_t = op(B)^T x_int of trans_cases.rhs_t.
    Bar.  R and C are reciprocals of maxima, not powers of two, so the scaled values round and array_equal is out; and these operators are built for exact
    elimination, not for conditioning (cond_2(B) = 1.7e18 for narrow, 7.7e14 for z_narrow): a fixed relative bar cannot hold for ANY floating-point solver
    (a numpy emulation of the same steps -- restated scaling, unpivoted LU in double, substitution -- gives relative errors of 1.6 and 3e-4).  What holds is
    the componentwise forward bound of an LU solve (Higham, Accuracy and Stability, Thm 9.4: (A' + dA) x^ = b', |dA| <= gamma_3n |L^||U^|), which is
    invariant under the diagonal scalings:   |x^ - x| <= gamma (1 / Dr) o ( |B^-T| |U0|^T |L0|^T |x_int| ),   gamma = 8 n 2^-53
    -- 3 n for the theorem, the rest for what it does not count: the rounding of the scaled values (2 u |A'| <= 2 u |L||U|), the two scalings of b and x
    (2 u), and the products with explicit inverses of the diagonal blocks in place of substitutions.  The emulation sits at 1e-5 of this bound.
    The scalings of 2^+-100 make the bound discriminate: R and C swapped, or one of them left out, moves x by factors of 2^100, the bound allows < 2^20."""
    import trans_cases as tc
    c = tc.prepared(name)[0]
    n, rp, ci = c.pattern_csr()
    rows = ec.rows_of(n, rp)
    assert np.count_nonzero(c.B) == np.count_nonzero(c.B[rows, ci])         # the pattern holds all of B
    rng = np.random.default_rng(11)
    Dr, Dc = 2.0 ** rng.choice([-100, 100], n), 2.0 ** rng.choice([-100, 100], n)
    v = (c.B[rows, ci] * Dr[rows]) * Dc[ci]
    conj = trans == "C"
    x_int, b_t = tc.rhs_t(c, 2, conj)
    b = np.asfortranarray(Dc[:, None] * b_t)
    xtrue = x_int / Dr[:, None]
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    h = driver.LUHandle.from_symbolic(symb, v)
    try:
        eq = h.equilibrate(n, rp, ci, v, symb.perm_c)
        assert eq["equed"] == "B" and eq["info"] == 0
        assert h.pdgstrf3d(0.5 * float(np.finfo(np.float32).eps) * eq["anorm"]) == 0
        x = h.gssvx_solve(b, trans=trans)
    finally:
        h.destroy(); symb.free()
    bound = 8 * n * EPS * (np.abs(np.linalg.inv(c.B)).T @ (np.abs(c.U0).T @ (np.abs(c.L0).T @ np.abs(x_int)))) / Dr[:, None]
    ratio = float((np.abs(x - xtrue) / bound).max())
    print(name, trans, "max error / bound", ratio, "max relative error", float((np.abs(x - xtrue) / np.abs(xtrue)).max()))
    assert np.all(np.isfinite(x)) and ratio <= 1.0


def test_complex16_wrapper_on_device_pointers():
    """sluamd_pzgssvx3d_solve_dev against the host-pointer call on an equilibrated complex16 handle, with padding rows"""
    n, rp, ci, v, perm, rs, cs = ec.scaled_operator(mode="a", z=True)
    b = _rhs(n, rp, ci, v)
    nrhs, ldb, ldx = b.shape[1], n + 3, n + 2
    symb, h = _create(n, rp, ci, v, perm)
    B = np.full((ldb, nrhs), np.nan + 0j, order="F"); B[:n] = b
    d_b, d_x = None, None
    try:
        eq = h.equilibrate(n, rp, ci, v, symb.perm_c)
        assert h.z and h.pdgstrf3d(0.5 * float(np.finfo(np.float32).eps) * eq["anorm"]) == 0
        x_host = h.gssvx_solve(b)
        d_b, d_x = _DevBuf(B), _DevBuf(np.full((ldx, nrhs), np.nan + 0j, order="F"))
        for tr in ("N", "C"):
            ref = h.gssvx_solve(b, trans=tr)
            h.gssvx_solve_dev(d_b.ptr.value, ldb, d_x.ptr.value, ldx, nrhs, trans=tr)
            X = d_x.host()
            y, yr = X[:n] / h.scalings()[1 if tr == "N" else 0][:, None], ref / h.scalings()[1 if tr == "N" else 0][:, None]
            assert np.all(np.isnan(X[n:])) and np.abs(y - yr).max() <= 1e-13 * np.abs(yr).max()        # compared before the unscaling, like the transposed test
        assert np.array_equal(d_b.host(), B, equal_nan=True)
        berr, steps = h.gssvx_solve_dev(d_b.ptr.value, ldb, d_x.ptr.value, ldx, nrhs, refine=True)
        assert np.all(berr <= 4 * EPS)
        e = ec.equilibrate(n, rp, ci, v)
        assert _resid_scaled(n, rp, ci, e, d_x.host()[:n], b) <= 1e-10 and _resid_scaled(n, rp, ci, e, x_host, b) <= 1e-10
    finally:
        for d in (d_b, d_x):
            if d is not None:
                d.free()
        h.destroy(); symb.free()


def test_c_example_with_equil():
    """examples/pddrive3d_amd N --equil through the C ABI: the EQUIL line and the residual (exit status 0 = ||b - A x|| / ||b|| < 1e-10)"""
    import os, re, subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "pddrive3d_amd")
    assert os.path.exists(exe), "examples/pddrive3d_amd not built"
    r = subprocess.run([exe, "8", "-nd", "--equil"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    m = re.search(r"EQUIL: equed = ([NRCB])  rowcnd (\S+)  colcnd (\S+)  amax (\S+)  info (\d+)", r.stdout)
    assert m and m.group(1) == "N" and float(m.group(4)) == 6.0 and int(m.group(5)) == 0       # Poisson: diagonal 6, rowcnd = colcnd = 1
    res = float(re.search(r"\|\|b-Ax\|\|_2/\|\|b\|\|_2 = (\S+)", r.stdout).group(1))
    assert res < 1e-10
