"""sluamd_p[dz]gsrfs3d_gmres[_dev]: GMRES refinement preconditioned by the resident factors, on the systems of tests/gmres_cases.py -- A' = A (I + W) attached
to handles holding the factors of A, rho(I - A^-1 A') = 3 -- on which the plain loop must fail.  What is asserted comes from numpy (gmres_cases): the
accuracy bound berr <= 4 max(2^-53, berr_ref), berr_ref the backward error of numpy.linalg.solve; the componentwise error bound from A'^-1; the premises.
Bitwise comparisons (numpy.array_equal on bit patterns): the E = 0 cases, the padding rows, repeatability.

The entry points return the total of applications of the factors per right-hand side and the number of outer steps, not the length of each cycle; a cycle of
k iterations costs k + 1.  "The first cycle takes at most t + 1 iterations" is therefore checked in two ways: solves <= steps (t + 2) on the default call, and
a call with restart = t + 1 and max_solves = t + 2 -- a first cycle of at most t + 1 iterations, and whatever the budget still pays for when that cycle
ended earlier -- must bring berr below 2^-20, the level above which the plain loop counts as failed (a Krylov space that needed more than t + 1 vectors
leaves such a cycle with a residual of the order it started from)."""
import ctypes as C
import json, os, subprocess, sys
import numpy as np
import pytest
import gmres_cases as gc
import refine_exact_cases as rx
from superlu_dist_amd import _lib, driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = gc.cases()
TRANS = {False: ("N", "T"), True: ("N", "T", "C")}
TCODE = {"N": 0, "T": 1, "C": 2}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _handle(c, **kw):
    """(handle, perm_c) holding the factors of c.A: exact ones for kind "diag" (asserted), the library's own factorisation for kind "lu" """
    if c.kind == "diag":
        fs0, expL, expU = rx.diag_store(c.n, c.z)
        fs = driver.FlatStore(fs0.n, fs0.xsup, fs0.Lrowind_off, fs0.Lrowind.copy(), fs0.Lnzval_off, fs0.Lnzval.copy(), fs0.Ufstnz_off, fs0.Ufstnz, fs0.Unzval_off,
                              fs0.Unzval.copy())
        h = driver.LUHandle.from_store(fs, **kw)
        assert h.z == c.z and h.pdgstrf3d(0.0) == 0
        if c.n < gc.LARGE_N:
            h.copy_to_host()
            assert np.array_equal(fs.Lnzval, expL) and np.array_equal(fs.Unzval, expU)
        return h, c.pc
    A = c.A
    x, info, st, h, symb = driver.pdgssvx3d(c.n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, np.ones(c.n, dtype=c.vt), keep=True, **kw)
    pc = np.array(symb.perm_c, dtype=np.int32)
    symb.free()
    assert info == 0
    return h, pc


def _attach(h, c, pc):
    rp, ci, av = c.csr()
    h.attach_matrix(c.n, rp, ci, av, pc)


def _padded(a, pad_rows, tag, z):
    """the columns of `a` over pad_rows sentinel rows (position-tagged NaN payloads), as uint64 [(n + pad_rows) vs, nrhs], column-major"""
    n, nrhs = a.shape
    vs = 2 if z else 1
    buf = np.zeros(((n + pad_rows) * vs, nrhs), dtype=np.uint64, order="F")
    for q in range(nrhs):
        buf[:n * vs, q] = np.ascontiguousarray(a[:, q]).view(np.uint64)
    buf[n * vs:, :] = 0x7FF8000000000000 + 256 * tag + 1 + np.arange(pad_rows * vs, dtype=np.uint64)[:, None] + 16 * np.arange(nrhs, dtype=np.uint64)[None, :]
    return buf


def _call(h, c, trans, B, X0, dev=False, torch=None, **opt):
    """the C entry point on blocks with ldb = n + 3, ldx = n + 5: dict(X, berr, steps, solves, pads) -- pads: B and the sentinel rows of X came back bitwise"""
    n, vs, nrhs = c.n, 2 if c.z else 1, B.shape[1]
    bB, bX = _padded(B, 3, 1, c.z), _padded(X0, 5, 2, c.z)
    o = driver._gmres_opt("gmres", opt.get("restart"), opt.get("inner_tol"), opt.get("max_solves"))
    berr, steps, solves = np.zeros(nrhs), C.c_int32(-1), np.full(nrhs, -1, dtype=np.int32)
    name = ("sluamd_pzgsrfs3d_gmres" if c.z else "sluamd_pdgsrfs3d_gmres") + ("_dev" if dev else "")
    if dev:
        dB, dX = (torch.from_numpy(np.ascontiguousarray(b.T).view(np.int64)).cuda() for b in (bB, bX))
        torch.cuda.synchronize()
        pB, pX = C.c_void_p(dB.data_ptr()), C.c_void_p(dX.data_ptr())
    else:
        gB, gX = bB.copy(order="F"), bX.copy(order="F")
        pB, pX = gB.ctypes.data_as(C.c_void_p), gX.ctypes.data_as(C.c_void_p)
    rc = _lib.entry(name)(h._h, TCODE[trans], pB, n + 3, pX, n + 5, nrhs, C.byref(o), berr.ctypes.data_as(C.POINTER(C.c_double)), C.byref(steps),
                          solves.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, _lib.load().sluamd_last_error().decode()
    if dev:
        torch.cuda.synchronize()
        gB, gX = (t.cpu().numpy().view(np.uint64).T for t in (dB, dX))
    X = np.stack([np.ascontiguousarray(gX[:n * vs, q]).view(c.vt) for q in range(nrhs)], axis=1)
    pads = bool(np.array_equal(gB, bB) and np.array_equal(gX[n * vs:, :], bX[n * vs:, :]))
    return dict(X=X, berr=berr, steps=int(steps.value), solves=solves, pads=pads)


def _rank_checks(h, c, pc, dev=False, torch=None):
    """every assertion of a rank-t case on one handle, all trans of its precision; returns the figures"""
    out = {}
    _attach(h, c, pc)
    for trans in TRANS[c.z]:
        B = c.rhs(trans)
        bnd, ref = gc.bound(c.name, trans), gc.reference(c.name, trans)[1]
        j = c.nrhs - 1
        if not dev:
            _, pberr, psteps = h.pdgsrfs3d(B.copy(order="F"), c.X0.copy(order="F"), trans=trans)
            out[trans + "_plain"] = (pberr.tolist(), psteps)
            assert pberr[j] >= 2.0 ** -20, (c.name, trans, "the plain loop", pberr.tolist())
        g = _call(h, c, trans, B, c.X0, dev=dev, torch=torch)
        out[trans] = dict(berr_ref=ref.tolist(), berr=g["berr"].tolist(), steps=g["steps"], solves=g["solves"].tolist())
        print(c.name, trans, "dev" if dev else "host", out[trans], out.get(trans + "_plain"))
        assert g["pads"], (c.name, trans, "B or the padding rows of X changed")
        assert np.all(g["berr"] <= bnd), (c.name, trans, g["berr"].tolist(), bnd.tolist())
        assert 0 < g["solves"][j] <= g["steps"] * (c.t + 2), (c.name, trans, g["solves"].tolist(), g["steps"])
        if c.m[0] < 0:                                          # distinct eigenvalues spread wide: the first cycle needs t or t + 1 iterations (+ its end), as the model's
            assert g["solves"][j] >= c.t + 1, (c.name, trans, g["solves"].tolist())
        assert gc.error_bound_ok(c, trans, g["X"], g["berr"]), (c.name, trans)
        if c.nrhs == 1:
            r = _call(h, c, trans, B, c.X0, dev=dev, torch=torch, restart=c.t + 1, max_solves=c.t + 2)
            print(c.name, trans, "one cycle of t + 1", r["berr"].tolist(), r["steps"], r["solves"].tolist())
            assert r["steps"] >= 1 and 2 <= r["solves"][0] <= c.t + 2 and r["berr"][0] < 2.0 ** -20, (c.name, trans, "one cycle of t + 1", r["steps"], r["berr"].tolist())
    return out


RANK1 = [k for k in gc.names(rank=True) if CASES[k].nrhs == 1]


@pytest.mark.parametrize("name", RANK1)
def test_rank_t_cases_host_form(name):
    c = CASES[name]
    h, pc = _handle(c)
    try:
        _rank_checks(h, c, pc)
    finally:
        h.destroy()


def _dev_child():
    import torch
    assert torch.cuda.is_available(), "torch sees no HIP device"
    out = {}
    for name in RANK1:
        c = CASES[name]
        if c.n not in (65, 513):
            continue
        h, pc = _handle(c)
        try:
            out[name] = _rank_checks(h, c, pc, dev=True, torch=torch)
            if c.t == 4:                                        # the Python twin, LUHandle.pdgsrfs3d_dev(method="gmres"), on plain n x 1 device blocks
                B = c.rhs("N")
                dB, dX = (torch.from_numpy(np.ascontiguousarray(a[:, 0]).view(np.float64).copy()).cuda() for a in (B, c.X0))
                torch.cuda.synchronize()
                berr, steps, solves = h.pdgsrfs3d_dev(dB.data_ptr(), c.n, dX.data_ptr(), c.n, 1, method="gmres", max_solves=60)
                torch.cuda.synchronize()
                X = dX.cpu().numpy().view(c.vt).reshape(c.n, 1)
                assert berr.shape == (1,) and solves.shape == (1,) and isinstance(steps, int) and 0 < solves[0] <= 60
                assert berr[0] <= gc.bound(name, "N")[0] and gc.error_bound_ok(c, "N", X, berr)
        finally:
            h.destroy()
    print("RESULT " + json.dumps(sorted(out)))


def test_rank_t_cases_dev_form():
    """the _dev entry points from a child process that imports torch first (torch.cuda reports no device once the library has initialised the HIP runtime in the
    process): the assertions of the host form on device blocks, orders 65 and 513, both kinds, both precisions, every trans"""
    code = ("import os, sys\nimport torch\nsys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\n"
            "import test_gpu_gmres_refine as t\nt._dev_child()\n")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-2500:]
    done = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert done == sorted(k for k in RANK1 if CASES[k].n in (65, 513)) and len(done) >= 8


@pytest.mark.parametrize("name", gc.names(rank=False))
def test_exact_start_takes_no_step(name):
    """E = 0, x0 = x*: no solve, no step, X untouched, and berr bitwise that of the plain entry point -- the first residual is the same kernel"""
    c = CASES[name]
    h, pc = _handle(c)
    try:
        _attach(h, c, pc)
        B = c.rhs("N")
        g = _call(h, c, "N", B, c.X0)
        _, pberr, psteps = h.pdgsrfs3d(B.copy(order="F"), c.X0.copy(order="F"))
        assert g["steps"] == 0 and g["solves"].tolist() == [0] and psteps == 0 and g["pads"]
        assert np.array_equal(_bits(g["X"]), _bits(c.X0)) and np.array_equal(_bits(g["berr"]), _bits(pberr))
    finally:
        h.destroy()


@pytest.mark.parametrize("name", ["d_diag_n513_t4_cluster", "z_lu_n513_t4_cluster"])
def test_restart(name):
    """restart = 2 on rank-4 cases whose cycle needs 5 iterations: every cycle is cut short (the j + 1 == restart exit) and the next resumes from the true
    residual -- more outer steps and more solves than the unrestarted call, three solves per step, the bounds still met"""
    c = CASES[name]
    h, pc = _handle(c)
    try:
        _attach(h, c, pc)
        B, bnd = c.rhs("N"), gc.bound(name, "N")
        full = _call(h, c, "N", B, c.X0)
        g = _call(h, c, "N", B, c.X0, restart=2)
        print(name, "restart 2", g["berr"].tolist(), g["steps"], g["solves"].tolist(), "unrestarted", full["steps"], full["solves"].tolist())
        assert g["steps"] > max(full["steps"], 1) and g["solves"][0] > full["solves"][0] and g["solves"][0] == 3 * g["steps"]
        assert np.all(g["berr"] <= bnd) and gc.error_bound_ok(c, "N", g["X"], g["berr"])
    finally:
        h.destroy()


@pytest.mark.parametrize("name", ["d_diag_n513_t10", "z_lu_n513_t10"])
def test_budget(name):
    """max_solves = 5 on rank-10 cases: the first cycle, which takes 11 iterations when left alone, is cut after 4 and finished into x; returns 0"""
    c = CASES[name]
    h, pc = _handle(c)
    try:
        _attach(h, c, pc)
        B = c.rhs("N")
        full = _call(h, c, "N", B, c.X0)
        assert full["solves"][0] >= c.t + 1
        g = _call(h, c, "N", B, c.X0, max_solves=5)
        print(name, "max_solves 5", g["berr"].tolist(), g["steps"], g["solves"].tolist())
        assert g["solves"].tolist() == [5] and g["steps"] == 1 and not np.array_equal(_bits(g["X"]), _bits(c.X0))
        g = _call(h, c, "N", B, c.X0, max_solves=1)              # one application: the plain step
        assert g["solves"].tolist() == [1] and g["steps"] == 1
    finally:
        h.destroy()


@pytest.mark.parametrize("name", [k for k in CASES if k.endswith("rhs3")])
def test_three_right_hand_sides(name):
    """one column exact from the start, one an eigenvector away, one from zero: solves per column, the bound on every column"""
    c = CASES[name]
    h, pc = _handle(c)
    try:
        _attach(h, c, pc)
        g = _call(h, c, "N", c.rhs("N"), c.X0)
        print(name, g["berr"].tolist(), g["steps"], g["solves"].tolist())
        s = g["solves"].tolist()
        assert s[0] == 0 and 0 < s[1] < s[2] and g["pads"]
        assert np.all(g["berr"] <= gc.bound(name, "N")) and gc.error_bound_ok(c, "N", g["X"], g["berr"])
        assert np.array_equal(_bits(g["X"][:, 0]), _bits(c.X0[:, 0]))
    finally:
        h.destroy()


@pytest.mark.parametrize("name", ["d_diag_n513_t4", "z_diag_n513_t4", "d_diag_large"])
def test_two_calls_give_the_same_bits(name):
    """"diag" cases on a deterministic handle: X, berr, steps and solves repeat bit for bit (no floating-point atomics in the reductions); d_diag_large wraps
    the grid-stride loops of the Krylov kernels and uses the padded last unit (n odd)"""
    c = CASES[name]
    h, pc = _handle(c, deterministic=True)
    try:
        _attach(h, c, pc)
        B = c.rhs("N")
        a, b = _call(h, c, "N", B, c.X0), _call(h, c, "N", B, c.X0)
        print(name, a["berr"].tolist(), a["steps"], a["solves"].tolist())
        assert np.array_equal(_bits(a["X"]), _bits(b["X"])) and np.array_equal(_bits(a["berr"]), _bits(b["berr"]))
        assert a["steps"] == b["steps"] and a["solves"].tolist() == b["solves"].tolist() and a["steps"] >= 1
        assert np.all(a["berr"] <= gc.bound(name, "N"))
    finally:
        h.destroy()


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_replaced_tiny_pivots_through_the_real_factorisation(z):
    """t = 3 pairs (p, p + 1) of a diagonally dominant matrix are cut off from the rest and hold the block [[4, 4], [4, 4 + 2^-38]]: whichever of the two is
    eliminated first, the other's pivot is about 2^-38 by cancellation, below thresh = 2^-24 ||A||_1, so replace_tiny_pivot puts +-thresh there and L U
    differs from A by an exact rank-3 term; (L U)^-1 A has three eigenvalues near 2^-14 / ||A||_1.  All rows are of order one.  The true matrix is attached.
    Asserted: the GMRES entry point meets the accuracy bound (the plain loop's result is printed, not asserted)."""
    import scipy.sparse as sp
    n, S = 257, (9, 100, 201)
    A = gc._lu_matrix(n, z).tolil()
    for p in S:
        for q in (p, p + 1):
            A[q, :] = 0; A[:, q] = 0
        A[p, p] = 4.0; A[p, p + 1] = 4.0; A[p + 1, p] = 4.0; A[p + 1, p + 1] = 4.0 + 2.0 ** -38
    A = A.tocsr(); A.eliminate_zeros(); A.sort_indices()
    vt = np.complex128 if z else np.float64
    i = np.arange(n)
    xs = ((((3 * i + 7) % 11) - 5) + (1j * (((5 * i + 1) % 7) - 3) if z else 0)).astype(vt).reshape(n, 1)
    b = np.asfortranarray(A @ xs)
    rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    x, info, st, h, symb = driver.pdgssvx3d(n, rp, ci, A.data, b, replace_tiny=True, keep=True)
    try:
        assert info == 0
        h.attach_matrix(n, rp, ci, A.data, symb.perm_c)
        aM = sp.csr_matrix((gc._abs1(A.data), A.indices, A.indptr), shape=A.shape)
        xref = np.linalg.solve(A.toarray(), b[:, 0])
        ref = gc.berr_of(A, aM, xref, b[:, 0], n)[1]
        _, pberr, psteps = h.pdgsrfs3d(b, x)
        xg, berr, steps, solves = h.pdgsrfs3d(b, x, method="gmres")
        print("tiny pivots", "z" if z else "d", "berr_ref", ref, "plain", pberr.tolist(), psteps, "gmres", berr.tolist(), steps, solves.tolist())
        assert berr[0] <= 4.0 * max(2.0 ** -53, ref), (berr.tolist(), ref)
    finally:
        h.destroy(); symb.free()


def _rc(h, z, trans, B, X, n, nrhs, opt, name=None, berr=True):
    name = name or ("sluamd_pzgsrfs3d_gmres" if z else "sluamd_pdgsrfs3d_gmres")
    be, steps = np.zeros(max(nrhs, 1)), C.c_int32(-7)
    rc = _lib.entry(name)(h, trans, B.ctypes.data_as(C.c_void_p), n, X.ctypes.data_as(C.c_void_p), n, nrhs, None if opt is None else C.byref(opt),
                          be.ctypes.data_as(C.POINTER(C.c_double)) if berr else None, C.byref(steps), None)
    return rc, _lib.load().sluamd_last_error().decode(), steps.value


def test_errors_and_nrhs_zero():
    c = CASES["d_diag_n65_t1"]
    h, pc = _handle(c)
    try:
        B, X = c.rhs("N"), c.X0.copy(order="F")
        rc, msg, _ = _rc(h._h, False, 0, B, X, c.n, 1, None)
        assert rc != 0 and "sluamd_dAttachMatrix" in msg                                                                               # no attached matrix
        _attach(h, c, pc)
        for kw, word in ((dict(restart=0), "restart"), (dict(restart=65), "restart"), (dict(max_solves=0), "max_solves"), (dict(inner_tol=0.0), "inner_tol"),
                         (dict(inner_tol=1.0), "inner_tol"), (dict(inner_tol=float("nan")), "inner_tol")):
            o = driver._gmres_opt("gmres", kw.get("restart"), kw.get("inner_tol"), kw.get("max_solves"))
            rc, msg, _ = _rc(h._h, False, 0, B, X, c.n, 1, o)
            assert rc != 0 and word in msg and msg.startswith("sluamd_pdgsrfs3d_gmres"), (kw, rc, msg)
            assert np.array_equal(_bits(X), _bits(c.X0))
        rc, msg, _ = _rc(h._h, False, 3, B, X, c.n, 1, None)
        assert rc != 0 and "trans" in msg
        rc, msg, _ = _rc(h._h, True, 0, B, X, c.n, 1, None)
        assert rc != 0 and "sluamd_pdgsrfs3d_gmres" in msg and "double handle" in msg                                                  # wrong precision
        rc, msg, _ = _rc(h._h, False, 0, B, X, c.n, 1, None, berr=False)
        assert rc != 0 and "bad refinement arguments" in msg
        rc, msg, steps = _rc(h._h, False, 0, B, X, c.n, 0, None)
        assert rc == 0 and steps == 0
        with pytest.raises(ValueError):
            h.pdgsrfs3d(B, X, method="krylov")
        with pytest.raises(ValueError):
            h.pdgsrfs3d(B, X, restart=3)
        with pytest.raises(ValueError):
            h.pdgsrfs3d(B, X, method="gmres", trans="X")
        with pytest.raises(ValueError):
            h.pdgsrfs3d(B.astype(np.complex128), X, method="gmres")
        with pytest.raises(ValueError):
            h.pdgsrfs3d(B, X[:-1], method="gmres")
        with pytest.raises(RuntimeError, match="restart"):
            h.pdgsrfs3d(B, X, method="gmres", restart=100)
    finally:
        h.destroy()


def test_batch_and_grid_handles_are_refused():
    from superlu_dist_amd import grid3d
    c = CASES["d_lu_n65_t1"]
    A = c.A
    rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    B, X = c.rhs("N"), c.X0.copy(order="F")
    vals = np.stack([A.data, 2 * A.data])
    xb, info, st = driver.pdgssvx3d_batch(c.n, rp, ci, vals, np.ones((2, c.n)), keep=True)
    bh = st["handle"]
    try:
        B2, X2 = np.zeros((2 * c.n, 1), order="F"), np.zeros((2 * c.n, 1), order="F")
        rc, msg, _ = _rc(bh.handle(), False, 0, B2, X2, 2 * c.n, 1, None)
        assert rc != 0 and "batch" in msg, (rc, msg)
    finally:
        bh.destroy()
    symb = driver.Symbolic(c.n, rp, ci, np.arange(c.n, dtype=np.int32), relax=4, maxsup=32)
    tree = symb.partition(2)
    comms = grid3d.local_comms(1, 1, 2)

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, A.data, comms[rank], tree)
        try:
            rpa, cia, ava = c.csr()
            h.attach_matrix(c.n, rpa, cia, ava, symb.perm_c)
            return _rc(h._h, False, 0, B, X.copy(order="F"), c.n, 1, None)
        finally:
            h.destroy()

    try:
        out = grid3d.run_ranks(2, body)
    finally:
        symb.free()
    for rc, msg, _ in out:
        assert rc != 0 and "1 x 1 x 1" in msg, (rc, msg)


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_python_surface(z):
    c = CASES["z_lu_n65_t1" if z else "d_lu_n65_t1"]
    h, pc = _handle(c)
    try:
        _attach(h, c, pc)
        B = c.rhs("N")
        out = h.pdgsrfs3d(B, c.X0)
        assert len(out) == 3 and out[0].shape == (c.n, 1) and out[1].shape == (1,) and isinstance(out[2], int)         # the default return is unchanged
        x, berr, steps, solves = h.pdgsrfs3d(B, c.X0, method="gmres", restart=8, inner_tol=2.0 ** -20, max_solves=50)
        assert x.shape == (c.n, 1) and berr.shape == (1,) and isinstance(steps, int) and solves.shape == (1,) and solves.dtype == np.int32
        assert berr[0] <= gc.bound(c.name, "N")[0] and 0 < solves[0] <= 50
        x1, berr1, steps1, solves1 = h.pdgsrfs3d(B[:, 0].copy(), c.X0[:, 0].copy(), method="gmres")                       # (n,) arguments
        assert berr1[0] <= gc.bound(c.name, "N")[0]
    finally:
        h.destroy()
    # the expert driver: refine="gmres" beside refine=True, with and without equilibration, on the factored matrix itself (nothing for GMRES to repair: the
    # accuracy of the plain refinement at no more outer steps)
    A = c.A
    rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    b = np.asfortranarray(A @ c.xs)
    import scipy.sparse as sp
    aM = sp.csr_matrix((gc._abs1(A.data), A.indices, A.indptr), shape=A.shape)
    ref = gc.berr_of(A, aM, np.linalg.solve(A.toarray(), b[:, 0]), b[:, 0], c.n)[1]             # (equilibration leaves this matrix alone or scales by powers near 1)
    for equil in (False, True):
        x, info, st = driver.pdgssvx3d(c.n, rp, ci, A.data, b, refine="gmres", equil=equil)
        xp, infop, stp = driver.pdgssvx3d(c.n, rp, ci, A.data, b, refine=True, equil=equil)
        print("driver", equil, st["berr"], st["refine_steps"], st["refine_solves"], stp["berr"], stp["refine_steps"])
        assert info == 0 and st["berr"][0] <= 4 * max(2.0 ** -53, ref) and "refine_solves" in st and "refine_solves" not in stp
        assert np.abs(x - c.xs).max() <= 2.0 ** -40 * np.abs(c.xs).max()
    with pytest.raises(ValueError):
        driver.pdgssvx3d(c.n, rp, ci, A.data, b, refine="gmres2")
    with pytest.raises(ValueError):
        driver.pdgssvx3d(c.n, rp, ci, A.data, b, refine="gmres", grid=(1, 1, 2))


def test_c_example_refine_gmres():
    """examples/pddrive3d_amd N --refine gmres: the C ABI from plain C with NULL options.  A check of the flag and of the call, not of accuracy (the cases above
    are): on the factored matrix itself berr only has to lie outside the failure region, and every cycle costs at most restart + 1 = 21 applications"""
    import re
    exe = os.path.join(ROOT, "examples", "pddrive3d_amd")
    r = subprocess.run([exe, "8", "--refine", "gmres"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    m = re.search(r"GMRES refinement: outer steps (\d+)  applications of the factors (\d+)", r.stdout)
    b = re.search(r"berr (\S+)", r.stdout)
    assert m and b and float(b.group(1)) < 2.0 ** -20 and int(m.group(2)) <= 21 * int(m.group(1)), r.stdout[-800:]
    r = subprocess.run([exe, "8", "--refine", "gmres", "--equil"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--refine gmres" in r.stderr
