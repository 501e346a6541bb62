"""Blocked iterative refinement (sluamd_p[dz]gsrfs3d_block[_dev], LUHandle.pdgsrfs3d(block=True)): the block kernels k_rfs_residual_block /
k_rfs_update_block and the panel loop of sluamd_brefine.cpp.

Exact part: tests/refine_block_cases.py predicts per column berr, the step count and the final X in integers (its designed facts are asserted by
test_refine_block_cases_cpu.py); every comparison of values is numpy.array_equal on bit patterns, the step counts are integers.  Rounding part: on diagonal
factors the correction is an exact scaling, so with non-dyadic data the trajectory is fixed by the residual and update kernels alone and the block form must
be bitwise the column form.  Then: the sweeps really run on blocks (SLUAMD_SOLVE_DEBUG), general data, grids, refusals, storage."""
import ctypes as C
import os, re, subprocess, sys
import numpy as np
import pytest
import scipy.sparse as sp
import refine_block_cases as bc
import refine_exact_cases as rx
import trans_cases as tc
from superlu_dist_amd import _lib, driver, grid3d, matgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = bc.cases()
EPS = 2.0 ** -53
TCODE = {"N": 0, "T": 1, "C": 2}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _copy(fs):
    return driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind.copy(), fs.Lnzval_off, fs.Lnzval.copy(), fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off,
                            fs.Unzval.copy())


def _factored(kind, n, z, **kw):
    """a handle holding the exact factors of a case kind (asserted)"""
    fs0, expL, expU = rx.diag_store(n, z) if kind == "diag" else tc.prepared(kind)[1:4]
    fs = _copy(fs0)
    h = driver.LUHandle.from_store(fs, **kw)
    assert h.z == z and h.pdgstrf3d(0.0) == 0
    h.copy_to_host()
    assert np.array_equal(fs.Lnzval, expL) and np.array_equal(fs.Unzval, expU), kind
    return h


class _Dev:
    """device memory through the HIP runtime itself (the library has initialised it; no second framework in the process)"""
    hip = None

    def __init__(self, a):
        if _Dev.hip is None:
            _Dev.hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.a = np.asfortranarray(a)
        self.ptr = C.c_void_p()
        assert _Dev.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(max(self.a.nbytes, 8))) == 0
        assert _Dev.hip.hipMemcpy(self.ptr, self.a.ctypes.data_as(C.c_void_p), C.c_size_t(self.a.nbytes), 1) == 0

    def host(self):
        out = np.empty_like(self.a, order="F")
        assert _Dev.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        _Dev.hip.hipFree(self.ptr)


def _padded(b):
    """(B, X0) of a case as 64-bit patterns with ldb = n + 3 and ldx = n + 5, the padding rows holding position-tagged NaN payloads"""
    c = b.c
    n, vs, nrhs = b.n, 2 if b.z else 1, b.nrhs
    bufs = []
    for a, pad_rows, tag in ((c.B, 3, 1), (c.X0, 5, 2)):
        buf = np.zeros(((n + pad_rows) * vs, nrhs), dtype=np.uint64, order="F")
        for q in range(nrhs):
            buf[:n * vs, q] = np.ascontiguousarray(a[:, q]).view(np.uint64)
        buf[n * vs:, :] = 0x7FF8000000000000 + 256 * tag + 1 + np.arange(pad_rows * vs, dtype=np.uint64)[:, None] + 64 * np.arange(nrhs, dtype=np.uint64)[None, :]
        bufs.append(buf)
    return bufs


def _raw(h, b, dev, with_steps=True):
    """the C entry point on padded blocks, host or device pointers: (X, berr, steps); B and the padding of X asserted bitwise unchanged"""
    n, vs, nrhs = b.n, 2 if b.z else 1, b.nrhs
    B0, X0 = _padded(b)
    fn = _lib.entry("sluamd_p%sgsrfs3d_block%s" % ("z" if b.z else "d", "_dev" if dev else ""))
    berr = np.full(nrhs, -1.0); steps = np.full(nrhs, -7, dtype=np.int32)
    ps = steps.ctypes.data_as(C.POINTER(C.c_int32)) if with_steps else None
    if dev:
        dB, dX = _Dev(B0), _Dev(X0)
        try:
            _lib.check(fn(h._h, TCODE[b.trans], dB.ptr, n + 3, dX.ptr, n + 5, nrhs, berr.ctypes.data_as(C.POINTER(C.c_double)), ps), b.name)
            gB, gX = dB.host(), dX.host()
        finally:
            dB.free(); dX.free()
    else:
        gB, gX = B0.copy(order="F"), X0.copy(order="F")
        _lib.check(fn(h._h, TCODE[b.trans], gB.ctypes.data_as(C.c_void_p), n + 3, gX.ctypes.data_as(C.c_void_p), n + 5, nrhs,
                      berr.ctypes.data_as(C.POINTER(C.c_double)), ps), b.name)
    assert np.array_equal(gB, B0) and np.array_equal(gX[n * vs:, :], X0[n * vs:, :]), (b.name, "B or the padding rows of X changed")
    vt = np.complex128 if b.z else np.float64
    X = np.stack([np.ascontiguousarray(gX[:n * vs, q]).view(vt) for q in range(nrhs)], axis=1)
    return X, berr, steps


def _check(name, got, what):
    X, berr, steps = got
    r = bc.expected(name)
    print(name, what, "steps", list(map(int, steps)), "expected", r["steps_all"], "berr", np.asarray(berr).tolist())
    assert list(map(int, steps)) == r["steps_all"], (name, what, list(map(int, steps)), r["steps_all"])
    assert np.array_equal(_bits(berr), _bits(r["berr"])), (name, what, np.asarray(berr).tolist(), r["berr"].tolist())
    bad = np.flatnonzero(_bits(np.asfortranarray(X)) != _bits(np.asfortranarray(r["X"])))
    assert bad.size == 0, (name, what, "X differs at", bad[:8].tolist())


def _groups():
    g = {}
    for k, b in CASES.items():
        g.setdefault((b.kind, b.n, b.z), []).append(k)
    return g


@pytest.mark.parametrize("key", list(_groups()), ids=lambda k: "%s-n%d-%s" % (k[0], k[1], "z" if k[2] else "d"))
def test_block_forms_follow_every_columns_exact_trajectory(key):
    """every case through LUHandle (host arrays), the host entry point and the device entry point with padded leading dimensions: berr[nrhs], steps[nrhs] and
    X of the simulator, bitwise; columns that stop at pass 0 come back untouched; the column entry points on the same handle give the same berr and X"""
    kind, n, z = key
    h = _factored(kind, n, z)
    try:
        for name in _groups()[key]:
            b = CASES[name]
            c = b.c
            h.attach_matrix(c.n, c.rp, c.ci, c.av, c.pc)
            B0, X0 = c.B.copy(), c.X0.copy()
            got = h.pdgsrfs3d(c.B, c.X0, trans=b.trans, block=True)
            _check(name, got, "LUHandle")
            assert np.array_equal(_bits(c.B), _bits(B0)) and np.array_equal(_bits(c.X0), _bits(X0))
            for j, s in enumerate(b.steps):
                if s == 0:
                    assert np.array_equal(_bits(got[0][:, j]), _bits(c.X0[:, j])), (name, j)
            _check(name, _raw(h, b, dev=False), "host, padded")
            _check(name, _raw(h, b, dev=True), "dev, padded")
            dB, dX = _Dev(c.B), _Dev(c.X0)                                                  # LUHandle's device form, ld = n
            try:
                be, stp = h.pdgsrfs3d_dev(dB.ptr.value, c.n, dX.ptr.value, c.n, b.nrhs, trans=b.trans, block=True)
                _check(name, (dX.host(), be, stp), "LUHandle.pdgsrfs3d_dev")
            finally:
                dB.free(); dX.free()
            xc, bec, stc = h.pdgsrfs3d(c.B, c.X0, trans=b.trans)                            # the column form
            assert stc == b.steps[-1] and np.array_equal(_bits(bec), _bits(got[1])) and np.array_equal(_bits(xc), _bits(got[0])), name
    finally:
        h.destroy()


def _rounding_system(n, z, seed):
    """diag(dvals) factors (rx.diag_store); attached: the factored matrix A[i, i] = d[pc[i]] plus four random off-diagonal entries per row of about 2^-14
    (a contraction of 2^-10 or better per step), values and right-hand sides random, nothing dyadic"""
    rng = np.random.default_rng(seed)
    pc = rx.perm(n)
    d = rx.dvals(n, z)
    rnd = (lambda *s: rng.uniform(0.5, 1.0, s) * rng.choice([-1.0, 1.0], s) + (1j * rng.uniform(-1.0, 1.0, s) if z else 0))
    rows = np.repeat(np.arange(n), 4)
    cols = (rows + rng.integers(1, n, rows.size)) % n
    A = sp.csr_matrix((rnd(rows.size) * 2.0 ** -14, (rows, cols)), shape=(n, n)) + sp.diags(d[pc])
    A = sp.csr_matrix(A); A.sum_duplicates(); A.sort_indices()
    B = np.asfortranarray(rnd(n, 17))
    X0 = np.asfortranarray(B / d[pc][:, None] * (1 + 2.0 ** -20 * rnd(n, 17).real))
    return pc, A, B, X0


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_block_form_rounds_like_the_column_form(z):
    """non-dyadic data on diagonal factors: the correction is an exact scaling in any sweep build, so an FMA contraction or an operand order of the block
    kernels that differed from the column kernels' would change bits.  nrhs 1, 4, 5, 17; N / T / C; X, berr and steps column by column"""
    n = 300
    pc, A, B, X0 = _rounding_system(n, z, 11 + z)
    h = _factored("diag", n, z)
    try:
        h.attach_matrix(n, A.indptr, A.indices, A.data, pc)
        for trans in ("N", "T", "C") if z else ("N", "T"):
            col = [h.pdgsrfs3d(B[:, j].copy(), X0[:, j].copy(), trans=trans) for j in range(17)]
            assert max(s for _, _, s in col) >= 2 and all(be[0] <= 2 * EPS for _, be, _ in col), [(s, be) for _, be, s in col]   # it converges, in a few steps
            for nrhs in (1, 4, 5, 17):
                X, berr, steps = h.pdgsrfs3d(B[:, :nrhs], X0[:, :nrhs], trans=trans, block=True)
                print(trans, nrhs, "steps", steps.tolist(), "berr / eps", (berr / EPS).tolist())
                for j in range(nrhs):
                    assert steps[j] == col[j][2], (trans, nrhs, j, steps.tolist(), [c_[2] for c_ in col])
                    assert _bits(berr)[j] == _bits(col[j][1])[0], (trans, nrhs, j)
                    assert np.array_equal(_bits(X[:, j]), _bits(col[j][0][:, 0])), (trans, nrhs, j)
    finally:
        h.destroy()


def _blocked_child(which):
    b = CASES["sw_narrow_N_16"]
    c = b.c
    h = _factored(b.kind, b.n, b.z)
    h.attach_matrix(c.n, c.rp, c.ci, c.av, c.pc)
    sys.stderr.write("[test] begin\n"); sys.stderr.flush()
    if which == "block":
        h.pdgsrfs3d(c.B, c.X0, block=True)
    else:
        h.pdgsrfs3d(c.B, c.X0)
    sys.stderr.write("[test] end\n"); sys.stderr.flush()
    print("LAUNCHES %d" % h.stats()["solve_launches"])
    h.destroy()
    print("RESULT ok")


def test_the_correction_of_a_panel_is_one_blocked_sweep():
    """a 16-column case whose columns all take at least one step, SLUAMD_SOLVE_DEBUG=1 in a child process: the first correction of the block form launches
    the rk = 16 (MFMA) builds of the sweeps and nothing narrower; the same case through the column entry point launches rk = 1 only"""
    assert min(CASES["sw_narrow_N_16"].steps) >= 1
    out = {}
    for which in ("block", "column"):
        code = ("import os, sys\nsys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\nimport test_gpu_refine_block as t\n"
                "t._blocked_child(%r)\n" % which)
        r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, SLUAMD_SOLVE_DEBUG="1"))
        assert r.returncode == 0 and "RESULT ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
        body = r.stderr.split("[test] begin")[1].split("[test] end")[0]
        out[which] = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"\[sluamd sweep\] .*nrhs=(\d+) rk=(\d+)", body)]
    blk, col = out["block"], out["column"]
    assert blk and col
    first = [rk for nrhs, rk in blk if nrhs == 16]
    assert first and set(first) == {16}, blk[:8]                                            # the first correction: all 16 columns, MFMA blocks
    assert blk[0][0] == 16 and all(nrhs < 16 for nrhs, _ in blk[len(first):])               # ... then the panel shrinks
    assert {nrhs for nrhs, _ in col} == {1} and {rk for _, rk in col} == {1}
    assert len(blk) < len(col)


def test_general_data_poisson_17_right_hand_sides():
    """7-point Poisson 12^3, 17 random right-hand sides, from the plain solve's X: every column's berr is at most eps, or at most twice the column form's
    (the stop rule's own granularity: a step is taken only while it halves berr); berr recomputed in numpy from the returned X"""
    N = 12
    n, rp, ci, v = matgen.poisson3d(N)
    perm = matgen.nd_perm_grid3d(N, N, N, leaf=27)
    rng = np.random.default_rng(3)
    b = np.asfortranarray(rng.standard_normal((n, 17)))
    x, info, st, h, symb = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=16, maxsup=128, keep=True)
    try:
        assert info == 0
        h.attach_matrix(n, rp, ci, v, symb.perm_c)
        xc, bec, _ = h.pdgsrfs3d(b, x)
        xb, beb, steps = h.pdgsrfs3d(b, x, block=True)
        A = sp.csr_matrix((v, ci, rp), shape=(n, n))
        host = (np.abs(A @ xb - b) / (abs(A) @ np.abs(xb) + np.abs(b))).max(axis=0)
        print("block berr / eps", (beb / EPS).tolist(), "column", (bec / EPS).tolist(), "host", (host / EPS).tolist(), "steps", steps.tolist())
        assert steps.shape == (17,) and np.all((beb <= EPS) | (beb <= 2 * bec))
        assert np.all(np.abs(host - beb) <= 4 * EPS * np.maximum(1.0, beb / EPS))          # the same berr up to the rounding of a residual of a few eps
        x2, _, st2 = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=16, maxsup=128, refine="block")
        assert np.asarray(st2["refine_steps"]).shape == (17,) and np.all(st2["berr"] <= np.maximum(EPS, 2 * bec))
    finally:
        h.destroy(); symb.free()


def _driver_child(form):
    """driver.pdgssvx3d(refine="block") against refine=True of the same form, 5 right-hand sides: equil_cases.scaled_operator (a), outcome equed = B, for the
    equilibrated forms (the scaled system is refined), 7-point Poisson 8^3 for the plain grid form"""
    import equil_cases as ec
    kw = {}
    if "equil" in form:
        n, rp, ci, v, perm, _, _ = ec.scaled_operator(mode="a", z=False)
        kw.update(equil=True, relax=8, maxsup=64)
    else:
        n, rp, ci, v = matgen.poisson3d(8)
        perm = matgen.nd_perm_grid3d(8, 8, 8, leaf=27)
        kw.update(relax=16, maxsup=64)
    if "grid" in form:
        kw.update(grid=(1, 1, 2))
    b = np.asfortranarray(np.random.default_rng(9).standard_normal((n, 5)))
    xc, ic, sc = driver.pdgssvx3d(n, rp, ci, v, b, perm, refine=True, **kw)
    xb, ib, sb = driver.pdgssvx3d(n, rp, ci, v, b, perm, refine="block", **kw)
    bec, beb, steps = np.asarray(sc["berr"]), np.asarray(sb["berr"]), np.asarray(sb["refine_steps"])
    print(form, sb.get("equed"), "block berr / eps", (beb / EPS).tolist(), "column", (bec / EPS).tolist(), "steps", steps.tolist(), "column (last)", sc["refine_steps"])
    assert ic == 0 and ib == 0 and ("equil" not in form or sb["equed"] == "B")
    assert steps.shape == (5,) and beb.shape == (5,) and xb.shape == xc.shape == (n, 5)
    assert np.all((beb <= EPS) | (beb <= 2 * bec))                                          # the bar of the general-data test
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    host = (np.abs(A @ xb - b) / (abs(A) @ np.abs(xb) + np.abs(b))).max(axis=0)               # the componentwise berr does not see R and C: the ORIGINAL system's
    print("host berr / eps", (host / EPS).tolist())
    assert np.all(np.abs(host - beb) <= 4 * EPS * np.maximum(1.0, beb / EPS))              # (the bar of the general-data test) x came back in the caller's ordering and scaling
    print("RESULT ok")


@pytest.mark.parametrize("form", ["equil", "grid", "grid_equil"])
def test_driver_forms_refine_block(form):
    """the forms of driver.pdgssvx3d that have refine=True beside the plain one (which the general-data test runs; the rowperm form refuses "block"), in a
    child process under a time limit because the grid forms are collective"""
    code = ("import os, sys\nsys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\nimport test_gpu_refine_block as t\n"
            "t._driver_child(%r)\n" % form)
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    sys.stdout.write(r.stdout[-3000:])
    assert r.returncode == 0 and "RESULT ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    with pytest.raises(ValueError):
        driver.pdgssvx3d(1, [0, 1], [0], [1.0], [1.0], refine="block", rowperm="LargeDiag_MC64")


def _grid_child(kind, Pr, Pc, Pz, expected):
    bc.preload_expected(expected)
    s = tc.prepared(kind)[0]
    n, rp, ci = s.pattern_csr()
    v = s.B[np.repeat(np.arange(n), np.diff(rp)), ci].copy()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=s.maxsup, unsym=True)
    tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)
    todo = [f"sw_{kind}_N_17", f"sw_{kind}_T_17"]
    x5, b5 = s.rhs(5)

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], tree)
        try:
            info = h.pdgstrf3d(0.0)
            y = h.pdgstrs3d(b5.copy(order="F"))
            c = CASES[todo[1]].c
            h.attach_matrix(c.n, c.rp, c.ci, c.av, c.pc)
            refused = None
            try:
                h.pdgsrfs3d(c.B, c.X0, trans="T", block=True)                                # transposed sweeps not planned yet: refused on every rank, before any collective step
            except RuntimeError as e:
                refused = str(e)
            h.plan_transposed()
            res = []
            for name in todo:
                b = CASES[name]
                h.attach_matrix(b.c.n, b.c.rp, b.c.ci, b.c.av, b.c.pc)
                res.append(h.pdgsrfs3d(b.c.B, b.c.X0, trans=b.trans, block=True))
        finally:
            h.destroy()
        return info, y, refused, res

    out = grid3d.run_ranks(Pr * Pc * Pz, body)
    symb.free()
    for rank, (info, y, refused, res) in enumerate(out):
        assert info == 0 and np.array_equal(y, x5), rank                                    # the factors are the exact ones
        assert refused and "sluamd_PlanTransposedSweeps" in refused, refused
        for name, got in zip(todo, res):
            _check(name, got, "rank %d of %s" % (rank, (Pr, Pc, Pz)))
    print("RESULT ok %d" % len(out))


@pytest.mark.parametrize("grid", [(1, 1, 2), (2, 1, 1)], ids=["1x1x2", "2x1x1"])
def test_grid_handles_follow_the_exact_trajectory_on_every_rank(grid, tmp_path):
    """replicated form on thread grids in a child process under a time limit (ranks that split into unmatched collective solves end the test instead of
    hanging it): the 17-column case of the "narrow" sweep kind under N and T; every rank returns the simulator's X, berr and steps.  A transposed call
    before sluamd_PlanTransposedSweeps is refused on every rank"""
    kind = "narrow"
    code = ("import os, sys\nsys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\nimport test_gpu_refine_block as t\n"
            "t._grid_child(%r, %d, %d, %d, sys.argv[2])\n" % ((kind,) + grid))
    bc.dump_expected(str(tmp_path / "expected.pkl"), [f"sw_{kind}_N_17", f"sw_{kind}_T_17"])
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(tmp_path / "expected.pkl")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "RESULT ok 2" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_refusals_and_null_steps():
    L = _lib.load()
    fd, fz = _lib.entry("sluamd_pdgsrfs3d_block"), _lib.entry("sluamd_pzgsrfs3d_block")
    fdd, fzd = _lib.entry("sluamd_pdgsrfs3d_block_dev"), _lib.entry("sluamd_pzgsrfs3d_block_dev")
    hd, hz = _factored("diag", 65, False), _factored("diag", 65, True)
    try:
        n = 65
        xd, xz = np.ones((n, 2), order="F"), np.ones((n, 2), dtype=np.complex128, order="F")
        berr = np.zeros(2); steps = np.full(2, 7, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        pb, ps = berr.ctypes.data_as(C.POINTER(C.c_double)), steps.ctypes.data_as(C.POINTER(C.c_int32))
        err = lambda: L.sluamd_last_error().decode()
        for trans in (0, 1, 2):                                                              # no matrix attached
            assert fd(hd._h, trans, p(xd), n, p(xd), n, 2, pb, ps) == -1 and "no matrix attached" in err()
            assert fz(hz._h, trans, p(xz), n, p(xz), n, 2, pb, ps) == -1 and "no matrix attached" in err()
        bd, bz = CASES["d_cols_2_N"], CASES["z_cols_2_N"]
        hd.attach_matrix(n, bd.c.rp, bd.c.ci, bd.c.av, bd.c.pc); hz.attach_matrix(n, bz.c.rp, bz.c.ci, bz.c.av, bz.c.pc)
        assert fd(hd._h, 3, p(xd), n, p(xd), n, 2, pb, ps) == -1 and "trans" in err()
        for trans in (0, 1, 2):                                                              # the other precision's call
            assert fd(hz._h, trans, p(xz), n, p(xz), n, 2, pb, ps) == -1 and "complex16 handle" in err() and "sluamd_pzgsrfs3d_block" in err()
            assert fzd(hd._h, trans, p(xd), n, p(xd), n, 2, pb, ps) == -1 and "double handle" in err()
            assert fdd(hz._h, trans, p(xz), n, p(xz), n, 2, pb, ps) == -1
        assert fd(hd._h, 0, p(xd), n - 1, p(xd), n, 2, pb, ps) == -1 and fd(hd._h, 0, p(xd), n, p(xd), n, 2, None, ps) == -1
        assert steps.tolist() == [7, 7] and np.array_equal(xd, np.ones((n, 2)))            # nothing was touched
        assert fd(hd._h, 0, p(xd), n, p(xd), n, 0, pb, ps) == 0 and steps.tolist() == [7, 7]   # nrhs == 0
        # steps == NULL is accepted
        _check("d_cols_2_N", _raw(hd, bd, dev=False, with_steps=False)[:2] + (bd.steps,), "steps = NULL")
        _check("z_cols_2_N", _raw(hz, bz, dev=True, with_steps=False)[:2] + (bz.steps,), "steps = NULL, dev")
        with pytest.raises(ValueError):
            hd.pdgsrfs3d(bd.c.B, bd.c.X0, block=True, method="gmres")
        with pytest.raises(ValueError):
            hd.pdgsrfs3d_dev(0, n, 0, n, 2, block=True, method="gmres")
        with pytest.raises(ValueError):
            hd.pdgsrfs3d(bd.c.B.astype(np.float32), bd.c.X0, block=True)
    finally:
        hd.destroy(); hz.destroy()


def test_a_batch_owned_handle_is_refused():
    """the handle of a batch (two diagonal matrices of order 8; the batch attaches its own block-diagonal matrix): SLUAMD_EINVAL, X untouched"""
    n = 8
    rp, ci = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=64, unsym=True)
    bh = driver.BatchHandle.create(symb, np.stack([np.full(n, 2.0), np.full(n, 4.0)]))
    try:
        x = np.ones((2 * n, 1), order="F"); berr = np.zeros(1)
        for name in ("sluamd_pdgsrfs3d_block", "sluamd_pdgsrfs3d_block_dev"):
            rc = _lib.entry(name)(bh.handle(), 0, x.ctypes.data_as(C.c_void_p), 2 * n, x.ctypes.data_as(C.c_void_p), 2 * n, 1,
                                  berr.ctypes.data_as(C.POINTER(C.c_double)), None)
            assert rc == -1 and "batch" in _lib.load().sluamd_last_error().decode(), name
        assert np.array_equal(x, np.ones((2 * n, 1)))
    finally:
        bh.destroy(); symb.free()


def test_a_second_block_call_allocates_nothing():
    """the panels are allocated on the first block call of each form and kept: the library's allocation counter stands still over a second call, also one
    with more right-hand sides and another trans"""
    cnt = _lib.load().sluamd_device_alloc_count
    b1, b2 = CASES["d_cols_2_N"], CASES["d_cols_33_N"]
    h = _factored("diag", 65, False)
    try:
        h.attach_matrix(65, b1.c.rp, b1.c.ci, b1.c.av, b1.c.pc)
        c0 = cnt()
        _check(b1.name, _raw(h, b1, dev=True), "first dev call")
        c1 = cnt()
        assert c1 - c0 >= 2                                                                  # the residual panel and the berr words (and what the sweeps grow for two columns)
        _check(b1.name, _raw(h, b1, dev=True), "second dev call")
        assert cnt() == c1
        _check(b1.name, _raw(h, b1, dev=False), "first host call")
        c2 = cnt()
        assert c2 - c1 >= 1                                                                  # the staged panels of B and X
        _check(b1.name, _raw(h, b1, dev=False), "second host call")
        assert cnt() == c2
        h.attach_matrix(65, b2.c.rp, b2.c.ci, b2.c.av, b2.c.pc)                              # re-attaching releases them with the matrix
        c3 = cnt()
        _check(b2.name, _raw(h, b2, dev=False), "33 columns")
        c4 = cnt()
        assert c4 - c3 >= 3
        _check(b2.name, _raw(h, b2, dev=False), "33 columns again")
        _check(b2.name, _raw(h, b2, dev=True), "33 columns, dev")
        assert cnt() == c4
    finally:
        h.destroy()
