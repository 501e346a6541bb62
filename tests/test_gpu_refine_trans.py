"""Iterative refinement of the transposed and conjugate-transposed systems (sluamd_p[dz]gsrfs3d_trans[_dev], LUHandle.pdgsrfs3d(trans=)): the residual kernels
k_rfs_residual<V, true, CONJ> over the transposed index, the transposed sweeps as the correction, the loop of sluamd_refine.h.

Exact part: tests/refine_trans_cases.py predicts berr of every pass, every stop decision, the step count and the final X in integers (its own bounds
asserted by test_refine_trans_cases_cpu.py); every comparison of values here is numpy.array_equal on bit patterns, the step counts are integers.
Floating-point part: one equilibrated system per precision, with the bar test_gpu_equil.py holds the untransposed path to (berr <= 4 * 2^-53).  All on
1 x 1 x 1 handles; the 1 x 1 x 2 grid only returns its error."""
import ctypes as C
import os
import numpy as np
import pytest
import scipy.sparse as sp
import equil_cases as ec
import refine_exact_cases as rx
import refine_trans_cases as rt
import trans_cases as tc
from superlu_dist_amd import _lib, driver, grid3d

pytestmark = pytest.mark.gpu
CASES = rt.cases()
EPS = 2.0 ** -53


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


def _check(name, got, what="", r=None):
    X, berr, steps = got
    r = rt.expected(name) if r is None else r
    print(name, what, "steps", steps, "expected", r["steps_all"], "berr", np.asarray(berr).tolist(), "expected", r["berr"].tolist())
    assert steps == r["steps"], (name, what, steps, r["steps_all"])
    assert np.array_equal(_bits(berr), _bits(r["berr"])), (name, what, np.asarray(berr).tolist(), r["berr"].tolist())
    bad = np.flatnonzero(_bits(X) != _bits(r["X"]))
    assert bad.size == 0, (name, what, "X differs at", bad[:8].tolist())


def _run(h, c, trans=None, attach=True):
    if attach:
        h.attach_matrix(c.n, c.rp, c.ci, c.av, c.pc)
    return h.pdgsrfs3d(c.B.copy(order="F"), c.X0.copy(order="F"), trans=trans or c.trans)


class _DevBuf:
    """device memory through the HIP runtime itself (the library has initialised it; no second framework in the process)"""
    hip = None

    def __init__(self, a):
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


def _run_dev(h, c):
    """the _dev form with ldb = n + 3 and ldx = n + 5, the padding rows holding position-tagged NaN payloads: (X, berr, steps), B and the padding of X
    asserted bitwise unchanged"""
    n, vs, nrhs = c.n, 2 if c.z else 1, c.nrhs
    bufs = []
    for a, pad_rows, tag in ((c.B, 3, 1), (c.X0, 5, 2)):
        buf = np.zeros(((n + pad_rows) * vs, nrhs), dtype=np.uint64, order="F")
        for q in range(nrhs):
            buf[:n * vs, q] = np.ascontiguousarray(a[:, q]).view(np.uint64)
        buf[n * vs:, :] = 0x7FF8000000000000 + 256 * tag + 1 + np.arange(pad_rows * vs, dtype=np.uint64)[:, None] + 16 * np.arange(nrhs, dtype=np.uint64)[None, :]
        bufs.append(buf)
    dB, dX = _DevBuf(bufs[0]), _DevBuf(bufs[1])
    try:
        berr, steps = h.pdgsrfs3d_dev(dB.ptr.value, n + 3, dX.ptr.value, n + 5, nrhs, trans=c.trans)
        gB, gX = dB.host(), dX.host()
    finally:
        dB.free(); dX.free()
    assert np.array_equal(gB, bufs[0]) and np.array_equal(gX[n * vs:, :], bufs[1][n * vs:, :]), c.name
    vt = np.complex128 if c.z else np.float64
    X = np.stack([np.ascontiguousarray(gX[:n * vs, q]).view(vt) for q in range(nrhs)], axis=1)
    return X, berr, steps


def _groups():
    """the cases by handle: (kind, n, z) -> names"""
    g = {}
    for k, c in CASES.items():
        g.setdefault((c.kind, c.n, c.z), []).append(k)
    return g


@pytest.mark.parametrize("key", list(_groups()), ids=lambda k: "%s-n%d-%s" % (k[0], k[1], "z" if k[2] else "d"))
def test_host_and_dev_forms_follow_the_exact_trajectory(key):
    """every case, host arrays and device pointers: X, berr and the step count of the simulator, bitwise; a second call returns the same bits.  The cases of
    one factored system share its handle, so every case but the first also runs behind another matrix's index, work vectors and maximum."""
    kind, n, z = key
    h = _factored(kind, n, z)
    try:
        for name in _groups()[key]:
            c = CASES[name]
            B0, X0 = c.B.copy(), c.X0.copy()
            first = _run(h, c)
            _check(name, first)
            assert np.array_equal(_bits(c.B), _bits(B0)) and np.array_equal(_bits(c.X0), _bits(X0))
            _check(name, _run_dev(h, c), "dev")
            again = _run(h, c, attach=False)                                                # the index, the work vectors and the maximum word are reused
            assert again[2] == first[2] and np.array_equal(_bits(again[0]), _bits(first[0])) and np.array_equal(_bits(again[1]), _bits(first[1])), name
    finally:
        h.destroy()


def test_three_right_hand_sides_report_the_steps_of_the_last():
    for name in ("t_d_rhs3", "c_z_rhs3", "sw_rhs3_t_narrow", "sw_rhs3_c_z_narrow"):
        c = CASES[name]
        r = rt.expected(name)
        assert r["steps_all"] == [0, 2, 1] and r["steps"] == 1
        h = _factored(c.kind, c.n, c.z)
        try:
            X, berr, steps = _run(h, c)
            assert steps == 1 and np.array_equal(_bits(berr), _bits(r["berr"])) and np.array_equal(_bits(X), _bits(r["X"]))
            for j, want in enumerate(r["steps_all"]):                                       # column by column: the counts differ
                x, be, st = h.pdgsrfs3d(c.B[:, j].copy(), c.X0[:, j].copy(), trans=c.trans)
                assert st == want and np.array_equal(_bits(x[:, 0]), _bits(r["X"][:, j])) and _bits(be)[0] == _bits(r["berr"])[j]
        finally:
            h.destroy()


def test_notrans_is_the_existing_refinement_and_conj_is_trans_on_a_double_handle():
    """trans = N through the new entry points against pdgsrfs3d on the same handle, bitwise: two kind-"diag" cases (their untransposed run is not designed,
    but a diagonal factor has one summation order) and rx's own exact untransposed case on the real sweeps"""
    for name in ("t_d_half_go", "t_z_half_go", "sw_nil_narrow"):
        c = CASES[name] if name in CASES else rx.cases()[name]
        h = _factored(c.kind, c.n, c.z, deterministic=True)
        try:
            h.attach_matrix(c.n, c.rp, c.ci, c.av, c.pc)
            ref = h.pdgsrfs3d(c.B.copy(order="F"), c.X0.copy(order="F"))                    # today's entry point
            fn = _lib.entry("sluamd_pzgsrfs3d_trans" if c.z else "sluamd_pdgsrfs3d_trans")
            X = c.X0.copy(order="F"); B = c.B.copy(order="F")
            berr = np.zeros(c.nrhs); steps = C.c_int32(-1)
            _lib.check(fn(h._h, 0, B.ctypes.data_as(C.c_void_p), c.n, X.ctypes.data_as(C.c_void_p), c.n, c.nrhs, berr.ctypes.data_as(C.POINTER(C.c_double)),
                          C.byref(steps)), "trans = N")
            assert steps.value == ref[2] and np.array_equal(_bits(X), _bits(ref[0])) and np.array_equal(_bits(berr), _bits(ref[1])), name
            assert "refine.transposed_index" not in h.setup_times()                       # ... and nothing else: no index was built
            if name in CASES and not c.z:
                t, cc = _run(h, c, "T", attach=False), _run(h, c, "C", attach=False)
                _check(name, t)
                assert t[2] == cc[2] and np.array_equal(_bits(t[0]), _bits(cc[0])) and np.array_equal(_bits(t[1]), _bits(cc[1])), name
                assert h.setup_times()["refine.transposed_index"] > 0
        finally:
            h.destroy()


def test_reattaching_another_pattern_rebuilds_the_index():
    """matrices of other patterns (and other numbers of entries) in turn on one handle: the trajectory is the attached matrix's"""
    for z, seq in ((False, ("t_d_half_go", "t_d_rhs3", "t_d_nilpotent", "t_d_half_go", "t_d_rows_last", "t_d_half_long")),
                   (True, ("c_z_half_go", "t_z_rhs3", "z_split_C", "z_split_T", "c_z_nilpotent", "t_z_half_go"))):
        assert len({(len(CASES[k].av), CASES[k].ci.tobytes()) for k in seq}) >= 4
        h = _factored("diag", 65, z)
        try:
            for name in seq:
                _check(name, _run(h, CASES[name]), "re-attached")
        finally:
            h.destroy()


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_update_values_reach_the_residual_through_the_index(z):
    """rt.update_pair: the first transposed run builds the index for the attached values v1; update_values(v2) rewrites the attached values in place; the
    run after it is the simulator's for v2 on the new factors.  An index that carried v1's values would compute rt.update_pair's `stale` run instead
    (another berr, asserted by the CPU test)."""
    u = rt.update_pair(z)
    n, rp, ci = u["n"], u["rp"], u["ci"]
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=64, unsym=True)
    h = driver.LUHandle.from_symbolic(symb, u["v0"])
    try:
        assert np.array_equal(symb.perm_c, u["first"].pc) and h.pdgstrf3d(0.0) == 0
        _check("upd_first", _run(h, u["first"]), "first values", rt.simulate(u["first"]))
        assert h.update_values(u["second"].av) is None and h.pdgstrf3d(0.0) == 0             # the handle and the attached matrix hold v2 now
        _check("upd_second", _run(h, u["second"], attach=False), "after update_values", rt.simulate(u["second"]))
    finally:
        h.destroy(); symb.free()


@pytest.mark.parametrize("z,trans", [(False, "T"), (True, "C")])
def test_equilibrated_transposed_system_end_to_end(z, trans):
    """equil_cases.scaled_operator case (a), equed = B.  By hand: b' = C o b, the transposed solve on Pc b', then the transposed refinement of the scaled
    system op(A_s) x' = b' (x = R o x').  berr <= 4 * 2^-53, the bar of the untransposed path in test_gpu_equil.py, and the residual is no worse than before"""
    n, rp, ci, v, perm, rs, cs = ec.scaled_operator(mode="a", z=z)
    e = ec.equilibrate(n, rp, ci, v)
    assert e["equed"] == "B"
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    opA = A.conj().T if trans == "C" else A.T
    rng = np.random.default_rng(5)
    xt = rng.choice([-1.0, 1.0], (n, 2)).astype(v.dtype)
    b = np.asfortranarray(opA @ xt)
    symb = driver.Symbolic(n, rp, ci, perm, relax=8, maxsup=64)
    h = driver.LUHandle.from_symbolic(symb, v)
    try:
        d = h.equilibrate(n, rp, ci, v, symb.perm_c)
        assert d["equed"] == "B" and h.pdgstrf3d(0.5 * float(np.finfo(np.float32).eps) * d["anorm"]) == 0
        R, Cs = h.scalings()
        assert np.array_equal(R, e["R"]) and np.array_equal(Cs, e["C"])
        bs = np.asfortranarray(Cs[:, None] * b)
        xp = np.zeros_like(bs, order="F"); xp[symb.perm_c, :] = bs
        x0 = np.asfortranarray(h.pdgstrs3d(xp, trans=trans)[symb.perm_c, :])
        As = sp.csr_matrix((e["vals"], ci, rp), shape=(n, n))
        opAs = As.conj().T if trans == "C" else As.T
        res0 = float(np.abs(opAs @ x0 - bs).max())
        x1, berr, steps = h.pdgsrfs3d(bs, x0, trans=trans)
        res1 = float(np.abs(opAs @ x1 - bs).max())
        a1 = lambda M: abs(M.real) + abs(M.imag)                                            # abs1; the modulus on real data
        r = opAs @ x1 - bs
        host_berr = (a1(r) / (a1(opAs) @ a1(x1) + a1(bs))).max(axis=0)
        print("berr / eps", (berr / EPS).tolist(), "host", (host_berr / EPS).tolist(), "steps", steps, "residual before", res0, "after", res1)
        assert np.all(berr <= 4 * EPS)
        assert res1 <= res0
    finally:
        h.destroy(); symb.free()


def test_error_codes():
    L = _lib.load()
    fd, fz = _lib.entry("sluamd_pdgsrfs3d_trans"), _lib.entry("sluamd_pzgsrfs3d_trans")
    fdd, fzd = _lib.entry("sluamd_pdgsrfs3d_trans_dev"), _lib.entry("sluamd_pzgsrfs3d_trans_dev")
    hd, hz = _factored("diag", 65, False), _factored("diag", 65, True)
    try:
        n = 65
        xd, xz = np.ones((n, 1), order="F"), np.ones((n, 1), dtype=np.complex128, order="F")
        berr = np.zeros(1); steps = C.c_int32(7)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        pb = berr.ctypes.data_as(C.POINTER(C.c_double))
        err = lambda: L.sluamd_last_error().decode()
        # no matrix attached
        for trans in (1, 2):
            assert fd(hd._h, trans, p(xd), n, p(xd), n, 1, pb, C.byref(steps)) == -1 and "no matrix attached" in err()
            assert fz(hz._h, trans, p(xz), n, p(xz), n, 1, pb, C.byref(steps)) == -1 and "no matrix attached" in err()
        cd, cz = CASES["t_d_half_go"], CASES["t_z_half_go"]
        hd.attach_matrix(cd.n, cd.rp, cd.ci, cd.av, cd.pc); hz.attach_matrix(cz.n, cz.rp, cz.ci, cz.av, cz.pc)
        # trans outside {0, 1, 2}
        for trans in (3, -1):
            assert fd(hd._h, trans, p(xd), n, p(xd), n, 1, pb, C.byref(steps)) == -1 and "trans" in err()
            assert fzd(hz._h, trans, p(xz), n, p(xz), n, 1, pb, C.byref(steps)) == -1 and "trans" in err()
        # the other precision's call
        for trans in (0, 1, 2):
            assert fd(hz._h, trans, p(xz), n, p(xz), n, 1, pb, C.byref(steps)) == -1 and "complex16 handle" in err()
            assert fdd(hz._h, trans, p(xz), n, p(xz), n, 1, pb, C.byref(steps)) == -1
            assert fz(hd._h, trans, p(xd), n, p(xd), n, 1, pb, C.byref(steps)) == -1 and "double handle" in err()
            assert fzd(hd._h, trans, p(xd), n, p(xd), n, 1, pb, C.byref(steps)) == -1
        assert steps.value == 7 and np.array_equal(xd, np.ones((n, 1)))                     # nothing was touched
        # nrhs == 0
        for trans in (0, 1, 2):
            steps.value = 7
            assert fd(hd._h, trans, p(xd), n, p(xd), n, 0, pb, C.byref(steps)) == 0 and steps.value == 0
            steps.value = 7
            assert fz(hz._h, trans, p(xz), n, p(xz), n, 0, pb, C.byref(steps)) == 0 and steps.value == 0
        with pytest.raises(ValueError):
            hd.pdgsrfs3d(xd, xd, trans="X")
    finally:
        hd.destroy(); hz.destroy()


def test_grid_handles_refuse_transposed_refinement_on_every_rank():
    """a 1 x 1 x 2 in-process grid: SLUAMD_EINVAL with the "1 x 1 x 1" message on both ranks, before any collective step; the untransposed refinement of the
    same handles still runs"""
    s = tc.prepared("narrow")[0]
    n, rp, ci = s.pattern_csr()
    v = s.B[np.repeat(np.arange(n), np.diff(rp)), ci].copy()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=s.maxsup, unsym=True)
    tree = symb.partition(2)
    comms = grid3d.local_comms(1, 1, 2)
    c = CASES["sw_nil_t_narrow"]
    u = rx.cases()["sw_nil_narrow"]
    fn = _lib.entry("sluamd_pdgsrfs3d_trans")

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], tree)
        try:
            info = h.pdgstrf3d(0.0)
            h.attach_matrix(c.n, c.rp, c.ci, c.av, c.pc)
            out = []
            for trans in (1, 2):
                X = c.X0.copy(order="F"); berr = np.zeros(1); steps = C.c_int32(7)
                rc = fn(h._h, trans, c.B.ctypes.data_as(C.c_void_p), n, X.ctypes.data_as(C.c_void_p), n, 1, berr.ctypes.data_as(C.POINTER(C.c_double)), C.byref(steps))
                out.append((rc, _lib.load().sluamd_last_error().decode(), bool(np.array_equal(X, c.X0)), steps.value))
            h.attach_matrix(u.n, u.rp, u.ci, u.av, u.pc)
            ref = h.pdgsrfs3d(u.B.copy(order="F"), u.X0.copy(order="F"))
        finally:
            h.destroy()
        return info, out, ref

    res = grid3d.run_ranks(2, body)
    symb.free()
    r = rx.expected("sw_nil_narrow")
    for info, out, ref in res:
        assert info == 0
        for rc, msg, untouched, steps in out:
            assert rc == -1 and "1 x 1 x 1" in msg and untouched and steps == 7, (rc, msg)
        assert ref[2] == r["steps"] and np.array_equal(_bits(ref[0]), _bits(r["X"]))
