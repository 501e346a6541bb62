"""Transposed and conjugate-transposed solves with the resident factors (sluamd_p[dz]gstrs3d_trans[_dev], LUHandle.pdgstrs3d(trans=), pdgssvx3d(trans=)).

Exact part: the sweep cases of tests/sweep_cases.py with the right-hand sides of tests/trans_cases.py -- b_t = U0^T L0^T x (conjugated for "C") in integer
arithmetic, the bounds of the transposed sweeps asserted below 2^53 -- so every comparison of values is numpy.array_equal with the integer x.
Floating-point part: the recorded fixtures; the yardstick is the normwise backward error of the UNTRANSPOSED solve of the same handle and the same xtrue
(that path is not the code under test): eta_T <= 10 max(eta_N, n eps) -- one order of magnitude because the same factors and inverses are applied in another
order and with atomics; an indexing error shows up as eta >= 1e-3."""
import ctypes as C
import json, os, subprocess, sys
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import pivot_cases as pc
import trans_cases as tc
from superlu_dist_amd import _lib, driver, grid3d, matgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)


def _copy(fs):
    return driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind.copy(), fs.Lnzval_off, fs.Lnzval.copy(), fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off,
                            fs.Unzval.copy())


def _factored(name, **kw):
    """a handle holding the exact factors of case `name` (asserted)"""
    c, fs0, expL, expU = tc.prepared(name)[:4]
    fs = _copy(fs0)
    h = driver.LUHandle.from_store(fs, **kw)
    assert h.pdgstrf3d(0.0) == 0
    h.copy_to_host()
    assert np.array_equal(fs.Lnzval, expL) and np.array_equal(fs.Unzval, expU), name
    return h


def _assert_exact(got, x, what):
    bad = np.flatnonzero((got != x).any(axis=0))
    assert np.array_equal(got, x), (what, "columns", bad.tolist()[:8], "first row", int(np.flatnonzero(got[:, bad[0]] != x[:, bad[0]])[0]))


@pytest.mark.parametrize("name", tc.D_CASES)
def test_double_transposed_solve_is_exact(name):
    """width classes 1 .. 256, partial 64-row strips, ragged skyline leads, levels of 66 / 1 / 33 supernodes, more than 256 near columns; nrhs 1 (RK = 1),
    2 .. 5 and 17 (blocks of four with 1 .. 3 surplus columns), 97 (more than one chunk of max_rhs_chunk on the 256-column cases); "C" is "T" on a double handle"""
    c = tc.prepared(name)[0]
    h = _factored(name)
    for nrhs in tc.NRHS:
        x, b = tc.rhs_t(c, nrhs)
        _assert_exact(h.pdgstrs3d(b.copy(order="F"), trans="T"), x, (name, nrhs))
    x, b = tc.rhs_t(c, 5)
    _assert_exact(h.pdgstrs3d(b.copy(order="F"), trans="C"), x, (name, "C"))
    h.destroy()


def test_leading_dimension_larger_than_n():
    """ldx = n + 3 through the C ABI: exact solution rows, and the padding rows -- NaNs with a payload that tells the position -- come back bitwise unchanged"""
    c = tc.prepared("widths")[0]
    h = _factored("widths")
    n = c.n
    for nrhs in (1, 5, 49):
        x, b = tc.rhs_t(c, nrhs)
        buf = np.zeros((n + 3, nrhs), dtype=np.uint64, order="F")
        for q in range(nrhs):
            buf[:n, q] = np.ascontiguousarray(b[:, q]).view(np.uint64)
        pad = 0x7FF8000000000000 + 1 + np.arange(3, dtype=np.uint64)[:, None] + 16 * np.arange(nrhs, dtype=np.uint64)[None, :]
        buf[n:, :] = pad
        _lib.check(_lib.entry("sluamd_pdgstrs3d_trans")(h._h, 1, buf.ctypes.data_as(C.c_void_p), n + 3, nrhs), "sluamd_pdgstrs3d_trans")
        got = np.stack([np.ascontiguousarray(buf[:n, q]).view(np.float64) for q in range(nrhs)], axis=1)
        _assert_exact(got, x, nrhs)
        assert np.array_equal(buf[n:, :], pad), nrhs
    h.destroy()


@pytest.mark.parametrize("name", tc.Z_CASES)
def test_complex16_transposed_and_conjugate_transposed_solves_are_exact(name):
    """substitution on U_kk^T / L_kk^T and their conjugates (supernodes of up to 200 columns), the 256-row L^T strips and the U^T chunks on zc values: the
    Gaussian-integer phases make the two systems different, and each solve returns the same x"""
    c = tc.prepared(name)[0]
    h = _factored(name)
    for nrhs in tc.Z_NRHS:
        (x, bt), (xc, bc) = tc.rhs_t(c, nrhs, False), tc.rhs_t(c, nrhs, True)
        assert np.array_equal(x, xc) and not np.array_equal(bt, bc)
        _assert_exact(h.pdgstrs3d(bt.copy(order="F"), trans="T"), x, (name, nrhs, "T"))
        _assert_exact(h.pdgstrs3d(bc.copy(order="F"), trans="C"), x, (name, nrhs, "C"))
    h.destroy()


GROUPS_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_trans_solve as t
c = t.tc.prepared("groups")[0]
h = t._factored("groups")
out = {}
for nrhs in t.tc.GROUPS_NRHS:
    x, b = t.tc.rhs_t(c, nrhs)
    out["T:%d" % nrhs] = bool(t.np.array_equal(h.pdgstrs3d(b.copy(order="F"), trans="T"), x))
    x0, b0 = c.rhs(nrhs)
    out["N:%d" % nrhs] = bool(t.np.array_equal(h.pdgstrs3d(b0.copy(order="F")), x0))
out["launches"] = [h.stats()["solve_launches"]]
h.destroy()
print("RESULT " + json.dumps(out))
"""


def test_a_handle_with_merged_chain_groups_solves_the_transposed_system_exactly():
    """SLUAMD_SOLVE_GROUPS=1 (read at creation): the transposed path does not use the contracted schedule and must not be disturbed by it"""
    r = subprocess.run([sys.executable, "-c", GROUPS_CHILD, ROOT], env=dict(os.environ, SLUAMD_SOLVE_GROUPS="1"), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == 2 * len(tc.GROUPS_NRHS) + 1 and all(res.values()), res


def _dev(a):
    """column-major n x nrhs array -> torch tensor on the device with the same memory image (nrhs x n, row-major)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda()


def _bits(a):
    return np.ascontiguousarray(a.T).view(np.uint64)


def _host(t):
    return np.asfortranarray(t.cpu().numpy().T)


def test_notrans_through_the_new_entry_points_is_the_existing_solve_bitwise():
    """deterministic handles: SLUAMD_NOTRANS calls the existing solve and nothing else; the complex16 device-pointer variant against the host-pointer call"""
    import torch
    for name in ("widths", "z_wide"):
        c = tc.prepared(name)[0]
        h = _factored(name, deterministic=True)
        x, b = c.rhs(5)
        ref = h.pdgstrs3d(b.copy(order="F"))
        assert np.array_equal(ref, x)
        got = b.copy(order="F")
        fn = _lib.entry("sluamd_pzgstrs3d_trans" if c.z else "sluamd_pdgstrs3d_trans")
        _lib.check(fn(h._h, 0, got.ctypes.data_as(C.c_void_p), c.n, 5), "trans N")
        assert np.array_equal(_bits(got), _bits(ref)), name
        t = _dev(b)
        h.pdgstrs3d_dev(t.data_ptr(), c.n, 5)                                                  # complex16: through sluamd_pzgstrs3d_trans_dev
        torch.cuda.synchronize()
        assert np.array_equal(_bits(_host(t)), _bits(ref)), (name, "dev")
        h.destroy()


@pytest.mark.parametrize("name", ["levels", "z_levels"])
def test_device_pointer_variants(name):
    import torch
    c = tc.prepared(name)[0]
    h = _factored(name)
    for trans in (("T", "C") if c.z else ("T",)):
        x, b = tc.rhs_t(c, 5, trans == "C")
        t = _dev(b)
        h.pdgstrs3d_dev(t.data_ptr(), c.n, 5, trans=trans)
        torch.cuda.synchronize()
        _assert_exact(_host(t), x, (name, trans))
    h.destroy()


def _eta(A, x, b, norm_a):
    return float(np.abs(A @ x - b).max() / (norm_a * np.abs(x).max() + np.abs(b).max()))


@pytest.mark.parametrize("case", ["unsym300", "poisson10_nd", "z_unsym200", "z_grid24_nd"])
def test_recorded_fixtures_backward_error(golden, case):
    """A1 from the fixture's pre-factorisation store; b = A1^T xtrue (A1^H for "C"); eta_T = |A1^T x - b|_inf / (|A1|_1 |x|_inf + |b|_inf) against eta_N,
    the same quantity (with |A1|_inf) of the untransposed solve of the same handle and xtrue"""
    g = golden(case)
    fs = driver.FlatStore.from_golden(g, 0, "pre")
    (lr, lc), (ur, uc) = pc.store_positions(fs)
    n = fs.n
    A1 = np.zeros((n, n), dtype=fs.Lnzval.dtype)
    A1[lr[lr >= 0], lc[lr >= 0]] = fs.Lnzval[lr >= 0]
    A1[ur[ur >= 0], uc[ur >= 0]] = fs.Unzval[ur >= 0]
    z = np.iscomplexobj(A1)
    h = driver.LUHandle.from_store(fs, replace_tiny=bool(g["r0__ReplaceTinyPivot"][0]))
    assert h.pdgstrf3d(float(g["r0__thresh"][0])) == int(g["r0__info"][0])
    rng = np.random.default_rng(11)
    n1, ninf = float(np.abs(A1).sum(axis=0).max()), float(np.abs(A1).sum(axis=1).max())
    for nrhs in (1, 6):
        xt = rng.standard_normal((n, nrhs)) + (1j * rng.standard_normal((n, nrhs)) if z else 0)
        eta_n = _eta(A1, h.pdgstrs3d(np.asfortranarray(A1 @ xt)), A1 @ xt, ninf)
        for trans in (("T", "C") if z else ("T",)):
            At = A1.conj().T if trans == "C" else A1.T
            b = At @ xt
            eta_t = _eta(At, h.pdgstrs3d(np.asfortranarray(b), trans=trans), b, n1)
            print(f"{case} nrhs={nrhs} trans={trans}: eta_T {eta_t:.3e} eta_N {eta_n:.3e}")
            assert eta_t <= 10 * max(eta_n, n * EPS), (case, nrhs, trans, "eta_T", eta_t, "eta_N", eta_n)
    h.destroy()


def test_driver_solves_the_transposed_system():
    """pdgssvx3d(trans="T") on an unsymmetric-valued 8^3 operator under a nested-dissection ordering: A^T x = b becomes A1^T (Pc x) = Pc b.  The same
    backward-error criterion, and the distance to scipy's solution of A^T within the forward-error bound kappa_1(A) (eta_T + eta_scipy) |x| (first order)"""
    N = 8
    n, rp, ci, v = matgen.poisson3d(N)
    rng = np.random.default_rng(3)
    v = v * (1.0 + 0.4 * rng.random(len(v)))                                                # same pattern, A != A^T
    perm = matgen.nd_perm_grid3d(N, N, N, leaf=27)
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    xt = rng.standard_normal((n, 2))
    b_t, b_n = A.T @ xt, A @ xt
    n1, ninf = float(abs(A).sum(axis=0).max()), float(abs(A).sum(axis=1).max())
    x_n, info, _ = driver.pdgssvx3d(n, rp, ci, v, b_n, perm, relax=16, maxsup=128)
    x_t, info_t, st = driver.pdgssvx3d(n, rp, ci, v, b_t, perm, relax=16, maxsup=128, trans="T")
    assert info == 0 and info_t == 0 and st["solve_launches"] > 0
    eta_n, eta_t = _eta(A, x_n, b_n, ninf), _eta(A.T, x_t, b_t, n1)
    assert eta_t <= 10 * max(eta_n, n * EPS), ("eta_T", eta_t, "eta_N", eta_n)
    x_s = spla.spsolve(sp.csc_matrix(A.T), b_t)
    kappa = float(np.linalg.cond(A.toarray(), 1))
    bound = 2 * kappa * (max(eta_t, n * EPS) + _eta(A.T, x_s, b_t, n1)) * float(np.abs(xt).max())
    assert np.abs(x_t - x_s).max() <= bound, (float(np.abs(x_t - x_s).max()), bound)
    with pytest.raises(ValueError, match="refine"):
        driver.pdgssvx3d(n, rp, ci, v, b_t, perm, relax=16, maxsup=128, trans="T", refine=True)


def test_errors():
    L = _lib.load()
    dt, zt = _lib.entry("sluamd_pdgstrs3d_trans"), _lib.entry("sluamd_pzgstrs3d_trans")
    dtd, ztd = _lib.entry("sluamd_pdgstrs3d_trans_dev"), _lib.entry("sluamd_pzgstrs3d_trans_dev")
    hd, hz = _factored("narrow"), _factored("z_narrow")
    nd, nz = tc.prepared("narrow")[0].n, tc.prepared("z_narrow")[0].n
    xd, xz = np.ones((nd, 1), order="F"), np.ones((nz, 1), dtype=np.complex128, order="F")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for trans in (3, -1):
        assert dt(hd._h, trans, p(xd), nd, 1) == -1 and b"trans" in L.sluamd_last_error()      # SLUAMD_EINVAL
        assert zt(hz._h, trans, p(xz), nz, 1) == -1
    for trans in (0, 1, 2):                                                                 # the other precision's call
        assert dt(hz._h, trans, p(xz), nz, 1) == -1 and dtd(hz._h, trans, p(xz), nz, 1) == -1
        assert zt(hd._h, trans, p(xd), nd, 1) == -1 and ztd(hd._h, trans, p(xd), nd, 1) == -1
        assert dt(hd._h, trans, p(xd), nd, 0) == 0 and zt(hz._h, trans, p(xz), nz, 0) == 0     # nrhs == 0
    assert np.array_equal(xd, np.ones((nd, 1)))                                             # nothing was touched
    with pytest.raises(ValueError):
        hd.pdgstrs3d(xd, trans="X")
    hd.destroy(); hz.destroy()


def test_grid_handles_refuse_transposed_solves_on_every_rank():
    """a 1 x 1 x 2 in-process grid: SLUAMD_EINVAL with the message, on both ranks, before any collective step (nothing to hang on); the untransposed solve
    of the same handles still works"""
    c = tc.prepared("narrow")[0]
    n, rp, ci = c.pattern_csr()
    v = c.B[np.repeat(np.arange(n), np.diff(rp)), ci].copy()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    tree = symb.partition(2)
    comms = grid3d.local_comms(1, 1, 2)
    x0, b0 = c.rhs(2)
    fn = _lib.entry("sluamd_pdgstrs3d_trans")

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], tree)
        info = h.pdgstrf3d(0.0)
        out = []
        for trans in (1, 2):
            b = b0.copy(order="F")
            out.append((fn(h._h, trans, b.ctypes.data_as(C.c_void_p), n, 2), _lib.load().sluamd_last_error().decode(), np.array_equal(b, b0)))
        y = h.pdgstrs3d(b0.copy(order="F"))
        h.destroy()
        return info, out, y

    res = grid3d.run_ranks(2, body)
    symb.free()
    for info, out, y in res:
        assert info == 0 and np.array_equal(y, x0)
        for rc, msg, untouched in out:
            assert rc == -1 and "1 x 1 x 1" in msg and untouched, (rc, msg)


def test_launch_count_of_a_transposed_solve():
    """stats()["solve_launches"]: one diagonal and one update launch per DAG level and sweep, per chunk of right-hand sides (sluamd_tsolve.cpp; restated in
    trans_cases.predicted_launches_t); t_solve_ms is filled"""
    c, _, _, _, sizes = tc.prepared("levels")
    assert sizes == [66, 1, 33, 4, 2, 1]
    h = _factored("levels")
    chunk = tc.max_rhs_chunk(max(c.widths))
    for nrhs in (1, 5, chunk + 1):
        x, b = tc.rhs_t(c, nrhs)
        _assert_exact(h.pdgstrs3d(b.copy(order="F"), trans="T"), x, nrhs)
        st = h.stats()
        assert st["solve_launches"] == tc.predicted_launches_t(sizes, nrhs, chunk) == 4 * len(sizes) * (2 if nrhs > chunk else 1), nrhs
        assert st["t_solve_ms"] > 0
    h.destroy()
