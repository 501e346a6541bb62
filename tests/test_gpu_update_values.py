"""Same-pattern value updates on the device (sluamd_[dz]UpdateValues[_dev], LUHandle.update_values, GridHandle.update_values): Fact =
SamePattern_SameRowPerm for handles created from the symbolic structure.

Exact part: the sweep cases (tests/sweep_cases.py through tests/trans_cases.py::prepared) -- their factorisation and sweeps are exact in any summation
order, so every comparison is numpy.array_equal: a handle created with OTHER values on the pattern (update_cases.wrong_values) must, after the update, hold
the exact factors and return the integer solution.
Floating-point part: an equilibrated handle reuses R and C bit for bit and stores (a r[i]) c[j] (compared bitwise with the numpy restatement); the
yardstick of the solves is a FRESH handle created (and equilibrated) with the new values, with the factor 10 of test_gpu_trans_solve.py -- the same
elimination on values scaled by other R and C; a stale matrix anywhere leaves errors of the order of the perturbation (>= 1e-3)."""
import ctypes as C
import os, re, subprocess
import numpy as np
import pytest
import scipy.sparse as sp
import equil_cases as ec
import trans_cases as tc
import update_cases as uc
from superlu_dist_amd import _lib, driver, grid3d, matgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


def _symb(c, n, rp, ci):
    return driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)


def _exact_solves(h, c, what):
    """the untransposed solve for nrhs 1 and 5 and the transposed one return the integer x"""
    for nrhs in (1, 5):
        x, b = c.rhs(nrhs)
        assert np.array_equal(h.pdgstrs3d(b.copy(order="F")), x), (what, nrhs)
    x, bt = tc.rhs_t(c, 5)
    assert np.array_equal(h.pdgstrs3d(bt.copy(order="F"), trans="T"), x), (what, "T")


def _factors(symb, h):
    """the handle's values in the store formats, through its copy-out (works for handles created from the symbolic structure: test_gpu_equil.py)"""
    fs = symb.flat_store(values=False)
    if h.z:
        fs = driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind, fs.Lnzval_off, fs.Lnzval.astype(np.complex128), fs.Ufstnz_off, fs.Ufstnz,
                              fs.Unzval_off, fs.Unzval.astype(np.complex128))
    h.copy_to_host(fs)
    return fs.Lnzval, fs.Unzval


def _diag_inv_rc(h, c):
    ns = int(c.xsup[1] - c.xsup[0])
    li, ui = np.zeros((ns, ns), order="F"), np.zeros((ns, ns), order="F")
    return _lib.load().sluamd_dGetDiagInv(h._h, 0, li.ctypes.data_as(_lib.P_dbl), ui.ctypes.data_as(_lib.P_dbl))


@pytest.mark.parametrize("name", ["narrow", "widths", "z_narrow"])
def test_update_then_factor_gives_the_exact_factors(name):
    """created with the wrong values, updated with v: info == 0, the factors read back through the handle's copy-out equal expL / expU, and the solves
    (nrhs 1 and 5, and the transposed one) return the integer x.  Fails on the parent commit: the entry point is missing."""
    c, n, rp, ci, v = uc.csr_case(name)
    expL, expU = tc.prepared(name)[2:4]
    symb = _symb(c, n, rp, ci)
    h = driver.LUHandle.from_symbolic(symb, uc.wrong_values(n, rp, ci, v))
    try:
        assert h.z == c.z
        assert h.update_values(v) is None
        assert h.pdgstrf3d(0.0) == 0
        L, U = _factors(symb, h)
        assert np.array_equal(L, expL) and np.array_equal(U, expU), name
        _exact_solves(h, c, name)
    finally:
        h.destroy(); symb.free()


def test_update_after_a_factorisation():
    """factor with the wrong values (the answer differs from x), update, factor, solve exactly; sluamd_dGetDiagInv refuses between the update and the
    second factorisation"""
    c, n, rp, ci, v = uc.csr_case("narrow")
    symb = _symb(c, n, rp, ci)
    h = driver.LUHandle.from_symbolic(symb, uc.wrong_values(n, rp, ci, v))
    try:
        h.pdgstrf3d(0.0)
        x, b = c.rhs(5)
        assert not np.array_equal(h.pdgstrs3d(b.copy(order="F")), x)
        assert _diag_inv_rc(h, c) == 0
        h.update_values(v)
        assert _diag_inv_rc(h, c) == -1 and b"no factorisation" in _lib.load().sluamd_last_error()
        assert h.pdgstrf3d(0.0) == 0
        assert _diag_inv_rc(h, c) == 0
        _exact_solves(h, c, "second factorisation")
    finally:
        h.destroy(); symb.free()


def test_reset_after_an_update_restores_the_new_values():
    c, n, rp, ci, v = uc.csr_case("narrow")
    expL, expU = tc.prepared("narrow")[2:4]
    symb = _symb(c, n, rp, ci)
    h = driver.LUHandle.from_symbolic(symb, uc.wrong_values(n, rp, ci, v))
    try:
        h.update_values(v)
        assert h.pdgstrf3d(0.0) == 0
        h.reset_values()
        assert h.pdgstrf3d(0.0) == 0
        L, U = _factors(symb, h)
        assert np.array_equal(L, expL) and np.array_equal(U, expU)
        _exact_solves(h, c, "after reset")
    finally:
        h.destroy(); symb.free()


_FORMS_CHILD = r"""
import json, os, sys
import numpy as np
import torch                                   # first: torch's HIP context must exist before the library initialises the runtime
assert torch.cuda.is_available(), "torch sees no HIP device"
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_update_values as t
out = {}
for name in ("narrow", "z_narrow"):
    c, n, rp, ci, v = t.uc.csr_case(name)
    expL, expU = t.tc.prepared(name)[2:4]
    symb = t._symb(c, n, rp, ci)
    wrong = t.uc.wrong_values(n, rp, ci, v)
    h = t.driver.LUHandle.from_symbolic(symb, wrong)
    for where in ("cuda", "cpu"):
        ten = torch.from_numpy(np.array(v))
        if where == "cuda":
            ten = ten.cuda()
            torch.cuda.synchronize()            # the copy ran on torch's stream: complete before the handle's stream reads the tensor
        h.update_values(ten)
        info = h.pdgstrf3d(0.0)                 # (synchronises: the tensor may go)
        del ten
        L, U = t._factors(symb, h)
        t._exact_solves(h, c, (name, where))
        out[name + ":" + where] = bool(info == 0 and np.array_equal(L, expL) and np.array_equal(U, expU))
        h.update_values(wrong)                  # back to the wrong values for the next form
    other = torch.zeros(len(v), dtype=torch.from_numpy(np.array(v)).dtype, device="meta")
    try:
        h.update_values(other)
        out[name + ":other device"] = False
    except ValueError:
        out[name + ":other device"] = True
    h.destroy(); symb.free()
print("RESULT " + json.dumps(out))
"""


def test_device_and_host_forms_agree():
    """a torch tensor on the device goes through sluamd_[dz]UpdateValues_dev with its data_ptr(), one on the CPU through the host form: the exact factors
    and solutions both times, double and complex16.  In a child process that initialises torch first (torch.cuda reports no device once the library has
    initialised the HIP runtime in the process: test_gpu_zrefine.py)."""
    import json, sys
    r = subprocess.run([sys.executable, "-c", _FORMS_CHILD, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == 6 and all(res.values()), res


@pytest.mark.parametrize("grid", [(1, 1, 2), (2, 2, 1)])
def test_grids_update_their_own_entries(grid):
    """in-process grids: every rank passes the complete array and updates its own entries; info == 0 and the integer x on every rank"""
    Pr, Pc, Pz = grid
    c, n, rp, ci, v = uc.csr_case("narrow")
    wrong = uc.wrong_values(n, rp, ci, v)
    symb = _symb(c, n, rp, ci)
    tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)
    x0, b0 = c.rhs(5)

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, wrong, comms[rank], tree)
        try:
            h.update_values(v)
            info = h.pdgstrf3d(0.0)
            return info, h.pdgstrs3d(b0.copy(order="F"))
        finally:
            h.destroy()

    res = grid3d.run_ranks(Pr * Pc * Pz, body)
    symb.free()
    for info, y in res:
        assert info == 0 and np.array_equal(y, x0)


# ---- floating point: scalings reused, attached matrix updated ----

def _eta(A, x, b):
    """normwise backward error |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf)"""
    return float(np.abs(A @ x - b).max() / (abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def _berr(A, x, b):
    """componentwise backward error max_i |b - A x|_i / (|A| |x| + |b|)_i, per column"""
    return (np.abs(b - A @ x) / (abs(A) @ np.abs(x) + np.abs(b))).max(axis=0)


def _store_of(symb, vals):
    symb.distribute_host(np.ascontiguousarray(vals))
    fs = symb.flat_store()
    return fs.Lnzval.copy(), fs.Unzval.copy()


def test_equilibrated_handle_reuses_its_scalings_bit_for_bit():
    """equil_cases "dense65_B" (equed = B; R and C reciprocals of random mantissas, so the order (a r) c matters): equilibrate with v1, update with
    v2 = v1 (1 + k / 8).  equed, R and C unchanged (bitwise); the store holds (v2 r[i]) c[j] bit for bit; anorm within k_max 2^-52 (the bound the header
    states for sluamd_equil_t::anorm) of the column-sum maximum; the solve's normwise backward error on A2 x = b within 10x that of a fresh handle
    created and equilibrated with v2; the attached copy took the new values: refine=True ends with berr <= 4 eps against A2's scaled system (with
    stale attached values it stagnates at O(|v2 - v1|))."""
    n, rp, ci, v1 = ec.case(uc.EQUIL_CASE)
    v2 = uc.second_values(n, rp, ci, v1)
    A2 = sp.csr_matrix((v2, ci, rp), shape=(n, n))
    b = np.asfortranarray(A2 @ np.random.default_rng(2).standard_normal((n, 2)))
    thr = lambda anorm: 0.5 * float(np.finfo(np.float32).eps) * anorm
    symb = driver.Symbolic(n, rp, ci, None, relax=8, maxsup=64)
    h = driver.LUHandle.from_symbolic(symb, v1)
    hf = driver.LUHandle.from_symbolic(symb, v2)
    try:
        d1 = h.equilibrate(n, rp, ci, v1, symb.perm_c)
        assert d1["equed"] == "B"
        R, Cs = h.scalings()
        assert not np.all(np.frexp(R)[0] == 0.5) and not np.all(np.frexp(Cs)[0] == 0.5)        # not all powers of two
        up = h.update_values(v2, want_norm=True)
        R2, C2 = h.scalings()
        assert up["equed"] == "B" and np.array_equal(R2.view(np.uint64), R.view(np.uint64)) and np.array_equal(C2.view(np.uint64), Cs.view(np.uint64))
        with pytest.raises(RuntimeError, match="already"):
            h.equilibrate(n, rp, ci, v2, symb.perm_c)
        s2 = uc.scaled_values(n, rp, ci, v2, R, Cs)
        expL, expU = _store_of(symb, s2)
        fs = symb.flat_store(values=False)
        h.copy_to_host(fs)
        assert np.array_equal(fs.Lnzval, expL) and np.array_equal(fs.Unzval, expU)
        ref, k = ec.anorm_exact(n, ci, s2)
        print("anorm", up["anorm"], ref, "k", k)
        assert abs(up["anorm"] - ref) <= k * 2.0 ** -52 * ref
        assert h.pdgstrf3d(thr(up["anorm"])) == 0
        x = h.gssvx_solve(b)
        df = hf.equilibrate(n, rp, ci, v2, symb.perm_c)
        assert hf.pdgstrf3d(thr(df["anorm"])) == 0
        xf = hf.gssvx_solve(b)
        eta, eta_f = _eta(A2, x, b), _eta(A2, xf, b)
        print("eta updated", eta, "eta fresh", eta_f)
        assert eta <= 10 * eta_f
        xr, berr, steps = h.gssvx_solve(b, refine=True)
        As = sp.csr_matrix((s2, ci, rp), shape=(n, n))
        berr_host = _berr(As, xr / Cs[:, None], R[:, None] * b)
        print("berr/eps device", (berr / EPS).tolist(), "host, against the scaled A2", (berr_host / EPS).tolist(), "steps", steps)
        # host figure: the device's bar plus one rounding each of x / C and R b (<= 1 eps of the denominator each), rounded up to 8 eps
        assert np.all(berr <= 4 * EPS) and np.all(berr_host <= 8 * EPS)
    finally:
        h.destroy(); hf.destroy(); symb.free()


def test_refinement_without_equilibration_refines_the_new_system():
    """attach_matrix with v1, update_values(v2), factor, pdgsrfs3d: the componentwise backward error against A2 (computed on the host) is within 10x of
    what a fresh handle reaches, and not >= 1e-3, where a stale attached matrix leaves it"""
    n, rp, ci, v1 = matgen.stencil3d_unsym(5, seed=3)
    perm = matgen.nd_perm_grid3d(5, 5, 5, leaf=27)
    v2 = uc.second_values(n, rp, ci, v1)
    A2 = sp.csr_matrix((v2, ci, rp), shape=(n, n))
    b = np.asfortranarray(A2 @ np.random.default_rng(4).standard_normal((n, 2)))
    symb = driver.Symbolic(n, rp, ci, perm, relax=8, maxsup=64)

    def refined(h):
        assert h.pdgstrf3d(driver.pivot_thresh(n, rp, ci, v2)) == 0
        xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b
        x0 = np.asfortranarray(h.pdgstrs3d(xp)[symb.perm_c, :])
        x, berr, steps = h.pdgsrfs3d(b, x0)
        return _berr(A2, x, b), berr

    h = driver.LUHandle.from_symbolic(symb, v1)
    hf = driver.LUHandle.from_symbolic(symb, v2)
    try:
        h.attach_matrix(n, rp, ci, v1, symb.perm_c)
        assert h.update_values(v2) is None
        got, dev = refined(h)
        hf.attach_matrix(n, rp, ci, v2, symb.perm_c)
        fresh, _ = refined(hf)
        print("berr/eps updated", (got / EPS).tolist(), "fresh", (fresh / EPS).tolist(), "device", (dev / EPS).tolist())
        assert np.all(got < 1e-3) and np.all(got <= 10 * fresh)
    finally:
        h.destroy(); hf.destroy(); symb.free()


# ---- errors ----

def test_errors_leave_the_handle_untouched():
    L = _lib.load()
    c, n, rp, ci, v = uc.csr_case("narrow")
    cz, nz, rpz, ciz, vz = uc.csr_case("z_narrow")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dU, dUd, zU, zUd = (_lib.entry("sluamd_" + s) for s in ("dUpdateValues", "dUpdateValues_dev", "zUpdateValues", "zUpdateValues_dev"))
    symb, symbz = _symb(c, n, rp, ci), _symb(cz, nz, rpz, ciz)
    h, hz = driver.LUHandle.from_symbolic(symb, v), driver.LUHandle.from_symbolic(symbz, vz)
    fs = tc.prepared("narrow")[1]
    hv = driver.LUHandle.from_store(driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind.copy(), fs.Lnzval_off, fs.Lnzval.copy(), fs.Ufstnz_off,
                                                     fs.Ufstnz, fs.Unzval_off, fs.Unzval.copy()))
    wrong, wrongz = uc.wrong_values(n, rp, ci, v), uc.wrong_values(nz, rpz, ciz, vz)
    try:
        # a view-created handle
        for fn in (dU, dUd):
            assert fn(hv._h, p(wrong), None) == -1 and b"sluamd_dSetValues" in L.sluamd_last_error()
        # the other precision
        for fn in (zU, zUd):
            assert fn(h._h, p(wrongz), None) == -1 and b"sluamd_dUpdateValues" in L.sluamd_last_error()
        for fn in (dU, dUd):
            assert fn(hz._h, p(wrong), None) == -1 and b"sluamd_zUpdateValues" in L.sluamd_last_error()
        # null pointers
        for fn in (dU, dUd):
            assert fn(h._h, None, None) == -1 and b"null" in L.sluamd_last_error()
            assert fn(None, p(wrong), None) == -1 and b"null" in L.sluamd_last_error()
        # Python: length, dtype, contiguity
        for bad in (wrong[:-1], wrong.astype(np.float32), wrong.astype(np.complex128), np.repeat(wrong, 2)[::2]):
            with pytest.raises(ValueError):
                h.update_values(bad)
        with pytest.raises(ValueError):
            hz.update_values(wrongz.real.copy())
        # the norm without an attached matrix
        with pytest.raises(RuntimeError, match="anorm needs an attached matrix"):
            h.update_values(wrong, want_norm=True)
        out = _lib.Update()
        assert zU(hz._h, p(wrongz), C.byref(out)) == -1 and b"attached" in L.sluamd_last_error()
        # nothing was touched: all three still factor and solve exactly
        for hh, cc in ((h, c), (hz, cz), (hv, c)):
            assert hh.pdgstrf3d(0.0) == 0
            _exact_solves(hh, cc, "after the refused calls")
    finally:
        h.destroy(); hz.destroy(); hv.destroy(); symb.free(); symbz.free()


# ---- the C example ----

def test_c_example_steps():
    """examples/pddrive3d_amd 12 --steps 2 through the C ABI: each extra step prints a residual below the 1e-10 the example asserts for its first solve"""
    exe = os.path.join(ROOT, "examples", "pddrive3d_amd")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
    for extra in ([], ["--equil"]):
        r = subprocess.run([exe, "12", "--steps", "2"] + extra, capture_output=True, text=True, timeout=120)
        print(r.stdout, r.stderr)
        assert r.returncode == 0, r.stdout + r.stderr
        res = [float(m) for m in re.findall(r"^STEP \d+: .*\|\|b-Ax\|\|_2/\|\|b\|\|_2 = (\S+)$", r.stdout, flags=re.M)]
        assert len(res) == 2 and all(x < 1e-10 for x in res), res
