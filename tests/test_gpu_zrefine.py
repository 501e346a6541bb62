"""Complex16 iterative refinement on the device (sluamd_zAttachMatrix / sluamd_pzgsrfs3d[_dev]: k_rfs_residual<double2> + k_rfs_update<double2>
around the complex triangular solves) against the reference's pzgsrfs3d records (IterRefine = SLU_DOUBLE) and the CPU oracle's
restatement of it; the refinement of grid handles (replicated form) in both precisions.  The bounds are those of
test_gpu_refine.py: X within 1e-12 max|x| of a reference record and within 1e-11 (relative) of the oracle, berr <= 4 eps,
refinement steps to one step, normwise residual < 1e-14."""
import ctypes as C
import numpy as np
import pytest
import oracle as orc
import refine_cases as rc

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
EINVAL = -1


def _residual(n, rp, ci, v, b, x):
    from superlu_dist_amd import matgen
    return np.linalg.norm(b - matgen.csr_matvec(n, rp, ci, v, x)) / np.linalg.norm(b)


def _oracle_store(symb, h):
    """The device's factors copied into a COMPLEX store of the symbolic structure, as an oracle store."""
    from superlu_dist_amd import driver
    f0 = symb.flat_store(values=False)
    fs = driver.FlatStore(f0.n, f0.xsup, f0.Lrowind_off, f0.Lrowind, f0.Lnzval_off, f0.Lnzval.astype(np.complex128), f0.Ufstnz_off, f0.Ufstnz,
                          f0.Unzval_off, f0.Unzval.astype(np.complex128))
    h.copy_to_host(fs)
    return orc.LUStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind, fs.Lnzval_off, fs.Lnzval, fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off, fs.Unzval)


def test_pzgssvx3d_refines_complex_systems():
    from superlu_dist_amd import driver, matgen
    N = 12
    n, rp, ci, v = matgen.poisson3d(N)
    v = matgen.complex_shift(v, rp, ci, seed=2)
    perm = matgen.nd_perm_grid3d(N, N, N, leaf=27)
    rng = np.random.default_rng(3)
    xt = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
    b = matgen.csr_matvec(n, rp, ci, v, xt)
    x, info, st = driver.pzgssvx3d(n, rp, ci, v, b, perm_c=perm, relax=8, maxsup=64, refine=True)
    assert info == 0 and x.dtype == np.complex128 and x.shape == (n, 2)
    res = _residual(n, rp, ci, v, b, x)
    print("berr/eps", (st["berr"] / EPS).round(3).tolist(), "steps", st["refine_steps"], "residual %.2e" % res)
    assert "refine_steps" in st and st["refine_steps"] >= 0
    assert np.all(st["berr"] <= 4 * EPS)
    assert res < 1e-14


@pytest.mark.parametrize("case", ["z_cg20_1x1x1", "z_cg20_1x1x1_nrhs2", "z_unsym200"])
def test_one_rank_fixtures_match_the_reference(golden, case):
    from superlu_dist_amd import driver
    g = golden(case)
    n, rp, ci, v, B, xref, Cs, pc = rc.equilibrated_system(g)
    fs = driver.FlatStore.from_golden(g, 0, "pre")
    h = driver.LUHandle.from_store(fs, replace_tiny=bool(g["r0__ReplaceTinyPivot"][0]))
    assert h.z and h.pzgstrf3d(float(g["r0__thresh"][0])) == int(g["r0__info"][0])
    xp = np.zeros_like(B, order="F"); xp[pc, :] = B
    X0 = np.asfortranarray(h.pzgstrs3d(xp)[pc, :])
    h.attach_matrix(n, rp, ci, v, pc)
    Xs, berr, steps = h.pzgsrfs3d(B, X0)
    # the oracle's pzgsrfs3d on the same factors (copied back), from its own solve
    fs2 = driver.FlatStore.from_golden(g, 0, "pre")
    h.copy_to_host(fs2)
    h.destroy()
    ost = orc.LUStore(fs2.n, fs2.xsup, fs2.Lrowind_off, fs2.Lrowind, fs2.Lnzval_off, fs2.Lnzval, fs2.Ufstnz_off, fs2.Ufstnz, fs2.Unzval_off, fs2.Unzval)
    Xo0 = np.asfortranarray(orc.dsolve(ost, xp)[pc, :])
    Xo, berr_o, steps_o = orc.dgsrfs(ost, rp, ci, v, pc, B, Xo0)
    X = Xs * Cs[:, None]
    err_ref = np.abs(X - xref).max() / np.abs(xref).max()
    err_orc = np.abs(Xs - Xo).max() / np.abs(Xo).max()
    print(case, "rel err vs record %.2e vs oracle %.2e" % (err_ref, err_orc), "berr/eps", (berr / EPS).round(3).tolist(),
          "oracle", (berr_o / EPS).round(3).tolist(), "steps", steps, "oracle", steps_o,
          "recorded berr/eps", (np.atleast_1d(g["r0__berr"]) / EPS).round(3).tolist())
    assert err_ref <= 1e-12
    assert err_orc <= 1e-11
    assert np.all(berr <= 4 * EPS) and np.all(berr_o <= 4 * EPS)
    assert abs(steps - steps_o) <= 1
    if "r0__RefineSteps" in g:
        assert abs(steps - int(g["r0__RefineSteps"][0])) <= 1


@pytest.mark.parametrize("case", ["z_cg20_1x1x2", "z_cg20_1x2x1", "z_cg20_2x1x1", "z_cg20_2x2x2"])
def test_grid_fixtures_match_the_reference(golden, case):
    rc.check_refined_fixture_on_grid(golden(case), check_steps=True)


def _hard_system():
    """A weakly diagonal random complex system (element growth without pivoting): the initial solve leaves a residual that takes
    several refinement steps.  (diag_scale 0.01 takes 14 steps and whether it converges depends on rounding: not used.)"""
    from superlu_dist_amd import matgen
    n, rp, ci, v = matgen.random_unsym(400, 0.02, 5, diag_scale=0.02)
    rng = np.random.default_rng(105)
    v = v.astype(np.complex128) * np.exp(1j * rng.uniform(-0.5, 0.5, v.size))
    rng = np.random.default_rng(1)
    xt = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
    b = matgen.csr_matvec(n, rp, ci, v, xt)
    return n, rp, ci, v, b


@pytest.fixture(scope="module")
def hard_device_result():
    """single-rank device refinement of _hard_system: (x, berr, steps, oracle x, oracle berr, oracle steps)"""
    from superlu_dist_amd import driver
    n, rp, ci, v, b = _hard_system()
    x, info, st, h, symb = driver.pzgssvx3d(n, rp, ci, v, b, relax=8, maxsup=64, keep=True, refine=True)
    try:
        assert info == 0
        ost = _oracle_store(symb, h)
        pc = symb.perm_c
        xp = np.zeros_like(b, order="F"); xp[pc, :] = b
        X0 = np.asfortranarray(orc.dsolve(ost, xp)[pc, :])
        Xo, berr_o, steps_o = orc.dgsrfs(ost, rp, ci, v, pc, b, X0)
    finally:
        h.destroy(); symb.free()
    return x, st["berr"], st["refine_steps"], Xo, berr_o, steps_o


def test_refinement_that_repeats_matches_the_oracle(hard_device_result):
    n, rp, ci, v, b = _hard_system()
    x, berr, steps, Xo, berr_o, steps_o = hard_device_result
    err = np.abs(x - Xo).max() / np.abs(Xo).max()
    res, res_o = _residual(n, rp, ci, v, b, x), _residual(n, rp, ci, v, b, Xo)
    print("steps", steps, "oracle", steps_o, "berr/eps", (berr / EPS).round(3).tolist(), "oracle", (berr_o / EPS).round(3).tolist(),
          "rel err vs oracle %.2e residual %.2e oracle %.2e" % (err, res, res_o))
    assert steps_o >= 2                      # precondition: the case really repeats
    assert abs(steps - steps_o) <= 1
    assert err <= 1e-11
    assert np.all(berr <= 4 * EPS) and np.all(berr_o <= 4 * EPS)
    assert res < 1e-14


@pytest.mark.parametrize("grid", [(1, 1, 2), (2, 1, 1), (2, 2, 2)])
def test_refinement_that_repeats_on_grids(hard_device_result, grid):
    from superlu_dist_amd import driver, grid3d
    n, rp, ci, v, b = _hard_system()
    x1, _, steps1 = hard_device_result[:3]
    Pr, Pc, Pz = grid
    symb = driver.Symbolic(n, rp, ci, None, relax=8, maxsup=64)
    sn_tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)
    pc = symb.perm_c
    thresh = driver.pivot_thresh(n, rp, ci, v)

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], sn_tree)
        try:
            assert h.z and h.pdgstrf3d(thresh) == 0          # pzgstrf3d on a complex16 grid handle
            xp = np.zeros_like(b, order="F"); xp[pc, :] = b
            X0 = np.asfortranarray(h.pdgstrs3d(xp)[pc, :])
            h.attach_matrix(n, rp, ci, v, pc)
            return h.pzgsrfs3d(b, X0)
        finally:
            h.destroy()

    out = grid3d.run_ranks(Pr * Pc * Pz, body)
    symb.free()
    X, berr, steps = out[0]
    for q, (Xq, bq, sq) in enumerate(out[1:], 1):
        assert np.array_equal(Xq, X) and np.array_equal(bq, berr) and sq == steps, q
    err = np.abs(X - x1).max() / np.abs(x1).max()
    print(grid, "steps", steps, "single rank", steps1, "berr/eps", (berr / EPS).round(3).tolist(), "rel err vs single rank %.2e" % err)
    assert err <= 1e-11
    assert abs(steps - steps1) <= 1


_DEV_CHILD = r"""
import json, sys
import numpy as np
import torch                                   # first: torch's HIP context must exist before the library initialises the runtime
if not torch.cuda.is_available():
    print(json.dumps({"skip": "torch sees no HIP device"})); sys.exit(0)
from superlu_dist_amd import driver, matgen
N = 12
n, rp, ci, v = matgen.poisson3d(N)
v = matgen.complex_shift(v, rp, ci, seed=2)
perm = matgen.nd_perm_grid3d(N, N, N, leaf=27)
rng = np.random.default_rng(3)
xt = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
b = matgen.csr_matvec(n, rp, ci, v, xt)
X0, info, st, h, symb = driver.pzgssvx3d(n, rp, ci, v, b, perm_c=perm, relax=8, maxsup=64, keep=True)
assert info == 0
h.attach_matrix(n, rp, ci, v, symb.perm_c)
Xh, berr_h, steps_h = h.pzgsrfs3d(b, X0)
# column-major n x nrhs on the device = a contiguous (nrhs, n) tensor
dB = torch.from_numpy(np.ascontiguousarray(b.T)).to("cuda")
dX = torch.from_numpy(np.ascontiguousarray(X0.T)).to("cuda")
assert dB.dtype == torch.complex128 and dX.dtype == torch.complex128
torch.cuda.synchronize()
berr_d, steps_d = h.pzgsrfs3d_dev(dB.data_ptr(), n, dX.data_ptr(), n, b.shape[1])
torch.cuda.synchronize()
Xd = dX.cpu().numpy().T
h.destroy(); symb.free()
print(json.dumps({"err": float(np.abs(Xd - Xh).max() / np.abs(Xh).max()), "steps_h": steps_h, "steps_d": steps_d,
                  "berr_h": berr_h.tolist(), "berr_d": berr_d.tolist()}))
"""


def test_dev_variant_matches_the_host_variant():
    """sluamd_pzgsrfs3d_dev on complex128 torch tensors on the device against sluamd_pzgsrfs3d from the same initial solution.  Runs in a
    child process that initialises torch first (torch.cuda reports no device once the library has initialised the HIP runtime in the
    process).  The system is test_pzgssvx3d_refines_complex_systems': diagonally dominant, so its few stopping decisions are not the
    long run of berr ~ 1.1-1.5 eps decisions of _hard_system -- the device solve accumulates with fp64 atomics, so two refinements of
    that system from the same start can take 3 and 4 steps."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _DEV_CHILD], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    if "skip" in out:
        pytest.skip(out["skip"])
    print(out)
    assert out["err"] <= 1e-12
    assert out["steps_d"] == out["steps_h"]
    assert np.abs(np.array(out["berr_d"]) - np.array(out["berr_h"])).max() <= 1e-12


def test_errors_of_the_complex_entry_points():
    from superlu_dist_amd import _lib, driver, matgen
    L = _lib.load()
    N = 4
    n, rp, ci, vd = matgen.poisson3d(N)
    vz = matgen.complex_shift(vd, rp, ci, seed=1)
    rp = np.ascontiguousarray(rp, dtype=np.int32); ci = np.ascontiguousarray(ci, dtype=np.int32)
    vd = np.ascontiguousarray(vd, dtype=np.float64); vz = np.ascontiguousarray(vz)
    pi = lambda a: a.ctypes.data_as(_lib.P_int)
    pv = lambda a: a.ctypes.data_as(C.c_void_p)
    pd = lambda a: a.ctypes.data_as(_lib.P_dbl)

    def last_error():
        return L.sluamd_last_error().decode()

    bz = np.asfortranarray(np.ones((n, 1), dtype=np.complex128)); bd = np.asfortranarray(np.ones((n, 1)))
    xd, info, _, hd, sd = driver.pdgssvx3d(n, rp, ci, vd, bd, relax=8, maxsup=16, keep=True)
    xz, info_z, _, hz, sz = driver.pzgssvx3d(n, rp, ci, vz, bz, relax=8, maxsup=16, keep=True)
    try:
        assert info == 0 and info_z == 0 and hz.z and not hd.z
        pcd, pcz = sd.perm_c, sz.perm_c
        berr = np.zeros(1); steps = C.c_int32(0)
        xz = np.asfortranarray(xz.copy())
        # zAttachMatrix on a double handle
        assert L.sluamd_zAttachMatrix(hd._h, n, pi(rp), pi(ci), pv(vz), pi(pcd)) == EINVAL
        assert "double handle" in last_error()
        # wrong n
        assert L.sluamd_zAttachMatrix(hz._h, n - 1, pi(rp), pi(ci), pv(vz), pi(pcz)) == EINVAL
        assert last_error()
        # refinement before attaching
        assert L.sluamd_pzgsrfs3d(hz._h, pv(bz), n, pv(xz), n, 1, pd(berr), C.byref(steps)) == EINVAL
        assert "no matrix attached" in last_error()
        assert L.sluamd_pzgsrfs3d_dev(hz._h, pv(bz), n, pv(xz), n, 1, pd(berr), C.byref(steps)) == EINVAL
        assert "no matrix attached" in last_error()
        # dAttachMatrix keeps refusing complex handles
        assert L.sluamd_dAttachMatrix(hz._h, n, pi(rp), pi(ci), pd(vd), pi(pcz)) == EINVAL
        assert "complex16 handle" in last_error()
        # precision mismatch: the double call on a complex handle with its complex matrix attached, and the complex call on a double one
        hz.attach_matrix(n, rp, ci, vz, pcz)
        hd.attach_matrix(n, rp, ci, vd, pcd)
        assert L.sluamd_pdgsrfs3d(hz._h, pd(bd), n, pd(xd), n, 1, pd(berr), C.byref(steps)) == EINVAL
        assert "complex16" in last_error()
        assert L.sluamd_pzgsrfs3d(hd._h, pv(bz), n, pv(xz), n, 1, pd(berr), C.byref(steps)) == EINVAL
        assert "double" in last_error()
        # nrhs = 0: nothing to do
        steps.value = 7
        assert L.sluamd_pzgsrfs3d(hz._h, pv(bz), n, pv(xz), n, 0, pd(berr), C.byref(steps)) == 0
        assert steps.value == 0
        # ... and the attached handles still refine
        X, berr2, st2 = hz.pzgsrfs3d(bz, xz)
        assert np.all(berr2 <= 4 * EPS) and _residual(n, rp, ci, vz, bz, X) < 1e-14
    finally:
        hd.destroy(); hz.destroy(); sd.free(); sz.free()


def test_copy_to_host_refuses_a_store_of_the_other_precision():
    from superlu_dist_amd import driver, matgen
    n, rp, ci, v = matgen.poisson3d(4)
    v = matgen.complex_shift(v, rp, ci, seed=1)
    x, info, st, h, symb = driver.pzgssvx3d(n, rp, ci, v, np.ones(n, dtype=np.complex128), relax=8, maxsup=16, keep=True)
    try:
        with pytest.raises(ValueError, match="complex16"):
            h.copy_to_host(symb.flat_store(values=False))       # a real store: half the bytes of the handle's factors
    finally:
        h.destroy(); symb.free()


@pytest.mark.parametrize("case", ["g20_1x1x2", "g20_2x1x1", "g20_2x2x2"])
def test_double_grid_fixtures_through_the_grid_handle(golden, case):
    rc.check_refined_fixture_on_grid(golden(case), check_steps=False)
