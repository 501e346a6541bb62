"""Transposed and conjugate-transposed solves, refinement and expert solves on process grids (GridHandle.pdgstrs3d(trans=), GridHandle.pdgsrfs3d(trans=),
pdgssvx3d(grid=, trans=); sluamd_tsolve.cpp's grid branch over LevelSched::xt_*).  Ranks are threads on one device over grid3d.local_comms.

Floating-point part: the operator of grid_cases.check_own_pipeline, made unsymmetric in values AND pattern (grid_trans_cases.System), so that a solve
that mixed up rows and columns, or ran untransposed, misses by O(1).  Both assertions are those grid_cases applies to untransposed grid solves, with the
same constant: residual on op(A) below 1e-10 and 1e-10 from the solution of a 1 x 1 x 1 handle (grid_trans_cases.check_solution), on every rank.
Exact part: the integer systems of trans_cases (any summation order gives the integer x, partial sums spread over ranks included: the bound is on absolute
values) through the view path on 1 x 1 x 2, with the untransposed solve of the same handles asserted exact first, which is what proves the factors.  The two
cases of this file ("levels", "z_levels") stay on 1 x 1 x 2: the view path on an XY grid needs the store cut into every rank's block-cyclic share, which no
helper of the tests does, the solve of an XY handle refuses values that were not factored on it, and a 2 x 2 x 1 handle made from the CSR values of "levels"
misses the integer x already in its UNTRANSPOSED solve (SweepCase does not bound the product-form panel solves of an XY layer entry by entry).  That is a
limitation of "levels", not of XY handles: the exact tests of the transposed sweeps, refinement and expert solve on XY grids -- the cases whose untransposed
solve IS exact there -- are in test_gpu_grid_trans_exact.py."""
import ctypes as C
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import grid_trans_cases as gt
import trans_cases as tc
from superlu_dist_amd import _lib, driver, grid3d, matgen

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)

# Z only; one XY direction each (a row / column mix-up shows here); square, Pr != Pc, XY and Z, a deep Z tree over a process row
GRIDS = [(1, 1, 2), (2, 1, 1), (1, 2, 1), (2, 2, 1), (3, 2, 1), (2, 2, 2), (1, 2, 4)]


def _system_for(grid):
    # (2, 2, 2) and (1, 2, 4) on the larger operator and wider supernodes (relax 32, maxsup 128); everything else at the smallest
    return gt.system(12, relax=32, maxsup=128) if grid[2] > 1 and grid != (1, 1, 2) else gt.system(10, relax=16, maxsup=64)


@pytest.mark.parametrize("grid", GRIDS)
def test_own_pipeline_transposed(grid):
    """nrhs 1 (RK = 1 kernels) and 3, trans T and C (the same system on a double handle) in ONE set of handles per grid; every rank's replicated result"""
    S = _system_for(grid)
    cases = [(nrhs, trans) + gt.reference(S, nrhs, trans) for nrhs in (1, 3) for trans in ("T", "C")]
    out = gt.solve_on_grid(S, grid, [(b, trans) for _, trans, b, _ in cases])
    assert len(out) == grid[0] * grid[1] * grid[2]
    for rank, (xs, _, launches) in enumerate(out):
        assert launches > 0
        for (nrhs, trans, b, x1), x in zip(cases, xs):
            gt.check_solution(S, trans, b, x1, x, (grid, rank, nrhs, trans))
    for xs, _, _ in out[1:]:                                   # replicated: the all-gather hands every rank the owners' bits
        for a, b in zip(out[0][0], xs):
            assert np.array_equal(a, b)


def test_a_transposed_solve_is_not_the_untransposed_one():
    """the yardstick has teeth: on this operator the solution of A x = b misses A^T x = b by O(1)"""
    S = gt.system(10, relax=16, maxsup=64)
    b, x1 = gt.reference(S, 1, "T")
    xn = spla.spsolve(S.A.tocsc(), b[:, 0])
    assert np.abs(xn - x1[:, 0]).max() > 1e-3 * np.abs(x1).max()


def test_more_right_hand_sides_than_one_chunk():
    """nrhs = 70 with supernodes of up to 256 columns on 2 x 2 x 1: more than max_rhs_chunk (asserted from the widest supernode of the plan)"""
    S = gt.system(13, relax=32, maxsup=256)
    b, x1 = gt.reference(S, 70, "T")
    out = gt.solve_on_grid(S, (2, 2, 1), [(b, "T")])
    for rank, (xs, widest, _) in enumerate(out):
        assert tc.max_rhs_chunk(widest) < 70, widest
        gt.check_solution(S, "T", b, x1, xs[0], ((2, 2, 1), rank, 70))


@pytest.mark.parametrize("grid", [(1, 1, 2), (2, 2, 1)])
def test_complex16_transposed_and_conjugate_transposed(grid):
    """the analogue of grid_cases.check_own_pipeline_complex16: A^T and A^H of a matrix with non-real entries, nrhs = 2; the two solutions of the SAME
    right-hand side differ by far more than the tolerance, so the conj flag reaches the kernels"""
    S = gt.system(10, relax=16, maxsup=64, unsym=True, z=True)
    bT, xT = gt.reference(S, 2, "T")
    bC, xC = gt.reference(S, 2, "C")
    out = gt.solve_on_grid(S, grid, [(bT, "T"), (bC, "C"), (bT, "C")])
    for rank, (xs, _, _) in enumerate(out):
        gt.check_solution(S, "T", bT, xT, xs[0], (grid, rank, "T"))
        gt.check_solution(S, "C", bC, xC, xs[1], (grid, rank, "C"))
        assert np.abs(xs[2] - xs[0]).max() > 1e-3 * np.abs(xs[0]).max()          # A^H y = bT is another system than A^T x = bT
        assert np.linalg.norm(bT - S.op("C") @ xs[2]) / np.linalg.norm(bT) < 1e-10


@pytest.mark.parametrize("name", ["levels", "z_levels"])
def test_exact_systems_on_z_layers(name):
    """the sweep cases "levels" (double: levels of 66 / 1 / 33 supernodes) and "z_levels" (complex16) through the view path on 1 x 1 x 2, the store filled as
    test_gpu_trans_solve.py fills it (layer 1 starts with zeroed ancestor panels, as grid_cases.check_wide_supernodes does); nrhs 1 and 5; x compared bitwise.
    The untransposed solve of the same handles returns its integer x too (the factors on the grid are the exact ones)"""
    import grid_cases
    c, fs0 = tc.prepared(name)[:2]
    n, rp, ci = c.pattern_csr()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    tree = symb.partition(2)
    symb.free()
    comms = grid3d.local_comms(1, 1, 2)
    x0, b0 = c.rhs(5)
    cases = [(nrhs, conj) + tc.rhs_t(c, nrhs, conj) for nrhs in (1, 5) for conj in ((False, True) if c.z else (False,))]

    def body(z):
        fs = driver.FlatStore(fs0.n, fs0.xsup, fs0.Lrowind_off, fs0.Lrowind.copy(), fs0.Lnzval_off, fs0.Lnzval.copy(), fs0.Ufstnz_off, fs0.Ufstnz,
                              fs0.Unzval_off, fs0.Unzval.copy(), grid=(1, 1, 2), coords=(0, 0, z))
        if z:
            for k in np.flatnonzero(tree < 1):
                fs.Lnzval[fs.Lnzval_off[k]:fs.Lnzval_off[k + 1]] = 0.0
                fs.Unzval[fs.Unzval_off[k]:fs.Unzval_off[k + 1]] = 0.0
        h = grid3d.GridHandle.from_store(fs, grid_cases.forests_from_partition(tree, 2, z), comms[z])
        try:
            info = h.pdgstrf3d(0.0)
            h.plan_transposed(); h.plan_transposed()                      # idempotent
            y = h.pdgstrs3d(b0.copy(order="F"))
            return info, y, [h.pdgstrs3d(b.copy(order="F"), trans="C" if conj else "T") for _, conj, _, b in cases]
        finally:
            h.destroy()

    for rank, (info, y, xs) in enumerate(gt.run_ranks(2, body)):
        assert info == 0 and np.array_equal(y, x0), (rank, "untransposed")
        for (nrhs, conj, x, _), got in zip(cases, xs):
            assert np.array_equal(got, x), (name, rank, nrhs, conj, int(np.count_nonzero(got != x)))


@pytest.mark.parametrize("grid", [(2, 2, 1), (1, 1, 2)])
def test_transposed_refinement_on_grids(grid):
    """pdgsrfs3d(b, x0, trans="T") from x0 = x (1 + 1e-6 noise): berr below eps n on every rank, berr and step count identical on all ranks (bitwise: they
    are computed from replicated data -- every rank holds the all-gathered correction and applies the same update kernel -- and the continue / stop
    decision is a min-all-reduce).  Against the 1 x 1 x 1 handle only the bound is asserted: the transposed sweeps sum with atomics, so corrections differ
    in their last bits between two runs of ONE handle already, and a berr that lands within a few ulps of eps decides the rule `berr > eps` either way --
    the step counts may legitimately differ by one (both are printed)."""
    S = gt.system(10, relax=16, maxsup=64)
    b, x1 = gt.reference(S, 1, "T")
    rng = np.random.default_rng(5)
    x0 = np.asfortranarray(x1 * (1.0 + 1e-6 * rng.standard_normal(x1.shape)))
    symb = S.symbolic()
    h1 = driver.LUHandle.from_symbolic(symb, S.v)
    try:
        assert h1.pdgstrf3d(0.0) == 0
        h1.attach_matrix(S.n, S.rp, S.ci, S.v, symb.perm_c)
        _, berr1, steps1 = h1.pdgsrfs3d(b.copy(order="F"), x0.copy(order="F"), trans="T")
    finally:
        h1.destroy(); symb.free()

    def body(h, symb, rank):
        h.attach_matrix(S.n, S.rp, S.ci, S.v, symb.perm_c)
        return h.pdgsrfs3d(b.copy(order="F"), x0.copy(order="F"), trans="T")

    out = gt.on_grid(S, grid, body)
    print(f"{grid}: berr {[float(o[1][0]) for o in out]} steps {[o[2] for o in out]}; 1 x 1 x 1: berr {float(berr1[0])} steps {steps1}")
    assert berr1[0] < EPS * S.n and steps1 >= 1
    for x, berr, steps in out:
        assert berr[0] < EPS * S.n and steps >= 1
        assert np.array_equal(berr, out[0][1]) and steps == out[0][2] and np.array_equal(x, out[0][0])
        assert np.linalg.norm(b - S.op("T") @ x) / np.linalg.norm(b) < 1e-10


def test_expert_solve_transposed_on_a_grid():
    """pdgssvx3d(grid=(2, 2, 1), equil=True, trans="T") on an unsymmetric-pattern stencil operator whose rows are scaled by 2^-30 .. 2^30: the residual
    against the UNSCALED A^T below 1e-10; the handle was row-equilibrated (R takes the place of C on the transposed system)"""
    N = 8
    n, rp, ci, v = matgen.stencil3d_unsym(N, seed=1)
    rng = np.random.default_rng(8)
    v = v * (2.0 ** rng.integers(-30, 31, n))[np.repeat(np.arange(n), np.diff(rp))]
    perm = matgen.nd_perm_grid3d(N, N, N, leaf=27)
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    xt = rng.standard_normal((n, 2))
    b = np.asfortranarray(A.T @ xt)
    x, info, st = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=16, maxsup=64, equil=True, trans="T", grid=(2, 2, 1))
    assert info == 0 and st["equed"] in ("R", "B")
    res = float(np.linalg.norm(b - A.T @ x) / np.linalg.norm(b))
    print(f"expert solve, trans=T on 2 x 2 x 1: equed {st['equed']}, residual {res:.3e}")
    assert res < 1e-10
    with pytest.raises(ValueError):
        driver.pdgssvx3d(n, rp, ci, v, b, perm, equil=True, trans="T", grid=(2, 2, 1), keep=True)


def test_argument_errors_are_collective():
    """a bad trans value and the other precision's call on a 2 x 2 x 1 grid handle: SLUAMD_EINVAL on every rank, the vector untouched, nobody left waiting
    in an exchange (the pool join has a deadline); the handles still solve afterwards"""
    S = gt.system(10, relax=16, maxsup=64)
    b, x1 = gt.reference(S, 1, "T")
    dt, zt = _lib.entry("sluamd_pdgstrs3d_trans"), _lib.entry("sluamd_pzgstrs3d_trans")

    def body(h, symb, rank):
        xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b
        w = xp.copy(order="F")
        rcs = [dt(h._h, 3, w.ctypes.data_as(C.c_void_p), S.n, 1), dt(h._h, -1, w.ctypes.data_as(C.c_void_p), S.n, 1),
               zt(h._h, 1, w.ctypes.data_as(C.c_void_p), S.n, 1), zt(h._h, 2, w.ctypes.data_as(C.c_void_p), S.n, 1)]
        msg = _lib.load().sluamd_last_error().decode()
        with pytest.raises(ValueError):
            h.pdgstrs3d(xp, trans="X")
        return rcs, msg, np.array_equal(w, xp), h.pdgstrs3d(xp, trans="T")[symb.perm_c, :]

    for rank, (rcs, msg, untouched, x) in enumerate(gt.on_grid(S, (2, 2, 1), body)):
        assert rcs == [-1, -1, -1, -1] and untouched and "double handle" in msg, (rank, rcs, msg)
        gt.check_solution(S, "T", b, x1, x, ("after the refused calls", rank))


def test_a_grid_handle_takes_transposed_solves_once_they_are_planned():
    """before GridHandle.plan_transposed() a 2 x 2 x 1 handle refuses on every rank, before any exchange (nobody left waiting) and with the call to make named
    in the message; the untransposed solve is unaffected; after the call the same handle solves the transposed system"""
    S = gt.system(10, relax=16, maxsup=64)
    b, x1 = gt.reference(S, 1, "T")

    def body(h, symb, rank):
        xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b
        with pytest.raises(RuntimeError, match="sluamd_PlanTransposedSweeps"):
            h.pdgstrs3d(xp, trans="T")
        xn = h.pdgstrs3d(xp)
        h.plan_transposed()
        return xn, h.pdgstrs3d(xp, trans="T")[symb.perm_c, :]

    for rank, (xn, x) in enumerate(gt.on_grid(S, (2, 2, 1), body, plan=False)):
        gt.check_solution(S, "T", b, x1, x, ("planned after a refusal", rank))
