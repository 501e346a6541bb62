"""The extra-precise refinement loop (sluamd_p[dz]gsrfs3d_extra[_dev], sluamd_xrefine.cpp).

Exact trajectories: tests/xrefine_cases.py attaches a matrix that is not the factored one to handles holding exact factors; the corrections shrink by a
fixed dyadic ratio, and every norm, ratio decision, state, step count, dxrel, rho, berr and X is predicted and compared on bit patterns -- CONVERGED by
ndx <= eps nx (met with equality) and by ndx == 0, NO_PROGRESS at ratio 3 / 4 (X is the one before the dropped correction), LIMIT at ratio exactly 1 / 2;
three columns ending in three states; a transposed system; one trajectory through the real sweeps.

One real factorisation: a tridiagonal integer matrix with cond_2 = 1.4e11 and an integer solution, where the fp64 loop stalls at a forward error of 6e-10
and the extra-precise one reaches the solution itself (on the CPU with a scipy LU and the restated residuals: err_plain = 5.9e-10, err_extra = 0)."""
import numpy as np
import pytest
import xrefine_cases as xc
from superlu_dist_amd import driver

pytestmark = pytest.mark.gpu
TRAJ = xc.trajectories()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check(name, r, X, berr, steps, dxrel, state, rho):
    print(name, "steps", list(steps), r["steps"], "state", list(state), r["state"], "dxrel", list(dxrel), r["dxrel"], "rho", list(rho), r["rho"], "berr", list(berr),
          r["berr"].tolist())
    assert list(state) == r["state"] and list(steps) == r["steps"], name
    assert np.array_equal(_bits(np.asarray(dxrel, dtype=np.float64)), _bits(np.array(r["dxrel"]))), name
    assert np.array_equal(_bits(np.asarray(rho, dtype=np.float64)), _bits(np.array(r["rho"]))), name
    assert np.array_equal(_bits(berr), _bits(r["berr"])), name
    bad = np.flatnonzero(_bits(X) != _bits(r["X"]))
    assert bad.size == 0, (name, "X differs at", bad[:8].tolist())


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_diag_handles_follow_the_exact_trajectory(z):
    """host form, every trajectory of this precision on one handle (so each also runs behind another matrix's work vectors and norm words)"""
    h = xc.factored("diag", 65, z)
    for name, (c, trans, _) in TRAJ.items():
        if c.z != z:
            continue
        h.attach_matrix(c.n, *xc.attached(c, trans), c.pc)
        X, berr, steps, dxrel, state = h.pdgsrfs3d(c.B.copy(order="F"), c.X0.copy(order="F"), method="extra", trans=trans)
        _check(name, xc.expected(name), X, berr, steps, dxrel, state, h.refine_rho)
    c = TRAJ[("z_" if z else "d_") + "noprog"][0]
    assert X is not None and not np.array_equal(xc.expected(("z_" if z else "d_") + "noprog")["X"], c.X0)
    h.destroy()


@pytest.mark.parametrize("name", ["d_rhs3", "z_rhs3", "d_trans"])
def test_dev_form_with_padded_leading_dimensions(name):
    """sluamd_p[dz]gsrfs3d_extra_dev: ldb = n + 3, ldx = n + 5; B and the padding rows of X come back bitwise unchanged"""
    c, trans, _ = TRAJ[name]
    n, nrhs = c.n, c.nrhs
    h = xc.factored("diag", n, c.z)
    h.attach_matrix(n, *xc.attached(c, trans), c.pc)
    dt = np.complex128 if c.z else np.float64
    B = np.full((n + 3, nrhs), np.nan, dtype=dt, order="F"); B[:n] = c.B
    X = np.full((n + 5, nrhs), np.nan, dtype=dt, order="F"); X[:n] = c.X0
    dB, dX = xc.Dev(B), xc.Dev(X)
    berr, steps, dxrel, state = h.pdgsrfs3d_dev(dB.ptr.value, n + 3, dX.ptr.value, n + 5, nrhs, method="extra", trans=trans)
    gB, gX = dB.host(), dX.host()
    dB.free(); dX.free()
    _check(name, xc.expected(name), np.asfortranarray(gX[:n]), berr, steps, dxrel, state, h.refine_rho)
    assert np.array_equal(_bits(gB), _bits(B)) and np.array_equal(_bits(gX[n:]), _bits(X[n:]))
    h.destroy()


def test_a_trajectory_through_the_real_sweeps():
    """the nilpotent chain of refine_exact_cases on the factors of the sweep case "narrow": three corrections, then a residual of zero and dx == 0"""
    c = xc.rx.cases()[xc.SWEEP_CASE]
    assert c.kind in xc.SWEEPS
    r = xc.sweep_expected()
    assert r["state"] == [xc.CONVERGED] and r["steps"] == [3] and r["dxrel"] == [0.0]
    h = xc.factored(c.kind, c.n, c.z)
    h.attach_matrix(c.n, c.rp, c.ci, c.av, c.pc)
    X, berr, steps, dxrel, state = h.pdgsrfs3d(c.B.copy(order="F"), c.X0.copy(order="F"), method="extra")
    _check(xc.SWEEP_CASE, r, X, berr, steps, dxrel, state, h.refine_rho)
    assert np.array_equal(X, c.expect["final"])
    h.destroy()


def test_an_ill_conditioned_system_reaches_the_solution():
    """cond_2 = 1.4e11 (checked on the CPU).  err = max|x - x_true| / max|x_true|.  The CPU loops (scipy LU, restated residuals): err_plain = 5.9e-10 at 0
    steps, err_extra = 0.  Asserted: err_extra <= 4 (the CPU loop's err_extra); err_plain >= 2^5 err_extra; CONVERGED; the estimate dxrel / (1 - rho) is at
    least err_extra / 4.  Measured on an MI355X: err_plain = 3.9e-07 (1 step, berr 1.0e-16), err_extra = 0 (1 step, CONVERGED by dx == 0)"""
    ic = xc.ill_case()
    cpu = xc.ill_cpu_loops()
    n, xt = ic["n"], ic["x_true"]
    err = lambda x: float(np.abs(np.asarray(x).reshape(-1) - xt).max() / np.abs(xt).max())
    xp, info, stp = driver.pdgssvx3d(n, ic["rp"], ic["ci"], ic["av"], ic["b"], refine=True)
    assert info == 0
    xe, info, ste = driver.pdgssvx3d(n, ic["rp"], ic["ci"], ic["av"], ic["b"], refine="extra")
    assert info == 0
    err_plain, err_extra = err(xp), err(xe)
    est = float(ste["refine_dxrel"][0] / (1.0 - ste["refine_rho"][0]))
    print("cond %.3e" % ic["cond"], "GPU: err_plain %.3e (steps %s, berr %.2e)" % (err_plain, stp["refine_steps"], stp["berr"][0]),
          "err_extra %.3e (steps %s, state %s, dxrel %.3e, rho %.3e, estimate %.3e, berr %.2e)" % (err_extra, ste["refine_steps"], ste["refine_state"], ste["refine_dxrel"][0],
                                                                                                   ste["refine_rho"][0], est, ste["berr"][0]), "CPU:", cpu)
    assert err_extra <= 4 * cpu["err_extra"]
    assert err_plain >= 2.0 ** 5 * err_extra and err_plain > 0
    assert int(ste["refine_state"][0]) == xc.CONVERGED
    assert est >= err_extra / 4
