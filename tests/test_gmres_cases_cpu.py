"""The cases of tests/gmres_cases.py hold what the GPU tests rely on, by numpy alone: the premises (rho(I - A^-1 A') > 1, cond_inf(A') <= 2^10), the plain
refinement loop failing (berr >= 2^-20 at its end), the float64 model of the GMRES refinement reaching berr <= 4 max(2^-53, berr_ref) with a first cycle of at
most t + 1 iterations -- and of MORE than 2 for t >= 2, more than 8 for t = 10: the eigenvalues 1 + m_k are distinct, so the ranks are different tests and
t = 10 runs past one pass of the Krylov kernels.  The E = 0 cases and the columns of the three-column cases that start exact or one eigenvector away are exempt from "plain fails":
there is nothing for it to fail at."""
import numpy as np
import pytest
import gmres_cases as gc

RANK = gc.names(rank=True, large=True)
TRANS = {False: ("N", "T"), True: ("N", "T", "C")}


@pytest.mark.parametrize("name", list(gc.cases()))
def test_premises(name):
    c = gc.cases()[name]
    rho, cond = gc.check_premises(c)
    print(name, "rho", rho, "cond_inf", cond)
    for trans in TRANS[c.z]:                                                                 # b = op(A') x* is exact: x* has backward error 0
        S = gc.system(name, trans)
        assert all(S.berr(c.xs[:, j], c.rhs(trans)[:, j])[1] == 0.0 for j in range(c.nrhs))


@pytest.mark.parametrize("name", RANK)
def test_plain_fails_and_the_model_converges(name):
    c = gc.cases()[name]
    for trans in (TRANS[c.z] if c.n < gc.LARGE_N else ("N",)):
        p = gc.model_plain(name, trans)
        m = gc.model_gmres_ir(name, trans)
        ref, bnd = gc.reference(name, trans)[1], gc.bound(name, trans)
        print(name, trans, "berr_ref", ref.tolist(), "plain", p["berr"].tolist(), p["steps"], "model", m["berr"].tolist(), m["steps"], m["solves"], m["iters"])
        j = c.nrhs - 1                                                                       # the column that starts from zero
        assert p["berr"][j] >= 2.0 ** -20
        assert np.all(m["berr"] <= bnd), (m["berr"], bnd)
        for its in m["iters"]:
            assert not its or its[0] <= c.t + 1
        first = m["iters"][j][0]
        assert first >= c.t or (c.m[0] > 0 and first >= 3), (first, c.t)                     # t + 1 from zero, or t where the estimate meets inner_tol one iteration early (n = 1: the space is spent); the clustered cases sooner
        assert first > 2 or c.t < 2
        assert first > 8 or c.t < gc.BIG_T
        if c.n < gc.LARGE_N:
            assert gc.error_bound_ok(c, trans, m["X"], m["berr"])


@pytest.mark.parametrize("name", gc.names(rank=False))
def test_exact_starts_take_no_step(name):
    m = gc.model_gmres_ir(name)
    assert m["steps"] == [0] and m["solves"] == [0] and m["berr"][0] == 0.0 and np.array_equal(m["X"], gc.cases()[name].X0)


@pytest.mark.parametrize("name", [k for k in gc.cases() if k.endswith("rhs3")])
def test_three_columns_take_different_numbers_of_solves(name):
    m = gc.model_gmres_ir(name)
    assert m["solves"][0] == 0 and 0 < m["solves"][1] < m["solves"][2], m["solves"]


@pytest.mark.parametrize("name", ["d_diag_n513_t4_cluster", "z_lu_n513_t4_cluster"])
def test_restart_in_the_model(name):
    """restart = 2 where a cycle needs 5 iterations: every cycle is cut at 2, more outer steps and more solves than unrestarted, the bound still met"""
    full, m = gc.model_gmres_ir(name), gc.model_gmres_ir(name, restart=2)
    assert all(k == 2 for k in m["iters"][0]) and full["iters"][0][0] > 2
    assert m["steps"][0] > full["steps"][0] and m["solves"][0] > full["solves"][0] and np.all(m["berr"] <= gc.bound(name, "N")), m


@pytest.mark.parametrize("name", ["d_diag_n513_t10", "z_lu_n513_t10"])
def test_budget_in_the_model(name):
    """max_solves = 5 cuts a first cycle that would have gone on to 11 iterations: 4 iterations and the end of the cycle"""
    full, m = gc.model_gmres_ir(name), gc.model_gmres_ir(name, max_solves=5)
    assert m["solves"] == [5] and m["iters"] == [[4]] and m["steps"] == [1] and full["iters"][0][0] > 4
    assert gc.model_gmres_ir(name, max_solves=1)["solves"] == [1]


def test_the_sweep_kinds_of_the_exact_cases_cannot_meet_the_conditioning_premise():
    """why kind "lu" stands where "narrow", "levels", "z_narrow", "z_wide" were asked for: cond_inf of their factored matrices by numpy, against 2^10"""
    import refine_exact_cases as rx
    import trans_cases as tc
    for kind in rx.SWEEPS:
        F = tc.prepared(kind)[0].B16.toarray() / 16
        cond = float(np.real(np.linalg.cond(F, np.inf)))
        print(kind, "cond_inf", cond)
        assert cond > 2.0 ** 40
