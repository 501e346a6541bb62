"""The case generators of zbatch_cases.py check themselves in numpy: the complex exact cases (L U = A exactly, small dyadic values, A^T x != A^H x), the condition
bound of the complex float cases, and the refinement cases of both precisions by an exact replay of the loop (predicted step counts, the SAFE1 branch, the
exact end point of the transposed systems)."""
import numpy as np
import pytest
import zbatch_cases as zc


def _gaussian_integers(a):
    return np.array_equal(a.real, np.round(a.real)) and np.array_equal(a.imag, np.round(a.imag))


@pytest.mark.parametrize("name", list(zc.SHAPES))
def test_exact_cases_are_exact(name):
    c = zc.exact_case(name)
    m = c.m
    assert c.dense.dtype == np.complex128 and c.values.shape == (c.count, c.nnz)
    for k in range(c.count):
        L, U, A = c.L[k], c.U[k], c.dense[k]
        assert np.array_equal(L @ U, A)
        S, D, T = L - np.eye(m), np.diag(np.diag(U)), U - np.diag(np.diag(U))
        assert not np.any(S @ S) and not np.any(T @ np.linalg.inv(D) @ T)          # the structural identities the exactness rests on
        # all values are representable: Gaussian integers of a few bits; the reciprocals of D powers of two times units
        assert _gaussian_integers(A) and max(np.abs(A.real).max(), np.abs(A.imag).max()) < 2 ** 10
        dg = np.diag(U)
        assert set(np.abs(dg)) <= {1.0, 2.0, 4.0} and np.all((dg.real == 0) != (dg.imag == 0))
        assert np.array_equal((1.0 / dg) * dg, np.ones(m))
        # the factors reproduce the inverse exactly: inv(L) = I - S, inv(U) = D^-1 - D^-1 T D^-1
        Di = np.diag(1.0 / dg)
        assert np.array_equal((np.eye(m) - S) @ L, np.eye(m)) and np.array_equal((Di - Di @ T @ Di) @ U, np.eye(m))
    for nrhs in zc.NRHS:
        x, b, bt, bh = c.rhs(nrhs)
        assert _gaussian_integers(x) and _gaussian_integers(b) and _gaussian_integers(bt) and _gaussian_integers(bh)
        assert not np.array_equal(bt, bh) and not np.array_equal(b, bt)
        for k in range(c.count):
            assert np.array_equal(c.dense[k] @ x[k], b[k]) and np.array_equal(c.dense[k].T @ x[k], bt[k]) and np.array_equal(c.dense[k].conj().T @ x[k], bh[k])


def test_singular_case_changes_one_matrix_only():
    reg, c = zc.exact_case("m100x5"), zc.exact_case("m100x5", singular=(2, 37))
    for k in range(c.count):
        assert np.array_equal(c.dense[k], reg.dense[k]) == (k != 2)
    assert zc.first_zero_pivot(c.dense[2], np.arange(c.m)) == 37 and zc.first_zero_pivot(c.dense[1], np.arange(c.m)) == -1


@pytest.mark.parametrize("name", ["m100x5", "m300x2"])
def test_float_cases_are_well_conditioned(name):
    c = zc.float_case(name)
    assert np.iscomplexobj(c.values) and np.abs(c.values.imag).max() > 0.5
    for k in range(c.count):
        cond = np.linalg.cond(c.dense[k], 2)
        print(f"{name} matrix {k}: cond_2 = {cond:.2f}")
        assert cond <= 100


@pytest.mark.parametrize("z,trans", [(False, "N"), (False, "T"), (True, "N"), (True, "T"), (True, "C")])
def test_refinement_cases_by_exact_replay(z, trans):
    m, count, d, A, N, b = zc.refine_case(z)
    assert not np.any(N[0]) and np.any(np.linalg.matrix_power(N[1], 3)) and not np.any(np.linalg.matrix_power(N[1], 4)) and not np.any(N[2] @ N[2])
    assert not np.array_equal(N[1], N[1].T) and not np.array_equal(N[2], N[2].T)
    steps = np.zeros((count, 2), dtype=int)
    for k in range(count):
        for j in range(2):
            x, berr, st, safe1_rows = zc.replay(d[k], A[k], b[k][:, j], trans, m)
            steps[k, j] = st
            Ao = zc.op(A[k], trans)
            assert np.array_equal(Ao @ x, b[k][:, j])                       # the nilpotent iteration ended at the exact solution
            if trans != "N" and k > 0:
                assert not np.array_equal(A[k] @ x, b[k][:, j])             # ... of the TRANSPOSED system
            if z and k > 0:
                other = zc.op(A[k], {"N": "T", "T": "C", "C": "T"}[trans])
                assert not np.array_equal(other @ x, b[k][:, j])
            assert safe1_rows == (k == 2)
            if k == 2:                                                      # SAFE1 from m, not from count m: it changes berr
                _, berr_big, _, _ = zc.replay(d[k], A[k], b[k][:, j], trans, count * m)
                t = zc.abs1(Ao) @ zc.abs1(x) + zc.abs1(b[k][:, j])
                assert berr == ((m + 1) * zc.SAFMIN / t).max() and berr != berr_big
            else:
                assert berr == 0.0
    print(f"z = {z}, trans = {trans}: steps per matrix and right-hand side", steps.tolist())
    assert not steps[0].any() and steps[1].min() >= 3 and steps[2].min() >= 1
