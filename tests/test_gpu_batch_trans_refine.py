"""Refinement of the transposed and conjugate-transposed systems on a batch (sluamd_[dz]BatchSolve with refine and trans != N): the exact trajectories of
zbatch_cases.refine_case -- double with T, complex16 with T and C -- against sluamd_p[dz]gsrfs3d_trans on each matrix alone and against the numpy replay of
the loop, and the transposed refinement of an equilibrated float batch."""
import numpy as np
import pytest
import batch_cases as bc
import zbatch_cases as zc
from test_gpu_batch import _equil_values
from superlu_dist_amd import driver

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


@pytest.mark.parametrize("z,trans", [(False, "T"), (True, "T"), (True, "C")])
def test_transposed_refinement_per_matrix_equals_each_matrix_alone(z, trans):
    m, count, d, A, N, b = zc.refine_case(z)
    drp, dci = np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32)
    s = driver.Symbolic(m, drp, dci, None, relax=8, maxsup=64)
    perm = s.perm_c.copy()
    bh = (driver.ZBatchHandle if z else driver.BatchHandle).create(s, d)
    assert not bh.factor().any()
    rp, ci, v = zc.csr(zc.block_diag(A))                    # diag(A'_0, A'_1, A'_2) attached to the batch's handle
    driver._attach_matrix(bh.handle(), z, count * m, rp, ci, v, np.concatenate([perm + k * m for k in range(count)]))
    x, berr, steps = bh.solve(b, trans=trans, refine=True)
    print(f"z = {z}, trans = {trans}: steps", steps, "berr", berr)
    # the conditions the CPU test establishes by replay: 0 steps, >= 3 steps, the SAFE1 matrix
    assert steps[0] == 0 and steps[1] >= 3 and steps[2] >= 1 and berr[0, 1] == 0.0
    for k in range(count):
        h = driver.LUHandle.from_symbolic(s, d[k])
        assert h.pdgstrf3d() == 0
        xp = np.zeros((m, 2), dtype=b.dtype, order="F"); xp[perm, :] = b[k]
        x0 = np.asfortranarray(h.pdgstrs3d(xp, trans=trans)[perm, :])
        rpk, cik, vk = zc.csr(A[k])
        h.attach_matrix(m, rpk, cik, vk, perm)
        xs, bes, st = h.pdgsrfs3d(np.asfortranarray(b[k]), x0, trans=trans)
        h.destroy()
        assert st == steps[k]
        assert np.array_equal(bes, berr[k]) and np.array_equal(xs, x[k]), k
        for j in range(2):
            xe, be, se, _ = zc.replay(d[k], A[k], b[k][:, j], trans, m)
            assert np.array_equal(x[k][:, j], xe) and berr[k, j] == be and (j == 0 or se == steps[k])
        assert np.array_equal(zc.op(A[k], trans) @ x[k], b[k])           # op(A') x = b exactly ...
        if k > 0:
            assert not np.array_equal(A[k] @ x[k], b[k])                 # ... and A' x != b where N != 0
            if z:
                assert not np.array_equal(zc.op(A[k], "C" if trans == "T" else "T") @ x[k], b[k])
    # SAFE1 from m, not from count m
    Ao = zc.op(A[2], trans)
    t = zc.abs1(Ao) @ zc.abs1(x[2][:, 1]) + zc.abs1(b[2][:, 1])
    assert berr[2, 1] == ((m + 1) * 2.0 ** -1022 / t).max() and berr[2, 1] != ((count * m + 1) * 2.0 ** -1022 / t).max()
    bh.destroy(); s.free()


def test_transposed_refinement_of_an_equilibrated_float_batch():
    """A_k^T x = b on the batch of test_gpu_batch's equilibration test (row and column scalings by 2^+-20 per matrix): the scaled transposed system is
    refined, B scaled by C and X by R; the bounds of test_python_driver_with_refinement"""
    c = bc.float_case("m100x5")
    v = _equil_values(c)
    rng = np.random.default_rng(4)
    b = rng.uniform(-1, 1, size=(c.count, c.m, 2))
    x, info, st = driver.pdgssvx3d_batch(c.m, c.rp, c.ci, v, b, relax=8, maxsup=64, equil=True, refine=True, trans="T")
    print("equed", st["equed"], "steps", st["refine_steps"])
    assert not info.any() and st["berr"].shape == (c.count, 2) and st["refine_steps"].shape == (c.count,)
    assert set(st["equed"]) > {"N"}                                     # some matrices are scaled: s_in / s_out matter
    for k in range(c.count):
        At = np.zeros((c.m, c.m)); At[c.ci, c.rows] = v[k]
        res = np.abs(At @ x[k] - b[k]).max() / (np.abs(At).sum(axis=1).max() * np.abs(x[k]).max())
        print(f"matrix {k}: residual {res:.3e}, berr {st['berr'][k]}")
        assert res <= 1e-14
    assert np.all(st["berr"] <= 4 * EPS)
