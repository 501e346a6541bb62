"""Shared bodies of the refinement tests on reference fixtures (IterRefine = SLU_DOUBLE records): the product library on a GPU
(test_gpu_zrefine.py) and, for double precision on process grids, the CPU test build of the host sources (test_zrefine_cpu.py).

The fixtures were recorded with Equil = YES and MC64: the `..._pre` stores hold the factors of Pc A' Pc^T with A' = diag(R) A diag(C)
and Pc = r0__perm_c.  The refinement runs on the system the reference refined -- A', B' = R o B, perm_c -- and the result X = C o X'
is compared with the recorded x.  perm_r is NOT applied: the row permutation is already inside the recorded factors' system."""
import numpy as np
from superlu_dist_amd import driver, grid3d
import grid_cases as gc

EPS = 2.0 ** -53


def equilibrated_system(g):
    """(n, rowptr, colind, A' values, B', recorded x, C, perm_c) assembled from the rows of ALL ranks: the 3-D driver spreads A over
    every layer, each rank holding the disjoint rows [A_fst_row, A_fst_row + A_m_loc)."""
    P = int(g["nranks"][0])
    n, nrhs = int(g["r0__n"][0]), int(g["r0__nrhs"][0])
    dt = g["r0__A_nzval"].dtype
    R, Cs, pc = g["r0__R"], g["r0__C"], g["r0__perm_c"]
    rows, cols, vals = [], [], []
    B = np.zeros((n, nrhs), dtype=dt, order="F"); X = np.zeros((n, nrhs), dtype=dt, order="F")
    seen = np.zeros(n, dtype=np.int64)
    for f0, q in sorted((int(g[f"r{q}__A_fst_row"][0]), q) for q in range(P)):
        p = f"r{q}__"
        ml = int(g[p + "A_m_loc"][0])
        if ml == 0:
            continue
        rp = g[p + "A_rowptr"]
        rows.append(np.repeat(np.arange(f0, f0 + ml), np.diff(rp[:ml + 1])))
        cols.append(g[p + "A_colind"][rp[0]:rp[ml]]); vals.append(g[p + "A_nzval"][rp[0]:rp[ml]])
        B[f0:f0 + ml, :] = g[p + "b"][:ml * nrhs].reshape((ml, nrhs), order="F")
        X[f0:f0 + ml, :] = g[p + "x"][:ml * nrhs].reshape((ml, nrhs), order="F")
        seen[f0:f0 + ml] += 1
    assert np.all(seen == 1)                      # the ranks' row ranges partition the rows
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    vs = (vals * R[rows]) * Cs[cols]
    return n, rowptr, cols.astype(np.int32), vs, np.asfortranarray(R[:, None] * B), X, Cs, pc


def refine_fixture_on_grid(g):
    """Every rank of the fixture's grid (threads over the in-process transport): factor its `..._pre` store, solve
    xp[perm_c] = B', attach A' and refine (GridHandle, replicated form).  Returns (recorded x, [(C o X', berr, steps) per rank])."""
    P = int(g["nranks"][0])
    Pr, Pc, Pz = [int(v) for v in g["grid"]]
    n, rp, ci, v, B, xref, Cs, pc = equilibrated_system(g)
    comms = grid3d.local_comms(Pr, Pc, Pz)

    def body(rank):
        p = f"r{rank}__"
        r, c, z = int(g[p + "myrow"][0]), int(g[p + "mycol"][0]), int(g[p + "myz"][0])
        st = driver.FlatStore.from_golden(g, rank, "pre")
        h = grid3d.GridHandle.from_store(st, gc.forests_of(g, rank), comms[(z * Pr + r) * Pc + c],
                                         replace_tiny=bool(g[p + "ReplaceTinyPivot"][0]))
        try:
            assert h.pdgstrf3d(float(g[p + "thresh"][0])) == int(g[p + "info"][0])
            xp = np.zeros_like(B, order="F"); xp[pc, :] = B
            X0 = np.asfortranarray(h.pdgstrs3d(xp)[pc, :])
            h.attach_matrix(n, rp, ci, v, pc)
            X, berr, steps = h.pdgsrfs3d(B, X0)
        finally:
            h.destroy()
        return X * Cs[:, None], berr, steps

    return xref, grid3d.run_ranks(P, body)


def check_refined_fixture_on_grid(g, check_steps):
    """Every rank returns the same X, berr and step count (bitwise); X matches the recorded x within 1e-12 max|x|; berr <= 4 eps;
    check_steps: the step count is the reference's RefineSteps to one step."""
    xref, out = refine_fixture_on_grid(g)
    X, berr, steps = out[0]
    for q, (Xq, bq, sq) in enumerate(out[1:], 1):
        assert np.array_equal(Xq, X) and np.array_equal(bq, berr) and sq == steps, q
    err = np.abs(X - xref).max() / np.abs(xref).max()
    print(f"rel err {err:.2e} berr/eps {(berr / EPS).round(3).tolist()} steps {steps}"
          + (f" ref {int(g['r0__RefineSteps'][0])}" if "r0__RefineSteps" in g else ""))
    assert err <= 1e-12
    assert np.all(berr <= 4 * EPS)
    if check_steps:
        assert abs(steps - int(g["r0__RefineSteps"][0])) <= 1     # pzgsmv uses |x| for off-process columns: the stopping test moves by a step
    return X, berr, steps
