"""The exchange plan of the TRANSPOSED grid sweeps (LevelSched::xt_red_* / xt_bc_*, built by sluamd_PlanTransposedSweeps on a handle that exists) on the CPU
test build of the library's host sources: the planner is the product's, read through sluamd_plan_xlists.  No sweep runs here (the CPU build has no
transposed kernels); what is checked is what keeps a transport from waiting forever and a sum from landing on the wrong rank:

  1. every send list of rank p to rank q equals the receive list of q from p at the same (Z level, DAG level): same runs, same order -- for the
     transposed lists and, for free, for the untransposed ones;
  2. direction and coverage.  The library broadcasts x_k to ALL other ranks of the process row / column where blocks that read it can live (the
     untransposed sweeps do the same down the column), so the receivers are checked against that set: on every layer that sweeps the forest of
     supernode k, x_k is broadcast exactly once from the diagonal owner (k % Pr, k % Pc) to every other rank of process ROW k % Pr -- the ranks that can
     hold a block of U(k, :) or a row block of L that reads x_k -- and to nobody else; the partial sums of x_k come exactly once from every other rank of
     process COLUMN k % Pc -- the ranks that can hold a block of U(:, k) or of L(:, k) -- to the owner.  The untransposed lists satisfy the mirror image."""
import numpy as np
import pytest
from superlu_dist_amd import driver, grid3d, matgen
import grid_cases

GRIDS = [(2, 2, 1), (3, 2, 1), (2, 2, 2)]


def _plans(grid):
    Pr, Pc, Pz = grid
    N = 8
    n, rp, ci, v = matgen.poisson3d(N)
    perm = matgen.nd_perm_grid3d(N, N, N, leaf=27)
    symb = driver.Symbolic(n, rp, ci, perm, relax=16, maxsup=64)
    xsup = symb.xsup()
    tree = symb.partition(Pz) if Pz > 1 else np.zeros(symb.nsupers, dtype=np.int32)
    comms = grid3d.local_comms(Pr, Pc, Pz)

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], tree if Pz > 1 else None)
        try:
            assert all(len(h.plan_xlists(w)) == 0 for w in driver.XLISTS[4:])      # planned on request only
            h.plan_transposed()
            return {w: h.plan_xlists(w) for w in driver.XLISTS}
        finally:
            h.destroy()

    plans = grid3d.run_ranks(Pr * Pc * Pz, body)
    symb.free()
    return xsup, tree, plans


def _by_message(rows):
    """{(Z level, DAG level, peer): [(first row, rows), ...] in list order}"""
    out = {}
    for zl, l, peer, r0, nr in rows.tolist():
        out.setdefault((zl, l, peer), []).append((r0, nr))
    return out


@pytest.mark.parametrize("grid", GRIDS)
def test_both_sides_of_every_message_agree(emul, grid):
    xsup, tree, plans = _plans(grid)
    P = len(plans)
    nmsg = 0
    for pre in ("xt_red", "xt_bc", "xs_red", "xs_bc"):
        snd = [_by_message(plans[p][pre + "_send"]) for p in range(P)]
        rcv = [_by_message(plans[p][pre + "_recv"]) for p in range(P)]
        for p in range(P):
            for (zl, l, q), runs in snd[p].items():
                assert rcv[q].get((zl, l, p)) == runs, (pre, "send", p, q, zl, l)
                nmsg += 1
            for (zl, l, q), runs in rcv[p].items():
                assert snd[q].get((zl, l, p)) == runs, (pre, "recv", p, q, zl, l)
    assert nmsg > 0


@pytest.mark.parametrize("grid", GRIDS)
def test_directions_and_coverage(emul, grid):
    Pr, Pc, Pz = grid
    xsup, tree, plans = _plans(grid)
    ns = len(xsup) - 1
    sn_of_row = np.repeat(np.arange(ns), np.diff(xsup))

    def moved(rows):
        """{(supernode, peer): times}; a run covers whole supernodes"""
        out = {}
        for zl, l, peer, r0, nr in rows.tolist():
            ks = np.unique(sn_of_row[r0:r0 + nr])
            assert xsup[ks[0]] == r0 and xsup[ks[-1] + 1] == r0 + nr
            for k in ks.tolist():
                out[(k, peer)] = out.get((k, peer), 0) + 1
        return out

    for z in range(Pz):
        fr = grid_cases.forests_from_partition(tree, Pz, z) if Pz > 1 else None
        swept = np.ones(ns, dtype=bool) if fr is None else np.zeros(ns, dtype=bool)
        if fr is not None:
            for lvl, t in enumerate(fr["myTreeIdxs"]):
                if not fr["myZeroTrIdxs"][lvl]:
                    swept |= tree == t
        rank = lambda r, c: (z * Pr + r) * Pc + c
        # expected (supernode, peer) sets per rank and list; (axis of the reduce, axis of the broadcast): transposed = (column, row), untransposed = (row, column)
        for pre, red_along_col in (("xt", True), ("xs", False)):
            for r in range(Pr):
                for c in range(Pc):
                    want = {w: {} for w in ("red_send", "red_recv", "bc_send", "bc_recv")}
                    for k in np.flatnonzero(swept).tolist():
                        kr, kc = k % Pr, k % Pc
                        col_peers = [rank(r2, kc) for r2 in range(Pr) if r2 != kr]      # the other ranks of process column k % Pc
                        row_peers = [rank(kr, c2) for c2 in range(Pc) if c2 != kc]      # the other ranks of process row k % Pr
                        red, bc = (col_peers, row_peers) if red_along_col else (row_peers, col_peers)
                        if (r, c) == (kr, kc):
                            for q in red:
                                want["red_recv"][(k, q)] = 1
                            for q in bc:
                                want["bc_send"][(k, q)] = 1
                        else:
                            if rank(r, c) in red:
                                want["red_send"][(k, rank(kr, kc))] = 1
                            if rank(r, c) in bc:
                                want["bc_recv"][(k, rank(kr, kc))] = 1
                    for w, exp in want.items():
                        assert moved(plans[rank(r, c)][f"{pre}_{w}"]) == exp, (pre, w, (r, c, z))
