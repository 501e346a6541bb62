"""Exact integer systems for the TRANSPOSED and CONJUGATE-TRANSPOSED solves on XY process grids (test helper for test_gpu_grid_trans_exact.py and
test_grid_trans_exact_cases_cpu.py; not a conftest).

What is exact on an XY grid.  A grid handle made from the CSR values of a case factors them itself, on an XY layer with the product form of the panel solves
(k_panel_gemm with inverted diagonal blocks).  sweep_cases.SweepCase bounds that form through max-row-sum products only, panel_cases.PanelCase.panel_bounds
entry by entry; the suite already asserts the UNTRANSPOSED integer x on XY grids for "widths", "z_narrow" (test_gpu_sweep_shapes.py), "narrow"
(test_gpu_refine_exact.py) and every panel case (test_gpu_panel_forms.py).  The sweep case "levels" misses its integer x there -- that is a limitation of
"levels", not of XY handles -- and is not part of this set.  Every test of the transposed path asserts the untransposed integer x of the SAME handles first:
that is what proves the factors, case by case and grid by grid.

The transposed right-hand sides are those of trans_cases.rhs_t.  Its two bounds are on absolute values, so they hold for any summation order, the partial
sums of a process column spread over ranks and added by the reduce included; PanelCase subclasses SweepCase, so rhs_t applies to the panel cases unchanged.
The bounds are never relaxed: a case that misses one at a wanted nrhs is run with narrow=True (x in {-1, 0, 1}; listed in NARROW, asserted by the CPU
tests), and a case that misses it even then is not part of the set.  Both panel cases hold every bound with their full integer x: none was narrowed or dropped.

CASES   widths (double, supernodes of 1 .. 256 columns: wider than 128), narrow (double, <= 64 columns), z_narrow (complex16), mixed_level (double panel
        case: narrow supernodes on levels of 64 .. 256-column ones under a 70-column top), z_chain (complex16 panel case: every width class up to 256)
GRIDS   one XY direction each, square, Pr != Pc, and XY with Z (the swapped Z roles of forest_runs together with the XY exchanges)

`coverage` recomputes what a (case, grid) pair exercises from the planner's exchange lists (sluamd_plan_xlists, read-only) and the exported structure
(the flat store of the symbolic factorisation, the partition into forests), never from the kernels."""
import functools
import numpy as np
import grid_trans_cases as gt
import panel_cases as pn
import pivot_cases as pc
import schur_cases as sc
import sweep_cases as sw
import trans_cases as tc
from superlu_dist_amd import driver, grid3d

SWEEP_CASES = ("widths", "narrow", "z_narrow")
PANEL_CASES = ("mixed_level", "z_chain")
CASES = SWEEP_CASES + PANEL_CASES
GRIDS = [(2, 1, 1), (1, 2, 1), (2, 2, 1), (3, 2, 1), (2, 2, 2)]
NRHS = (1, 5)                                      # RK = 1 kernels; RK = 4 with a remainder
NARROW = set()                                     # cases whose x had to be narrowed to {-1, 0, 1} to keep a transposed bound: none

XT_LISTS = ("xt_red_send", "xt_red_recv", "xt_bc_send", "xt_bc_recv")
TAG_L_ROWS = "L panel rows on two process rows"
TAG_U_COLS = "U columns on two process columns"
TAG_WIDE_PEER = "supernode wider than 64 columns with panel on a rank that does not own its diagonal block"
TAG_XY_AND_Z = "ancestor level with an XY exchange and a Z exchange"
TAGS = XT_LISTS + (TAG_L_ROWS, TAG_U_COLS, TAG_WIDE_PEER, TAG_XY_AND_Z)
# the (case, grid) pair each tag was chosen for (the CPU test names it when the tag is missing)
SUPPLIERS = {"xt_red_send": ("narrow", (2, 1, 1)), "xt_red_recv": ("narrow", (2, 1, 1)), "xt_bc_send": ("narrow", (1, 2, 1)), "xt_bc_recv": ("narrow", (1, 2, 1)),
             TAG_L_ROWS: ("widths", (2, 1, 1)), TAG_U_COLS: ("widths", (1, 2, 1)), TAG_WIDE_PEER: ("widths", (2, 2, 1)), TAG_XY_AND_Z: ("widths", (2, 2, 2))}


def is_z(name):
    return name.startswith("z_")


# (case, grid, nrhs): one right-hand side more than a chunk -- 48 under the 256-column supernode of "widths", 96 under the 64 complex16 columns of "z_narrow"
# (trans_cases.max_rhs_chunk of the widest supernode; asserted by the CPU tests and, from every rank's plan, by the GPU tests)
CHUNK_RUNS = [("widths", (2, 2, 1), 49), ("z_narrow", (2, 1, 1), 97)]


def runs():
    """every (case, nrhs, conj) the GPU tests ask of tc.rhs_t"""
    out = [(name, nrhs, conj) for name in CASES for nrhs in NRHS for conj in ((False, True) if is_z(name) else (False,))]
    for name, _, nrhs in CHUNK_RUNS:
        out += [(name, nrhs, conj) for conj in ((False, True) if is_z(name) else (False,))]
    return out


@functools.lru_cache(maxsize=None)
def prepared(name):
    """(filled case, flat store of the structure, sources): built once, host code only"""
    if name in SWEEP_CASES:
        c, fs = tc.prepared(name)[:2]
    else:
        c = pn.CASES[name]()
        n, rp, ci = c.pattern_csr()
        symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
        assert symb.xsup().tolist() == c.xsup.tolist()
        fs = symb.flat_store(values=False)
        symb.free()
        c.fill(fs)                                 # (asserts panel_bounds)
    assert c.z == is_z(name)
    return c, fs, sc.sources(fs)


@functools.lru_cache(maxsize=None)
def csr(name):
    """(n, rowptr, colind, values) a grid handle of the case is created from: B on the designed pattern (sweep cases, as test_gpu_sweep_shapes.py) or on
    the stored pattern, closed under fill (panel cases, as test_gpu_panel_forms.py: the symbolic factorisation lowers leads and B holds values there)"""
    c, fs, _ = prepared(name)
    if name in SWEEP_CASES:
        n, rp, ci = c.pattern_csr()
    else:
        (lr, lc), (ur, uc) = pc.store_positions(fs)
        mask = np.zeros((c.n, c.n), dtype=bool)
        mask[lr[lr >= 0], lc[lr >= 0]] = True
        mask[ur[ur >= 0], uc[ur >= 0]] = True
        n, ci = c.n, np.nonzero(mask)[1].astype(np.int32)
        rp = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    v = c.B[np.repeat(np.arange(n), np.diff(rp)), ci].copy()
    assert np.count_nonzero(v) == np.count_nonzero(c.B)                                     # the pattern holds all of B
    for a in (rp, ci, v):
        a.setflags(write=False)
    return n, rp, ci, v


@functools.lru_cache(maxsize=None)
def rhs_t(name, nrhs, conj=False):
    """(x, b_t) of tc.rhs_t (its bounds asserted there), read-only"""
    x, b = tc.rhs_t(prepared(name)[0], nrhs, conj, narrow=name in NARROW)
    x.setflags(write=False); b.setflags(write=False)
    return x, b


def _symbolic(name):
    c = prepared(name)[0]
    n, rp, ci, _ = csr(name)
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    assert np.array_equal(symb.perm_c, np.arange(n)) and symb.xsup().tolist() == c.xsup.tolist()
    return symb


def solve_exact(name, grid, requests):
    """Handles of case `name` on every rank of `grid` (threads over grid3d.local_comms) from the case's CSR values; on every rank pdgstrf3d(0.0), the
    untransposed solve of case.rhs(5), plan_transposed(), then the requests in order: (trans, b) -> h.pdgstrs3d(b, trans=trans), or a callable f(h, rank).
    Returns per rank (info, untransposed solution, widest supernode of the rank's plan, [results]); the caller asserts info == 0 and that the
    untransposed solution is the integer x BEFORE anything is asked of the transposed results."""
    c = prepared(name)[0]
    v = csr(name)[3]
    Pr, Pc, Pz = grid
    symb = _symbolic(name)
    tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)
    b5 = c.rhs(5)[1]

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], tree)
        try:
            info = h.pdgstrf3d(0.0)
            y = h.pdgstrs3d(b5.copy(order="F"))
            h.plan_transposed()
            res = [r(h, rank) if callable(r) else h.pdgstrs3d(r[1].copy(order="F"), trans=r[0]) for r in requests]
            return info, y, int(h.plan_table()[:, 3].max()), res
        finally:
            h.destroy()

    try:
        return gt.run_ranks(Pr * Pc * Pz, body)
    finally:
        symb.free()


def plans(name, grid):
    """per rank {list name: rows (Z level, DAG level, peer, first row, rows)} of the four transposed exchange lists, and the forest of every supernode"""
    v = csr(name)[3]
    Pr, Pc, Pz = grid
    symb = _symbolic(name)
    tree = symb.partition(Pz) if Pz > 1 else np.zeros(symb.nsupers, dtype=np.int32)
    comms = grid3d.local_comms(Pr, Pc, Pz)

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], tree if Pz > 1 else None)
        try:
            h.plan_transposed()
            return {w: h.plan_xlists(w).copy() for w in XT_LISTS}
        finally:
            h.destroy()

    try:
        return gt.run_ranks(Pr * Pc * Pz, body), tree
    finally:
        symb.free()


def coverage(name, grid, planned=None):
    """the set of TAGS the pair exercises"""
    c, fs, srcs = prepared(name)
    Pr, Pc, Pz = grid
    per_rank, tree = planned or plans(name, grid)
    vs = 2 if c.z else 1                                                                     # the lists count doubles: complex16 rows count twice
    sn_of_row = np.repeat(np.arange(len(c.widths)), np.diff(c.xsup))
    out = set()
    for w in XT_LISTS:
        if any(len(p[w]) for p in per_rank):
            out.add(w)
    for s in srcs:
        k, w = s["k"], s["w"]
        lrows = {g % Pr for g, _ in s["lblocks"]}
        ucols = {g % Pc for g, _ in s["ublocks"]}
        if len(lrows) >= 2:
            out.add(TAG_L_ROWS)
        if len(ucols) >= 2:
            out.add(TAG_U_COLS)
        if w > 64 and (lrows - {k % Pr} or ucols - {k % Pc}):
            out.add(TAG_WIDE_PEER)
    if Pz > 1:
        anc = np.flatnonzero(tree < Pz - 1)                                                 # heap order: the leaves are the forests Pz - 1 .. 2 Pz - 2
        for rank, p in enumerate(per_rank):
            r, cc, _ = grid3d.grid_coords(rank, Pr, Pc, Pz)
            zrows = {int(k) for k in anc if k % Pc == cc or k % Pr == r}                     # partial sums go up from the process column, solved rows come down the process row
            for w in XT_LISTS:
                for zl, l, peer, r0, nr in p[w].tolist():
                    if zl >= 1 and zrows & set(sn_of_row[r0 // vs:(r0 + nr) // vs].tolist()):
                        out.add(TAG_XY_AND_Z)
    return out
