"""Matrices whose factors, diagonal inverses and solution are known EXACTLY and whose whole difficulty sits in the panel chain of the factorisation --
diagonal LU -> Linv / Uinv -> L and U panel solves -- over the forms it takes at run time (test helper for test_gpu_panel_forms.py and
test_panel_cases_cpu.py; not a conftest).

Construction: sweep_cases.SweepCase -- B = L0 U0 from small integers and dyadic fractions, diagonal blocks with DENSE exactly known inverses, dense
off-diagonal panels -- so an indexing error in a strip, a chunk or a block of an inverse multiplies non-zeros.  What this module adds:

  * `panel_bounds`: both forms of the panel solves must be exact, so both are bounded entry by entry (sparse products of the absolute values of the
    scaled INTEGER images, maxima compared as Python integers; the coarse row-sum bounds of SweepCase.fill certify that no int64 product wrapped):
      product form (k_panel_gemm):      |B_below| |Uinv_kk|  and  |Linv_kk| |B_right|  -- every partial sum of a row of the panel with a column of the inverse;
      blocked substitution on the 32 x 32 inverses (k_panel_trsm): with L0_panel and U0_row exact by induction over the 32-column blocks, the right-hand
        side of block j is B_j - sum_{i < j} X_i U0_kk[i, j], bounded by |B| + |L0_panel| |U0_kk outside the 32 x 32 diagonal sub-blocks|, and the
        result is that times the 32 x 32 inverse -- which IS the diagonal sub-block of Uinv_kk (triangular); likewise for the U rows with L0_kk, Linv_kk;
      complex16 (kz_panel_trsm[_quad] substitute on the factored block, column by column): |B| + |L0_panel| |strict upper part of U0_kk| and the mirror
        image; the division by the pivot (a unit of the Gaussian integers times 2^e) is exact.
    In units of the last place (1 / 64 and 1 / 256 for the double cases, 1 / 16 for complex16) every bound stays below 2^53 / 64: the factor-64 margin of
    the sweep cases.

  * the decision rules of the chain restated from level sizes, widths and position (`predicted_lines`; sluamd_factor.cpp: run_factor_sched, the launch
    wrappers of sluamd_kernels.hip, sluamd_plan.cpp: build_schedule and build_panel_split with the tile rules it reads), never from the kernels: the
    tests compare the restatement with the `[sluamd panel]` lines of SLUAMD_FACTOR_DEBUG, so a change of a rule shows up as a failed test, not as a
    case that silently runs another form.

The sign of a stored zero: the rule of schur_cases.py (IEEE equality: numpy.array_equal)."""
import numpy as np
import scipy.sparse as sp
import schur_cases as sc
import sweep_cases as sw

LIMIT = 2 ** 53
MARGIN = 64


class PanelCase(sw.SweepCase):
    def fill(self, fs, pos=None):
        out = super().fill(fs, pos)
        self.bounds = panel_bounds(self)
        return out


def _blockdiag_mask(xsup, sub=None):
    """boolean CSR mask of the diagonal blocks of the supernodes (sub: of their sub x sub diagonal sub-blocks, aligned at each supernode's first column)"""
    blocks = []
    for a, e in zip(xsup[:-1], xsup[1:]):
        w = int(e - a)
        if sub is None:
            blocks.append(np.ones((w, w), dtype=np.int64))
        else:
            i = np.arange(w) // sub
            blocks.append((i[:, None] == i[None, :]).astype(np.int64))
    return sp.block_diag(blocks, format="csr")


def panel_bounds(c):
    """the bounds of the module docstring for a filled case: dict(name -> Python integer, in units of the last place); asserts each one times MARGIN below 2^53"""
    n = c.n
    blk = _blockdiag_mask(c.xsup)
    aL, aU, aLi, aUi, aB = c.aL, c.aU, c.aLi, c.aUi, sw._absint(c.B16)
    for prod in ((aB, aUi), (aLi, aB), (aL, aU, aUi), (aLi, aL, aU)):                       # no int64 product below can wrap: the coarse bounds are Python integers
        assert sw._prod_bound(*prod) * n < 2 ** 62
    lowmask = sp.tril(sp.csr_matrix(np.ones((n, n), dtype=np.int64)), -1, format="csr")
    offd = sp.csr_matrix(np.ones((n, n), dtype=np.int64)) - blk                             # outside the diagonal blocks
    below, right = offd.multiply(lowmask).tocsr(), offd.multiply(lowmask.T).tocsr()
    aB_below, aB_right = aB.multiply(below).tocsr(), aB.multiply(right).tocsr()
    aL_below, aU_right = aL.multiply(below).tocsr(), aU.multiply(right).tocsr()
    out = {}
    mx = lambda M: int(M.max()) if M.nnz else 0
    if c.z:     # substitution on the factored block, column by column (row by row for U): the right-hand sides; the pivot division is exact
        aUkk = sp.triu(aU.multiply(blk), 1, format="csr")
        aLkk = sp.tril(aL.multiply(blk), -1, format="csr")
        out["z: |B| + |L0 panel| |U0_kk strict|"] = mx(aB_below + aL_below @ aUkk)
        out["z: |B| + |L0_kk strict| |U0 row|"] = mx(aB_right + aLkk @ aU_right)
    else:
        blk32 = _blockdiag_mask(c.xsup, 32)
        out["gemm: |B_below| |Uinv|"] = mx(aB_below @ aUi)                                  # units 1/16 * 1/16
        out["gemm: |Linv| |B_right|"] = mx(aLi @ aB_right)                                  # units 1/4 * 1/16
        aUkk = (aU.multiply(blk) - aU.multiply(blk32)).tocsr()
        aLkk = (aL.multiply(blk) - aL.multiply(blk32)).tocsr()
        out["trsm: (|B| + |L0 panel| |U0_kk|) |Uinv32|"] = mx((aB_below + aL_below @ aUkk) @ aUi.multiply(blk32).tocsr())
        out["trsm: |Linv32| (|B| + |L0_kk| |U0 row|)"] = mx(aLi.multiply(blk32).tocsr() @ (aB_right + aLkk @ aU_right))
    for k, v in out.items():
        assert isinstance(v, int) and v * MARGIN < LIMIT, (c.name, k, v)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# The cases.  The rules of the symbolic factorisation they rely on are those of schur_cases.py (no panel holds row 0 of a later supernode, a guard's
# single row excepted; a source that carries skyline leads is not a leaf).  Two further rules of this module's designs:
#   * a supernode that holds L rows in t and U columns in a later u makes t hold U columns in u (fill), and the mirror image: two supernodes meant to
#     share a DAG level never have a common predecessor;
#   * the rows (columns) a supernode holds in a far ancestor are held by every supernode between them that it reaches: the designs nest them.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _leads(i, w):
    """ragged skyline leads with an EMPTY column between segments: column offset -> lead, for the first w columns of a destination (offset 0 is never held)"""
    return {c: [0, 3, 1, 17, 2, 33, 0, 5][(c + i) % 8] for c in range(1, w + 2) if c != 1 + w // 2}


def _link(L, U, s, t, rows, cols, ws):
    L.setdefault(s, {})[t] = list(rows)
    U.setdefault(s, {})[t] = {c: min(ld, ws - 1) for c, ld in cols.items()}


def chain_wide():
    """two guarded leaves (5 and 17 columns) under a chain of single-supernode levels of 33, 65, 129, 200, 256 and 256 columns.  Every chain member holds
    rows and columns of the next one only: L panels of 1, 63, 64, 65 and 130 rows below the diagonal block (partial, full and one-past-full 64-row strips,
    three strips), U rows of 1, 63, 64, 65 and 130 non-empty columns with an empty column between the segments (the designed ragged leads survive the symbolic
    factorisation on the guarded leaves only: it stores the U row of a supernode behind a wide predecessor at full height; `rs32` and `split` carry them on single-supernode levels).  Levels: guards, leaves,
    then one level per chain member -- with SLUAMD_TRSM_TAIL / SLUAMD_DIAG_TAIL = 2 the two 256-column levels are tail levels and the four below are not."""
    w = [1, 5, 1, 17, 33, 65, 129, 200, 256, 256]
    L, U = {}, {}
    for g, k in ((0, 1), (2, 3)):
        L[g], U[g] = {k: [0]}, {k: {0: 0}}
        _link(L, U, k, 4, range(1, 33, 1 + g // 2), {c: (c + g) % 3 for c in range(1, 33) if c != 9}, w[k])
    counts = [1, 63, 64, 65, 130]
    for i, cnt in enumerate(counts):
        s, t = 4 + i, 5 + i
        cols = _leads(i, cnt)
        assert len(cols) == cnt and max(cols) < w[t] and cnt < w[t]
        _link(L, U, s, t, range(1, 1 + cnt), cols, w[s])
    return PanelCase("chain_wide", "single-supernode levels of every width class, tail and non-tail", w, L, U, guards=[0, 2])


def tail_boundary():
    """a chain of 73 single-supernode levels of 1 .. 8 columns (n = 326): at the defaults the rule l >= nlevels - 64 is crossed inside the case, levels
    0 .. 8 take the product form with the inverses on the chain, levels 9 .. 72 the substitution with the inverses deferred.  A one-column member can
    only be reached through its row 0: its predecessor is a guard in the sense of schur_cases.py (the structures differ in size, they do not merge)."""
    cyc = [2, 3, 4, 5, 6, 7, 8, 1]
    w = cyc * 9 + [2]                                        # (a last member of one column would nest into its predecessor)
    L, U, guards = {}, {}, []
    for s in range(len(w) - 1):
        t, wt = s + 1, w[s + 1]
        if wt == 1:
            guards.append(s)
            _link(L, U, s, t, [0], {0: 0}, w[s])
        else:
            _link(L, U, s, t, range(1, wt, 1 + s % 2), {c: (c + s) % 3 for c in range(1, wt)}, w[s])
    return PanelCase("tail_boundary", "the tail rule crossed at the defaults", w, L, U, guards=guards)


def mixed_level():
    """four levels that each hold a 3-column, a 17-column and a wide supernode -- 64, 128, 200, 256 columns: one level per class of the widest supernode
    (<= 64, <= 128, > 128 twice) -- under a 70-column top.  The narrow ones go through the kernels chosen for the wide one.  Each kind is fed by its own
    kind one level down (no common predecessors: the three stay on one level): the 3-column ones have a panel of 1 row, the 17-column ones of 65 rows
    (16 in their successor, 49 in the top; the last one 65 in the top), the wide ones of 127, 100, 130 and 65 rows."""
    wide = [64, 128, 200, 256]
    w, L, U = [3] * 4 + [17] * 4 + wide + [70], {}, {}      # (numbered chain by chain: the postorder of the elimination tree)
    top = 12
    for x in range(4):
        a, b, c = x, 4 + x, 8 + x
        if x < 3:
            _link(L, U, a, a + 1, [1], {2: 1}, 3)
            _link(L, U, b, b + 1, range(1, 17), {cc: cc % 5 for cc in range(1, 17)}, 17)
            L[b][top] = list(range(1, 50)); U[b][top] = {cc: (cc * 3) % 17 for cc in range(1, 50)}
            nr = [127, 100, 130][x]
            st = 2 if x == 1 else 1
            _link(L, U, c, c + 1, range(1, 1 + st * nr, st), _leads(x, 65 + 30 * x), wide[x])
        else:
            _link(L, U, a, top, [1], {2: 1}, 3)
            _link(L, U, b, top, range(1, 66), {cc: (cc * 3) % 17 for cc in range(1, 66)}, 17)
            _link(L, U, c, top, range(1, 66), _leads(3, 65), wide[x])
    return PanelCase("mixed_level", "narrow supernodes on levels of wide ones", w, L, U)


def rs32():
    """a guarded chain of 129, 160, 200 and 256 columns under a 129-column top, each holding 31, 32, 33 and 97 rows (and as many columns) of the next:
    all single-supernode tail levels wider than 128 columns -- the 32-row strips of SLUAMD_TRSM_RS32 (k_panel_trsm<32>): one short strip, one full strip, one
    row into the second strip, one row into the fourth."""
    w = [1, 129, 160, 200, 256, 129]
    L, U = {0: {1: [0]}}, {0: {1: {0: 0}}}
    for i, cnt in enumerate([31, 32, 33, 97]):
        _link(L, U, 1 + i, 2 + i, range(1, 1 + cnt), _leads(i + 1, cnt), w[1 + i])
    return PanelCase("rs32", "32-row strips", w, L, U, guards=[0])


def split():
    """a guarded chain a, b, c (48 columns), d, e (130) under a 200-column top: the levels build_panel_split looks at.
      a: rows and columns of b only -- every unit urgent: refused
      b: rows of c and of the top, columns of the top only -- no tile lands on c's diagonal block, nothing is urgent: refused
      c: 40 rows of d and 70 of the top (64 x 64 tiles; the merged row tile 0 .. 63 runs across the block boundary inside strip 0): strip 0 and chunk 0
         urgent, strip 1 and chunk 1 not
      d: 60 rows of e and 196 of the top, 128 columns of each (128 x 128 tiles: the merged row tile 0 .. 127 starts in e's block, so strip 1 -- rows of the
         top alone -- is urgent too): strips 0, 1 and chunks 0, 1 urgent, strips 2, 3 and chunks 2, 3 not
      e: the last level but one, rows and columns of the top only: refused"""
    w = [1, 48, 48, 48, 130, 130, 200]
    g, a, b, c, d, e, top = range(7)
    L, U = {g: {a: [0]}}, {g: {a: {0: 0}}}
    _link(L, U, a, b, range(1, 41), {cc: cc % 4 for cc in range(1, 41)}, 48)
    L[b] = {c: list(range(1, 31)), top: list(range(1, 51))}
    U[b] = {top: {cc: cc % 3 for cc in range(1, 51)}}
    L[c] = {d: list(range(1, 41)), top: list(range(1, 71))}
    U[c] = {d: {cc: cc % 5 for cc in range(1, 41)}, top: {cc: (2 * cc) % 7 for cc in range(1, 71)}}
    L[d] = {e: list(range(1, 61)), top: list(range(1, 197))}
    U[d] = {e: {cc: cc % 4 for cc in range(1, 129)}, top: {cc: (3 * cc) % 33 for cc in range(1, 129)}}
    L[e] = {top: list(range(1, 200))}
    U[e] = {top: {cc: cc % 2 for cc in range(1, 200)}}
    return PanelCase("split", "split panel solves: urgent and other units, the refusals, merged row tiles", w, L, U, guards=[g])


Z_WIDTHS = [3, 8, 9, 16, 17, 32, 33, 64, 65, 200, 256]


def z_chain():
    """complex16: a chain of 3, 8, 9, 16, 17, 32, 33, 64, 65, 200 and 256 columns (every class of zdiag_lu and zpanel_trsm, both sides of each boundary)
    beside a chain of narrow supernodes of its own (no common predecessors): every level holds one member of each, the narrow one 3 columns wide -- 17 on
    the level of the 200-column member -- so that a 3-column block shares a level with the 65- and 256-column ones and a 17-column block with the 200-column one."""
    side = [2, 3, 3, 3, 3, 3, 3, 3, 3, 17, 3]
    w, L, U = Z_WIDTHS + side, {}, {}                        # (numbered chain by chain: the postorder of the elimination forest)
    for i in range(10):
        s, t = i, i + 1
        wt = w[t]
        cnt = min(wt - 1, [2, 7, 8, 15, 16, 31, 32, 64, 65, 130][i])
        _link(L, U, s, t, range(1, 1 + cnt), {c: ld for c, ld in _leads(i, cnt).items() if c < wt}, w[s])
        s, t = 11 + i, 12 + i
        _link(L, U, s, t, range(1, w[t]), {c: c % 2 for c in range(1, w[t])}, w[s])
    return PanelCase("z_chain", "complex16: every width class; narrow blocks on wide levels", w, L, U, complex16=True)


CASES = {"chain_wide": chain_wide, "tail_boundary": tail_boundary, "mixed_level": mixed_level, "rs32": rs32, "split": split, "z_chain": z_chain}


# ---------------------------------------------------------------------------------------------------------------------------------------
# The decision rules of the panel chain, restated (1 x 1 x 1 handles)
# ---------------------------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(trsm_tail=64, diag_tail=64, rs32=False, trsm_panels=False, no_full_inv64=False, panel_split=1024, no_lookahead=False, deterministic=False,
                diag_v1=False, zlu4=0, no_quad=False)
# the variants of the tests: name -> (environment of the switch, settings it changes); "deterministic" is an option of the handle, not a variable
VARIANTS = {
    "default": ({}, {}),
    "trsm_tail0": ({"SLUAMD_TRSM_TAIL": "0"}, {"trsm_tail": 0}),
    "trsm_tail2": ({"SLUAMD_TRSM_TAIL": "2"}, {"trsm_tail": 2}),
    "diag_tail0": ({"SLUAMD_DIAG_TAIL": "0"}, {"diag_tail": 0}),
    "diag_tail2": ({"SLUAMD_DIAG_TAIL": "2"}, {"diag_tail": 2}),
    "rs32": ({"SLUAMD_TRSM_RS32": "1"}, {"rs32": True}),
    "trsm_panels": ({"SLUAMD_TRSM_PANELS": "1"}, {"trsm_panels": True}),
    "trsm_panels_rs32": ({"SLUAMD_TRSM_PANELS": "1", "SLUAMD_TRSM_RS32": "1"}, {"trsm_panels": True, "rs32": True}),      # 32-row strips on levels of several supernodes
    "panel_split0": ({"SLUAMD_PANEL_SPLIT": "0"}, {"panel_split": 0}),
    "no_lookahead": ({"SLUAMD_NO_LOOKAHEAD": "1"}, {"no_lookahead": True}),
    "deterministic": ({}, {"deterministic": True}),
    "diag_v1": ({"SLUAMD_DIAG_V1": "1"}, {"diag_v1": True}),
    # read when the library is loaded: a process of its own each
    "no_full_inv64": ({"SLUAMD_NO_FULL_INV64": "1"}, {"no_full_inv64": True}),
    "zlu4": ({"SLUAMD_ZLU4_MAX_NODES": str(2 ** 30)}, {"zlu4": 2 ** 30}),
    "no_ztrsm_quad": ({"SLUAMD_NO_ZTRSM_QUAD": "1"}, {"no_quad": True}),
}
PER_HANDLE = ["default", "trsm_tail0", "trsm_tail2", "diag_tail0", "diag_tail2", "rs32", "trsm_panels", "trsm_panels_rs32", "panel_split0", "no_lookahead", "deterministic", "diag_v1"]
AT_LOAD = ["no_full_inv64", "zlu4", "no_ztrsm_quad"]


def settings(variant):
    return dict(DEFAULTS, **VARIANTS[variant][1])


def _ceil(a, b):
    return -(-a // b)


def level_table(srcs, lev):
    """per DAG level: (supernodes, widest supernode, [sources of the level in schedule order])"""
    nl = max(lev) + 1
    per = [[s for s in srcs if lev[s["k"]] == l] for l in range(nl)]
    return [(len(p), max(s["w"] for s in p), p) for p in per]


def rows_below(s):
    return sum(len(r) for _, r in s["lblocks"])


def ucols(s):
    return sum(len(c) for _, c in s["ublocks"])


def urgent_units(s, lev, z=False):
    """build_panel_split for one supernode: (urgent 64-row strips, urgent 64-column chunks) as sets -- the units that the tiles landing on the DIAGONAL block
    of a supernode of the next level read.  Tiles: 128 x 128 for a big source, else 64 x 64; the row tiles of a U block are the merged ones (all rows from the
    first block at or behind the U block's supernode on, cut every tile height, each tile named after the block of its first row) when that saves a tile."""
    l = lev[s["k"]]
    tm = 128 if sc.source_is_big(s, z) else 64
    offs, o = [], 0
    for _, r in s["lblocks"]:
        offs.append(o); o += len(r)
    total = o
    gids = [g for g, _ in s["lblocks"]]
    assert gids == sorted(gids)
    lurg, uurg, coff = set(), set(), 0
    for jb, cols in s["ublocks"]:
        nc = len(cols)
        if lev[jb] == l + 1:
            later = [b for b, g in enumerate(gids) if g >= jb]
            tiles = []
            if len(later) >= 2:
                regular = sum(_ceil(len(s["lblocks"][b][1]), tm) for b in later)
                row0 = offs[later[0]]
                if _ceil(total - row0, tm) < regular:
                    for r0 in range(row0, total, tm):
                        b = max(b for b in later if offs[b] <= r0)
                        tiles.append((r0, min(tm, total - r0), gids[b]))
            if not tiles:
                tiles = [(offs[b] + r0, min(tm, len(s["lblocks"][b][1]) - r0), gids[b]) for b in later for r0 in range(0, len(s["lblocks"][b][1]), tm)]
            diag = [(r0, nr) for r0, nr, g in tiles if g == jb]
            for r0, nr in diag:
                lurg |= set(range(r0 // 64, (r0 + nr - 1) // 64 + 1))
            if diag:
                uurg |= set(range(coff // 64, (coff + nc - 1) // 64 + 1))
        coff += nc
    return lurg, uurg


def split_parts(level, lev, cfg, l, nlevels):
    """[(part, nl, nu)] of a split level, or None: the rules of build_panel_split and level_split"""
    nn, mx, per = level
    lookahead = not (cfg["no_lookahead"] or cfg["deterministic"])
    if not lookahead or cfg["panel_split"] <= 0 or cfg["trsm_panels"] or l == 0 or l + 1 == nlevels or nn > cfg["panel_split"]:
        return None
    if cfg["rs32"] and ((mx + 31) & ~31) > 128:
        return None
    nl = [0, 0]; nu = [0, 0]
    for s in per:
        lu, uu = urgent_units(s, lev)
        ns_, nc_ = _ceil(rows_below(s), 64), _ceil(ucols(s), 64)
        nl[0] += len(lu); nl[1] += ns_ - len(lu); nu[0] += len(uu); nu[1] += nc_ - len(uu)
    if nl[0] + nu[0] == 0 or nl[1] + nu[1] == 0:
        return None
    return [(p, nl[p], nu[p]) for p in (0, 1)]


def predicted_lines(srcs, lev, z, cfg):
    """the `[sluamd panel]` lines of one factorisation on a 1 x 1 x 1 handle, as a sorted list of (family, form, level, nn, mx, nl, nu, part, where)"""
    tab = level_table(srcs, lev)
    nlv = len(tab)
    out = []
    for l, (nn, mx, per) in enumerate(tab):
        if z:
            form = ("zwave_small8" if mx <= 8 else "zwave_small16" if mx <= 16 else "zwave_small32" if mx <= 32 else
                    "zwave4" if mx <= 64 and nn <= cfg["zlu4"] else "zwave" if mx <= 64 else "zlu")
            out.append(("diag_lu", form, l, nn, mx, 0, 0, "whole", "chain"))
            nl, nu = sum(_ceil(rows_below(s), 64) for s in per), sum(_ceil(ucols(s), 64) for s in per)
            form = "ztrsm" if cfg["no_quad"] or mx > 64 else "zquad4" if mx <= 16 else "zquad8" if mx <= 32 else "zquad16"
            if nl + nu:
                out.append(("panel", form, l, nn, mx, nl, nu, "whole", "chain"))
            continue
        gemm = not cfg["trsm_panels"]
        tail = gemm and cfg["trsm_tail"] > 0 and l >= nlv - cfg["trsm_tail"] and nn == 1
        if not cfg["diag_v1"] and mx > 64:
            form = "lu2_1" if cfg["diag_tail"] > 0 and nn == 1 and l >= nlv - cfg["diag_tail"] else "lu2_2"
        else:
            form = "wave" if mx <= 64 else "v1_128" if mx <= 128 else "v1_256"
        out.append(("diag_lu", form, l, nn, mx, 0, 0, "whole", "chain"))
        if gemm:
            out.append(("full_inv", "inv64" if mx <= 64 and not cfg["no_full_inv64"] else "inv", l, nn, mx, 0, 0, "whole", "bulk" if tail else "chain"))
        pform = ("gemm16" if mx <= 64 else "gemm32" if mx <= 128 else "gemm64") if gemm and not tail else None
        parts = split_parts((nn, mx, per), lev, cfg, l, nlv)
        if parts:
            for p, nl, nu in parts:
                if nl + nu:
                    out.append(("panel", pform or "trsm64", l, nn, mx, nl, nu, str(p), "chain"))
            continue
        rs = 32 if cfg["rs32"] and ((mx + 31) & ~31) > 128 else 64
        nl, nu = sum(_ceil(rows_below(s), rs) for s in per), sum(_ceil(ucols(s), rs) for s in per)
        if nl + nu:
            out.append(("panel", pform or ("trsm32" if rs == 32 else "trsm64"), l, nn, mx, nl, nu, "whole", "chain"))
    return sorted(out)


def predicted_grid_forms(srcs, lev, cfg=DEFAULTS):
    """double cases on a 2 x 1 x 1 grid (an XY layer): what EVERY rank launches per level, as a sorted list of (family, form, level, nn, part, where).  One
    process column: every rank holds the L slot of every supernode, so it has (owns or receives) every diagonal block -- after the exchange it inverts the
    32 x 32 sub-blocks of the copies (family diag_inv) and builds Linv / Uinv of all of them on the chain; there are no tail levels on an XY layer
    (run_factor_sched: trsm_tail = 0), so every panel solve is the product form, whole; SLUAMD_DIAG_TAIL still chooses the diagonal LU build."""
    out = []
    tab = level_table(srcs, lev)
    for l, (nn, mx, per) in enumerate(tab):
        form = ("lu2_1" if cfg["diag_tail"] > 0 and nn == 1 and l >= len(tab) - cfg["diag_tail"] else "lu2_2") if mx > 64 else "wave"
        out += [("diag_lu", form, l, nn, "whole", "chain"), ("diag_inv", "inv", l, nn, "whole", "chain"),
                ("full_inv", "inv64" if mx <= 64 else "inv", l, nn, "whole", "chain")]
        if any(rows_below(s) + ucols(s) for s in per):
            out.append(("panel", "gemm16" if mx <= 64 else "gemm32" if mx <= 128 else "gemm64", l, nn, "whole", "chain"))
    return sorted(out)


def parse_lines(text):
    """the `[sluamd panel]` lines of a stderr text as the tuples of predicted_lines (unsorted, in order)"""
    out = []
    for ln in text.splitlines():
        if ln.startswith("[sluamd panel] "):
            f = dict(tok.split("=") for tok in ln.split()[2:])
            out.append((f["family"], f["form"], int(f["level"]), int(f["nn"]), int(f["mx"]), int(f["nl"]), int(f["nu"]), f["part"], f["where"]))
    return out


def tags(lines, srcs, lev):
    """coverage tags of a set of lines: (family, form, part, single / multi, narrow-in-wide) -- the last from the structure: the level holds a supernode of at
    most 17 columns while its widest has more than 64"""
    tab = level_table(srcs, lev)
    out = set()
    for fam, form, l, nn, mx, nl, nu, part, where in lines:
        narrow = mx > 64 and min(s["w"] for s in tab[l][2]) <= 17
        out.add((fam, form, part, "single" if nn == 1 else "multi", "narrow-in-wide" if narrow else "plain"))
    return out
