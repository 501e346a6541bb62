"""Matrices whose factors, diagonal inverses and solution are known EXACTLY and whose whole difficulty sits in the triangular sweeps (test
helper for test_gpu_sweep_shapes.py; not a conftest).

Construction.  The block patterns, the guards, the symbolic path and the off-diagonal values are those of schur_cases.py (`Case`, `val`, `zval`);
the one change is the diagonal block.  With L0_kk = I and U0_kk diagonal (schur_cases) every off-diagonal element of Linv / Uinv is zero and an
indexing error in the diagonal strips of the sweeps multiplies zeros.  Here, with d = +-2^e (e in {0, 1, 2} on period 3, signs on period 8), d' a
second such vector (other periods), p the pivots of schur_cases (+-2^e), S the sub-diagonal shift, all indexed by the GLOBAL row:
  double:     L0_kk = D (I - S) D^-1                        ->  Linv_kk[i, j] = d_i / d_j            for all i >= j  (dense, in +-{1/4 .. 4})
              U0_kk = diag(p) (D' (I - S) D'^-1)^T          ->  Uinv_kk[i, j] = d'_j / (d'_i p_j)    for all i <= j  (dense, in +-{1/16 .. 4})
              neighbouring entries of a row or column of an inverse differ (consecutive d differ), so a misplaced element is another number.
  complex16:  the roles are swapped (the complex path keeps no inverses and substitutes on the factored block): L0_kk = D tril(1) D^-1 and
              U0_kk = diag(p) (D' tril(1) D'^-1)^T are the DENSE ones, their inverses the bidiagonal ones; d, d', p carry units of the Gaussian integers.
Every value is an integer multiple of 2^-2 (L0, U0, Linv), 2^-4 (Uinv, B = L0 U0, b) -- the cases keep scaled INTEGER images (L0 * 4, U0 * 4, ...)
and form B, y = U0 x and b = B x from them in integer arithmetic.  Bounds (`fill`, `rhs`): with every operand scaled to integers,
sum |L0| |U0|, |B| |Uinv|, |Linv| |B|, |Linv| |L0| |Linv|, |Uinv| |U0| |Uinv| (factorisation, panel solves, inverse kernels) and
|Linv| (|b| + |L0| |y|), |Uinv| (|y| + |U0| |x|) (sweeps) stay below 2^53, all bounded through max row sum x max entry; products of operands whose
units are 2^-2 / 2^-4 have a unit of at most 2^-12, so every partial sum of any summation order is an exact double.  The block-triangle inverses of a
merged chain group (SLUAMD_SOLVE_GROUPS) are bounded by running their recurrence X = |inv| + |inv| |off-diagonal blocks| X on the absolute values in
Python integers, scale included.

Sign of a stored zero: the rule of schur_cases.py (IEEE equality: numpy.array_equal).

The schedule rules the designs rely on are restated here (`levels_of`, `joined`, `predicted_launches`, `near_columns`, `forward_sources`); the tests
assert the restatements against plan_table() and stats()["solve_launches"], so a schedule change shows up as a failed coverage test."""
import numpy as np
import scipy.sparse as sp
import pivot_cases as pc
import schur_cases as sc

LIMIT = 2 ** 53
WIDTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 255, 256]


def dvec(k, z=False):
    """d: the scaling of L's diagonal blocks"""
    d = ((1 << (k % 3)) * np.where((k // 4) % 2 == 0, 1, -1)).astype(np.complex128 if z else np.int64)
    return d * np.array([1, 1j, -1, -1j])[(k // 5) % 4] if z else d


def dvec2(k, z=False):
    """d': the scaling of U's diagonal blocks"""
    d = ((1 << ((2 * k + 1) % 3)) * np.where((k // 5) % 2 == 0, 1, -1)).astype(np.complex128 if z else np.int64)
    return d * np.array([1, -1j, -1, 1j])[(k // 7) % 4] if z else d


def pvec(k, z=False):
    """p: U's diagonal (the pivots), as in schur_cases"""
    d = ((1 << (k % 3)) * np.where((k // 3) % 2 == 0, 1, -1)).astype(np.complex128 if z else np.int64)
    return d * np.array([1, 1j, -1, -1j])[(k // 6) % 4] if z else d


def _absint(M):
    """|M| of a scaled-integer sparse matrix as int64 (|re| + |im| for Gaussian integers: bounds both parts of every partial sum)"""
    M = M.tocsr()
    if np.iscomplexobj(M.data):
        assert np.all(M.data.real == np.rint(M.data.real)) and np.all(M.data.imag == np.rint(M.data.imag))
        d = np.abs(M.data.real).astype(np.int64) + np.abs(M.data.imag).astype(np.int64)
    else:
        assert np.all(M.data == np.rint(M.data))
        d = np.abs(M.data).astype(np.int64)
    return sp.csr_matrix((d, M.indices.copy(), M.indptr.copy()), shape=M.shape)                # copies: sorting |M| in place must not permute M's own index array under its data


def _rowsum_max(A):
    return int(np.asarray(A.sum(axis=1)).max()) if A.nnz else 0


def _prod_bound(*mats):
    """an upper bound, in Python integers, of every entry of |M1| |M2| ... (operands scaled to integers): max row sum of each factor but the last,
    times the largest entry of the last"""
    b = int(mats[-1].max()) if mats[-1].nnz else 0
    for M in mats[:-1]:
        b *= _rowsum_max(M)
    return b


class SweepCase(sc.Case):
    group = None                                    # (first supernode, members) of the merged chain group of the case, if it has one

    def fill(self, fs, pos=None):
        """as schur_cases.Case.fill, with the diagonal blocks of the module docstring: returns (expL, expU); sets L0, U0, B (dense, exact), Linv / Uinv
        (double cases: dense n x n block diagonals) and the scaled images the right-hand sides are built from"""
        (lr, lc), (ur, uc) = pos or pc.store_positions(fs)
        assert fs.xsup.tolist() == self.xsup.tolist(), fs.xsup.tolist()
        n, z = self.n, self.z
        f = sc.zval if z else sc.val
        dt = np.complex128 if z else np.int64
        k = np.arange(n)
        sn = np.searchsorted(self.xsup, k, side="right") - 1
        d, d2, p = dvec(k, z), dvec2(k, z), pvec(k, z)
        if self.group:                                                                      # unit magnitudes inside the group (signs stay): its block-triangle inverse stays small
            a, e = int(self.xsup[self.group[0]]), int(self.xsup[self.group[0] + self.group[1]])
            d[a:e], d2[a:e] = np.sign(d[a:e]), np.sign(d2[a:e])
        # the diagonal blocks, scaled by 4 (a ratio d_i / d_j enters as d_i (4 / d_j))
        for v in (d, d2, p):
            assert np.all(np.isin(np.abs(v) ** 2, (1, 4, 16)))
        q = lambda v: (np.conj(v) * 4) / (np.abs(v) ** 2)                                   # 4 / v, exact: |v|^2 in {1, 4, 16}
        rows, cols, lv, uv = [], [], [], []
        for s in range(len(self.widths)):
            a, e = int(self.xsup[s]), int(self.xsup[s + 1])
            i = np.arange(a, e)
            if z:                                                                            # dense triangles
                I, J = np.meshgrid(i, i, indexing="ij")
                m = I > J
                rows.append(I[m]); cols.append(J[m]); lv.append(d[I[m]] * q(d[J[m]]))
                uv.append(p[J[m]] * d2[I[m]] * q(d2[J[m]]))                               # U0[j, i] = p_j d'_i / d'_j at (row J, column I), I > J
            else:                                                                            # bidiagonals
                I, J = i[1:], i[:-1]
                rows.append(I); cols.append(J); lv.append(-d[I] * q(d[J]))
                uv.append(-p[J] * d2[I] * q(d2[J]))                                        # U0[j, j + 1] = -p_j d'_{j+1} / d'_j
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        lv, uv = np.concatenate(lv), np.concatenate(uv)
        assert np.all(lv == np.rint(lv.real) + (1j * np.rint(lv.imag) if z else 0)) and np.all(uv == np.rint(uv.real) + (1j * np.rint(uv.imag) if z else 0))
        below = (lr >= 0) & (sn[np.maximum(lr, 0)] > sn[np.maximum(lc, 0)])
        up = ur >= 0
        L4 = (sp.csr_matrix((4 * f(lr[below], lc[below]).astype(dt), (lr[below], lc[below])), shape=(n, n)) + 4 * sp.identity(n, dtype=dt, format="csr")
              + sp.csr_matrix((lv.astype(dt), (rows, cols)), shape=(n, n))).tocsr()
        U4 = (sp.csr_matrix((4 * f(ur[up], uc[up]).astype(dt), (ur[up], uc[up])), shape=(n, n)) + 4 * sp.diags(p.astype(dt), format="csr")
              + sp.csr_matrix((uv.astype(dt), (cols, rows)), shape=(n, n))).tocsr()
        B16 = (L4 @ U4).tocsr()
        aL, aU = _absint(L4), _absint(U4)
        bound = aL @ aU
        assert bound.max() < LIMIT
        self.bound = int(bound.max())
        vt = np.complex128 if z else np.float64
        self.L4, self.U4, self.B16 = L4, U4, B16
        self.L0, self.U0, self.B = L4.toarray().astype(vt) / 4, U4.toarray().astype(vt) / 4, B16.toarray().astype(vt) / 16
        stored = np.zeros((n, n), dtype=bool)
        stored[lr[lr >= 0], lc[lr >= 0]] = True
        stored[ur[up], uc[up]] = True
        assert not np.any(self.B[~stored] != 0)                                             # B lives on the stored pattern
        # the inverses of the diagonal blocks (block diagonal n x n): Linv * 4, Uinv * 16
        ir, ic, liv, uiv = [], [], [], []
        for s in range(len(self.widths)):
            i = np.arange(int(self.xsup[s]), int(self.xsup[s + 1]))
            if z:
                I, J = i[1:], i[:-1]
                ir.append(np.concatenate([i, I])); ic.append(np.concatenate([i, J]))
                liv.append(np.concatenate([np.full(len(i), 4, dtype=dt), -d[I] * q(d[J])]))
                uiv.append(np.concatenate([4 * q(p[i]), -d2[I] * q(d2[J]) * q(p[I])]))      # Uinv[j, j + 1] = -(d'_{j+1} / d'_j) / p_{j+1}
            else:
                I, J = np.meshgrid(i, i, indexing="ij")
                m = I >= J
                ir.append(I[m]); ic.append(J[m]); liv.append(d[I[m]] * q(d[J[m]]))
                uiv.append(d2[I[m]] * q(d2[J[m]]) * q(p[I[m]]))                           # Uinv[j, i] = d'_i / (d'_j p_i) at (row J, column I), I >= J
        ir, ic = np.concatenate(ir), np.concatenate(ic)
        Li4 = sp.csr_matrix((np.concatenate(liv).astype(dt), (ir, ic)), shape=(n, n))
        Ui16 = sp.csr_matrix((np.concatenate(uiv).astype(dt), (ic, ir)), shape=(n, n))
        self.Li4, self.Ui16 = Li4, Ui16
        # they ARE the inverses of the diagonal blocks (integer arithmetic): Linv L0_kk = I, U0_kk Uinv = I
        blk = sp.block_diag([np.ones((w, w), dtype=bool) for w in self.widths], format="csr")
        assert ((Li4 @ L4.multiply(blk)) != 16 * sp.identity(n, dtype=dt)).nnz == 0
        assert ((U4.multiply(blk) @ Ui16) != 64 * sp.identity(n, dtype=dt)).nnz == 0
        aLi, aUi, aB = _absint(Li4), _absint(Ui16), _absint(B16)
        for prod in ((aB, aUi), (aLi, aB), (aLi, aL, aLi), (aUi, aU, aUi)):
            assert _prod_bound(*prod) < LIMIT, _prod_bound(*prod)
        self.aL, self.aU, self.aLi, self.aUi = aL, aU, aLi, aUi
        assert (B16 != L4 @ U4).nnz == 0                                                    # nothing above sorted an index array that B16 shares
        self.gL = self.gU = None
        if self.group:                                                                      # |inverse of the group's block triangle|, by its recurrence, int64
            a, e = int(self.xsup[self.group[0]]), int(self.xsup[self.group[0] + self.group[1]])
            gb = blk[a:e, a:e].toarray()
            out = []
            for Mi, M in ((aLi, aL), (aUi, aU)):
                Mi, Mo = Mi[a:e, a:e].toarray().astype(object), (np.where(gb, 0, M[a:e, a:e].toarray()) // 4).astype(object)      # Python integers: no overflow; off-diagonal blocks hold integers
                T = Mi.copy()
                for _ in range(self.group[1] - 1):
                    T = Mi + Mi.dot(Mo.dot(T))                                              # scaled by a further 4 (16: U) per round; bounds every partial product
                    assert int(T.max()) < LIMIT
                out.append(T)
            self.gL, self.gU = out
        if not z:
            self.Linv, self.Uinv = Li4.toarray() / 4.0, Ui16.toarray() / 16.0
        if z and not fs.z:
            fs.Lnzval, fs.Unzval, fs.z = fs.Lnzval.astype(vt), fs.Unzval.astype(vt), True
            fs._build_view()
        fs.Lnzval[:] = np.where(lr >= 0, self.B[np.maximum(lr, 0), np.maximum(lc, 0)], 0)
        fs.Unzval[:] = np.where(ur >= 0, self.B[np.maximum(ur, 0), np.maximum(uc, 0)], 0)
        # the factored store: a panel's diagonal block holds U0 on and above the diagonal, L0 below it (the unit diagonal is implied)
        on = (lr >= 0) & (sn[np.maximum(lr, 0)] == sn[np.maximum(lc, 0)])
        expL = np.where(below, self.L0[np.maximum(lr, 0), np.maximum(lc, 0)], 0).astype(vt)
        expL[on] = np.where(lr[on] <= lc[on], self.U0[lr[on], lc[on]], self.L0[lr[on], lc[on]])
        expU = np.where(up, self.U0[np.maximum(ur, 0), np.maximum(uc, 0)], 0).astype(vt)
        return expL, expU

    def rhs(self, nrhs):
        """integer x (every column a different vector), b = B x and y = U0 x from the scaled integer images; the bounds of the sweeps asserted"""
        n = self.n
        i = np.arange(n)[:, None]; j = np.arange(nrhs)[None, :]
        x = ((3 * i + 7 * j + (j // 11) * (i % 5) + (j // 55) * (i % 13)) % 11) - 5
        if self.z:
            x = x + 1j * (((5 * i + j + (j // 7) * (i % 3)) % 7) - 3)
        assert np.unique(x, axis=1).shape[1] == nrhs                                        # no two columns agree
        y4 = self.U4 @ x
        b16 = self.L4 @ y4
        ax = np.abs(x.real).astype(np.int64) + (np.abs(x.imag).astype(np.int64) if self.z else 0)
        ay = np.abs(y4.real).astype(np.int64) + (np.abs(y4.imag).astype(np.int64) if self.z else 0)
        ab = np.abs(b16.real).astype(np.int64) + (np.abs(b16.imag).astype(np.int64) if self.z else 0)
        fwd = self.aLi @ (4 * ab + self.aL @ (4 * ay))                                      # |Linv| (|b| + |L0| |y|), scaled by 4 * 64
        bwd = self.aUi @ (4 * ay + self.aU @ ax)                                            # |Uinv| (|y| + |U0| |x|), scaled by 16 * 16
        assert int(fwd.max()) * 64 < LIMIT and int(bwd.max()) * 64 < LIMIT
        if self.group:                                                                      # ... and through the group's block-triangle inverses
            a, e = int(self.xsup[self.group[0]]), int(self.xsup[self.group[0] + self.group[1]])
            inner_f = (ab + self.aL @ ay)[a:e].astype(object); inner_b = (ay + self.aU @ ax)[a:e].astype(object)      # scaled by 16 / 4: their units
            assert int(self.gL.dot(inner_f).max()) < LIMIT and int(self.gU.dot(inner_b).max()) < LIMIT, (int(self.gL.dot(inner_f).max()), int(self.gU.dot(inner_b).max()))
        vt = np.complex128 if self.z else np.float64
        return np.asfortranarray(x.astype(vt)), np.asfortranarray(b16.astype(vt) / 16)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The schedule of the sweeps restated from the exported structure (sluamd_plan.cpp: DAG levels; sluamd_factor.cpp: level_joined and the drivers)
# ---------------------------------------------------------------------------------------------------------------------------------------
def levels_of(srcs):
    """DAG level of every supernode: longest path over its L and U blocks"""
    lev = [0] * len(srcs)
    for s in srcs:
        for g in [g for g, _ in s["lblocks"]] + [g for g, _ in s["ublocks"]]:
            lev[g] = max(lev[g], lev[s["k"]] + 1)
    return lev


def level_sizes(lev):
    return np.bincount(lev).tolist()


def joined(sizes, m, nrhs, join_max_nodes=32, solve_join=True, has_group=None):
    """level_joined (sluamd_factor.cpp)"""
    if not solve_join or nrhs >= 4 or (has_group and has_group[m]):
        return False
    return sizes[m] <= join_max_nodes


def predicted_launches(sizes, nrhs, join_max_nodes=32, solve_join=True, has_group=None):
    """stats()["solve_launches"] of one chunk of right-hand sides on a 1 x 1 x 1 double handle: solve_fwd_join + solve_bwd_join, or the two-launch
    drivers when the joined tables are off (SLUAMD_SOLVE_JOIN=0)"""
    nl = len(sizes)
    if not solve_join:
        return 2 * nl + 1 + 2 * nl
    J = lambda m, r=nrhs: joined(sizes, m, r, join_max_nodes, True, has_group)
    n = 1
    for l in range(nl):                              # forward: the link above level l takes the form of level l + 1 (the last one: joined below four right-hand sides)
        n += 1 if nrhs < 4 and (l + 1 == nl or J(l + 1, 1)) else 2
    n += 1
    for l in range(nl):
        n += 1 if J(l) else 2
    return n


def forward_sources(srcs, lev, g, xsup):
    """per 64-row block of supernode g: the number of panels of the previous level that hold rows of it (the sources of its joined forward units)"""
    f, w = int(xsup[g["k"]]), g["w"]
    out = []
    for c in range(-(-w // 64)):
        out.append(sum(1 for s in srcs if lev[s["k"]] + 1 == lev[g["k"]]
                       for t, rows in s["lblocks"] if t == g["k"] and any(f + 64 * c <= r < f + 64 * c + 64 for r in rows)))
    return out


def near_columns(s, lev):
    """the U columns of supernode s in supernodes of the next level (the near columns of its joined backward units)"""
    return sum(len(cols) for g, cols in s["ublocks"] if lev[g] == lev[s["k"]] + 1)


def strips(s, lev):
    """the 64-row strips of the panel of s below its diagonal block: (rows in the strip, rows of the next level among them)"""
    rows = [(r, g) for g, rr in s["lblocks"] for r in rr]
    return [(len(rows[a:a + 64]), sum(1 for _, g in rows[a:a + 64] if lev[g] == lev[s["k"]] + 1)) for a in range(0, len(rows), 64)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# The cases (the rules of the symbolic factorisation they rely on: schur_cases.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _fan(name, purpose, src_widths, dst_widths, rows, cols, **kw):
    c = sc._fan(name, purpose, src_widths, dst_widths, rows, cols, **kw)
    c.__class__ = SweepCase
    return c


def _rows_mixed(s, t, wt):
    return [range(wt), range(1, wt, 2), range(min(wt, 34)), range(wt)][s % 4]


def widths():
    """guarded sources of every width class -- 1, 2, 15 .. 17, 31 .. 33, 63 .. 65 (the narrow / wide boundary, the 64-column blocks of the inverses),
    127 .. 129, 200, 255, 256 (slices cpp = ceil(ns / NP) that are no multiples of the batch) -- over a chain of destinations that receive 1, 63, 64, 65 and 130
    rows each (partial strips); U rows with the skyline leads of schur_cases._lead_cols (ragged columns in the backward units)"""
    return _fan("widths", "width classes, partial strips, skyline leads", WIDTHS, [2, 64, 65, 66, 131], sc._all_rows, sc._lead_cols)


def narrow():
    """every supernode at most 64 columns wide: the narrow build on every level (in `widths` the wide sources share their level with the narrow ones)"""
    return _fan("narrow", "the narrow build", [1, 2, 15, 16, 17, 31, 32, 33, 63, 64], [2, 33, 64, 64], _rows_mixed, sc._lead_cols)


def wide_launch():
    """a level of 65 .. 256-column sources with 4 to 5 strips of 64 rows each: launches of dozens of wide units (builds 1 and 5 under
    SLUAMD_SWEEP_WIDE_MIN=1), slices whose steady loops and tails run (256 = 2 x 8 x 16: two batches of build 1; 200, 129, 65: tails)"""
    return _fan("wide_launch", "launches of many wide units", [256, 255, 200, 129, 128, 65, 100, 72], [131, 66, 65, 40], sc._all_rows, sc._lead_cols)


def levels():
    """a DAG with levels of 66, 1, 33, 4, 2 and 1 supernodes of mixed widths: a level of one supernode BELOW a level of 33, so that joined and two-launch
    links meet in both orders.
    level 0: 34 guards and 32 relaxed leaves of 2 / 3 / 5 columns, which update a level-3 supernode and the top (far rows only)
    level 1: Y, 100 columns, guarded, with no L panel and a U row that holds columns of ALL 33 supernodes of level 2 (more than 256 near columns under a wide
             level; ragged leads); it adds no fill
    level 2: 33 guarded sources of 5 .. 64 columns; each holds rows of ONE level-3 supernode (near) and of its level-4 parent and the top (far) -- near and
             far rows share 64-row strips; the 64-row blocks of the level-3 supernodes have 1, 3, 4 and 6 + sources.  The sources of the 100- and 90-column
             supernodes hold up to 99 near columns under levels of at most 64 columns ... (see the coverage test for what is counted where)
    level 3: 48, 40 (under A), 100 and 90 columns (under B); level 4: A = 200 and B = 150 columns; level 5: the top, 129 columns"""
    W1 = [8, 16, 33, 40, 64, 17, 5, 24, 63, 31, 12]
    w2, w3, wt = [48, 40, 100, 90], [200, 150], 129
    feed = [0] + [1] * 3 + [2] * 10 + [3] * 19
    widths_, L, U, guards = [1, 100], {0: {1: [0]}, 1: {}}, {0: {1: {0: 0}}, 1: {}}, [0]      # the guard of Y, and Y
    pend = []                                        # (node, level-2 index, kind, i): blocks are filled in once every supernode has its number
    l2, l3 = [None] * 4, [None] * 2
    for t in range(4):
        for i in [i for i in range(33) if feed[i] == t]:
            guards.append(len(widths_)); widths_ += [1, W1[i % len(W1)]]
            pend.append((len(widths_) - 1, t, "src", i))
        for j in range(8 * t, 8 * t + 8):
            widths_.append((2, 3, 5)[j % 3]); pend.append((len(widths_) - 1, t, "leaf", j))
        l2[t] = len(widths_); widths_.append(w2[t])
        if t % 2:
            l3[t // 2] = len(widths_); widths_.append(w3[t // 2])
    top = len(widths_); widths_.append(wt)
    lc = sc._lead_cols
    for k, t, kind, i in pend:
        W, par, wp = w2[t], l3[t // 2], w3[t // 2]
        if kind == "leaf":
            L[k] = {l2[t]: sorted({1} | set(range(1 + i % 3, W, 2))), top: range(1 + i, 40 + i)}
            U[k] = {l2[t]: {c: 0 for c in range(1, W, 1 + i % 2)}, top: {c: 0 for c in range(1, 50 + i)}}
            continue
        g, ws = k - 1, widths_[k]
        L[g], U[g] = {k: [0]}, {k: {0: 0}}
        U[1][k] = {c: (c * 7 + i) % 100 for c in range(1, ws)}      # Y's U row: columns of every source, ragged leads
        if t == 2:
            near = range(1, 30) if i < 10 else range(64 + (i % 3), 100, 1 + i % 2)
        elif t == 3:
            near = range(1 + i % 4, W, 1 + i % 3)
        else:
            near = range(1 + (i % 2), W, 1 + (i % 2))
        L[k] = {l2[t]: sorted({1} | set(near)), par: range(1 + i % 5, 40 + i), top: range(1, 20 + 3 * i)}      # (row 1 in every child: siblings keep their order)
        U[k] = {l2[t]: {c: min(ld, ws - 1) for c, ld in lc(i % 6, 0, W, ws).items() if c > 0},
                par: {c: min(ld, ws - 1) for c, ld in lc((i + 1) % 6, 0, wp, ws).items() if 0 < c < 60 + i},
                top: {c: min(ld, ws - 1) for c, ld in lc((i + 2) % 6, 0, wt, ws).items() if c > 0}}
    for t, k in enumerate(l2):
        wp = w3[t // 2]
        L[k] = {l3[t // 2]: range(1, wp, 1 + t % 2), top: range(1, wt)}
        U[k] = {l3[t // 2]: {c: c % 5 for c in range(1, wp)}, top: {c: c % 3 for c in range(1, wt)}}
    for k in l3:
        L[k] = {top: range(wt)}
        U[k] = {top: {c: 0 for c in range(wt)}}
    return SweepCase("levels", "level sizes, joined and two-launch links, sources and near columns of the joined units", widths_, L, U, guards=guards)


def groups():
    """two guarded leaves under a chain of four pieces of 64, 64, 64 and 48 columns (SLUAMD_SOLVE_GROUPS=1 merges them into one group; every piece's panel
    and U row hold a row and a column of each LATER group member: dead rows and columns) and a top supernode above the chain.  Inside the group D and D' have unit magnitude and
    the pieces are coupled by a few rows and columns, so that the absolute-value recurrence of the group's block-triangle inverse stays below 2^53."""
    L = {0: {1: [0]}, 2: {3: [0]}}
    U = {0: {1: {0: 0}}, 2: {3: {0: 0}}}
    ch, gw, top = [4, 5, 6, 7], [64, 64, 64, 48], 8
    for leaf, step in ((1, 1), (3, 2)):
        L[leaf] = {ch[0]: range(1, gw[0], step), top: range(1, 65)}                               # (rows of the first member only: no fill between the members)
        U[leaf] = {ch[0]: {cc: (cc % 3 if leaf == 3 else 0) for cc in range(1, gw[0], 5)}, top: {cc: 0 for cc in range(1, 65, 7)}}
    for a, c in enumerate(ch):
        L[c] = {d: [5 + a] for b_, d in enumerate(ch) if b_ > a}; L[c][top] = range(65)       # one row and one column per pair of members
        U[c] = {d: {7 + a: a % 2} for b_, d in enumerate(ch) if b_ > a}; U[c][top] = {cc: 0 for cc in range(65)}
    c = SweepCase("groups", "merged chain groups", [1, 4, 1, 3] + gw + [65], L, U, guards=[0, 2])
    c.group = (4, 4)
    return c


def z_narrow():
    c = _fan("z_narrow", "complex16: the fused links (every supernode at most 64 columns)", [1, 2, 15, 16, 17, 31, 32, 33, 63, 64], [2, 33, 64, 64], _rows_mixed,
             sc._lead_cols, complex16=True)
    return c


def z_wide():
    return _fan("z_wide", "complex16: supernodes of more than 64 columns (the in-place pair, kz_solve_diag)", [65, 128, 33, 200], [66, 131], sc._all_rows, sc._lead_cols,
                complex16=True)


def z_levels():
    """complex16: a tree with levels of 20 (guards and leaves), 17, 3 and 1 supernodes, all at most 64 columns: the fused links and the in-place pair meet
    across SLUAMD_ZFUSE_MAX_NODES = 16"""
    ns, w2 = 17, [40, 33, 64]
    widths_, L, U, guards, pend, l2 = [], {}, {}, [], [], []
    for t in range(3):
        for i in range(t, ns, 3):
            guards.append(len(widths_)); widths_ += [1, (8, 16, 33, 5, 64, 17)[i % 6]]
            pend.append((len(widths_) - 1, t, i))
        widths_.append(1 + t); pend.append((len(widths_) - 1, t, -1))
        l2.append(len(widths_)); widths_.append(w2[t])
    top = len(widths_); widths_.append(50)
    for k, t, i in pend:
        if i < 0:
            L[k] = {l2[t]: range(1, w2[t], 2), top: range(1, 30)}
            U[k] = {l2[t]: {c: 0 for c in range(1, w2[t])}, top: {c: 0 for c in range(1, 20)}}
            continue
        L[k - 1], U[k - 1] = {k: [0]}, {k: {0: 0}}
        ws = widths_[k]
        L[k] = {l2[t]: sorted({1} | set(range(1 + i % 2, w2[t], 1 + i % 3))), top: range(1, 10 + 2 * i)}
        U[k] = {l2[t]: {c: min(ld, ws - 1) for c, ld in sc._lead_cols(i % 6, 0, w2[t], ws).items() if c > 0}, top: {c: 0 for c in range(1, 50, 1 + i % 2)}}
    for k in l2:
        L[k] = {top: range(1, 50)}
        U[k] = {top: {c: c % 3 for c in range(1, 50)}}
    return SweepCase("z_levels", "complex16: fused and in-place levels", widths_, L, U, complex16=True, guards=guards)


CASES = {"widths": widths, "narrow": narrow, "levels": levels, "wide_launch": wide_launch, "groups": groups, "z_narrow": z_narrow, "z_wide": z_wide, "z_levels": z_levels}
