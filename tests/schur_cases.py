"""Matrices whose factors are known EXACTLY and whose whole difficulty sits in the Schur update (test helper for test_gpu_schur_shapes.py;
not a conftest).

Construction.  A case is a designed block pattern: supernodes (widths), per supernode s the rows of later supernodes its L panel holds and
the columns of later supernodes its U row block holds, each U column with the first stored row inside s (the skyline lead).  The pattern is
handed, explicit zeros and all, to the library's exact unsymmetric symbolic factorisation, which closes it under fill; the stored structure
that comes back is filled with L0 (unit lower) and U0:
  * diagonal blocks: L0 = I, U0 = diag(+-2^e), e in {0, 1, 2}.  Linv / Uinv, the diagonal LU and both panel solves are then one-term sums and
    power-of-two scalings: exact.  The only kernel whose arithmetic matters is k_schur.
  * off-diagonal stored positions: the small integer ((5 i + 3 j) mod 7) - 3 of (row, column) (zero included, so that stored zeros occur),
    Gaussian integers for complex16: a misplaced element is another number, not the same one.
B = L0 U0 is formed in int64; `Case` asserts that every sum_k |L0[i,k]| |U0[k,j]| is below 2^53, so every intermediate of ANY summation
order (MFMA k-blocking, fp64 atomics, K-fusion, split-K) is an exact double and the factorisation of B must return L0 and U0, every stored
entry, with no tolerance.

The sign of a stored zero.  The update A - L U with exact operands gives +0.0 in round-to-nearest unless both terms are -0.0, and B's
zeros are +0.0; but a zero of L then goes through the panel solve with its pivot, and 0 / (negative pivot) is -0.0 in the reference's
dtrsm while a multiplication by an explicit inverse summed with other +0.0 terms gives +0.0.  Both are what exact arithmetic allows for a
ZERO, so the comparisons here are IEEE equality of every stored value (numpy.array_equal: +0.0 == -0.0, NaN equals nothing): every non-zero
bitwise, every zero a zero of either sign.

The planner rules the designs rely on are restated in `source_is_big` (sluamd_plan.cpp, count_one); the tests assert the restatement
against stats()["flops_schur_exact_big"], so a planner change shows up as a failed coverage test, not as a silently idle case."""
import numpy as np
import scipy.sparse as sp
import pivot_cases as pc

LIMIT = 2 ** 53


def val(i, j):
    return ((5 * i + 3 * j) % 7) - 3


def zval(i, j):
    return val(i, j) + 1j * (((3 * i + 5 * j) % 5) - 2)


class Case:
    """widths: supernode widths.  L[s][t] = row offsets inside supernode t held by the panel of s (t > s).  U[s][t] = {column offset inside t:
    lead} -- the column is stored from row `lead` of s down.  Rows that fill would add to only SOME columns of a later supernode are added
    to all of them here (`_close`), so that the designed partition survives the symbolic factorisation; everything else is left to it."""

    def __init__(self, name, purpose, widths, L, U, complex16=False, maxsup=256, guards=()):
        self.name, self.purpose, self.z, self.maxsup, self.guards = name, purpose, complex16, maxsup, set(guards)
        self.widths = [int(w) for w in widths]
        self.xsup = np.concatenate([[0], np.cumsum(self.widths)]).astype(np.int64)
        self.n = int(self.xsup[-1])
        ns = len(widths)
        self.L = {s: {t: sorted(set(int(r) for r in rows)) for t, rows in L.get(s, {}).items()} for s in range(ns)}
        self.U = {s: {t: {int(c): int(ld) for c, ld in cols.items()} for t, cols in U.get(s, {}).items()} for s in range(ns)}
        self._close()
        for s in range(ns):                      # no panel holds row 0 of a later supernode (a guard's single row excepted): see the cases' notes
            if s not in self.guards:
                self.L[s] = {t: [r for r in rows if r > 0] for t, rows in self.L[s].items()}
        xs = self.xsup
        P = sp.lil_matrix((self.n, self.n), dtype=np.int8)
        for s in range(ns):
            f, w = int(xs[s]), self.widths[s]
            P[f:f + w, f:f + w] = 1
            for t, rows in self.L[s].items():
                assert t > s and all(0 <= r < self.widths[t] for r in rows)
                for r in rows:
                    P[int(xs[t]) + r, f:f + w] = 1
            for t, cols in self.U[s].items():
                assert t > s
                for c, ld in cols.items():
                    assert 0 <= c < self.widths[t] and 0 <= ld < w
                    P[f + ld:f + w, int(xs[t]) + c] = 1
        self.P = P.tocsr()
        self.P.sort_indices()

    def _close(self):
        ns = len(self.widths)
        for s in range(ns):
            for t in sorted(self.U[s]):
                if not self.U[s][t]:
                    continue
                for u, rows in self.L[s].items():
                    if u > t and rows:
                        cur = self.L[t].setdefault(u, [])
                        self.L[t][u] = sorted(set(cur) | set(rows))

    def pattern_csr(self):
        return self.n, self.P.indptr.astype(np.int32), self.P.indices.astype(np.int32)

    def fill(self, fs, pos=None):
        """L0, U0 (scipy CSR, int64 or Gaussian-integer complex128) on the stored positions of the flat store `fs`, B = L0 U0, and the
        store's Lnzval / Unzval holding B.  Asserts the 2^53 bound and that B's support lies inside the stored pattern."""
        (lr, lc), (ur, uc) = pos or pc.store_positions(fs)
        assert fs.xsup.tolist() == self.xsup.tolist(), fs.xsup.tolist()
        n = self.n
        f = zval if self.z else val
        dt = np.complex128 if self.z else np.int64
        sn = np.searchsorted(self.xsup, np.arange(n), side="right") - 1
        below = (lr >= 0) & (sn[np.maximum(lr, 0)] > sn[np.maximum(lc, 0)])                  # L panel entries under the diagonal block
        L0 = sp.csr_matrix((f(lr[below], lc[below]).astype(dt), (lr[below], lc[below])), shape=(n, n)) + sp.identity(n, dtype=dt, format="csr")
        k = np.arange(n)
        d = ((1 << (k % 3)) * np.where((k // 3) % 2 == 0, 1, -1)).astype(dt)             # diag(+-2^e): +1 +2 +4 -1 -2 -4 ...
        if self.z:
            d = d * np.array([1, 1j, -1, -1j])[(k // 6) % 4]                                 # ... times a unit of the Gaussian integers: 1 / d stays exact
        up = ur >= 0
        U0 = sp.csr_matrix((f(ur[up], uc[up]).astype(dt), (ur[up], uc[up])), shape=(n, n)) + sp.diags(d, format="csr")
        B = (L0 @ U0).tocsr()
        if self.z:                                                                        # |re| + |im| bounds both parts of every partial sum
            aL = abs(L0.real).astype(np.int64) + abs(L0.imag).astype(np.int64); aU = abs(U0.real).astype(np.int64) + abs(U0.imag).astype(np.int64)
        else:
            aL, aU = abs(L0), abs(U0)
        bound = (aL @ aU)
        assert bound.nnz == 0 or bound.max() < LIMIT
        self.bound = int(bound.max()) if bound.nnz else 0
        Bd = B.toarray()
        stored = np.zeros((n, n), dtype=bool)
        stored[lr[lr >= 0], lc[lr >= 0]] = True
        stored[ur[up], uc[up]] = True
        assert not np.any(Bd[~stored] != 0)                                                # B lives on the stored pattern
        vt = np.complex128 if self.z else np.float64
        self.L0, self.U0, self.B = L0.toarray().astype(vt), U0.toarray().astype(vt), Bd.astype(vt)
        self.Bint = B
        if self.z and not fs.z:
            fs.Lnzval, fs.Unzval, fs.z = fs.Lnzval.astype(vt), fs.Unzval.astype(vt), True
            fs._build_view()
        fs.Lnzval[:] = np.where(lr >= 0, self.B[np.maximum(lr, 0), np.maximum(lc, 0)], 0)
        fs.Unzval[:] = np.where(ur >= 0, self.B[np.maximum(ur, 0), np.maximum(uc, 0)], 0)
        # what the factored store must hold: the diagonal block of a panel holds U's (L's unit diagonal is implied), its strict lower part L0's zeros
        on = (lr >= 0) & (sn[np.maximum(lr, 0)] == sn[np.maximum(lc, 0)])
        expL = np.where(below, self.L0[np.maximum(lr, 0), np.maximum(lc, 0)], 0).astype(vt)
        expL[on] = np.where(lr[on] == lc[on], self.U0[lr[on], lc[on]], 0)
        expU = np.where(up, self.U0[np.maximum(ur, 0), np.maximum(uc, 0)], 0).astype(vt)
        return expL, expU

    def rhs(self, nrhs):
        """integer x, b = B x and the intermediate y = U0 x, all in int64 (Gaussian integers for complex16), bounds asserted"""
        n = self.n
        i = np.arange(n)[:, None]; j = np.arange(nrhs)[None, :]
        x = ((3 * i + 7 * j) % 11) - 5
        if self.z:
            x = x + 1j * (((5 * i + j) % 7) - 3)
        U0 = sp.csr_matrix(self.U0.astype(np.complex128 if self.z else np.int64))
        y = U0 @ x
        b = self.Bint @ x
        # the sweeps add products of stored entries with integers below 2^53 / (n * 8): exact whatever their order
        assert self.bound * 16 * n < LIMIT and np.abs(y).max() * 8 * n < LIMIT and np.abs(b).max() < LIMIT
        vt = np.complex128 if self.z else np.float64
        return np.asfortranarray(x.astype(vt)), np.asfortranarray(b.astype(vt))


# ---------------------------------------------------------------------------------------------------------------------------------------
# Structure of a flat store, per source supernode: what the coverage test reads
# ---------------------------------------------------------------------------------------------------------------------------------------
def sources(fs):
    """per supernode k: dict(w, lblocks=[(gid, [global rows])] without the diagonal block, ublocks=[(gid, {column offset in gid: lead})] with
    the non-empty columns only, in stored order)"""
    xs = fs.xsup
    out = []
    for k in range(len(xs) - 1):
        f, w = int(xs[k]), int(xs[k + 1] - xs[k])
        lb, ub = [], []
        o = int(fs.Lrowind_off[k])
        if fs.Lrowind_off[k + 1] > o:
            nb = int(fs.Lrowind[o]); p = o + 2
            for _ in range(nb):
                gid, nr = int(fs.Lrowind[p]), int(fs.Lrowind[p + 1])
                if gid != k:
                    lb.append((gid, fs.Lrowind[p + 2:p + 2 + nr].tolist()))
                p += 2 + nr
        o = int(fs.Ufstnz_off[k])
        if fs.Ufstnz_off[k + 1] > o:
            nb = int(fs.Ufstnz[o]); p = o + 3
            for _ in range(nb):
                gid = int(fs.Ufstnz[p]); gw = int(xs[gid + 1] - xs[gid])
                fst = fs.Ufstnz[p + 2:p + 2 + gw]
                cols = {c: int(fst[c]) - f for c in range(gw) if fst[c] < f + w}
                if cols:
                    ub.append((gid, cols))
                p += 2 + gw
        out.append(dict(k=k, w=w, lblocks=lb, ublocks=ub))
    return out


def source_is_big(src, z=False, big_min_cols=96, big_util_pct=50):
    """the tile configuration of a source: a restatement of count_one (sluamd_plan.cpp) for a 1 x 1 x 1 store -- 128 x 128 tiles when the
    supernode is at least big_min_cols wide (48 in complex16) and its blocks fill at least big_util_pct % of the 128 x 128 tiles they span"""
    tmr = 64 if z else 128
    t128r = sum(-(-len(r) // tmr) for _, r in src["lblocks"])
    t128c = sum(-(-len(c) // 128) for _, c in src["ublocks"])
    cells = sum(len(r) for _, r in src["lblocks"]) * sum(len(c) for _, c in src["ublocks"])
    util = cells / (t128r * t128c * tmr * 128.0) if t128r * t128c else 0.0
    return src["w"] >= (48 if z else big_min_cols) and util >= 0.01 * big_util_pct


def exact_flops(src):
    """flops_schur_exact of one source as the planner counts it: 2 x panel rows below the diagonal block x stored U values"""
    rows = sum(len(r) for _, r in src["lblocks"])
    return 2.0 * rows * sum(src["w"] - ld for _, cols in src["ublocks"] for ld in cols.values())


def tiles(src, big, z=False):
    """the (unmerged) tiles of a source: (rows of the tile, [leads of its columns], [column offsets], row block gid, column block gid)"""
    tm = (128 if big else 64) // (2 if z else 1)
    tn = 128 if big else 64
    for gi, rows in src["lblocks"]:
        for r0 in range(0, len(rows), tm):
            for gj, cols in src["ublocks"]:
                cs = sorted(cols)
                for c0 in range(0, len(cs), tn):
                    cc = cs[c0:c0 + tn]
                    yield rows[r0:r0 + tm], [cols[c] for c in cc], cc, gi, gj


def kbeg_of(src):
    """first k the kernel visits for this source: U is zero above its tallest segment (kbeg_own = (ns - ldu) & ~3)"""
    ldu = max((src["w"] - ld for _, cols in src["ublocks"] for ld in cols.values()), default=0)
    return (src["w"] - ldu) & ~3


# ---------------------------------------------------------------------------------------------------------------------------------------
# The cases.  Rules of the symbolic factorisation (sluamd_dsymbfact_unsym, the reference's) that the designs rely on, with relax = 1:
#   * column j + 1 joins the supernode of column j when its structure is that of column j without row j + 1.  No panel here holds row 0 of a
#     later supernode (Case strips it), so the last column of a supernode never nests into the first of the next one: the designed partition
#     stands (the tests assert it).  Destinations are therefore one column wider than the row count they are meant to receive.
#   * a column without children in the elimination tree starts a RELAXED supernode, whose U segments are always full height (no skyline).
#     Every source that is to carry leads is therefore preceded by a GUARD: a one-column supernode holding row 0 and column 0 of it (the one
#     exception to the rule above; it cannot merge, the structures differ in size).  A guard is itself a source with K = 1.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _fan(name, purpose, src_widths, dst_widths, rows, cols, **kw):
    """guarded independent sources updating a chain of destinations: rows(s, t, wt) -> row offsets in destination t, cols(s, t, wt, ws) ->
    {column: lead}.  Supernode 2 s is the guard of source s (supernode 2 s + 1), the destinations follow."""
    ns, nd = len(src_widths), len(dst_widths)
    L, U = {}, {}
    for s in range(ns):
        g, k = 2 * s, 2 * s + 1
        L[g], U[g] = {k: [0]}, {k: {0: 0}}
        L[k] = {2 * ns + t: rows(s, t, dst_widths[t]) for t in range(nd)}
        U[k] = {2 * ns + t: {c: min(ld, src_widths[s] - 1) for c, ld in cols(s, t, dst_widths[t], src_widths[s]).items() if c > 0} for t in range(nd)}
        L[k] = {t: r for t, r in L[k].items() if len(r)}
        U[k] = {t: c for t, c in U[k].items() if len(c)}
    # the destinations form a chain of their own (each holds every later one, dense): a closed pattern whatever the sources do
    for t in range(nd):
        L[2 * ns + t] = {2 * ns + u: range(dst_widths[u]) for u in range(t + 1, nd)}
        U[2 * ns + t] = {2 * ns + u: {c: 0 for c in range(dst_widths[u])} for u in range(t + 1, nd)}
    widths = [w for ws in src_widths for w in (1, ws)] + list(dst_widths)
    return Case(name, purpose, widths, L, U, guards=range(0, 2 * ns, 2), **kw)


def _all_rows(s, t, wt):
    return range(wt)


def _clean_cols(s, t, wt, ws):
    return {c: 0 for c in range(wt)}


def k_big():
    """K of the source, 128 x 128 tiles: 256, 255, 111 (16 m + 15), 97 (16 m + 1, odd), 96 (16 m), 112 -- clean sources (the LDS-DMA loader and its
    partial last chunk); destinations that receive 129, 127, 128 and 65 rows and as many columns (tiles of 128 + 1, 127, 128 and 65).  (The last
    source stands next to its first destination: the planner may K-fuse it, so the coverage test does not count on it.)"""
    return _fan("k_big", "K of the source; tile rows and columns (128 x 128)", [256, 255, 111, 97, 96, 112], [130, 128, 129, 129, 129, 66], _all_rows, _clean_cols)


def k_small():
    """K of the source, 64 x 64 tiles: 1 (the guards), 8 (< 16), 16, 33 (16 m + 1), 47 (16 m + 15), 64; destinations that receive 65, 64, 63, 1
    and 129 rows and as many columns"""
    return _fan("k_small", "K of the source; tile rows and columns (64 x 64)", [8, 16, 33, 47, 64], [66, 65, 64, 2, 130], _all_rows, _clean_cols)


def _lead_cols(s, t, wt, ws):
    K = ws
    if s == 0:                                          # clean
        return {c: 0 for c in range(wt)}
    if s == 1:                                          # one column with lead 1, the rest clean
        return {c: (1 if c == 5 else 0) for c in range(wt)}
    if s == 2:                                          # odd and even leads; the two columns of a swizzle pair (c, c ^ 1) differ
        return {c: (c % 4) + (c & 1) * 2 for c in range(wt)}
    if s == 3:                                          # leads that change from one eight-column group to the next; whole chunks of zeros; empty segments
        return {c: [0, 3, 16, 17, 33, 2, K - 1, 18][(c // 8) % 8] for c in range(wt) if c % 3 != 1}
    if s == 4:                                          # every column: lead >= 16 (the source starts late: kbeg_own > 0), one stored element in some
        return {c: (K - 1 if c % 7 == 0 else 16 + (c % 5)) for c in range(wt)}
    return {c: (c * 7) % K for c in range(wt)}          # anything


def leads(big):
    """U leads inside one tile: sources 0..5 (see _lead_cols), all into the same destinations -- a clean and several unclean sources of one
    destination.  big: sources of 128 / 127 columns (128 x 128 tiles); otherwise 40 / 33 (64 x 64)"""
    w = [128, 128, 127, 128, 127, 128] if big else [40, 40, 33, 40, 33, 40]
    return _fan("leads_big" if big else "leads_small", "U leads inside one tile", w, [129, 129, 129, 130] if big else [130, 65, 64], _all_rows, _lead_cols)


def _row_cases(s, t, wt):
    if s == 0:                                          # odd row counts per block: in a merged row tile the pairs straddle the block boundaries
        return range(0, min(wt, 2 * (t + 1) + 2))
    if s == 1:                                          # every other row; 1 and 2 rows in a block
        return [range(1, wt, 2), [3], [4, 9], range(2, wt, 2)][t % 4]
    return range(wt)


def rows_and_merges():
    """tile rows: 1, 2 and odd row counts per block, row pairs that straddle two L blocks of the source (merged row tiles), many small L and
    U blocks per destination panel / U row (what the tile merge joins), U columns with empty segments between stored ones; the case of
    SLUAMD_NO_MERGE_TILES and of shuffle_block_rows"""
    def cols(s, t, wt, ws):
        if s == 0:
            return {c: 0 for c in range(1, wt, 3)}
        if s == 1:
            return {c: c % 3 for c in range(min(wt, 6))}
        return {c: 0 for c in range(wt)}
    return _fan("rows_and_merges", "tile rows; merged tiles", [128, 100, 48], [8, 10, 13, 6, 22, 34, 65, 131], _row_cases, cols)


def _chain(name, purpose, wa, rows_missing, lead_a, lead_b, three=False, wtop=201, **kw):
    """a guarded chain a -> b -> top (three: a0 -> a -> b -> top) of supernodes on consecutive DAG levels, what the planner K-fuses: b applies
    a's deferred update with its own.  rows_missing: rows of top that the predecessors lack and b holds; lead_a / lead_b: column -> lead of
    the U columns in top (the first member is guarded, so that its leads are kept)"""
    m = 3 if three else 2
    top = m + 1
    L, U = {0: {1: [0]}}, {0: {1: {0: 0}}}
    for i in range(m):
        s = i + 1
        L[s], U[s] = {}, {}
        for t in range(s + 1, m + 1):
            L[s][t] = range(wa)
            U[s][t] = {c: 0 for c in range(wa)}
        last = i == m - 1
        L[s][top] = [r for r in range(wtop) if last or r not in rows_missing]
        U[s][top] = {c: (lead_b if last else lead_a)(c) for c in range(1, wtop)}
    return Case(name, purpose, [1] + [wa] * m + [wtop], L, U, guards=[0], **kw)


def fuse_clean():
    return _chain("fuse_clean", "K-fusion: predecessor with all rows present, same leads", 128, (), lambda c: 0, lambda c: 0)


def fuse_absent():
    """the predecessor lacks single rows at even and odd positions of its successor's panel (the FIRST row of one pair, the SECOND of another),
    both rows of a pair, and a run of three that shifts the parity of everything behind it; its U leads differ from the successor's"""
    return _chain("fuse_absent", "K-fusion: l_has0 / l_has1, leads that differ", 128, (10, 21, 40, 41, 60, 61, 62),
                  lambda c: (c % 5), lambda c: (c % 3 == 0) * 2)


def fuse_three():
    return _chain("fuse_three", "K-fusion: a group of three", 112, (7, 30), lambda c: c % 2, lambda c: 0, three=True)


def fuse_two_tops():
    """a guarded chain a -> b with TWO destinations above it (192 and 61 columns), for the store in which a lists its L blocks in another order
    than b (permute_l_blocks: what l3_source and build_pair_maps handle).  b holds 191 rows of the first top and 60 of the second: 251 rows
    that merge into two 128-row tiles, so the pair (190, 191) of b's panel is the LAST row of the first top and the FIRST of the second.  a lacks
    the former (the planner fuses only when rows present in both panels stay neighbours, which two blocks in swapped order are not) and holds
    the latter: a pair whose only present row comes from a block that lies BEFORE its neighbour's block in a's panel.  a also lacks one row
    inside each block."""
    L = {0: {1: [0]}, 1: {2: range(128), 3: [r for r in range(192) if r not in (50, 191)], 4: [r for r in range(61) if r != 7]},
         2: {3: range(192), 4: range(61)}, 3: {4: range(61)}}
    U = {0: {1: {0: 0}}, 1: {2: {c: 0 for c in range(128)}, 3: {c: c % 3 for c in range(1, 129)}}, 2: {3: {c: 0 for c in range(1, 129)}},
         3: {4: {c: 0 for c in range(61)}}}
    return Case("fuse_two_tops", "K-fusion: predecessor's L blocks in another order", [1, 128, 128, 192, 61], L, U, guards=[0])


def permute_l_blocks(fs, k, order, values=()):
    """the off-diagonal L blocks of panel k of the flat store `fs` in the order `order` (a permutation of range(number of such blocks)): index
    entries and the rows of Lnzval alike; every array in `values` (same layout as fs.Lnzval, e.g. the expected factors) is permuted with it"""
    a = int(fs.Lrowind_off[k])
    li = fs.Lrowind[a:int(fs.Lrowind_off[k + 1])]
    nb, nsupr = int(li[0]), int(li[1])
    w = int(fs.xsup[k + 1] - fs.xsup[k])
    blocks, p, r0 = [], 2, 0
    for b in range(nb):
        nr = int(li[p + 1])
        blocks.append((li[p:p + 2 + nr].copy(), r0, nr))
        p += 2 + nr; r0 += nr
    assert int(blocks[0][0][0]) == k and sorted(order) == list(range(nb - 1))
    new = [blocks[0]] + [blocks[1 + i] for i in order]
    li[2:] = np.concatenate([d for d, _, _ in new])
    rows = np.concatenate([np.arange(r, r + nr) for _, r, nr in new])
    v0, v1 = int(fs.Lnzval_off[k]), int(fs.Lnzval_off[k + 1])
    for arr in (fs.Lnzval,) + tuple(values):
        arr[v0:v1] = arr[v0:v1].reshape((nsupr, w), order="F")[rows, :].reshape(-1, order="F")


def chain_top():
    """two leaves under a 512-column separator that maxsup = 256 cuts into a chain of two: the diagonal-block destinations of the second piece
    are the chain tiles (split-K instantiation, SLUAMD_KSPLIT)"""
    L = {0: {2: range(256), 3: range(256)}, 1: {2: range(0, 256, 2), 3: range(255)}, 2: {3: range(256)}}
    U = {0: {2: {c: 0 for c in range(256)}, 3: {c: 0 for c in range(256)}}, 1: {2: {c: 0 for c in range(256)}, 3: {c: 0 for c in range(255)}},
         2: {3: {c: 0 for c in range(256)}}}
    return Case("chain_top", "chain tiles (split K)", [128, 130, 256, 256], L, U, guards=[2])


def last_slot():
    """the LAST Schur source of the store has an odd panel height, an odd width and U segments of odd length: its last panel column ends on a
    lone row and its last U pair ends the value slot (the one-double over-read of the 16-byte loader must not change a value)"""
    L = {0: {1: [0]}, 1: {2: range(63), 3: [1]}, 2: {3: [1, 2]}}
    U = {0: {1: {0: 0}}, 1: {2: {c: c % 2 for c in range(63)}, 3: {1: 2}}, 2: {3: {1: 0, 2: 0}}}
    return Case("last_slot", "last slot of the arena", [1, 97, 63, 3], L, U, guards=[0])


def z_leads():
    """complex16: odd and even panel rows per tile, odd K, leads as in the double case (fetch_into with zoff / zsgn)"""
    def rows(s, t, wt):
        return [range(wt), range(1, wt, 2), range(min(wt, 34))][s % 3]
    return _fan("z_leads", "complex16", [8, 64, 33, 40, 17, 96], [66, 34, 65], rows, _lead_cols, complex16=True)


def z_chain():
    """complex16, wide sources (128-row tiles of the real embedding = 64 panel rows): every row and every other row of the destinations"""
    L = {0: {1: [0]}, 1: {3: range(129), 4: range(64)}, 2: {3: range(1, 129, 2), 4: range(65)}, 3: {4: range(65)}}
    U = {0: {1: {0: 0}}, 1: {3: {c: 0 for c in range(1, 129)}, 4: {c: c % 4 for c in range(1, 65)}}, 2: {3: {c: 0 for c in range(1, 129)}, 4: {c: 0 for c in range(1, 65)}},
         3: {4: {c: 0 for c in range(65)}}}
    return Case("z_chain", "complex16: wide sources", [1, 49, 64, 129, 65], L, U, complex16=True, guards=[0])


CASES = {"k_big": k_big, "k_small": k_small, "leads_big": lambda: leads(True), "leads_small": lambda: leads(False), "rows_and_merges": rows_and_merges,
         "fuse_clean": fuse_clean, "fuse_absent": fuse_absent, "fuse_three": fuse_three, "fuse_two_tops": fuse_two_tops, "chain_top": chain_top, "last_slot": last_slot,
         "z_leads": z_leads, "z_chain": z_chain}
