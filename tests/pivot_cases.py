"""Matrices whose unpivoted elimination meets pivots known EXACTLY in advance (test helper for test_gpu_pivots.py; not a conftest).

Construction: the factored matrix is B = L0 U0 with L0 unit lower and U0 upper triangular, both supported on the filled pattern of a
nested-dissection-like tree of dense blocks (every block dense, coupled densely to all its ancestors: a pattern closed under fill, so the
symbolic factorisation adds nothing to it).  Off-diagonal entries are small dyadic numbers, ordinary pivots powers of two: every partial
sum the elimination forms is an exact double whatever the summation order (MFMA k-order, fp64 atomics, K-fusion, split-K), so the pivot
column j meets is exactly U0[j, j].  An EVENT column has a chosen pivot value (zero, -0.0, 2^-40, +-thresh, complex corner cases) and no
coupling to the right of its pivot (U0[j, j+1:] = 0), but dyadic entries below it: the elimination scales them by the reciprocal of the
pivot it USES (the replacement, when the pivot was replaced), so L[i, j] = L0[i, j] * value / pivot used is an exact number the tests
check, while column j's Schur contribution L[:, j] U[j, j+1:] stays zero and every other pivot stays exact and known.

A pivot arrives by one of three routes: (i) on B's diagonal (nothing updates it), (ii) by elimination inside its own diagonal block
(L0[j, k] U0[k, j] != 0 for k < j in the same supernode), (iii) by the Schur update of a descendant supernode (k in a child block).
"""
import numpy as np

THRESH = 2.0 ** -20                  # the tiny-pivot threshold the tests pass (a power of two: the replaced pivots are exact)
TINY = 2.0 ** -40                    # far below THRESH


class Block:
    def __init__(self, width, children=()):
        self.width, self.children = int(width), list(children)


def _postorder(root):
    out = []

    def walk(b, anc):
        for c in b.children:
            walk(c, anc + [b])
        out.append((b, anc))
    walk(root, [])
    return out


def tree_pattern(root):
    """n, the dense boolean pattern (n x n) of the block tree with its columns in postorder, and (first column, width) of every block."""
    order = _postorder(root)
    col0 = {}
    c = 0
    for b, _ in order:
        col0[id(b)] = c
        c += b.width
    n = c
    P = np.zeros((n, n), dtype=bool)
    blocks = []
    for b, anc in order:
        s = col0[id(b)]
        P[s:s + b.width, s:s + b.width] = True
        for a in anc:
            t = col0[id(a)]
            P[s:s + b.width, t:t + a.width] = True
            P[t:t + a.width, s:s + b.width] = True
        blocks.append((s, b.width))
    return n, P, blocks


class Case:
    """B = L0 U0 on a block tree with pivot events: (global column j, pivot value, source column k < j or None).  k = None: the pivot stands on
    B's diagonal (route i); otherwise L0[j, k] = U0[k, j] = 1 and B[j, j] = value + 1, so the pivot arrives by the update from column k --
    route ii when k lies in j's supernode, iii when in another one (decided against the symbolic result: Case.route)."""

    def __init__(self, name, root, events, complex16=False, relax=1, maxsup=256, seed=0, density=0.05, expect=None):
        self.name, self.z, self.relax, self.maxsup, self.expect = name, complex16, relax, maxsup, expect or {}
        self.n, self.P, self.blocks = tree_pattern(root)
        n = self.n
        rng = np.random.default_rng(seed)
        dt = np.complex128 if complex16 else np.float64
        mask = self.P & (rng.random((n, n)) < density)
        vals = rng.choice([-0.25, 0.25, 0.5, -0.5], size=(n, n))
        if complex16:
            vals = vals + 1j * rng.choice([-0.25, 0.25, 0.0], size=(n, n))
        L0 = np.where(np.tril(mask, -1), vals, 0).astype(dt) + np.eye(n, dtype=dt)
        U0 = np.where(np.triu(mask, 1), vals.T, 0).astype(dt)
        piv = rng.choice([2.0, -2.0, 4.0, -4.0], size=n).astype(dt)
        if complex16:
            piv = piv * rng.choice([1.0, 1j, 1 + 1j, 1 - 1j], size=n)
        U0[np.arange(n), np.arange(n)] = piv
        cols = [int(e[0]) for e in events]
        assert len(set(cols)) == len(cols)
        below = self.P & np.tril(rng.random((n, n)) < 0.3, -1)
        for j, val, k in events:
            U0[j, j + 1:] = 0                                       # decoupled to the right ...
            L0[j + 1:, j] = np.where(below[j + 1:, j], vals[j + 1:, j], 0)   # ... coupled below: the scaling by the pivot is observed
            L0[j, :j] = 0; U0[:j, j] = 0
        for j, val, k in events:
            U0[j, j] = val
            if k is not None:
                assert k < j and k not in cols and self.P[j, k]
                L0[j, k] = 1; U0[k, j] = 1
        self.events = [(int(j), val, k) for j, val, k in events]
        self.L0, self.U0 = L0, U0
        self.B = L0 @ U0                                            # exact: dyadic entries, short sums
        assert np.all(self.B[~self.P] == 0)
        for j, val, k in self.events:                               # B carries the event on its diagonal only on route (i)
            assert (self.B[j, j] == val) == (k is None)
            if k is not None:
                assert self.B[j, j] - 1 == val                      # ... and the elimination recovers it exactly

    def route(self, j, xsup):
        k = dict((e[0], e[2]) for e in self.events)[j]
        if k is None:
            return "diag"
        sn = np.searchsorted(xsup, [j, k], side="right") - 1
        return "block" if sn[0] == sn[1] else "schur"

    # ---- inputs for the library ----
    def csr(self):
        """B as CSR on its full (filled) pattern, explicit zeros kept: the symbolic factorisation must see the tree, not B's accidental zeros."""
        rows, cols = np.nonzero(self.P)
        rp = np.zeros(self.n + 1, dtype=np.int32)
        np.add.at(rp, rows + 1, 1)
        rp = np.cumsum(rp).astype(np.int32)
        return self.n, rp, cols.astype(np.int32), self.B[rows, cols].copy()

    def tiny_cols(self, replace_tiny, thresh=THRESH):
        """0-based columns whose pivot the reference's rule replaces"""
        out = []
        for j, val, _ in self.events:
            if not replace_tiny:
                continue
            if self.z:
                if abs(val.real) + abs(val.imag) < thresh and val.real != 0 and val.imag != 0:
                    out.append(j)
            elif abs(val) < thresh:
                out.append(j)
        return sorted(out)

    def zero_cols(self, replace_tiny, thresh=THRESH):
        """0-based columns left with an exact zero pivot (info)"""
        tiny = set(self.tiny_cols(replace_tiny, thresh))
        return sorted(j for j, val, _ in self.events if val == 0 and j not in tiny)

    def expected_L(self, replace_tiny, thresh=THRESH):
        """L after the factorisation (no zero pivot left): L0, with the column of every replaced pivot scaled by value / replacement"""
        L = self.L0.copy()
        d = self.expected_diag(replace_tiny, thresh)
        for j in self.tiny_cols(replace_tiny, thresh):
            L[j + 1:, j] *= self.U0[j, j] / d[j]
        return L

    def expected_diag(self, replace_tiny, thresh=THRESH):
        """U's diagonal after the factorisation: U0's, with the replaced pivots at (sign) thresh"""
        d = np.diag(self.U0).copy()
        for j in self.tiny_cols(replace_tiny, thresh):
            re = d[j].real if self.z else d[j]
            d[j] = -thresh if re < 0 else thresh
        return d


def store_positions(fs):
    """(row, col) of every entry of a flat 1 x 1 x 1 store's Lnzval and Unzval (layout: oracle/slu_oracle.c)"""
    xs = fs.xsup
    ns = len(xs) - 1
    lr = np.full(len(fs.Lnzval), -1, dtype=np.int64); lc = lr.copy()
    ur = np.full(len(fs.Unzval), -1, dtype=np.int64); uc = ur.copy()
    for k in range(ns):
        f, w = int(xs[k]), int(xs[k + 1] - xs[k])
        o = int(fs.Lrowind_off[k])
        if fs.Lrowind_off[k + 1] > o:
            nb, lda = int(fs.Lrowind[o]), int(fs.Lrowind[o + 1])
            p = o + 2
            rows = []
            for _ in range(nb):
                nr = int(fs.Lrowind[p + 1]); rows += fs.Lrowind[p + 2:p + 2 + nr].tolist(); p += 2 + nr
            assert len(rows) == lda
            base = int(fs.Lnzval_off[k])
            for c in range(w):
                lr[base + c * lda:base + (c + 1) * lda] = rows
                lc[base + c * lda:base + (c + 1) * lda] = f + c
        o = int(fs.Ufstnz_off[k])
        if fs.Ufstnz_off[k + 1] > o:
            nb = int(fs.Ufstnz[o]); p = o + 3
            base = int(fs.Unzval_off[k])
            for _ in range(nb):
                gid = int(fs.Ufstnz[p]); gf, gw = int(xs[gid]), int(xs[gid + 1] - xs[gid])
                fst = fs.Ufstnz[p + 2:p + 2 + gw]
                for c in range(gw):
                    seg = int(f + w - fst[c])
                    ur[base:base + seg] = np.arange(int(fst[c]), f + w); uc[base:base + seg] = gf + c
                    base += seg
                p += 2 + gw
    return (lr, lc), (ur, uc)


def dense_factors(fs, pos=None):
    """L (unit diagonal implied: the store's diagonal is U's) and U of a factored flat store as dense arrays"""
    (lr, lc), (ur, uc) = pos or store_positions(fs)
    n = fs.n
    dt = fs.Lnzval.dtype
    L = np.zeros((n, n), dtype=dt); U = np.zeros((n, n), dtype=dt)
    m = lr >= 0
    below = m & (lr > lc)
    L[lr[below], lc[below]] = fs.Lnzval[below]
    on = m & (lr <= lc)
    U[lr[on], lc[on]] = fs.Lnzval[on]
    mu = ur >= 0
    U[ur[mu], uc[mu]] = fs.Unzval[mu]
    return L + np.eye(n, dtype=dt), U


# ------------------------------------------------------------------------------------------------------------------------------------------
# The cases.  Library rules they rely on (sluamd_dsymbfact): an etree subtree of at most `relax` columns is one relaxed supernode, and a
# chain of columns continues into its parent block -- so every block with children gets a last child of two columns (a relaxed "guard"
# leaf) that keeps it from merging with its last real child.  Each case states the supernode partition (xsup) and the levels
# ((supernodes, widest) per DAG level, plan_table columns 2 and 3) it expects; the tests assert both, so that the dispatch branch every
# event runs through is proved, not assumed.
#   double diag_lu:   widest <= 64 -> k_diag_lu_wave;  > 64 and ONE supernode at the top of the tree -> k_diag_lu2<1>;  otherwise
#                     (two or more wide supernodes, or SLUAMD_DIAG_TAIL=0) -> k_diag_lu2<2>
#   complex zdiag_lu: widest <= 8 / 16 / 32 -> kz_diag_lu_wave_small<8|16|32>;  <= 64 -> kz_diag_lu_wave;  > 64 -> kz_diag_lu
# ------------------------------------------------------------------------------------------------------------------------------------------
T, H = TINY, THRESH
ZT = complex(T, T)


def _g():
    return Block(2)


def _ra():      # leaves of 64 (wave), two separators of 100 (a level of two wide supernodes), a top separator of 200 (single wide level)
    return Block(200, [Block(100, [Block(64), Block(64), _g()]), Block(100, [Block(64), Block(64), _g()]), _g()])


def _rb():      # one 300-column supernode over two leaves: refined into pieces of 160 and 140 columns inside the library
    return Block(300, [Block(64), Block(64), _g()])


def _rc():      # a 512-column separator with maxsup 256: a chain of two 256-column supernodes, K-fused
    return Block(512, [Block(64), Block(64), _g()])


def _za():      # complex: leaves of 8, separators of 16, top of 32
    return Block(32, [Block(16, [Block(8), Block(8), _g()]), Block(16, [Block(8), Block(8), _g()]), _g()])


def _zb():      # complex: leaves of 64 (kz_diag_lu_wave), top of 150 (kz_diag_lu)
    return Block(150, [Block(64), Block(64), _g()])


def _zc():      # complex: one 300-column supernode (refined)
    return Block(300, [Block(64), Block(64), _g()])


SPECS = {
    # name: (tree, complex16, relax, maxsup, events (column, value, source or None), xsup, levels, DAG level of every column range)
    "ra": (_ra, False, 64, 256,
           [(1, -T, None), (31, 0.0, 2), (32, -0.0, None), (33, H, 3), (63, -H, 4), (64, T, None), (127, 0.0, 65),
            (130, -T, 10), (131, 0.0, 70), (161, T, 135), (162, -0.0, None), (163, H, 20), (193, -T, 136), (194, 0.0, 137), (229, -H, 100),
            (360, 0.0, 240), (392, T, 361),
            (462, T, 140), (463, 0.0, 370), (493, -T, None), (494, H, 470), (495, 0.0, 471), (525, -0.0, None), (526, -T, 300),
            (589, T, 473), (590, 0.0, 50), (661, -H, 474)],
           [0, 64, 128, 130, 230, 294, 358, 360, 460, 462, 662], [(7, 64), (2, 100), (1, 200)], [(0, 130, 0), (130, 230, 1), (230, 360, 0), (360, 460, 1), (460, 462, 0), (462, 662, 2)]),
    "rb": (_rb, False, 64, 300,
           [(5, T, None), (70, 0.0, 66), (130, -T, 20), (131, 0.0, None), (257, T, 140), (258, 0.0, 141), (289, -H, None), (290, -T, 142),
            (291, 0.0, 100), (386, T, 143), (387, -0.0, None), (400, -T, 150), (410, 0.0, 151), (429, H, 152)],
           [0, 64, 128, 130, 430], [(3, 64), (1, 160), (1, 140)], [(0, 130, 0), (130, 290, 1), (290, 430, 2)]),
    "rc": (_rc, False, 64, 256,
           [(10, 0.0, 3), (200, T, 131), (201, 0.0, None), (385, -T, 132), (386, T, 133), (387, 0.0, 134), (391, -T, 137),
            (600, 0.0, 138), (641, -0.0, 139)],
           [0, 64, 128, 130, 386, 642], [(3, 64), (1, 256), (1, 256)], [(0, 130, 0), (130, 386, 1), (386, 642, 2)]),
    "za": (_za, True, 8, 256,
           [(0, ZT, None), (1, complex(-T, T), None), (7, complex(T, 0), 3), (9, complex(0, T), None), (15, 0j, 10),
            (18, complex(-T, T), 5), (19, 0j, None), (33, ZT, 20), (52, complex(T, 0), 40), (67, complex(-H / 2, H / 2), None),
            (70, complex(0, T), 30), (71, ZT, 72 - 60), (101, 0j, 75), (100, complex(-T, -T), None)],
           [0, 8, 16, 18, 34, 42, 50, 52, 68, 70, 102], [(7, 8), (2, 16), (1, 32)], [(0, 18, 0), (18, 34, 1), (34, 52, 0), (52, 68, 1), (68, 70, 0), (70, 102, 2)]),
    "zb": (_zb, True, 64, 256,
           [(0, complex(T, 0), None), (1, ZT, None), (31, 0j, 3), (32, complex(-T, T), 2), (33, complex(0, T), 4), (63, complex(H / 2, H / 2), 5),
            (64, 0j, None), (127, ZT, 66),
            (130, ZT, 6), (131, 0j, 67), (161, complex(-T, T), 140), (162, complex(T, 0), None), (163, 0j, 141), (193, complex(0, -T), 142),
            (194, ZT, 143), (257, complex(-T, -T), 70), (258, 0j, 144), (279, complex(T, -T), None)],
           [0, 64, 128, 130, 280], [(3, 64), (1, 150)], [(0, 130, 0), (130, 280, 1)]),
    "zc": (_zc, True, 64, 300,
           [(130, complex(-T, T), 7), (131, 0j, None), (257, ZT, 140), (258, 0j, 141), (386, complex(T, 0), 142), (387, 0j, 143),
            (388, complex(T, -T), None), (429, ZT, 144)],
           [0, 64, 128, 130, 430], [(3, 64), (1, 160), (1, 140)], [(0, 130, 0), (130, 290, 1), (290, 430, 2)]),
}


def level_of(name, j):
    for c0, c1, lv in SPECS[name][7]:
        if c0 <= j < c1:
            return lv
    raise AssertionError(j)


def make(name, zero_level=None, repair=False):
    """The case `name`.  zero_level = l: the exact-zero events outside DAG level l become ordinary pivots (the zero-pivot tests look at one
    dispatch branch at a time); repair=True: every exact-zero event becomes an ordinary pivot (same pattern, same other values)."""
    tree, z, relax, maxsup, events, xsup, levels, ranges = SPECS[name]
    ev = []
    for j, val, k in events:
        if val == 0 and (repair or (zero_level is not None and level_of(name, j) != zero_level)):
            val = 2.0 + 0j if z else 2.0
        ev.append((j, complex(val) if z else val, k))
    return Case(name, tree(), ev, complex16=z, relax=relax, maxsup=maxsup, seed=len(name) + sum(map(ord, name)),
                expect=dict(xsup=xsup, levels=levels, ranges=ranges))
