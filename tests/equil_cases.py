"""Equilibration test helper (test_equil_cases_cpu.py, test_gpu_equil.py; not a conftest): our own numpy restatement of the reference's
pdgsequ + pdlaqgs and the case matrices of the tests.

Restated (every operation is one IEEE double operation, so a device that follows the same statements returns the same bits):
  pdgsequ (SRC/double/pdgsequ.c)
    :126-127  smlnum = dmach("S") = 2^-1022, bignum = 1 / smlnum
    :130-138  r[i] = max_j |a_ij|          complex16: abs1(z) = |re| + |im| (pzgsequ.c:136)
    :141-156  rcmin = min(bignum, min r), rcmax = max(0, max r), amax = rcmax
    :158-164  rcmin == 0: info = (first i with r[i] == 0) + 1, return (c, rowcnd, colcnd not computed: reported as 0 here)
    :167-170  r[i] = 1 / min(max(r[i], smlnum), bignum); rowcnd = max(rcmin, smlnum) / min(rcmax, bignum)
    :174-185  c[j] = max_i |a_ij| * r[i]   (pzgsequ.c:182: abs1)
    :195-208  rcmin / rcmax of c; rcmin == 0: info = n + (first j with c[j] == 0) + 1, return (colcnd reported as 0)
    :211-214  c[j] = 1 / min(max(c[j], smlnum), bignum); colcnd likewise
  pdlaqgs (SRC/double/pdlaqgs.c)
    :89, :108-109  THRESH = 0.1, small = dmach("Safe minimum") / dmach("Precision") = 2^-1022 / 2^-52, large = 1 / small
    :111-125  rowcnd >= THRESH and small <= amax <= large: colcnd >= THRESH -> 'N', else a *= c[j] -> 'C'
    :126-134  else colcnd >= THRESH: a *= r[i] -> 'R'
    :135-145  else a = (a * r[i]) * c[j] -> 'B'   (C evaluates a * r * c left to right; the library keeps this order for complex16 too,
              where pzlaqgs.c:141 forms r[i] * c[j] first)
When info > 0 nothing is scaled and equed = 'N' (pdgssvx3d.c:700-716 applies pdlaqgs only when iinfo == 0).
R and C are reported as all ones where that side is not applied (what LUHandle.scalings returns)."""
import numpy as np

SMLNUM = 2.0 ** -1022
BIGNUM = 1.0 / SMLNUM
THRESH = 0.1
SMALL = SMLNUM / 2.0 ** -52
LARGE = 1.0 / SMALL


def abs1(v):
    return np.abs(v.real) + np.abs(v.imag) if np.iscomplexobj(v) else np.abs(v)


def rows_of(n, rowptr):
    return np.repeat(np.arange(n), np.diff(np.asarray(rowptr)))


def equilibrate(n, rowptr, colind, vals):
    """dict(equed, info, rowcnd, colcnd, amax, R, C, vals (scaled copy), r_raw / c_raw (the scalings pdgsequ computed, None if not reached))"""
    rows, cols = rows_of(n, rowptr), np.asarray(colind)
    vals = np.asarray(vals)
    a = abs1(vals)
    out = dict(equed="N", info=0, rowcnd=0.0, colcnd=0.0, amax=0.0, R=np.ones(n), C=np.ones(n), vals=vals.copy(), r_raw=None, c_raw=None)
    with np.errstate(over="ignore", under="ignore"):
        r = np.zeros(n)
        np.maximum.at(r, rows, a)
        rcmin, rcmax = min(BIGNUM, float(r.min())), max(0.0, float(r.max()))
        out["amax"] = rcmax
        if rcmin == 0.0:
            out["info"] = int(np.flatnonzero(r == 0.0)[0]) + 1
            return out
        r = 1.0 / np.minimum(np.maximum(r, SMLNUM), BIGNUM)
        out["rowcnd"] = max(rcmin, SMLNUM) / min(rcmax, BIGNUM)
        out["r_raw"] = r
        c = np.zeros(n)
        np.maximum.at(c, cols, a * r[rows])
        rcmin, rcmax = min(BIGNUM, float(c.min())), max(0.0, float(c.max()))
        if rcmin == 0.0:
            out["info"] = n + int(np.flatnonzero(c == 0.0)[0]) + 1
            return out
        c = 1.0 / np.minimum(np.maximum(c, SMLNUM), BIGNUM)
        out["colcnd"] = max(rcmin, SMLNUM) / min(rcmax, BIGNUM)
        out["c_raw"] = c
        if out["rowcnd"] >= THRESH and SMALL <= out["amax"] <= LARGE:
            if out["colcnd"] < THRESH:
                out.update(equed="C", C=c, vals=vals * c[cols])
        elif out["colcnd"] >= THRESH:
            out.update(equed="R", R=r, vals=vals * r[rows])
        else:
            out.update(equed="B", R=r, C=c, vals=(vals * r[rows]) * c[cols])
    return out


def anorm_exact(n, colind, vals):
    """(max column sum of the moduli, longest column), moduli and sums in extended precision (error k 2^-64, far below the bound under test)"""
    cols = np.asarray(colind)
    if np.iscomplexobj(vals):
        m = np.hypot(vals.real.astype(np.longdouble), vals.imag.astype(np.longdouble))
    else:
        m = np.abs(vals).astype(np.longdouble)
    sums = np.zeros(n, dtype=np.longdouble)
    np.add.at(sums, cols, m)
    return float(sums.max()), int(np.bincount(cols, minlength=n).max())


# ---- case matrices: (n, rowptr, colind, vals), CSR with ascending columns, the diagonal stored in every row unless the case says otherwise ----

def _csr(n, rows_cols, fill):
    rp = np.zeros(n + 1, dtype=np.int32)
    ci = []
    for i, cs in enumerate(rows_cols):
        cs = sorted(set(int(c) for c in cs))
        ci.extend(cs); rp[i + 1] = len(ci)
    ci = np.array(ci, dtype=np.int32)
    return n, rp, ci, fill(rows_of(n, rp), ci)


def pattern(n, k, seed, dense_row=None, dense_len=0):
    """k entries per row: the diagonal + k - 1 random other columns (k <= n); dense_row gets dense_len entries"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kk = min(dense_len if i == dense_row else k, n)
        others = rng.choice(np.delete(np.arange(n), i), size=kk - 1, replace=False) if kk > 1 else []
        out.append([i, *others])
    return out


def _mant(rng, m):
    """magnitudes in [0.5, 1) with random signs"""
    return rng.uniform(0.5, 1.0, m) * rng.choice([-1.0, 1.0], m)


def case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "n1":                       # one entry: rowcnd = colcnd = 1 -> N
        return _csr(1, [[0]], lambda r, c: np.array([-3.0]))
    if name == "diag63_R":                 # rows of 1 entry, magnitudes 2^-30 .. 2^30: rowcnd tiny, every column maximum 1 after the row scaling -> R
        return _csr(63, [[i] for i in range(63)], lambda r, c: _mant(rng, 63) * 2.0 ** rng.integers(-30, 31, 63))
    if name == "rows7_64_N":               # well scaled, 7 entries per row -> N
        return _csr(64, pattern(64, 7, 1), lambda r, c: _mant(rng, len(r)))
    if name == "dense65_B":                # dense rows of 65 entries (64 lanes per row), rows and columns scaled by 2^+-20 -> B
        rs, cs = 2.0 ** rng.integers(-20, 21, 65), 2.0 ** rng.integers(-20, 21, 65)
        return _csr(65, pattern(65, 65, 2), lambda r, c: _mant(rng, len(r)) * rs[r] * cs[c])
    if name == "neg257_C":                 # all-negative rows of 7 entries; every fifth column scaled by 2^-10, its own diagonal row aside every row keeps a full-size entry -> C
        cs = np.where(np.arange(257) % 5 == 0, 2.0 ** -10, 1.0)
        pat = pattern(257, 7, 3)
        for i, row in enumerate(pat):
            if all(c % 5 == 0 for c in row):
                row.append((i + 1) if (i + 1) % 5 else (i + 2))
        return _csr(257, pat, lambda r, c: -np.abs(_mant(rng, len(r))) * cs[c])
    if name == "clamp1030":                # rows of 7 and one dense row of 300; a row of 1e-320 entries (below smlnum), a row holding 1.5e308 (above bignum), 1e300 elsewhere
        def fill(r, c):
            v = _mant(rng, len(r)) * np.where(c % 7 == 3, 2.0 ** -20, 1.0)      # (small columns: colcnd < 0.1 -> B)
            v[r == 5] = 1e-320 * np.sign(v[r == 5])
            v[(r == 9) & (c == 9)] = -1.5e308
            v[(r == 11) & (c == 11)] = 1e300
            return v
        return _csr(1030, pattern(1030, 7, 4, dense_row=700, dense_len=300), fill)
    if name == "tiny_amax_R":              # every entry ~ 2^-1000: amax < small forces the row branch although rowcnd >= 0.1
        return _csr(64, pattern(64, 7, 5), lambda r, c: _mant(rng, len(r)) * 2.0 ** -1000)
    if name == "huge_amax_R":              # every entry ~ 2^1000: amax > large
        return _csr(65, pattern(65, 7, 6), lambda r, c: _mant(rng, len(r)) * 2.0 ** 1000)
    if name == "zero_row":                 # row 40: only -0.0 and 0.0 stored; row 77 empty; row 200 zero too: info = 41
        pat = pattern(257, 7, 7); pat[77] = []

        def fill(r, c):
            v = _mant(rng, len(r))
            k = np.flatnonzero(r == 40); v[k] = 0.0; v[k[::2]] = -0.0
            v[r == 200] = 0.0
            return v
        return _csr(257, pat, fill)
    if name == "empty_row0":               # the empty row is row 0 of a matrix of rows of 1 entry
        return _csr(63, [[]] + [[i] for i in range(1, 63)], lambda r, c: _mant(rng, len(r)))
    if name == "zero_col":                 # no entry in column 30; column 12 holds explicit zeros only; every row keeps a nonzero: info = n + 13
        pat = [[c for c in row if c != 30] for row in pattern(64, 7, 8)]
        pat[30] = [c for c in pat[30]] or [31]
        for row in pat:
            if len(row) < 2:
                row.append(33)

        def fill(r, c):
            v = _mant(rng, len(r)); v[c == 12] = 0.0
            return v
        return _csr(64, pat, fill)
    if name == "z_abs1":                   # complex16: in row 0, 3+4i (abs1 7, modulus 5) against 6 (abs1 6, modulus 6); scaled rows and columns -> B
        rs, cs = 2.0 ** rng.integers(-20, 21, 65), 2.0 ** rng.integers(-20, 21, 65)

        def fill(r, c):
            v = (_mant(rng, len(r)) + 1j * _mant(rng, len(r))) * 0.25
            k = np.flatnonzero(r == 0)
            v = v * rs[r] * cs[c]
            v[k] = 0.01 * rs[0]; v[k[0]] = (3 + 4j) * rs[0]; v[k[1]] = 6.0 * rs[0]
            return v
        return _csr(65, pattern(65, 7, 9), fill)
    if name == "z_rows1_R":                # complex16 rows of 1 entry
        return _csr(63, [[i] for i in range(63)], lambda r, c: (_mant(rng, 63) + 1j * _mant(rng, 63)) * 2.0 ** rng.integers(-30, 31, 63))
    if name == "z_dense64_C":              # complex16, 64 lanes per row, columns scaled
        cs = np.where(np.arange(64) % 4 == 0, 2.0 ** -12, 1.0)
        return _csr(64, pattern(64, 64, 10), lambda r, c: (_mant(rng, len(r)) + 1j * _mant(rng, len(r))) * cs[c])
    raise KeyError(name)


EXPECT = {   # name -> (equed, info)
    "n1": ("N", 0), "diag63_R": ("R", 0), "rows7_64_N": ("N", 0), "dense65_B": ("B", 0), "neg257_C": ("C", 0), "clamp1030": ("B", 0),
    "tiny_amax_R": ("R", 0), "huge_amax_R": ("R", 0), "zero_row": ("N", 41), "empty_row0": ("N", 1), "zero_col": ("N", 64 + 13),
    "z_abs1": ("B", 0), "z_rows1_R": ("R", 0), "z_dense64_C": ("C", 0),
}


# ---- end-to-end systems: a diagonally dominant operator under row / column scalings by powers of two ----

def scaled_operator(N=6, mode="a", z=False, seed=0):
    """(n, rowptr, colind, vals, perm, rs, cs): unsymmetric stencil operator of matgen (diagonally dominant) with row scalings rs and column scalings cs.
    mode "a": 2^+-40 on rows and columns at random; mode "b": rows alternating 2^520 / 2^-520 (A and b stay finite, amax inside [small, large])."""
    from superlu_dist_amd import matgen
    n, rp, ci, v = matgen.stencil3d_unsym(N, seed=seed)
    perm = matgen.nd_perm_grid3d(N, N, N, leaf=27)
    rng = np.random.default_rng(100 + seed)
    if z:
        v = matgen.complex_shift(v, rp, ci, seed=seed)
    if mode == "a":
        rs, cs = 2.0 ** rng.choice([-40, 40], n), 2.0 ** rng.choice([-40, 40], n)
    else:
        rs, cs = 2.0 ** np.where(np.arange(n) % 2 == 0, 520, -520), np.ones(n)
    rows = rows_of(n, rp)
    return n, rp, ci, (v * rs[rows]) * cs[ci], perm, rs, cs
