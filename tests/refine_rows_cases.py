"""Batch refinement runs that reach every branch of the shared residual row (test helper for test_gpu_refine_rows.py and test_refine_rows_cases_cpu.py; not
a conftest): a structurally EMPTY row of op(A) (t == 0, q = 0), a row in the SAFE1 branch (0 < t <= safe2) and rows above safe2, in batches whose waves span
several matrices and whose last wave is partial -- m = 3 x count = 30 (21 matrices to a wave) and m = 65 x count = 2 -- for double and complex16 and
op = N, T, C.  The single-matrix forms reach the same branches in refine_exact_cases.py / refine_trans_cases.py; batches had no empty row.

A case.  The factors are diag(d_k), d signed powers of two (times a unit of the Gaussian integers for complex16); the attached block k is
A'_k = diag(d_k) (I + N_k / 256), N_k a nilpotent chain, so x <- x + D^-1 (b - op(A') x) ends at the exact solution after at most three steps.  The SPECIAL
matrices (every third one) carry two rows of their own, J1 and J2, both without a diagonal entry:
    A'[J1, c] = s_c 2^-1000 for the columns c of COLS,     A'[c, J2] = s'_c 2^-1000 for the rows c of COLS,     row J2 and column J1 empty.
op = N: row J1 of A' holds entries and a right-hand side of the order 2^-1000 (SAFE1 branch in every pass), row J2 is empty and b_J2 = 0 (t == 0); x_J2 = 0
for ever, so column J2 adds exact zeros to the rows of COLS.  op = T / C: the same with J1 and J2 exchanged (row J2 of A'^T is column J2 of A').  b at the
SAFE1 row is sum_c op(a) x*_c for the exact solution x*, so its residual dies with the chains and the run ends on the SAFE1 floor q = safe1 / t.

`predict` replays the loop of sluamd_refine.h per matrix in float64 numpy, with SAFE1 from m; `verify` repeats it in Fractions and asserts that every term of
every row of every pass is an exact double and that t, which bounds every partial sum of r's parts and of t itself in ANY order, stays below 2^53 / 64 units
of the lowest set bit of any term -- so any summation order and any multiply-add contraction give the same doubles, and X, berr and steps are compared
bitwise.  |r| and t being exact, q is the IEEE quotient, (safe1 + |r|) / t in that order in the middle branch."""
import functools
from fractions import Fraction
import numpy as np
import zbatch_cases as zc

EPS, SAFMIN = zc.EPS, zc.SAFMIN
SHAPES = {"m3x30": (3, 30), "m65x2": (65, 2)}
FORMS = [(False, "N"), (False, "T"), (True, "N"), (True, "T"), (True, "C")]        # (complex16, op); double with op = C is the T form
SPECIAL = {"m3x30": dict(J1=0, J2=1, COLS=(2,)), "m65x2": dict(J1=64, J2=0, COLS=(10, 20))}   # m65x2: J2 in the wave that spans both matrices, J1 the last global row
NRHS = 2


def is_special(name, k):
    return k % 3 == 1


@functools.lru_cache(maxsize=None)
def case(name, z, trans):
    """(m, count, d [count, m], A' [count, m, m], b [count, m, NRHS]) for the system op(A'_k) x = b_k"""
    m, count = SHAPES[name]
    sp = SPECIAL[name]
    J1, J2, COLS = sp["J1"], sp["J2"], sp["COLS"]
    rng = np.random.default_rng(101 + 2 * len(name) + int(z))
    vt = np.complex128 if z else np.float64
    d = rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], size=(count, m)).astype(vt)
    if z:
        d = d * rng.choice(zc.UNITS, size=(count, m))
    A = np.zeros((count, m, m), dtype=vt)
    b = rng.integers(1, 8, size=(count, m, NRHS)).astype(vt)
    if z:
        b = b + 1j * rng.integers(-3, 4, size=(count, m, NRHS))
    b[:, :, 0] *= 2.0
    for k in range(count):
        N = np.zeros((m, m), dtype=vt)
        for i in range(m - 1):
            if i % 4 != 3 and (k % 3 != 0 or i % 2 == 0) and not (is_special(name, k) and {i, i + 1} & {J1, J2}):
                N[i, i + 1] = rng.choice(zc.UNITS) if z else rng.choice([-1.0, 1.0])
        A[k] = np.diag(d[k]) @ (np.eye(m) + N / 256.0)
        if not is_special(name, k):
            continue
        A[k][[J1, J2], :] = 0; A[k][:, [J1, J2]] = 0
        for n_, c in enumerate(COLS):
            g = zc.UNITS[(k + n_) % 4] if z else 1.0
            A[k][J1, c] = (2 * n_ + 1) * g * 2.0 ** -1000
            A[k][c, J2] = -(n_ + 2) * g * 2.0 ** -1000
        safe_row, empty_row = (J1, J2) if trans == "N" else (J2, J1)
        b[k][[J1, J2], :] = 0
        Ao = zc.op(A[k], trans)
        fo = d[k].conj() if trans == "C" else d[k]
        for j in range(NRHS):                                                                # x*: the fixed point of the rows that have a diagonal
            x = b[k][:, j] / fo
            for _ in range(4):
                x = x + (b[k][:, j] - Ao @ x) / fo
            assert not (b[k][:, j] - Ao @ x)[[i for i in range(m) if i != safe_row]].any()
            b[k][safe_row, j] = Ao[safe_row] @ x
            assert b[k][safe_row, j] != 0 and b[k][empty_row, j] == 0
    for a in (d, A, b):
        a.setflags(write=False)
    return m, count, d, A, b


def rows_of(name, trans):
    """(SAFE1 row, empty row) of op(A') inside a special matrix"""
    sp = SPECIAL[name]
    return (sp["J1"], sp["J2"]) if trans == "N" else (sp["J2"], sp["J1"])


def replay(d, A, b, trans, safe_n):
    """The loop on one matrix and one right-hand side in float64: (x, berr, steps, census) -- census: per pass, the rows with t == 0, in the SAFE1 branch and
    above safe2"""
    Ao, fo = zc.op(A, trans), (d.conj() if trans == "C" else d)
    safe1 = (safe_n + 1) * SAFMIN; safe2 = safe1 / EPS
    x = b / fo
    lstres, steps, census = 3.0, 0, []
    while True:
        r = b - Ao @ x
        t = zc.abs1(Ao) @ zc.abs1(x) + zc.abs1(b)
        big = t > safe2
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(big, zc.abs1(r) / t, np.where(t != 0.0, (safe1 + zc.abs1(r)) / t, 0.0))
        census.append((np.flatnonzero(t == 0.0), np.flatnonzero((t != 0.0) & ~big), np.flatnonzero(big)))
        berr = q.max()
        if not (berr > EPS and berr * 2 <= lstres and steps < 20):
            return x, berr, steps, census
        x = x + r / fo
        lstres = berr
        steps += 1


@functools.lru_cache(maxsize=None)
def predict(name, z, trans):
    """(x [count, m, NRHS], berr [count, NRHS], steps [count] of the last right-hand side, census[k][j])"""
    m, count, d, A, b = case(name, z, trans)
    x = np.zeros_like(b); berr = np.zeros((count, NRHS)); steps = np.zeros(count, dtype=np.int32); census = []
    for k in range(count):
        census.append([])
        for j in range(NRHS):
            x[k][:, j], berr[k, j], steps[k], cs = replay(d[k], A[k], b[k][:, j], trans, m)
            census[k].append(cs)
    return x, berr, steps, census


# ---- the same in Fractions ----
def _f(v):
    return Fraction(float(v))


def _isd(f):
    return f == 0 or (Fraction(float(f)) == f and abs(f) >= Fraction(1, 2 ** 1074))


def _lowbit(f):
    p = abs(f.numerator)
    return Fraction(p & -p, f.denominator)


def verify(name, z, trans):
    """Replays every matrix in exact arithmetic; asserts the bounds of the module docstring and that the float64 replay gave the same X, |r|, t and steps"""
    m, count, d, A, b = case(name, z, trans)
    xe, berr_e, steps_e, _ = predict(name, z, trans)
    for k in range(count):
        Ao, fo = zc.op(A[k], trans), (d[k].conj() if trans == "C" else d[k])
        rows = [[(c, _f(Ao[i, c].real), _f(Ao[i, c].imag)) for c in np.flatnonzero(Ao[i])] for i in range(m)]
        for j in range(NRHS):
            bj = [(_f(v.real), _f(v.imag)) for v in b[k][:, j]]
            x = [(_f(v.real), _f(v.imag)) for v in b[k][:, j] / fo]
            for i in range(m):                                                                # x0 = b / d exactly
                dr, di = _f(fo[i].real), _f(fo[i].imag)
                assert x[i][0] * dr - x[i][1] * di == bj[i][0] and x[i][0] * di + x[i][1] * dr == bj[i][1]
            lstres, steps = 3.0, 0
            safe1 = (m + 1) * SAFMIN; safe2 = safe1 / EPS
            while True:
                r, qs = [], []
                for i in range(m):
                    terms, t = [bj[i][0], bj[i][1]], abs(bj[i][0]) + abs(bj[i][1])
                    axr = axi = Fraction(0)
                    for c, ar, ai in rows[i]:
                        xr, xi = x[c]
                        terms += [ar * xr, ai * xi, ar * xi, ai * xr, (abs(ar) + abs(ai)) * (abs(xr) + abs(xi))]
                        assert _isd(abs(ar) + abs(ai)) and _isd(abs(xr) + abs(xi))
                        axr += ar * xr - ai * xi; axi += ar * xi + ai * xr
                        t += (abs(ar) + abs(ai)) * (abs(xr) + abs(xi))
                    rr, ri = bj[i][0] - axr, bj[i][1] - axi
                    nz = [v for v in terms if v != 0]
                    assert all(_isd(v) for v in nz + [rr, ri, t, abs(rr) + abs(ri)])
                    if nz:
                        assert t / min(_lowbit(v) for v in nz) < 2 ** 53 // 64, (name, z, trans, k, j, i)
                    r.append((rr, ri))
                    ar_, tf = float(abs(rr) + abs(ri)), float(t)
                    qs.append(ar_ / tf if tf > safe2 else (safe1 + ar_) / tf if tf != 0.0 else 0.0)
                berr = max(qs)
                if not (berr > EPS and berr * 2 <= lstres and steps < 20):
                    break
                for i in range(m):                                                            # dx = r / d: d is a unit times a power of two
                    dr, di = _f(fo[i].real), _f(fo[i].imag)
                    n2 = dr * dr + di * di
                    dxr, dxi = (r[i][0] * dr + r[i][1] * di) / n2, (r[i][1] * dr - r[i][0] * di) / n2
                    x[i] = (x[i][0] + dxr, x[i][1] + dxi)
                    assert _isd(dxr) and _isd(dxi) and _isd(x[i][0]) and _isd(x[i][1])
                lstres = berr
                steps += 1
            assert berr == berr_e[k, j] and (j < NRHS - 1 or steps == steps_e[k])
            assert all(float(x[i][0]) == xe[k][i, j].real and float(x[i][1]) == xe[k][i, j].imag for i in range(m))
