"""The extra-precise residual and refinement loop restated in Python (test helper for test_gpu_xresidual.py, test_gpu_xrefine.py and
test_xrefine_cases_cpu.py; not a conftest).

The accumulation of k_xrfs_residual (sluamd_xkernels.inc), per part of the residual and per entry in the row's stored order, from s = b_i, c = 0:
    p = a * x (rounded);  pe = a x - p (exact: fractions.Fraction);  (s, se) = TwoSum(s, -p) in IEEE doubles;  c = c + (se - pe);  at the end r_i = s + c
complex16: the real part takes + a.x x.x then - a.y x.y, the imaginary part + a.x x.y then + a.y x.x, each part with its own (s, c).  Python's float IS the IEEE
double and pe is always a double (absent underflow), so `xrow` is bitwise what the kernel computes for ANY data.  The weight t = sum |a||x| + |b_i| (abs1)
is restated with one rounded product and one rounded sum per entry; the compiler may fuse that pair, so the cases keep every such product exact or first
in its row (asserted by `check_case`), where both forms give the same double.

The stored order: the CSR's for trans = "N"; for "T" / "C" the transposed index lists a row of op(A) by ascending column (sluamd_trefine.cpp).  A case is
written as M = op(A); `attached` returns the CSR of the A to attach.

The loop of sluamd_xrefine.cpp (`xsimulate`), per column, with ndx = max abs1(dx), nx = max abs1(x) before the update:
    residual -> berr;  count == 20: LIMIT;  dx = solve;  ndx == 0: CONVERGED;  count > 0 and 2 ndx > prev: NO_PROGRESS (dx dropped);  x += dx;  ++count;
    count > 1: rho = max(rho, ndx / prev);  ndx <= eps nx: closing residual, CONVERGED;  prev = ndx
on the exact factors of refine_exact_cases (`perm`, `diag_store`, `dvals`, `_solve`: imported, not copied): the correction of a "diag" handle is an exact
scaling, that of a sweep kind is exact under the bounds `_solve` asserts; x + dx is asserted representable, so the trajectory is known bitwise."""
import ctypes as C
import functools
import os
from fractions import Fraction
import numpy as np
import refine_exact_cases as rx

EPS, SAFMIN, ITMAX = rx.EPS, rx.SAFMIN, rx.ITMAX
ORDERS, MAXPOS, SWEEPS = rx.ORDERS, rx.MAXPOS, rx.SWEEPS
CONVERGED, NO_PROGRESS, LIMIT = 0, 1, 2
TRANS = {False: ("N", "T"), True: ("N", "T", "C")}
U30 = 1.0 + 2.0 ** -30                                # (1 + 2^-30)^2 needs 61 bits: a product that is not a double


# ---------------------------------------------------------------------------------------------------------------------------------------
# the accumulation
# ---------------------------------------------------------------------------------------------------------------------------------------
def two_sum(a, b):
    s = a + b
    bb = s - a
    aa = s - bb
    return s, (a - aa) + (b - bb)


def sub_prod(s, c, a, x):
    """(s, c) -= a x"""
    p = a * x
    pe = Fraction(a) * Fraction(x) - Fraction(p)
    assert Fraction(float(pe)) == pe                                                         # (no underflow in the cases)
    s, se = two_sum(s, -p)
    return s, c + (se - float(pe))


def xrow(entries, b, z):
    """r_i of the kernel, bitwise: entries = [(a, x)] in the stored order, a = op(a) already"""
    if not z:
        s, c = float(b), 0.0
        for a, x in entries:
            s, c = sub_prod(s, c, float(a), float(x))
        return s + c
    b = complex(b)
    sr, cr, si, ci = b.real, 0.0, b.imag, 0.0
    for a, x in entries:
        a, x = complex(a), complex(x)
        sr, cr = sub_prod(sr, cr, a.real, x.real)
        sr, cr = sub_prod(sr, cr, -a.imag, x.imag)
        si, ci = sub_prod(si, ci, a.real, x.imag)
        si, ci = sub_prod(si, ci, a.imag, x.real)
    return complex(sr + cr, si + ci)


def plain_row(entries, b, z):
    """the fp64 pass in the same order, one rounding per operation (rfs_row without fused multiply-adds)"""
    if not z:
        acc = 0.0
        for a, x in entries:
            acc += float(a) * float(x)
        return float(b) - acc
    ar = ai = 0.0
    for a, x in entries:
        a, x = complex(a), complex(x)
        ar += a.real * x.real - a.imag * x.imag
        ai += a.real * x.imag + a.imag * x.real
    return complex(complex(b).real - ar, complex(b).imag - ai)


def exact_row(entries, b, z):
    """b - sum a x in rational arithmetic: (re, im) Fractions"""
    b = complex(b)
    re, im = Fraction(b.real), Fraction(b.imag)
    for a, x in entries:
        a, x = complex(a), complex(x)
        ar, ai, xr, xi = Fraction(a.real), Fraction(a.imag), Fraction(x.real), Fraction(x.imag)
        re -= ar * xr - ai * xi
        im -= ar * xi + ai * xr
    return re, im


def abs1(v):
    v = complex(v)
    return abs(v.real) + abs(v.imag)


def weight(entries, b):
    """t of the row: abs1 products in the stored order, |b_i| last"""
    t = 0.0
    for a, x in entries:
        t += abs1(a) * abs1(x)
    return t + abs1(b)


def quot(r, t, n):
    safe1 = (n + 1) * SAFMIN
    safe2 = safe1 / EPS
    if t > safe2:
        return abs1(r) / t
    if t != 0.0:
        return (safe1 + abs1(r)) / t
    return 0.0


def weight_is_order_free(entries):
    """every abs1 product but the first is exact, so a fused multiply-add and a product followed by a sum give the same t"""
    return all(Fraction(abs1(a)) * Fraction(abs1(x)) == Fraction(abs1(a) * abs1(x)) for a, x in entries[1:])


# ---------------------------------------------------------------------------------------------------------------------------------------
# one-pass cases: M = op(A) by rows, x, b
# ---------------------------------------------------------------------------------------------------------------------------------------
class XCase:
    def __init__(self, n, z, rows, b, x, max_row):
        self.n, self.z, self.rows, self.max_row = n, z, rows, max_row
        dt = np.complex128 if z else np.float64
        self.b, self.x = np.asarray(b, dtype=dt), np.asarray(x, dtype=dt)

    def kernel_rows(self, trans):
        """per row the (a, x_j) pairs in the order the kernel of `trans` meets them"""
        out = []
        for row in self.rows:
            if trans != "N":
                row = sorted(row, key=lambda e: e[0])
            out.append([(a, self.x[j]) for j, a in row])
        return out

    def attached(self, trans):
        """CSR (rowptr, colind, values) of the matrix to attach: M itself, its transpose, or its conjugate transpose"""
        return csr_of(self.n, self.rows, self.z, trans)

    @functools.lru_cache(maxsize=None)
    def expected(self, trans):
        rows = self.kernel_rows(trans)
        n, z = self.n, self.z
        dt = np.complex128 if z else np.float64
        rx_ = np.array([xrow(e, self.b[i], z) for i, e in enumerate(rows)], dtype=dt)
        rp_ = np.array([plain_row(e, self.b[i], z) for i, e in enumerate(rows)], dtype=dt)
        t = [weight(e, self.b[i]) for i, e in enumerate(rows)]
        qx, qp = [quot(rx_[i], t[i], n) for i in range(n)], [quot(rp_[i], t[i], n) for i in range(n)]
        return dict(extra=rx_, plain=rp_, berr_extra=max(qx), berr_plain=max(qp), q_extra=qx)


def csr_of(n, rows, z, trans):
    dt = np.complex128 if z else np.float64
    if trans == "N":
        lists = rows
    else:                                                   # A = M^T / M^H: row j of A takes (i, op(m_ij)), i ascending
        lists = [[] for _ in range(n)]
        for i, row in enumerate(rows):
            for j, a in row:
                lists[j].append((i, np.conj(a) if trans == "C" else a))
    rp = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int32)
    ci = np.array([j for r in lists for j, _ in r], dtype=np.int32)
    av = np.array([a for r in lists for _, a in r], dtype=dt)
    return rp, ci, av


@functools.lru_cache(maxsize=None)
def xcase(n, z, m):
    """order n, the maximum q in row m.  Rows: one entry (the background), no entry, 70 entries in scrambled column order, the cancelling row
    2^60, 1, -2^60 over three equal x, and rows of ONE product that is not a double with b_i = its rounded value -- the fp64 pass returns 0 there, the doubled
    one the product's error, and a pass that contracted s - a x into one multiply-add returns twice that error"""
    g = (lambda re, im=0.0: complex(re, im)) if z else (lambda re, im=0.0: float(re))
    j = np.arange(n)
    x = [g(1 + (k // 3) % 3, 1 + (k // 3) % 2) for k in j]
    rows, b = [None] * n, [None] * n
    for i in range(n):                                      # background: r_i = 1 / 4
        a = g(1 + i % 7, (i % 5) - 2) * (-1) ** i
        rows[i] = [(i, a)]
        b[i] = a * x[i] + 0.25
    if n == 1:
        x[0] = g(U30, 1 + 2.0 ** -31)
        rows[0] = [(0, g(U30))]
        b[0] = g(U30 * x[0].real, U30 * x[0].imag) if z else U30 * U30
        return XCase(n, z, rows, b, x, 0)
    m = m % n
    assert n >= 63 and m not in (7, 11, 13, 14, 20)
    rows[7], b[7] = [], 0.0
    rows[11], b[11] = [(0, g(2.0 ** 60)), (1, g(1.0)), (2, g(-2.0 ** 60))], g(5, 3)
    x[13] = x[14] = g(U30, 1 + 2.0 ** -31)
    rows[13] = [(13, g(U30))]                                # complex16: a real: the first and third product of the four
    b[13] = g(U30 * x[13].real, U30 * x[13].imag) if z else U30 * U30
    if z:
        rows[14] = [(14, complex(0.0, U30))]                # a imaginary: the second and fourth
        b[14] = complex(-(U30 * x[14].imag), U30 * x[14].real)
    else:
        rows[14] = [(14, -U30)]
        b[14] = -(U30 * U30)
    cols = [int(c) for c in (np.arange(90) * 37 + 11) % n if c not in (13, 14)][:70]
    rows[20] = [(c, g(((k % 7) + 1) * (-1) ** k, (k % 3) - 1)) for k, c in enumerate(cols)]
    b[20] = sum(a * x[c] for c, a in rows[20]) + 1
    rows[m] = [(m, g(3, 1))]
    b[m] = g(3, 1) * x[m] + g(64, 64)
    return XCase(n, z, rows, b, x, m)


def xcase_list():
    """(n, m) of the one-pass cases: every order with the maximum in its last row, the two largest with it at every position of MAXPOS"""
    return [(n, -1) for n in ORDERS if n not in (257, 513)] + [(n, m) for n in (257, 513) for m in MAXPOS]


def check_case(c, trans):
    """what the GPU test relies on, from the data alone: the restatement returns the exact residual, t does not depend on fusing, the designated row
    holds the maximum alone, and the two passes differ"""
    rows = c.kernel_rows(trans)
    e = c.expected(trans)
    for i, ent in enumerate(rows):
        re, im = exact_row(ent, c.b[i], c.z)
        r = complex(e["extra"][i])
        assert Fraction(r.real) == re and Fraction(r.imag) == im, (c.n, trans, i)
        assert weight_is_order_free(ent), (c.n, trans, i)
    q = e["q_extra"]
    assert q[c.max_row] == e["berr_extra"] and sum(1 for v in q if v == e["berr_extra"]) == 1, (c.n, trans)
    assert not np.array_equal(e["extra"], e["plain"])
    lens = {len(r) for r in rows}
    assert (c.n == 1 or {0, 1, 3, 70} <= lens)


# ---------------------------------------------------------------------------------------------------------------------------------------
# handles and device memory
# ---------------------------------------------------------------------------------------------------------------------------------------
def factored(kind, n, z, **kw):
    """a handle holding the exact factors of a kind of refine_exact_cases (asserted)"""
    import trans_cases as tc
    from superlu_dist_amd import driver
    fs0, expL, expU = rx.diag_store(n, z) if kind == "diag" else tc.prepared(kind)[1:4]
    fs = driver.FlatStore(fs0.n, fs0.xsup, fs0.Lrowind_off, fs0.Lrowind.copy(), fs0.Lnzval_off, fs0.Lnzval.copy(), fs0.Ufstnz_off, fs0.Ufstnz, fs0.Unzval_off,
                          fs0.Unzval.copy())
    h = driver.LUHandle.from_store(fs, **kw)
    assert h.z == z and h.pdgstrf3d(0.0) == 0
    h.copy_to_host()
    assert np.array_equal(fs.Lnzval, expL) and np.array_equal(fs.Unzval, expU), kind
    return h


class Dev:
    """device memory through the HIP runtime itself (the library has initialised it; no second framework in the process)"""
    hip = None

    def __init__(self, a):
        if Dev.hip is None:
            Dev.hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.a = np.asfortranarray(a)
        self.ptr = C.c_void_p()
        assert Dev.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(max(self.a.nbytes, 8))) == 0
        assert Dev.hip.hipMemcpy(self.ptr, self.a.ctypes.data_as(C.c_void_p), C.c_size_t(self.a.nbytes), 1) == 0

    def host(self):
        out = np.empty_like(self.a, order="F")
        assert Dev.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        Dev.hip.hipFree(self.ptr)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------------
def _restated_pass(c, trans, xr, xi):
    """the extra pass of an RCase holding M = op(A), by the restatement: (r re, r im as Fractions, berr)"""
    n, z = c.n, c.z
    x = np.array([float(v) for v in xr]) + (1j * np.array([float(v) for v in xi]) if z else 0)
    rr, ri, qs = [], [], []
    for i in range(n):
        ent = [(int(c.ci[k]), c.av[k]) for k in range(c.rp[i], c.rp[i + 1])]
        if trans != "N":
            ent.sort(key=lambda e: e[0])
        ent = [(a, x[j]) for j, a in ent]
        assert weight_is_order_free(ent), (c.name, i)
        r = xrow(ent, c._b[i], z)
        qs.append(quot(r, weight(ent, c._b[i]), n))
        r = complex(r)
        rr.append(Fraction(r.real)); ri.append(Fraction(r.imag))
    return rr, ri, max(qs) if qs else 0.0


def _exact_pass(c, A, xr, xi, bints, eb):
    """the pass of a case whose rows meet the margin of refine_exact_cases._pass (asserted there): every partial sum of any order is an exact double, so the
    doubled accumulation returns the exact residual with c = 0, and t and q are the plain form's"""
    n = c.n
    xints, ex = rx._ints(xr + xi)
    rr, ri, q, _, _ = rx._pass(c, A, xints[:n], xints[n:], ex, bints[:n], bints[n:], eb, True)
    return rr, ri, max(q) if q else 0.0


def xsimulate(c, trans="N", exact=False):
    """the whole run of RCase c (c holds M = op(A); `attached(c, trans)` is what to attach): dict(X, berr, steps, state, dxrel, rho, ndx = the norms of every
    correction computed, per column).  exact=True: the residual by refine_exact_cases._pass (sweep kinds: 10^5 entries and more, all within its margin)"""
    n, z = c.n, c.z
    out = dict(X=np.zeros_like(c.X0), berr=np.zeros(c.nrhs), steps=[], state=[], dxrel=[], rho=[], ndx=[])
    A = None
    if exact:
        assert trans == "N" and not c.tight
        nnz = c.av.size
        i64, ea = rx._ints_np(np.concatenate([c.av.real, c.av.imag if z else np.zeros(nnz)]))
        assert i64 is not None
        A = (i64[:nnz].tolist(), i64[nnz:].tolist(), ea, (i64[:nnz], i64[nnz:]))
    for j in range(c.nrhs):
        c._b = c.B[:, j]
        br, bi = rx._frs(c.B[:, j])
        bints, eb = rx._ints(br + bi)
        xr, xi = rx._frs(c.X0[:, j])
        count, prev, rho, dxrel, ndxs = 0, float("inf"), 0.0, 0.0, []
        while True:
            rr, ri, berr = _exact_pass(c, A, xr, xi, bints, eb) if exact else _restated_pass(c, trans, xr, xi)
            if count == ITMAX:
                state = LIMIT
                break
            dr, di = rx._solve(c, rr, ri, True)
            assert all(rx._isdouble(v) for v in dr + di)
            ndx = max(float(abs(a)) + float(abs(b)) for a, b in zip(dr, di))
            nx = max(float(abs(a)) + float(abs(b)) for a, b in zip(xr, xi))
            ndxs.append(ndx)
            dxrel = 0.0 if ndx == 0.0 else ndx / nx
            if ndx == 0.0:
                state = CONVERGED
                break
            if count > 0 and 2 * ndx > prev:
                state = NO_PROGRESS
                break
            xr, xi = [a + b for a, b in zip(xr, dr)], [a + b for a, b in zip(xi, di)]
            assert all(rx._isdouble(v) for v in xr + xi), (c.name, j, count)
            count += 1
            if count > 1:
                rho = max(rho, ndx / prev)
            if ndx <= EPS * nx:
                rr, ri, berr = _exact_pass(c, A, xr, xi, bints, eb) if exact else _restated_pass(c, trans, xr, xi)
                state = CONVERGED
                break
            prev = ndx
        out["X"][:, j] = np.array([float(v) for v in xr]) + (1j * np.array([float(v) for v in xi]) if z else 0)
        out["berr"][j] = berr
        out["steps"].append(count); out["state"].append(state); out["dxrel"].append(dxrel); out["rho"].append(rho); out["ndx"].append(ndxs)
    return out


def attached(c, trans):
    """CSR to attach for an RCase that holds M = op(A)"""
    if trans == "N":
        return c.rp, c.ci, c.av
    rows = [[(int(c.ci[k]), c.av[k]) for k in range(c.rp[i], c.rp[i + 1])] for i in range(c.n)]
    return csr_of(c.n, rows, c.z, trans)


def _traj(z):
    """the trajectories on "diag" handles of order 65: name -> (RCase, trans, designed facts)"""
    n = 65
    out = {}
    p = "z_" if z else "d_"

    def half(D, i, col=None):                               # the error 2^20 of row i halves at every step (ratio exactly 1 / 2)
        D.half(i, D.zz(2.0 ** 21, i), 2.0 ** 20)

    def quarter(D, i, cols=slice(None)):                    # A'_ii = A_ii / 4: the error shrinks by 3 / 4 only
        xs = D.zz(2.0 ** 21, i)
        D.rows[i] = [(i, D.dp[i] / 4)]
        D.X[i, :] = xs; D.B[i, :] = D.dp[i] / 4 * xs
        D.X[i, cols] += 2.0 ** 20

    D = rx._Diag(n, z)
    half(D, 10)
    out[p + "limit"] = (D.case("x_limit"), "N", dict(state=[LIMIT], steps=[ITMAX], rho=[0.5]))
    D = rx._Diag(n, z)
    quarter(D, 10)
    out[p + "noprog"] = (D.case("x_noprog"), "N", dict(state=[NO_PROGRESS], steps=[1], rho=[0.0], dxrel_ratio=0.75))
    D = rx._Diag(n, z)                                      # nx = 2^52: the fifth correction, 2^-1, meets eps nx exactly
    D.half(10, D.zz(2.0 ** 21, 10), 2.0 ** 4)
    D.frozen(30, 2.0 ** 52)
    out[p + "eps"] = (D.case("x_eps"), "N", dict(state=[CONVERGED], steps=[5], rho=[0.5], last_ndx=0.5))
    D = rx._Diag(n, z)                                      # the factors are the attached matrix's: one correction, then dx == 0
    D.X[33, :] += 2.0 ** 10
    out[p + "zero"] = (D.case("x_zero"), "N", dict(state=[CONVERGED], steps=[1], rho=[0.0], dxrel=[0.0]))
    D = rx._Diag(n, z, nrhs=3)                              # three columns, three states
    D.half(10, D.zz(2.0 ** 21, 10), 0.0)
    D.X[10, 0] += 2.0 ** 20
    quarter(D, 20, cols=1)
    D.X[33, 2] += 2.0 ** 10
    out[p + "rhs3"] = (D.case("x_rhs3"), "N", dict(state=[LIMIT, NO_PROGRESS, CONVERGED], steps=[ITMAX, 1, 1]))
    D = rx._Diag(n, z)                                      # the transposed index: M has an entry off the diagonal over a frozen column
    half(D, 10)
    D.rows[10] = [(40, 3.0), (10, D.dp[10] / 2)]
    D.B[10, :] += 3.0 * D.X[40, 0]
    out[p + "trans"] = (D.case("x_trans"), "T", dict(state=[LIMIT], steps=[ITMAX], rho=[0.5]))
    return out


@functools.lru_cache(maxsize=None)
def trajectories():
    out = {}
    out.update(_traj(False)); out.update(_traj(True))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    c, trans, _ = trajectories()[name]
    return xsimulate(c, trans)


SWEEP_CASE = "sw_nil_narrow"                                # the nilpotent chain of refine_exact_cases through the real sweeps: three corrections, then dx == 0


@functools.lru_cache(maxsize=None)
def sweep_expected():
    return xsimulate(rx.cases()[SWEEP_CASE], "N", exact=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# one real factorisation: an integer matrix with cond_2 ~ 1e11
# ---------------------------------------------------------------------------------------------------------------------------------------
ILL_N = 100


@functools.lru_cache(maxsize=None)
def ill_case():
    """A = L U with L = I + (-1/3 | -2/3 below the diagonal) and U = 3 I + (-3 | -6 above it): A is a tridiagonal INTEGER matrix (entries up to 7), its
    factors are not doubles, and U^-1 doubles at every third column: cond_2 ~ 1e11 at n = 100.  No pivoting is needed (the pivots are 3).  x_true integer,
    b = A x_true exact.  Returns dict(n, rp, ci, av, A dense, x_true, b, cond)"""
    import scipy.sparse as sp
    n = ILL_N
    k = np.arange(n)
    sub = np.where(k[1:] % 2 == 0, -2.0, -1.0) / 3
    sup = np.where(k[1:] % 3 == 0, -6.0, -3.0)
    LU = (np.eye(n) + np.diag(sub, -1)) @ (3 * np.eye(n) + np.diag(sup, 1))
    Ad = np.round(LU)
    assert np.abs(Ad - LU).max() < 1e-9 and np.abs(Ad).max() <= 7
    A = sp.csr_matrix(Ad)
    A.sort_indices()
    x_true = ((7 * k + 3) % 19 - 9).astype(np.float64)
    x_true[x_true == 0] = 5.0
    b = Ad @ x_true
    assert np.all(np.abs(b) < 2 ** 20) and np.all(b == np.round(b))
    return dict(n=n, rp=A.indptr.astype(np.int32), ci=A.indices.astype(np.int32), av=A.data.astype(np.float64), A=Ad, x_true=x_true, b=b,
                cond=float(np.linalg.cond(Ad, 2)))


def _csr_rows(ic, x):
    return [[(ic["av"][k], x[ic["ci"][k]]) for k in range(ic["rp"][i], ic["rp"][i + 1])] for i in range(ic["n"])]


@functools.lru_cache(maxsize=None)
def ill_cpu_loops():
    """both loops on the CPU with a scipy LU and the restated residuals: dict(err_plain, err_extra, steps_plain, steps_extra, state, dxrel, rho), errors
    = max|x - x_true| / max|x_true|"""
    import scipy.linalg as sl
    ic = ill_case()
    n, b, xt = ic["n"], ic["b"], ic["x_true"]
    lu = sl.lu_factor(ic["A"])
    err = lambda x: float(np.abs(x - xt).max() / np.abs(xt).max())
    # the plain loop: the reference's rule on berr
    x = sl.lu_solve(lu, b)
    lstres, count = 3.0, 0
    while True:
        rows = _csr_rows(ic, x)
        r = np.array([plain_row(e, b[i], False) for i, e in enumerate(rows)])
        sv = max(quot(r[i], weight(e, b[i]), n) for i, e in enumerate(rows))
        if not (sv > EPS and sv * 2 <= lstres and count < ITMAX):
            break
        x = x + sl.lu_solve(lu, r)
        lstres = sv
        count += 1
    out = dict(err_plain=err(x), steps_plain=count)
    # the extra loop
    x = sl.lu_solve(lu, b)
    count, prev, rho, dxrel = 0, float("inf"), 0.0, 0.0
    while True:
        r = np.array([xrow(e, b[i], False) for i, e in enumerate(_csr_rows(ic, x))])
        if count == ITMAX:
            state = LIMIT
            break
        dx = sl.lu_solve(lu, r)
        ndx, nx = float(np.abs(dx).max()), float(np.abs(x).max())
        dxrel = 0.0 if ndx == 0.0 else ndx / nx
        if ndx == 0.0:
            state = CONVERGED
            break
        if count > 0 and 2 * ndx > prev:
            state = NO_PROGRESS
            break
        x = x + dx
        count += 1
        if count > 1:
            rho = max(rho, ndx / prev)
        if ndx <= EPS * nx:
            state = CONVERGED
            break
        prev = ndx
    out.update(err_extra=err(x), steps_extra=count, state=state, dxrel=dxrel, rho=rho)
    return out
