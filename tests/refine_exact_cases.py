"""Refinement runs whose whole trajectory is known EXACTLY (test helper for test_gpu_refine_exact.py and test_refine_exact_cases_cpu.py; not a conftest).

sluamd_[dz]AttachMatrix accepts any CSR matrix of the handle's order.  With a matrix A' that is NOT the factored one the handle iterates
    x <- x + Pc^T (L0 U0)^-1 Pc (b - A' x)
which need not converge; with dyadic data and exactly known factors every intermediate is an exact double, and `simulate` predicts berr of every pass, every
stop decision, the step count and the final X in Python integers.  The loop is the reference's (pdgsrfs.c:345-510, pzgsrfs.c:365-514, restated in
sluamd_refine.h):
    r = b - A' x;  t = sum |a||x| + |b|  (abs1(z) = |re| + |im| for complex16)
    q = |r| / t  if t > safe2;   (safe1 + |r|) / t  if 0 < t <= safe2;   0  if t == 0        safe1 = (n + 1) safmin, safe2 = safe1 / eps, eps = 2^-53
    berr = max q;   go on iff berr > eps and 2 berr <= lstres and count < 20   (lstres = 3 at first)

Factored systems.  kind "diag": F = diag(d), d signed powers of two (times a unit of the Gaussian integers for complex16), of any order n, stored through
driver.Symbolic / flat_store (`diag_store`); the correction is an exact scaling.  kind = a name of trans_cases.prepared ("narrow", "levels", "z_narrow",
"z_wide"): F = L0 U0 of that sweep case; the correction passes through the real sweeps.  The matrix the factors belong to is A = Pc^T F Pc, A[i, j] =
F[pc[i], pc[j]], with a perm_c that is neither the identity nor an involution (`perm`).

Bounds (asserted by `simulate`).  Every row of every pass: with all terms of the row -- the products re/im, the abs1 products, b_i -- written as integers in a
common unit, t < 2^53 / 64 in units of the lowest set bit of any term (t bounds every partial sum of r's parts and of t itself in ANY order; 64 is the margin
factor of the other helpers), nothing below 2^-1074.  Rows named in `tight` are exempt from the margin: the eps boundary needs t / |r| = 2^53, so no margin can
exist; for them the partial sums in the order every implementation uses (entries in CSR order, b_i last) are checked representable one by one -- they have two
entries.  The corrections: kind "diag" divides by a power of two (checked representable); the sweep kinds assert the two bounds of sweep_cases.SweepCase.rhs,
|Linv| (|b| + |L0| |y|) and |Uinv| (|y| + |U0| |x|) through aL, aU, aLi, aUi, with the margin 64, on the exact z = F^-1 Pc r (verified in integers:
L4 U4 z == 16 Pc r).  x + dx is checked representable.  So any summation order, FMA contraction and the atomics of the sweeps give the same doubles.

|r| and t being exact doubles, the expected q is the IEEE quotient (Python's float division), in the middle branch (safe1 + |r|) / t in that order."""
import functools
from fractions import Fraction
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -53
SAFMIN = 2.0 ** -1022
assert SAFMIN == 2.2250738585072014e-308
ITMAX = 20
LIMIT = 2 ** 53
MARGIN = 64
ORDERS = (1, 63, 64, 65, 255, 256, 257, 513)
MAXPOS = (5, 71, 137, 255, -1, 0)                  # the four waves of the first workgroup, the last row, row 0
SWEEPS = ("narrow", "levels", "z_narrow", "z_wide")
P53 = float(2 ** 53)


# ---------------------------------------------------------------------------------------------------------------------------------------
# integers
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tz(v):
    return (v & -v).bit_length() - 1


def _rep(v, e):
    """|v| 2^e is an exact double"""
    v = abs(v)
    if v == 0:
        return True
    z = _tz(v)
    return v.bit_length() - z <= 53 and e + z >= -1074 and e + v.bit_length() <= 1024


def _ints(fr):
    """list of dyadic Fractions -> (integers, e): fr[k] = integers[k] 2^e"""
    den = max((f.denominator for f in fr), default=1)
    assert den & (den - 1) == 0
    out = [f.numerator * (den // f.denominator) for f in fr]
    g = 0
    for v in out:
        g |= abs(v)
    s = _tz(g) if g else 0
    return [v >> s for v in out], s - (den.bit_length() - 1)


def _ints_np(a):
    """_ints of a float64 array in int64 where the integers fit: (int64 array, e), or (None, None)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    nz = a[a != 0]
    if nz.size == 0:
        return np.zeros(a.shape, dtype=np.int64), 0
    m, ex = np.frexp(nz)
    I = np.abs(np.ldexp(m, 53)).astype(np.int64)                                            # the 53-bit significands, exact
    tz = np.log2((I & -I).astype(np.float64)).astype(np.int64)
    e = int((ex.astype(np.int64) - 53 + tz).min())
    with np.errstate(over="ignore"):
        v = np.ldexp(a, -e)
    if not np.all(np.abs(v) < 2.0 ** 62):
        return None, None
    return v.astype(np.int64), e


def _flt(v, e):
    return float(Fraction(v) * Fraction(2) ** e)


def _frs(a):
    a = np.asarray(a)
    return [Fraction(float(v)) for v in a.real], [Fraction(float(v)) for v in (a.imag if np.iscomplexobj(a) else np.zeros(a.shape))]


def _isdouble(f):
    ints, e = _ints([f])
    return _rep(ints[0], e)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
class RCase:
    def __init__(self, name, kind, z, pc, A, B, X0, d=None, tight=(), expect=None, max_row=None):
        A = sp.csr_matrix(A) if not isinstance(A, tuple) else A
        self.name, self.kind, self.z, self.pc = name, kind, z, np.ascontiguousarray(pc, dtype=np.int32)
        if isinstance(A, tuple):
            self.rp, self.ci, self.av = A
        else:
            self.rp, self.ci, self.av = A.indptr, A.indices, A.data
        vt = np.complex128 if z else np.float64
        self.rp, self.ci, self.av = np.ascontiguousarray(self.rp, dtype=np.int32), np.ascontiguousarray(self.ci, dtype=np.int32), np.ascontiguousarray(self.av, dtype=vt)
        self.B, self.X0 = np.asfortranarray(np.asarray(B, dtype=vt).reshape(len(pc), -1)), np.asfortranarray(np.asarray(X0, dtype=vt).reshape(len(pc), -1))
        self.n, self.nrhs = len(pc), self.B.shape[1]
        self.d, self.tight = d, frozenset(tight)
        self.expect = expect or {}                 # designed facts, asserted by the CPU test from the simulator alone
        self.max_row = max_row                     # the row meant to hold the maximum q of the last pass of the last column

    def __repr__(self):
        return self.name


def perm(n):
    """perm_c[old] = new: a rotation by 1 + n // 3 -- neither the identity nor its own inverse for n >= 3"""
    return ((np.arange(n) + 1 + n // 3) % n).astype(np.int32)


def dvals(n, z):
    """the diagonal factor: +-2^(-2 .. 2), times a unit of the Gaussian integers for complex16"""
    k = np.arange(n)
    d = np.ldexp(1.0, (k % 5) - 2) * np.where((k // 3) % 2 == 0, 1.0, -1.0)
    return d * np.array([1, 1j, -1, -1j])[(k // 7) % 4] if z else d


@functools.lru_cache(maxsize=None)
def diag_store(n, z):
    """(flat store holding diag(dvals(n, z)), the same values as the expected factors): n supernodes of one column, through the symbolic path"""
    import pivot_cases as pcs
    from superlu_dist_amd import driver
    rp, ci = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=64, unsym=True)
    fs = symb.flat_store(values=False)
    symb.free()
    (lr, lc), (ur, uc) = pcs.store_positions(fs)
    assert np.all(lr >= 0) and np.array_equal(lr, lc) and sorted(lr.tolist()) == list(range(n)) and not np.any(ur >= 0)
    d = dvals(n, z)
    if z:
        fs.Lnzval, fs.Unzval, fs.z = fs.Lnzval.astype(np.complex128), fs.Unzval.astype(np.complex128), True
        fs._build_view()
    fs.Lnzval[:] = d[lr]
    return fs, fs.Lnzval.copy(), fs.Unzval.copy()


class _Diag:
    """rows of a kind-"diag" case: every row starts `frozen` (A'_ii = A_ii, b_i = A_ii x_i: r_i = 0 for ever)"""

    def __init__(self, n, z, nrhs=1):
        self.n, self.z, self.pc, self.d = n, z, perm(n), dvals(n, z)
        self.dp = self.d[self.pc]                                                            # A_ii = d[pc[i]]
        vt = np.complex128 if z else np.float64
        self.rows = [None] * n
        self.B, self.X = np.zeros((n, nrhs), dtype=vt), np.zeros((n, nrhs), dtype=vt)
        self.tight = set()
        for i in range(n):
            self.frozen(i, self.zz(3 + (7 * i) % 11, i))

    def zz(self, v, i=0):
        """complex16: an imaginary part of another magnitude, never zero"""
        return v + 1j * (v // 8 + 1 + i % 3) if self.z else v

    def frozen(self, i, x):
        self.rows[i] = [(i, self.dp[i])]
        self.X[i, :] = x; self.B[i, :] = self.dp[i] * np.asarray(x)

    def stall(self, i, x0, delta):
        """A'_ii = 2 A_ii, b_i = A_ii (2 x0 + delta): x1 = x0 + delta, r1 = -r0 -- the second pass does not halve and its q is returned"""
        self.rows[i] = [(i, 2 * self.dp[i])]
        self.X[i, :] = x0; self.B[i, :] = self.dp[i] * (2 * x0 + delta)

    def half(self, i, c, e):
        """A'_ii = A_ii / 2, b_i = A_ii c, x0 = 2 c + e: the error e halves exactly at every step"""
        self.rows[i] = [(i, self.dp[i] / 2)]
        self.X[i, :] = 2 * c + e; self.B[i, :] = self.dp[i] * c

    def off(self, i, entries, rho, x0=0):
        """a row without its own column over frozen columns: r_i = rho for ever (b_i = sum a x + rho)"""
        self.rows[i] = list(entries)
        self.X[i, :] = x0
        self.B[i, :] = sum(a * self.X[j, 0] for j, a in entries) + np.asarray(rho)

    def background(self, skip=()):
        for i in range(self.n):
            if i not in skip:
                self.stall(i, self.zz(2 ** 20 + 3 * i, i), self.zz(1, i))

    def case(self, name, **kw):
        rp = np.concatenate([[0], np.cumsum([len(r) for r in self.rows])])
        ci = np.array([j for r in self.rows for j, _ in r], dtype=np.int32)
        av = np.array([a for r in self.rows for _, a in r], dtype=np.complex128 if self.z else np.float64)
        return RCase(("z_" if self.z else "d_") + name, "diag", self.z, self.pc, (rp, ci, av), self.B, self.X, d=self.d, tight=self.tight, **kw)


def _diag_cases(z):
    out = []
    g = 1j if z else 1.0
    # orders and the position of the maximum: every row stalls, the designated row with eight times the residual
    for n, rows in [(n, (-1,)) for n in ORDERS if n not in (257, 513)] + [(257, MAXPOS), (513, MAXPOS)]:
        for m in rows:
            m = m % n
            D = _Diag(n, z)
            D.background()
            D.stall(m, D.zz(2 ** 20 + 3 * m, m), D.zz(8, m))
            out.append(D.case(f"max_n{n}_r{m}", max_row=m, expect=dict(steps=[1], strict_max=True)))
    # row lengths: a row of 300 entries in scrambled column order over frozen columns holds the maximum; rows of 0 (b_i = 0: t == 0), 1 and 2 entries
    n = 513
    D = _Diag(n, z)
    m, empty = 400, 17
    cols = [int(j) for j in (np.arange(303) * 37 + 11) % n if j not in (m, empty)][:300]
    assert len(set(cols)) == len(cols) == 300
    D.background(skip=set(cols) | {m, empty})
    free = [i for i in range(n) if i not in cols and i not in (m, empty)]
    for k, i in enumerate((free[3], free[80], free[-2])):                                   # two entries, the off-diagonal one first or last
        j = cols[5 * k]
        D.rows[i] = [(j, 3.0 * g), (i, D.dp[i])] if k % 2 == 0 else [(i, D.dp[i]), (j, 3.0 * g)]
        D.X[i, :] = D.zz(40 + k, i); D.B[i, :] = D.dp[i] * D.X[i, 0] + 3.0 * g * D.X[j, 0] + 1
    D.rows[empty] = []; D.X[empty, :] = 0; D.B[empty, :] = 0
    D.off(m, [(j, ((k % 7) + 1) * (-1) ** k * (g if k % 3 == 0 else 1.0)) for k, j in enumerate(cols)], D.zz(5, m))
    out.append(D.case("rows_long", max_row=m, expect=dict(steps=[2], lengths=(0, 1, 2, 300), zero_t_row=empty)))
    # the last entry of the row is the only one that matters (the others meet x_j = 0)
    D = _Diag(65, z)
    m = 40
    D.background(skip={m, 3, 9, 12, 20, 50})
    for j in (3, 9, 12, 20):
        D.frozen(j, 0)
    D.frozen(50, D.zz(9, 50))
    D.off(m, [(3, 5.0), (9, -2.0 * g), (12, 7.0), (20, 1.0), (50, 3.0 * g)], D.zz(2, m))
    out.append(D.case("rows_last", max_row=m, expect=dict(steps=[1])))
    # an empty row with b_i != 0: t = |b_i|, q = 1
    D = _Diag(64, z)
    D.background(skip={21})
    D.rows[21] = []; D.X[21, :] = 0; D.B[21, :] = D.zz(5, 21)
    out.append(D.case("empty_b", max_row=21, expect=dict(steps=[1], berr=[1.0])))
    # SAFE1 / SAFE2
    for n in (5, 65):
        D = _Diag(n, z)
        D.rows[2] = []; D.X[2, :] = 0; D.B[2, :] = SAFMIN * g
        out.append(D.case(f"safe1_stop_n{n}", max_row=2, expect=dict(steps=[0], berr=[float(n + 2)], untouched=True, branch=2)))
    D = _Diag(5, z)
    D.rows[2] = []; D.X[2, :] = 0; D.B[2, :] = 8 * SAFMIN * g
    out.append(D.case("safe_mid_stop", max_row=2, expect=dict(steps=[0], berr=[1.75], untouched=True, branch=2)))
    D = _Diag(5, z)
    D.X[2, :] = 2.0 ** -1000 * g; D.B[2, :] = D.dp[2] * 3 * 2.0 ** -1000 * g
    out.append(D.case("safe_mid_run", max_row=2, expect=dict(steps=[2], branch=2)))
    u = 2.0 ** -969                                                                         # safe2 = 6 u at n = 5
    m = 2
    for name, extra in (("safe2_eq", 0.0), ("safe2_above", 2.0 ** -1013)):                  # a row over a frozen column: the same t and q in every pass, so the LAST pass sits on safe2
        D = _Diag(5, z)
        D.frozen(0, 4 * u * g)
        D.rows[m] = [(0, 1.0)]; D.X[m, :] = 0; D.B[m, :] = (2 * u + extra) * g
        out.append(D.case(name, max_row=m, expect=dict(steps=[1], first_t=6 * u + extra, first_branch=2 if extra == 0 else 1)))
    # the eps boundary: r = 2 (stop, berr == eps) and r = 4 (goes on) over t = 2^54
    for name, p1, p2, ex in (("eps_stop", P53 - 1, P53 - 1, dict(steps=[0], berr=[EPS], untouched=True)), ("eps_go", P53 - 2, P53, dict(steps=[1], berr=[2 * EPS]))):
        D = _Diag(5, z)
        D.frozen(0, p1); D.frozen(3, p2)
        D.rows[2] = [(0, g), (3, -g)]; D.X[2, :] = 0; D.B[2, :] = 2 * g
        D.tight = {0, 2, 3}
        out.append(D.case(name, max_row=2, expect=dict(first_t=2.0 ** 54, **ex)))
    # the halving boundary
    for name in ("half_long", "half_go", "half_stop"):
        D = _Diag(65, z)
        c = D.zz(2.0 ** 21, 16)
        e = 2.0 ** 20
        k, k2, m, f = 10, 30, 45, 52
        D.half(k, c, e)
        if name != "half_stop":                                                             # (half_stop: row k alone, t_k = 2 |c| + |e| / 2 shrinks with e and the second q falls just short of half)
            D.half(k2, c, -e)                                                                # x_k = 2 c + e, x_k2 = 2 c - e: t_m = 4 |c| for ever, r_m = -2 g e halves exactly
            D.rows[m] = [(k, g), (k2, -g)]; D.X[m, :] = 0; D.B[m, :] = 0
        if name == "half_go":
            D.frozen(7, D.zz(8, 7))
            D.off(f, [(7, 3.0)], D.zz(2, f) / 4)                                          # a constant q that ends the run
        ex = dict(half_long=dict(steps=[ITMAX], halves=ITMAX), half_go=dict(halves=3), half_stop=dict(steps=[1], short_of_half=True))[name]
        out.append(D.case(name, max_row=dict(half_long=m, half_go=f, half_stop=k)[name], expect=ex))
    # nilpotent: A' = A (I + N), N a chain of three nodes scaled by 2^-8; x0 is off by 2^16 at the end of the chain
    D = _Diag(65, z)
    a0, a1, a2, nu = 8, 44, 23, 2.0 ** -8
    xs = D.X[:, 0].copy()
    xs[[a0, a1, a2]] = [D.zz(768, 1), D.zz(-1280, 2), D.zz(512, 3)]
    for i, j in ((a0, a1), (a1, a2)):
        D.rows[i] = [(j, D.dp[i] * nu), (i, D.dp[i])]
        D.B[i, :] = D.dp[i] * (xs[i] + nu * xs[j])
    D.B[a2, :] = D.dp[a2] * xs[a2]
    D.X[:, 0] = xs; D.X[a2, 0] += 2.0 ** 16
    out.append(D.case("nilpotent", expect=dict(steps=[3], berr=[0.0], final=xs.reshape(-1, 1))))
    # three right-hand sides taking 0, 2 and 1 steps: SAFE1 stop; a wrong x0 at one row over a constant row; the constant row alone
    D = _Diag(65, z, nrhs=3)
    m, f, a = 2, 52, 33
    D.rows[m] = []; D.X[m, :] = 0; D.B[m, :] = [SAFMIN * g, 0, 0]
    D.frozen(7, D.zz(8, 7))
    D.off(f, [(7, 3.0)], [0, D.zz(2, f) / 64, D.zz(3, f) / 16])
    D.X[a, 1] += 2.0 ** 10
    out.append(D.case("rhs3", max_row=f, expect=dict(steps=[0, 2, 1], nonzero_berr=True, zero_t_row=m)))
    return out


def _sweep_cases(name):
    """A' = A M on the factors of sweep case `name`, b = A c: x <- c + (I - M) x in integers"""
    import trans_cases as tc
    sc_ = tc.prepared(name)[0]
    n, z = sc_.n, sc_.z
    pc = perm(n)
    A16 = sc_.B16.tocsr()[pc, :][:, pc].tocsr()                                             # 16 A, A[i, j] = F[pc[i], pc[j]]
    assert (A16 != (sc_.L4 @ sc_.U4).tocsr()[pc, :][:, pc]).nnz == 0
    vt = np.complex128 if z else np.float64
    i = np.arange(n)
    xs = (((3 * i + 7) % 11) - 5).astype(vt)
    if z:
        xs = xs + 1j * (((5 * i + 1) % 7) - 3)
    out = []
    a0, a1, a2, m = n // 7, n // 2 + 1, n // 3, n // 5
    # nilpotent chain
    N = sp.csr_matrix(([2.0 ** -8, 2.0 ** -8], ([a0, a1], [a1, a2])), shape=(n, n), dtype=vt)
    M = sp.identity(n, dtype=vt, format="csr") + N
    Ap = (A16.astype(vt) @ M).tocsr() / 16
    Ap.eliminate_zeros()
    xs1 = xs.copy(); xs1[[a1, a2]] *= 256                                                    # N x stays an integer vector
    b = (A16.astype(vt) @ (M @ xs1)) / 16
    x0 = xs1.copy(); x0[a2] += 2.0 ** 16
    out.append(RCase(f"sw_nil_{name}", name, z, pc, Ap, b, x0, expect=dict(steps=[3], berr=[0.0], final=xs1.reshape(-1, 1))))
    # three right-hand sides: M = I - e_m e_m^T (column m of A' is empty: x_m never enters, r = c_m A e_m is constant)
    M = sp.identity(n, dtype=vt, format="lil"); M[m, m] = 0; M = M.tocsr(); M.eliminate_zeros()
    Ap = (A16.astype(vt) @ M).tocsr() / 16
    Ap.eliminate_zeros()
    C = np.stack([xs, xs[::-1], np.roll(xs, 3)], axis=1).astype(vt)
    C[m, :] = [0, 1 / 64, 1 / 16]
    if z:
        C[m, :] *= (1 + 2j)
    B = (A16.astype(vt) @ C) / 16
    X0 = C.copy(); X0[a0, 1] += 2.0 ** 10
    out.append(RCase(f"sw_rhs3_{name}", name, z, pc, Ap, B, X0, expect=dict(steps=[0, 2, 1], nonzero_berr=True)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _diag_cases(False) + _diag_cases(True)
    for name in SWEEPS:
        out += _sweep_cases(name)
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


def names(kind=None, z=None):
    return [k for k, c in cases().items() if (kind is None or (c.kind == "diag") == (kind == "diag")) and (z is None or c.z == z)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the simulator
# ---------------------------------------------------------------------------------------------------------------------------------------
def _row_sums_int64(c, A64, xr, xi, sa):
    """the row sums of _pass (re, im, t, the OR of all terms) in int64 where nothing can overflow; None otherwise (the caller then loops in Python integers)"""
    n = c.n
    if A64 is None or A64[0].size == 0:
        return None
    ar, ai = A64
    ma, mx = int(max(np.abs(ar).max(), np.abs(ai).max())), max((abs(v) for v in xr + xi), default=0)
    if (4 * ma * mx << sa) * max(1, int(np.diff(c.rp).max())) >= 2 ** 62:
        return None
    xr, xi = (np.array(v, dtype=np.int64) for v in (xr, xi))
    j, row = c.ci, np.repeat(np.arange(n), np.diff(c.rp))
    p1, p2, p3, p4 = (ar * xr[j]) << sa, (ai * xi[j]) << sa, (ar * xi[j]) << sa, (ai * xr[j]) << sa
    tt = ((np.abs(ar) + np.abs(ai)) * (np.abs(xr[j]) + np.abs(xi[j]))) << sa
    out = [np.zeros(n, dtype=np.int64) for _ in range(4)]
    np.add.at(out[0], row, p1 - p2); np.add.at(out[1], row, p3 + p4); np.add.at(out[2], row, tt)
    np.bitwise_or.at(out[3], row, np.abs(p1) | np.abs(p2) | np.abs(p3) | np.abs(p4) | tt)
    return out


def _pass(c, A, xr, xi, ex, br, bi, eb, check):
    """one residual pass in integers: (r as Fractions (re, im), q, branch, t) per row"""
    ar, ai, ea, A64 = A
    n = c.n
    e = min(ea + ex, eb)
    sa, sb = ea + ex - e, eb - e
    safe1 = (n + 1) * SAFMIN
    safe2 = safe1 / EPS
    rp, ci = c.rp.tolist(), c.ci.tolist()
    two = Fraction(2) ** e
    rr_, ri_, q_, br_, t_ = [], [], [], [], []
    fast = None if c.tight else _row_sums_int64(c, A64, xr, xi, sa)
    for i in range(n):
        sr = si = t = bits = 0
        tight = i in c.tight
        if fast:
            sr, si, t, bits = (int(v[i]) for v in fast)
        for k in (() if fast else range(rp[i], rp[i + 1])):
            j = ci[k]
            p1, p2, p3, p4 = (ar[k] * xr[j]) << sa, (ai[k] * xi[j]) << sa, (ar[k] * xi[j]) << sa, (ai[k] * xr[j]) << sa
            tt = ((abs(ar[k]) + abs(ai[k])) * (abs(xr[j]) + abs(xi[j]))) << sa
            bits |= abs(p1) | abs(p2) | abs(p3) | abs(p4) | tt
            if tight and check:
                assert _rep(sr + p1, e) and _rep(si + p3, e), (c.name, i)
            sr += p1 - p2; si += p3 + p4; t += tt
            if tight and check:
                assert _rep(sr, e) and _rep(si, e) and _rep(t, e) and _rep(tt, e), (c.name, i)
        bR, bI = br[i] << sb, bi[i] << sb
        rr, ri = bR - sr, bI - si
        t += abs(bR) + abs(bI)
        bits |= abs(bR) | abs(bI)
        av = abs(rr) + abs(ri)
        if check:
            if tight:
                assert _rep(rr, e) and _rep(ri, e) and _rep(t, e) and _rep(av, e), (c.name, i)
            elif bits:
                assert t * MARGIN < LIMIT * (bits & -bits), (c.name, "row", i, "t in units of the last place: 2^%.1f" % np.log2(t / (bits & -bits)))
                assert e + _tz(bits) >= -1074 and e + t.bit_length() <= 1024, (c.name, i)
        tf, af = _flt(t, e), _flt(av, e)
        if tf > safe2:
            q, branch = af / tf, 1
        elif tf != 0.0:
            q, branch = (safe1 + af) / tf, 2
        else:
            q, branch = 0.0, 0
        rr_.append(rr * two); ri_.append(ri * two); q_.append(q); br_.append(branch); t_.append(tf)
    return rr_, ri_, q_, br_, t_


@functools.lru_cache(maxsize=None)
def _triangles(kind):
    """rows of L4 (strictly lower) and U4 (strictly upper, and the diagonal) of a sweep case as Python integers"""
    import trans_cases as tc
    s = tc.prepared(kind)[0]
    L, U = s.L4.tocsr(), s.U4.tocsr()
    L.sort_indices(); U.sort_indices()
    lo, up, dg = [], [], []
    for i in range(s.n):
        a, b = L.indptr[i], L.indptr[i + 1]
        lo.append([(int(j), int(v.real), int(v.imag)) for j, v in zip(L.indices[a:b], L.data[a:b].astype(np.complex128)) if j < i])
        a, b = U.indptr[i], U.indptr[i + 1]
        up.append([(int(j), int(v.real), int(v.imag)) for j, v in zip(U.indices[a:b], U.data[a:b].astype(np.complex128)) if j > i])
        v = complex(U[i, i])
        dg.append((int(v.real), int(v.imag)))
    return lo, up, dg


def _sweep_solve(c, zr, zi, check):
    """z = F^-1 (Pc r) of a sweep kind: substitution in rational arithmetic on the rows of L0 = L4 / 4 and U0 = U4 / 4, verified in integers
    (L4 U4 z == 16 Pc r); the bounds of SweepCase.rhs are asserted on it"""
    import trans_cases as tc
    s = tc.prepared(c.kind)[0]
    lo, up, dg = _triangles(c.kind)
    n = c.n
    rints, er = _ints(list(zr) + list(zi))
    S = 2 * n + 64                                                                          # every division below is by 4 or by |U4_ii|^2 <= 2^8: exact in units of 2^(er - S), asserted
    yr, yi = [v << S for v in rints[:n]], [v << S for v in rints[n:]]
    for i in range(n):                                                                      # L0 y = Pc r (unit diagonal)
        sr = si = 0
        for j, a, b in lo[i]:
            if yr[j] or yi[j]:
                sr += a * yr[j] - b * yi[j]; si += a * yi[j] + b * yr[j]
        assert sr % 4 == 0 and si % 4 == 0
        yr[i] -= sr >> 2; yi[i] -= si >> 2
    wr, wi = [0] * n, [0] * n
    for i in range(n - 1, -1, -1):                                                          # U0 z = y
        sr, si = 4 * yr[i], 4 * yi[i]
        for j, a, b in up[i]:
            if wr[j] or wi[j]:
                sr -= a * wr[j] - b * wi[j]; si -= a * wi[j] + b * wr[j]
        a, b = dg[i]
        m2 = a * a + b * b
        pr_, pi_ = sr * a + si * b, si * a - sr * b
        assert pr_ % m2 == 0 and pi_ % m2 == 0
        wr[i], wi[i] = pr_ // m2, pi_ // m2
    scale = Fraction(2) ** (er - S)
    wr, wi = [v * scale for v in wr], [v * scale for v in wi]
    ints, e = _ints(wr + wi)
    assert max(abs(v) for v in ints) < 2 ** 30, (c.name, "the correction does not fit the integer check")
    n = c.n
    zi_ = np.array(ints[:n], dtype=np.int64) + (1j * np.array(ints[n:], dtype=np.int64) if c.z else 0)
    y4 = s.U4 @ zi_
    b16 = s.L4 @ y4
    u = Fraction(2) ** e / 16
    assert all(Fraction(int(v)) * u == f for v, f in zip(b16.real, zr)) and all(Fraction(int(v)) * u == f for v, f in zip(b16.imag if c.z else np.zeros(n), zi)), c.name
    if check:
        ab = lambda v: np.abs(v.real).astype(np.int64) + (np.abs(v.imag).astype(np.int64) if c.z else 0)
        ax, ay, ab_ = ab(zi_), ab(y4), ab(b16)
        fwd = s.aLi @ (4 * ab_ + s.aL @ (4 * ay))
        bwd = s.aUi @ (4 * ay + s.aU @ ax)
        assert int(fwd.max()) * MARGIN < LIMIT and int(bwd.max()) * MARGIN < LIMIT, (c.name, int(fwd.max()), int(bwd.max()))
        assert e - 12 >= -1000
    return wr, wi


def _solve(c, rr, ri, check):
    """dx = Pc^T F^-1 Pc r"""
    n, pc = c.n, c.pc.tolist()
    zr, zi = [None] * n, [None] * n
    for i in range(n):
        zr[pc[i]], zi[pc[i]] = rr[i], ri[i]
    if c.kind == "diag":
        dr, di = _frs(c.d)
        wr, wi = [], []
        for k in range(n):
            m2 = dr[k] * dr[k] + di[k] * di[k]
            wr.append((zr[k] * dr[k] + zi[k] * di[k]) / m2); wi.append((zi[k] * dr[k] - zr[k] * di[k]) / m2)
    else:
        wr, wi = _sweep_solve(c, zr, zi, check)
    return [wr[pc[i]] for i in range(n)], [wi[pc[i]] for i in range(n)]


def simulate(c, av=None, check=True):
    """the whole run of case c: dict(berr[nrhs], steps (of the last column), steps_all, passes (berr of every pass, per column), X, and per column the
    q / branch / t of every row in every pass and the x each pass started from)"""
    a = np.asarray(c.av if av is None else av)
    nnz = a.size
    i64, ea = _ints_np(np.concatenate([a.real, a.imag if c.z else np.zeros(nnz)]))
    if i64 is not None:                                                                     # the integer image of A' (numpy where it fits: the sweep kinds hold ~10^6 entries)
        A = (i64[:nnz].tolist(), i64[nnz:].tolist(), ea, (i64[:nnz], i64[nnz:]))
    else:
        ar_, ai_ = _frs(a)
        ints, ea = _ints(ar_ + ai_)
        A = (ints[:nnz], ints[nnz:], ea, None)
    n = c.n
    out = dict(berr=np.zeros(c.nrhs), steps_all=[], passes=[], X=np.zeros_like(c.X0), q=[], branch=[], t=[], x=[])
    for j in range(c.nrhs):
        br, bi = _frs(c.B[:, j])
        bints, eb = _ints(br + bi)
        xr, xi = _frs(c.X0[:, j])
        lstres, count = 3.0, 0
        passes, qs, brs, ts, xs = [], [], [], [], []
        while True:
            xints, ex = _ints(xr + xi)
            rr, ri, q, branch, t = _pass(c, A, xints[:n], xints[n:], ex, bints[:n], bints[n:], eb, check)
            sv = max(q) if q else 0.0
            passes.append(sv); qs.append(np.array(q)); brs.append(np.array(branch)); ts.append(np.array(t))
            xs.append(np.array([float(v) for v in xr]) + (1j * np.array([float(v) for v in xi]) if c.z else 0))
            if not (sv > EPS and sv * 2 <= lstres and count < ITMAX):
                break
            dr, di = _solve(c, rr, ri, check)
            xr, xi = [a + b for a, b in zip(xr, dr)], [a + b for a, b in zip(xi, di)]
            if check:
                assert all(_isdouble(v) for v in dr + di + xr + xi), (c.name, j, count)
            lstres = sv
            count += 1
        out["berr"][j] = passes[-1]
        out["steps_all"].append(count); out["passes"].append(passes)
        out["X"][:, j] = xs[-1]
        out["q"].append(qs); out["branch"].append(brs); out["t"].append(ts); out["x"].append(xs)
    out["steps"] = out["steps_all"][-1] if c.nrhs else 0
    return out


_PRELOADED = {}


def dump_expected(path, names_):
    """what the GPU tests compare with (berr, steps, X) of the named cases into a file, for the child processes of the GPU tests: they load it instead of
    simulating again"""
    import pickle
    with open(path, "wb") as f:
        pickle.dump({k: {q: expected(k)[q] for q in ("berr", "steps", "steps_all", "X")} for k in names_}, f)


def preload_expected(path):
    import pickle
    with open(path, "rb") as f:
        _PRELOADED.update(pickle.load(f))


@functools.lru_cache(maxsize=None)
def expected(name):
    return _PRELOADED[name] if name in _PRELOADED else simulate(cases()[name])
