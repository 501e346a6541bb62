"""Systems on which the plain refinement loop must fail and GMRES preconditioned by the same factors must not (test helper for test_gmres_cases_cpu.py and
test_gpu_gmres_refine.py; not a conftest).

A handle holds the factors of A (order n, perm_c = refine_exact_cases.perm(n) for kind "diag", the symbolic structure's own for kind "lu").  Attached is
    A' = A (I + W),   W = sum_k (m_k e_{a_k} + e_{c_k} / 2) e_{a_k}^T,   k < t,   the a_k distinct, no c_k among them
so E = A' - A = A W has rank t, is sparse (column a_k of E is m_k A[:, a_k] + A[:, c_k] / 2: entries on and off the diagonal) and A^-1 A' = I + W has the
eigenvalues 1 and 1 + m_k.  The m_k are DISTINCT, all of modulus > 1 (MULT: -3, 3, -5, 7, ...: rho(I - A^-1 A') = max |m_k| >= 3, the stationary loop
x <- x + A^-1 (b - A' x) multiplies the error along e_{a_k} by -m_k per step), so I + W is diagonalisable with t + 1 distinct eigenvalues and GMRES on
A' d = r preconditioned by A needs exactly t + 1 iterations from a residual with a component along each of them -- never fewer than that short of rounding,
which is what makes t = 1, 2, 4 and 10 different tests; t = 10 runs past the 8 basis vectors one pass of the Krylov kernels takes.  The cases named
"..._cluster" take m_k = 2 + k / 64 instead: eigenvalues 1 and a tight cluster at 3, on which GMRES restarted every 2 iterations still contracts by more than
a half per cycle.  All data are dyadic and small, so b = op(A') x* is formed exactly.

kind "diag": A = Pc^T diag(+-2^k) Pc (refine_exact_cases.diag_store: exact factors, exact corrections, any order).
kind "lu":   A = 4 I + three off-diagonal entries per row of modulus <= 1 (times units of the Gaussian integers for complex16): strictly diagonally dominant,
             factored by the library itself, so the corrections pass through the real sweeps in every trans.  (The sweep kinds of refine_exact_cases -- "narrow",
             "levels", "z_narrow", "z_wide" -- have cond_inf between 4e13 and 2e23 by numpy and cannot meet the premise cond_inf(A') <= 2^10 below; they
             are built for exact integer sweeps, not for conditioning.)
Premises, asserted per case by `check_premises` with numpy alone: rho(I - A^-1 A') > 1 and cond_inf(A') <= 2^10.

LARGE_N: one "diag" order beyond one full sweep of the reduction grid of the Krylov kernels (sluamd_gkernels.inc: GM_GRID x GM_BLOCK = 1024 x 256 units of 16
bytes = 524288 doubles), odd, so that the grid-stride loops wrap and the padded last unit is used.  Its premises and its reference solution come from the
sparse structure (scipy), not from dense numpy.

model_gmres_ir / model_plain: float64 numpy restatements of the two loops (same stop rule, same berr formula, CGS2, Givens rotations, budget)."""
import functools
import numpy as np
import scipy.sparse as sp
import refine_exact_cases as rx

EPS = 2.0 ** -53
SAFMIN = 2.0 ** -1022
ITMAX = 20
ORDERS = (1, 63, 64, 65, 257, 513)
RANKS = (1, 2, 4)
BIG_T = 10                                                                                   # more basis vectors than one pass of the kernels takes (GM_CHUNK = 8)
MULT = (-3.0, 3.0, -5.0, 7.0, -9.0, 5.0, -7.0, 9.0, -11.0, 11.0)                             # 1 + m_k: -2, 4, -4, 8, -8, 6, -6, 10, -10, 12
CLUSTER = tuple(2.0 + k / 64.0 for k in range(4))
LARGE_N = 524288 + 4097
DEFAULTS = dict(restart=20, max_solves=100, inner_tol=2.0 ** -30)


def _lu_matrix(n, z):
    """4 I + entries at (i, i - 1), (i, i + 1), (i, (7 i + 3) mod n) of modulus 1, 1/2, 1 (duplicates and the diagonal position dropped)"""
    vt = np.complex128 if z else np.float64
    i = np.arange(n)
    unit = np.array([1, 1j, -1, -1j]) if z else np.array([1.0, -1.0, 1.0, -1.0])
    rows, cols, vals = [i], [i], [np.full(n, 4.0, dtype=vt)]
    for k, (j, m) in enumerate((((i - 1) % n, 1.0), ((i + 1) % n, 0.5), ((7 * i + 3) % n, 1.0))):
        rows.append(i); cols.append(j); vals.append((m * unit[(i + k) % 4]).astype(vt))
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    key = r * n + c
    _, first = np.unique(key, return_index=True)                                             # the first entry of a position wins (the diagonal's 4 first of all)
    A = sp.csr_matrix((v[first], (r[first], c[first])), shape=(n, n), dtype=vt)
    A.sort_indices()
    return A


class GCase:
    def __init__(self, name, kind, n, z, t, X0=None, xs=None, mult=MULT):
        self.name, self.kind, self.n, self.z, self.t = name, kind, n, z, t
        self.m = list(mult[:t])
        vt = np.complex128 if z else np.float64
        self.vt = vt
        if kind == "diag":
            self.pc = rx.perm(n)
            d = rx.dvals(n, z)
            self.A = sp.diags(d[self.pc]).tocsr().astype(vt)                                 # A[i, i] = d[pc[i]]
        else:
            self.pc = None                                                                   # the symbolic structure's, known once the handle exists
            self.A = _lu_matrix(n, z)
        self.a = [(5 + 37 * k) % n for k in range(t)]
        self.c = [(x + 11) % n for x in self.a] if n > 1 else []
        assert len(set(self.a)) == t and not set(self.a) & set(self.c)
        rows = list(self.a) + list(self.c)
        vals = self.m + [0.5] * len(self.c)
        self.W = sp.csr_matrix((np.array(vals, dtype=vt), (rows, list(self.a) + list(self.a)[:len(self.c)])), shape=(n, n), dtype=vt)
        self.Ap = (self.A @ (sp.identity(n, dtype=vt, format="csr") + self.W)).tocsr()
        self.Ap.eliminate_zeros(); self.Ap.sort_indices()
        i = np.arange(n)
        x = (((3 * i + 7) % 11) - 5).astype(vt)
        if z:
            x = x + 1j * (((5 * i + 1) % 7) - 3)
        self.xs = np.asfortranarray(x.reshape(n, 1) if xs is None else xs(x))
        self.nrhs = self.xs.shape[1]
        self.X0 = np.asfortranarray(np.zeros_like(self.xs) if X0 is None else X0(self.xs))
        self.max_row = int(np.diff(self.Ap.indptr).max()) if n else 0

    def op(self, trans, M=None):
        M = self.Ap if M is None else M
        return (M if trans == "N" else M.T if trans == "T" or not self.z else M.conj().T).tocsr()

    def rhs(self, trans):
        """b = op(A') x*: dyadic terms far below 2^53 in units of their last place, exact in any order"""
        return np.asfortranarray(self.op(trans) @ self.xs)

    def csr(self):
        return self.Ap.indptr.astype(np.int32), self.Ap.indices.astype(np.int32), self.Ap.data.astype(self.vt)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for z in (False, True):
        p = "z" if z else "d"
        for n in ORDERS:
            for t in RANKS:
                if t <= n and (n in (65, 513) or t == (1 if n == 1 else 2 if n in (63, 257) else 4)):
                    out.append(GCase(f"{p}_diag_n{n}_t{t}", "diag", n, z, t))
        for n, t in ((65, 1), (257, 2), (513, 4)):
            out.append(GCase(f"{p}_lu_n{n}_t{t}", "lu", n, z, t))
        for kind in ("diag", "lu"):
            out.append(GCase(f"{p}_{kind}_n513_t{BIG_T}", kind, 513, z, BIG_T))
        out.append(GCase(f"{p}_{'lu' if z else 'diag'}_n513_t4_cluster", "lu" if z else "diag", 513, z, 4, mult=CLUSTER))
        for kind, n in (("diag", 65), ("lu", 257)):
            out.append(GCase(f"{p}_{kind}_n{n}_same", kind, n, z, 0, X0=lambda xs: xs.copy()))   # E = 0, exact from the start
        # three right-hand sides: exact from the start; off by 2^10 at one row outside the a_k and c_k (its residual is an eigenvector of A' A^-1: one
        # iteration); from zero (t + 1 iterations)
        def x3(x):
            return np.stack([x, x[::-1], np.roll(x, 3)], axis=1)
        def x03(xs):
            X = xs.copy(); X[:, 2] = 0; X[2, 1] += 2.0 ** 10
            return X
        out.append(GCase(f"{p}_diag_n65_rhs3", "diag", 65, z, 2, xs=x3, X0=x03))
        out.append(GCase(f"{p}_lu_n65_rhs3", "lu", 65, z, 2, xs=x3, X0=x03))
    out.append(GCase("d_diag_large", "diag", LARGE_N, False, 2))
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


def names(kind=None, z=None, rank=None, large=False):
    return [k for k, c in cases().items() if (kind is None or c.kind == kind) and (z is None or c.z == z) and (rank is None or (c.t > 0) == rank)
            and (large or c.n < LARGE_N)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# numpy: premises, reference, models
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_premises(c):
    """rho(I - A^-1 A') > 1 (cases with E != 0) and cond_inf(A') <= 2^10; returns (rho, cond)"""
    if c.n < LARGE_N:
        A, Ap = c.A.toarray(), c.Ap.toarray()
        rho = float(np.abs(np.linalg.eigvals(np.eye(c.n) - np.linalg.solve(A, Ap))).max()) if c.n else 0.0
        cond = float(np.real(np.linalg.cond(Ap, np.inf)))
    else:                                                                                    # diagonal A: the eigenvalues of -W are those of its a x a block; the
        S = np.array(c.a)                                                                    # inverse of A' = A (I + W) column by column from the sparse solve
        rho = float(np.abs(np.linalg.eigvals(-c.W[S, :][:, S].toarray())).max())
        # (I + W)^-1 differs from I in the columns a_k only: 1 / (1 + m_k) on the diagonal, -1 / (2 (1 + m_k)) at row c_k (dyadic for m = -3, 3);
        # |A'^-1| row sums follow
        Mi = sp.identity(c.n, format="lil", dtype=c.vt)
        for k, a in enumerate(c.a):
            Mi[a, a] = 1.0 / (1.0 + c.m[k]); Mi[c.c[k], a] = -0.5 / (1.0 + c.m[k])
        Ai = (Mi.tocsr() @ sp.diags(1.0 / c.A.diagonal())).tocsr()
        assert abs(Ai @ c.Ap - sp.identity(c.n)).max() == 0.0                                # dyadic: the inverse is exact
        cond = float(abs(Ai).sum(axis=1).max() * abs(c.Ap).sum(axis=1).max())
    if c.t:
        assert rho > 1.0, (c.name, rho)
    assert cond <= 2.0 ** 10, (c.name, cond)
    return rho, cond


def _abs1(v):
    return np.abs(v.real) + np.abs(v.imag) if np.iscomplexobj(v) else np.abs(v)


def berr_of(M, aM, x, b, n):
    """the backward error of the refinement kernels in float64: max_i |r_i| / (|M| |x| + |b|)_i with the SAFE1 / SAFE2 guards (abs1 for complex16)"""
    safe1 = (n + 1) * SAFMIN
    safe2 = safe1 / EPS
    r = b - M @ x
    t = aM @ _abs1(x) + _abs1(b)
    ar = _abs1(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(t > safe2, ar / t, np.where(t != 0.0, (safe1 + ar) / t, 0.0))
    return r, float(q.max()) if q.size else 0.0


class _Sys:
    """op(A') and the preconditioner op(A)^-1 of a case in numpy / scipy"""

    def __init__(self, c, trans):
        self.c, self.n = c, c.n
        self.M = c.op(trans)
        self.aM = sp.csr_matrix((_abs1(self.M.data), self.M.indices, self.M.indptr), shape=self.M.shape)
        F = c.op(trans, c.A)
        if c.kind == "diag":
            d = F.diagonal()
            self.minv = lambda v: v / d
        else:
            import scipy.linalg as sl
            lu = sl.lu_factor(F.toarray())
            self.minv = lambda v: sl.lu_solve(lu, v)

    def berr(self, x, b):
        return berr_of(self.M, self.aM, x, b, self.n)


@functools.lru_cache(maxsize=None)
def system(name, trans):
    return _Sys(cases()[name], trans)


@functools.lru_cache(maxsize=None)
def reference(name, trans):
    """(x_ref, berr_ref[nrhs]): numpy.linalg.solve(op(A'), b) and its backward error by the same formula (LARGE_N: scipy's sparse LU stands in for LAPACK)"""
    c, S = cases()[name], system(name, trans)
    B = c.rhs(trans)
    if c.n < LARGE_N:
        X = np.linalg.solve(S.M.toarray(), B)
    else:
        import scipy.sparse.linalg as spl
        X = spl.splu(S.M.tocsc()).solve(B)
    return X, np.array([S.berr(X[:, j], B[:, j])[1] for j in range(c.nrhs)])


def bound(name, trans):
    """the accuracy bound per right-hand side: 4 max(2^-53, berr_ref)"""
    return 4.0 * np.maximum(EPS, reference(name, trans)[1])


def model_plain(name, trans="N"):
    """x <- x + op(A)^-1 (b - op(A') x) with the reference's stop rule: dict(X, berr, steps)"""
    c, S = cases()[name], system(name, trans)
    B, X = c.rhs(trans), c.X0.copy()
    berr, steps = np.zeros(c.nrhs), []
    for j in range(c.nrhs):
        x, lstres, count = X[:, j].copy(), 3.0, 0
        while True:
            r, sv = S.berr(x, B[:, j])
            berr[j] = sv
            if not (sv > EPS and sv * 2 <= lstres and count < ITMAX):
                break
            x = x + S.minv(r)
            lstres = sv; count += 1
        X[:, j] = x; steps.append(count)
    return dict(X=X, berr=berr, steps=steps)


def _cycle(S, r, restart, inner_tol, max_solves, solves):
    """one GMRES cycle on op(A') d = r, right-preconditioned by op(A), d_0 = 0: (d, iterations, solves)"""
    n = S.n
    beta = float(np.sqrt(np.vdot(r, r).real))
    V = np.zeros((n, restart + 1), dtype=r.dtype)
    V[:, 0] = r / beta
    R = np.zeros((restart, restart), dtype=np.complex128)
    g = np.zeros(restart + 1, dtype=np.complex128); g[0] = beta
    cs, sn = np.zeros(restart), np.zeros(restart, dtype=np.complex128)
    kdim = 0
    for j in range(restart):
        w = S.M @ S.minv(V[:, j]); solves += 1
        Vj = V[:, :j + 1]
        h = Vj.conj().T @ w; w = w - Vj @ h                                                  # CGS2
        h2 = Vj.conj().T @ w; w = w - Vj @ h2
        col = np.zeros(j + 2, dtype=np.complex128); col[:j + 1] = h + h2
        hn = float(np.sqrt(np.vdot(w, w).real))
        for i in range(j):
            t = cs[i] * col[i] + sn[i] * col[i + 1]
            col[i + 1] = -np.conj(sn[i]) * col[i] + cs[i] * col[i + 1]
            col[i] = t
        aa = abs(col[j]); den = float(np.hypot(aa, hn))
        if not den > 0.0:
            break
        ph = col[j] / aa if aa > 0 else 1.0
        cs[j], sn[j] = aa / den, ph * (hn / den)
        col[j] = ph * den
        R[:j + 1, j] = col[:j + 1]
        g[j + 1] = -np.conj(sn[j]) * g[j]; g[j] = cs[j] * g[j]
        kdim = j + 1
        if abs(g[j + 1]) <= inner_tol * beta or hn == 0.0 or j + 1 == restart or solves + 2 > max_solves:
            break
        V[:, j + 1] = w / hn
    y = np.linalg.solve(R[:kdim, :kdim], g[:kdim]) if kdim else np.zeros(0)
    u = V[:, :kdim] @ (y if np.iscomplexobj(r) else y.real)
    return S.minv(u), kdim, solves + 1


def model_gmres_ir(name, trans="N", restart=20, inner_tol=2.0 ** -30, max_solves=100):
    """the algorithm of sluamd_p[dz]gsrfs3d_gmres in float64 numpy: dict(X, berr, steps (per column), solves (per column), iters (per column: iterations of every cycle))"""
    c, S = cases()[name], system(name, trans)
    B, X = c.rhs(trans), c.X0.copy()
    berr, steps, solves_all, iters = np.zeros(c.nrhs), [], [], []
    for j in range(c.nrhs):
        x, lstres, count, solves, its = X[:, j].copy(), 3.0, 0, 0, []
        while True:
            r, sv = S.berr(x, B[:, j])
            berr[j] = sv
            if not (sv > EPS and sv * 2 <= lstres and count < ITMAX and solves < max_solves):
                break
            if max_solves - solves < 2:
                d = S.minv(r); solves += 1
            else:
                d, k, solves = _cycle(S, r, restart, inner_tol, max_solves, solves)
                its.append(k)
            x = x + d
            lstres = sv; count += 1
        X[:, j] = x; steps.append(count); solves_all.append(solves); iters.append(its)
    return dict(X=X, berr=berr, steps=steps, solves=solves_all, iters=iters)


def error_bound_ok(c, trans, X, berr):
    """|x - x*| <= |A'^-1| (|A'| |x| + |b|) (berr + (k + 2) 2^-52) componentwise, k the longest row, A'^-1 from numpy: x* - x = A'^-1 r and |r| <= berr t
    by the definition of berr; the slack covers the rounding of the computed residual the kernels took berr from"""
    M = c.op(trans).toarray()
    Ai = np.abs(np.linalg.inv(M))
    B = c.rhs(trans)
    k = int(np.diff(c.op(trans).indptr).max())
    for j in range(c.nrhs):
        t = _abs1(M) @ _abs1(X[:, j]) + _abs1(B[:, j])                                       # (abs1, as berr is defined)
        if not np.all(np.abs(X[:, j] - c.xs[:, j]) <= (Ai @ t) * (berr[j] + (k + 2) * 2.0 ** -52)):
            return False
    return True
