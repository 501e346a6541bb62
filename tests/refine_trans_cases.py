"""Transposed and conjugate-transposed refinement runs whose whole trajectory is known EXACTLY (test helper for test_gpu_refine_trans.py and
test_refine_trans_cases_cpu.py; not a conftest).  Builds on refine_exact_cases (rx) and trans_cases (tc) by import.

sluamd_p[dz]gsrfs3d_trans iterates, for an attached matrix A' that is NOT the factored one,
    x <- x + Pc^T F^-op Pc (b - op(A') x)            op = transpose ("T") or conjugate transpose ("C"), F the exact factors of Pc A Pc^T
so the run is the UNTRANSPOSED run of the matrix op(A') on the factored system op(F).  Every case here keeps the attached data (rp, ci, av, B, X0, pc) the
device gets, and `op_case` forms op(A') from it as CSR exactly as the device does -- `transpose_index`, a numpy restatement of the library's stable counting
sort by column: column pointers, rows ascending inside a column, positions into the CSR value array; the values are av[tpos], conjugated for "C".

Kind "diag" (F = diag(d), rx.diag_store): op(F) = diag(d) for "T" and diag(conj(d)) for "C", and rx.simulate on an rx.RCase holding op(A') and that d
predicts berr of every pass, every stop decision, the step count and the final X in integers, asserting its own bounds (rx's docstring).  The cases:
  t_<name>   every kind-"diag" case of rx with A' = M^T for its matrix M: op(A') = M, the designed trajectory of rx, on the transposed path.  The orders
             rx.ORDERS, the maximising COLUMN of A' at every position of rx.MAXPOS, an empty column with b_j = 0 (rows_long, rhs3) and with b_j != 0
             (empty_b), the SAFE1 / SAFE2 branches, the three stop reasons (eps_stop: berr <= eps; the stalls: 2 berr > lstres; half_long: count = 20),
             three right-hand sides of 0, 2 and 1 steps (rhs3).
  c_<name>   complex16 only: the conjugate of that run -- A' = M^T again (A'^H = conj(M)), conj(B), conj(X0), op(F) = diag(conj(d)): conjugation is an
             automorphism that abs1 does not see, so berr and the step counts are those of t_<name> and X is its conjugate.
  *_dense_col    one dense column of A' (n = 257 entries in one thread's loop, the own entry among them) over frozen columns; it carries berr
  *_dense_row    one dense row of A': every column holds that row's entry and its own diagonal, before or after it
  z_split_T / z_split_C    ONE attached complex16 matrix, b and x0 under "T" and under "C": non-zero imaginary parts everywhere, the first-pass berr differs
Patterns with A' != A'^T: every case above but the purely diagonal ones; `untransposed_steps` runs the attached matrix UNTRANSPOSED through the simulator
(without the bounds: that run is not designed), and the CPU test asserts that its step count differs from the transposed one for ASYM.

Through the real sweeps (kinds "narrow", double, and "z_narrow", complex16, of tc.prepared): A' = (op(A) M)^op^-1 for the factored A = Pc^T L0 U0 Pc, b = op(A) c,
so that x <- c + (I - M) x whatever the factors: the correction of a step is dx = c - M x in integers.  `_simulate_sweep` verifies it against the factors in
integers -- op(U4)^T op(L4)^T (Pc dx) == 16 Pc r -- and asserts the two bounds of the transposed sweeps with tc.bounds_t (margin 64 included there) on the
integer image of Pc dx, so that the sweeps return it exactly in any summation order; the residual passes are rx._pass with rx's bounds.  sw_nil_*: a
nilpotent chain, 3 steps to berr = 0; sw_rhs3_*: three right-hand sides of 0, 2, 1 steps.  The wide kinds ("levels", "z_wide") are left out for time only: their
transposed sweeps are exactly tested by test_gpu_trans_solve.py, and nothing of the refinement depends on the supernode widths."""
import functools
from fractions import Fraction
import numpy as np
import scipy.sparse as sp
import refine_exact_cases as rx
import trans_cases as tc

SWEEPS = ("narrow", "z_narrow")
ASYM = ("t_d_half_go", "t_z_half_go", "t_d_dense_col", "t_d_rhs3")   # cases whose untransposed run takes other step counts (asserted by the CPU test)


def transpose_index(n, rp, ci):
    """(tcp, tri, tpos) of a CSR pattern: the stable counting sort by column of sluamd_trefine.cpp -- a stable sort of the entries by column visits the rows
    in ascending order inside every column, which is all the counting sort's placement loop does"""
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    nnz = int(rp[n])
    tcp = np.concatenate([[0], np.cumsum(np.bincount(ci[:nnz], minlength=n))])
    tpos = np.argsort(ci[:nnz], kind="stable")
    tri = np.repeat(np.arange(n), np.diff(rp))[tpos]
    return tcp.astype(np.int32), tri.astype(np.int32), tpos.astype(np.int32)


def counting_sort_loop(n, rp, ci):
    """the same, entry by entry as the library's host loop runs (for the CPU test: small cases)"""
    nnz = int(rp[n])
    tcp = np.zeros(n + 1, dtype=np.int64)
    for e in range(nnz):
        tcp[ci[e] + 1] += 1
    tcp = np.cumsum(tcp)
    nxt, tri, tpos = tcp[:-1].copy(), np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=np.int32)
    for i in range(n):
        for e in range(rp[i], rp[i + 1]):
            p = nxt[ci[e]]; nxt[ci[e]] += 1
            tri[p], tpos[p] = i, e
    return tcp.astype(np.int32), tri, tpos


class TCase:
    """what the device gets (rp, ci, av, B, X0, pc, trans) and the kind of the factored system"""

    def __init__(self, name, trans, kind, z, pc, A, B, X0, d=None, tight=(), expect=None, max_col=None, design=None):
        self.name, self.trans, self.kind, self.z = name, trans, kind, z
        self.pc = np.ascontiguousarray(pc, dtype=np.int32)
        self.n = len(self.pc)
        vt = np.complex128 if z else np.float64
        rp, ci, av = A
        self.rp, self.ci, self.av = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(av, dtype=vt)
        self.B, self.X0 = np.asfortranarray(np.asarray(B, dtype=vt).reshape(self.n, -1)), np.asfortranarray(np.asarray(X0, dtype=vt).reshape(self.n, -1))
        # conjugated data carries -0.0 where a part was +0.0; the simulator (Fractions) knows one zero only, and x0 = -0.0 would keep its sign through
        # x + dx: every zero the device gets is +0.0
        self.av, self.B, self.X0 = self.av + 0.0, np.asfortranarray(self.B + 0.0), np.asfortranarray(self.X0 + 0.0)
        self.nrhs = self.B.shape[1]
        self.d, self.tight, self.expect, self.max_col, self.design = d, frozenset(tight), expect or {}, max_col, design

    @property
    def conj(self):
        return self.z and self.trans == "C"

    def __repr__(self):
        return self.name


def op_csr(c, av=None):
    """op(A') of a case as CSR arrays, through the transposed index"""
    tcp, tri, tpos = transpose_index(c.n, c.rp, c.ci)
    v = np.asarray(c.av if av is None else av)[tpos]
    return tcp, tri, (v.conj() if c.conj else v)


def op_case(c, av=None):
    """the rx.RCase whose untransposed run is the transposed run of c: the matrix op(A'), and for kind "diag" d (T) or conj(d) (C)"""
    d = None if c.d is None else (np.conj(c.d) if c.conj else c.d)
    return rx.RCase(c.name, c.kind, c.z, c.pc, op_csr(c, av), c.B, c.X0, d=d, tight=c.tight, expect=c.expect, max_row=c.max_col)


def _transposed(n, rp, ci, av):
    """M (CSR arrays) -> M^T as CSR arrays"""
    tcp, tri, tpos = transpose_index(n, rp, ci)
    return tcp, tri, np.asarray(av)[tpos]


def _from_rx(r):
    """t_<name> (and c_<name> for complex16) of a kind-"diag" case of rx"""
    At = _transposed(r.n, r.rp, r.ci, r.av)
    out = [TCase("t_" + r.name, "T", "diag", r.z, r.pc, At, r.B, r.X0, d=r.d, tight=r.tight, expect=r.expect, max_col=r.max_row)]
    if r.z:
        out.append(TCase("c_" + r.name, "C", "diag", True, r.pc, At, r.B.conj(), r.X0.conj(), d=r.d, tight=r.tight, expect=r.expect, max_col=r.max_row))
    return out


def _dense_cases(z):
    out = []
    g = 1j if z else 1.0
    n, m = 257, 137
    # one dense column m of A' = a dense row m of M: every column is frozen but m, whose own entry stalls (A'_mm = 2 A_mm, r_m = +- A_mm delta)
    D = rx._Diag(n, z)
    x0, delta = D.zz(2 ** 10 + 5, m), D.zz(4, m)
    row = [(j, ((j % 5) + 1) * (-1) ** j * (g if j % 3 == 0 else 1.0)) for j in range(n) if j != m]
    row.insert(m, (m, 2 * D.dp[m]))
    D.rows[m] = row
    D.X[m, :] = x0
    D.B[m, :] = sum(a * D.X[j, 0] for j, a in row if j != m) + D.dp[m] * (2 * x0 + delta)
    out.append(("dense_col", D.case("dense_col", max_row=m, expect=dict(steps=[1], lengths=(1, n)))))
    # one dense row m of A' = a dense column m of M: x_m is frozen, every other row holds (m, a_i) and a stalling diagonal, in column order
    D = rx._Diag(n, z)
    D.frozen(m, D.zz(9, m))
    for i in range(n):
        if i == m:
            continue
        a = ((i % 3) + 1) * (g if i % 2 else 1.0)
        x0, delta = D.zz(2 ** 12 + 3 * i, i), D.zz(8 if i == 200 else 1, i)
        D.rows[i] = sorted([(m, a), (i, 2 * D.dp[i])])
        D.X[i, :] = x0
        D.B[i, :] = a * D.X[m, 0] + D.dp[i] * (2 * x0 + delta)
    out.append(("dense_row", D.case("dense_row", max_row=200, expect=dict(steps=[1], strict_max=True, lengths=(1, 2)))))
    res = []
    for _, r in out:
        res += _from_rx(r)
    return res


def _split_cases():
    """ONE attached complex16 matrix, b, x0 under T and under C: every diagonal entry stalls under T; under C the rows whose A_ii is imaginary see
    conj(A'_ii) = -A'_ii and a residual of the size of b"""
    D = rx._Diag(65, True)
    D.background()
    r = D.case("split")
    At = _transposed(r.n, r.rp, r.ci, r.av)
    return [TCase("z_split_" + t, t, "diag", True, r.pc, At, r.B, r.X0, d=r.d) for t in ("T", "C")]


def _sweep_cases(name):
    out = []
    s = tc.prepared(name)[0]
    n, z = s.n, s.z
    pc = rx.perm(n)
    vt = np.complex128 if z else np.float64
    A16 = s.B16.tocsr()[pc, :][:, pc].tocsr().astype(vt)                                     # 16 A, A[i, j] = F[pc[i], pc[j]]
    i = np.arange(n)
    xs = (((3 * i + 7) % 11) - 5).astype(vt)
    if z:
        xs = xs + 1j * (((5 * i + 1) % 7) - 3)
    a0, a1, a2, m = n // 7, n // 2 + 1, n // 3, n // 5
    for trans in (("T", "C") if z else ("T",)):
        opA16 = (A16.conj().T if trans == "C" else A16.T).tocsr()

        def attached(M):
            opAp = (opA16 @ M).tocsr() / 16                                                  # op(A') = op(A) M
            opAp.eliminate_zeros()
            Ap = (opAp.conj().T if trans == "C" else opAp.T).tocsr()
            Ap.sort_indices()
            return Ap.indptr, Ap.indices, Ap.data
        tag = f"{trans.lower()}_{name}"
        # nilpotent chain
        N = sp.csr_matrix(([2.0 ** -8, 2.0 ** -8], ([a0, a1], [a1, a2])), shape=(n, n), dtype=vt)
        M = (sp.identity(n, dtype=vt, format="csr") + N).tocsr()
        xs1 = xs.copy(); xs1[[a1, a2]] *= 256
        Cm = (M @ xs1).reshape(-1, 1)
        b = (opA16 @ Cm) / 16
        x0 = xs1.copy(); x0[a2] += 2.0 ** 16
        out.append(TCase(f"sw_nil_{tag}", trans, name, z, pc, attached(M), b, x0, expect=dict(steps=[3], berr=[0.0], final=xs1.reshape(-1, 1)), design=(M, Cm)))
        # three right-hand sides: M = I - e_m e_m^T
        M = sp.identity(n, dtype=vt, format="lil"); M[m, m] = 0; M = M.tocsr(); M.eliminate_zeros()
        Cm = np.stack([xs, xs[::-1], np.roll(xs, 3)], axis=1).astype(vt)
        Cm[m, :] = [0, 1 / 64, 1 / 16]
        if z:
            Cm[m, :] *= (1 + 2j)
        B = (opA16 @ Cm) / 16
        X0 = Cm.copy(); X0[a0, 1] += 2.0 ** 10
        out.append(TCase(f"sw_rhs3_{tag}", trans, name, z, pc, attached(M), B, X0, expect=dict(steps=[0, 2, 1], nonzero_berr=True), design=(M, Cm)))
    return out


@functools.lru_cache(maxsize=None)
def update_pair(z):
    """The same-pattern update (test_gpu_refine_trans.py): dict(n, rp, ci, v0, first, second, stale).  A CSR pattern of a diagonal and one entry off it per
    row; a handle created with v0 = (d1, explicit zeros) holds the exact factors diag(d1).  `first`: the attached matrix (2 d1, non-zero off-diagonals) on
    those factors -- unsymmetric, every row stalls; its transposed run builds the index.  `second`: update_values(v2) rewrites the handle AND the attached
    matrix with v2 = (d2, zeros); factored again, the run is one exact step to berr = 0.  `stale`: what an index that had copied the first values would
    compute for the second call."""
    from superlu_dist_amd import driver
    n = 65
    vt = np.complex128 if z else np.float64
    i = np.arange(n)
    off = (i + 7) % n
    assert not np.any(off == i)
    rp = 2 * np.arange(n + 1, dtype=np.int32)
    ci = np.stack([np.minimum(i, off), np.maximum(i, off)], axis=1).reshape(-1).astype(np.int32)
    isdiag = ci == np.repeat(i, 2)
    d1 = rx.dvals(n, z)
    d2 = np.roll(d1, 4) * 2
    g = 1j if z else 1.0
    trans = "C" if z else "T"

    def values(d, offv):
        v = np.zeros(2 * n, dtype=vt)
        v[isdiag] = d; v[~isdiag] = offv
        return v
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=64, unsym=True)
    pc = np.array(symb.perm_c, dtype=np.int32)
    symb.free()
    xs = ((i % 9) - 4 + 2.0 ** 12).astype(vt) * (1 + (0.5j if z else 0))

    def case(name, av, dfac):
        A = sp.csr_matrix((av, ci, rp), shape=(n, n))
        opA = (A.conj().T if z else A.T).tocsr()
        b = opA @ xs + (np.conj(dfac) if z else dfac) * (((i % 3) + 1) * 2 * g)
        dd = np.empty(n, dtype=vt); dd[pc] = dfac                                            # F[pc[i], pc[i]] = A_ii
        return TCase(name, trans, "diag", z, pc, (rp, ci, av), b, xs, d=dd)
    first = case("upd_first", values(2 * d1, ((i % 4) + 1) * g), d1)
    second = case("upd_second", values(d2, 0.0), d2)
    stale = TCase("upd_stale", trans, "diag", z, pc, (rp, ci, first.av), second.B, second.X0, d=second.d)
    return dict(n=n, rp=rp, ci=ci, v0=values(d1, 0.0), first=first, second=second, stale=stale)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for r in rx.cases().values():
        if r.kind == "diag":
            out += _from_rx(r)
    out += _dense_cases(False) + _dense_cases(True) + _split_cases()
    for name in SWEEPS:
        out += _sweep_cases(name)
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


def names(kind=None, z=None, trans=None):
    return [k for k, c in cases().items() if (kind is None or (c.kind == "diag") == (kind == "diag")) and (z is None or c.z == z)
            and (trans is None or c.trans == trans)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the sweep kinds: the loop of rx.simulate with the designed correction, verified against the factors
# ---------------------------------------------------------------------------------------------------------------------------------------
class _Proxy:
    """a sweep case whose rhs() is a given integer vector: tc.bounds_t evaluates the bounds of the transposed sweeps for it"""

    def __init__(self, s, x):
        self._s, self._x = s, x

    def __getattr__(self, k):
        return getattr(self._s, k)

    def rhs(self, nrhs):
        return self._x, None


def _check_correction(c, dr, di, rr, ri):
    """dx (Fractions, original ordering) is the exact transposed solve of r with the factors, and the sweeps compute it exactly"""
    s = tc.prepared(c.kind)[0]
    n, pc = c.n, c.pc
    ints, e = rx._ints(list(dr) + list(di))
    assert max(abs(v) for v in ints) < 2 ** 30, (c.name, "the correction does not fit the integer check")
    zp = np.zeros(n, dtype=np.complex128 if c.z else np.int64)
    zp[pc] = np.array(ints[:n], dtype=np.int64) + (1j * np.array(ints[n:], dtype=np.int64) if c.z else 0)
    op = (lambda M: M.conj()) if c.conj else (lambda M: M)
    y4 = op(s.L4).T.tocsr() @ zp
    b16 = op(s.U4).T.tocsr() @ y4                                                            # 16 op(F)^T (Pc dx) in units of 2^e
    u = Fraction(2) ** e / 16
    rp_r, rp_i = [None] * n, [None] * n
    for i in range(n):
        rp_r[pc[i]], rp_i[pc[i]] = rr[i], ri[i]
    assert all(Fraction(int(v)) * u == f for v, f in zip(np.real(b16), rp_r)), c.name
    assert all(Fraction(int(v)) * u == f for v, f in zip(np.imag(b16) if c.z else np.zeros(n), rp_i)), c.name
    fwd, bwd = tc.bounds_t(_Proxy(s, zp.reshape(-1, 1)), 1, conj=c.conj, narrow=False)         # (the margin 64 is inside)
    assert fwd < tc.LIMIT and bwd < tc.LIMIT, (c.name, fwd, bwd)
    assert e - 12 >= -1000
    return fwd, bwd


def _simulate_sweep(c, check=True):
    o = op_case(c)
    M, Cm = c.design
    M = M.tocsr()
    a = np.asarray(o.av)
    nnz, n = a.size, c.n
    i64, ea = rx._ints_np(np.concatenate([a.real, a.imag if c.z else np.zeros(nnz)]))
    assert i64 is not None
    A = (i64[:nnz].tolist(), i64[nnz:].tolist(), ea, (i64[:nnz], i64[nnz:]))
    mrp, mci = M.indptr.tolist(), M.indices.tolist()
    mr, mi = rx._frs(M.data)
    out = dict(berr=np.zeros(c.nrhs), steps_all=[], passes=[], X=np.zeros_like(c.X0), bounds=[])
    for j in range(c.nrhs):
        br, bi = rx._frs(c.B[:, j])
        bints, eb = rx._ints(br + bi)
        cr, ci_ = rx._frs(Cm[:, j])
        xr, xi = rx._frs(c.X0[:, j])
        lstres, count, passes = 3.0, 0, []
        while True:
            xints, ex = rx._ints(xr + xi)
            rr, ri, q, branch, t = rx._pass(o, A, xints[:n], xints[n:], ex, bints[:n], bints[n:], eb, check)
            sv = max(q) if q else 0.0
            passes.append(sv)
            if not (sv > rx.EPS and sv * 2 <= lstres and count < rx.ITMAX):
                break
            dr, di = [], []                                                                  # dx = c - M x
            for i in range(n):
                sr = si = Fraction(0)
                for k in range(mrp[i], mrp[i + 1]):
                    jj = mci[k]
                    sr += mr[k] * xr[jj] - mi[k] * xi[jj]; si += mr[k] * xi[jj] + mi[k] * xr[jj]
                dr.append(cr[i] - sr); di.append(ci_[i] - si)
            if check:
                out["bounds"].append(_check_correction(c, dr, di, rr, ri))
            xr, xi = [p + q_ for p, q_ in zip(xr, dr)], [p + q_ for p, q_ in zip(xi, di)]
            if check:
                assert all(rx._isdouble(v) for v in dr + di + xr + xi), (c.name, j, count)
            lstres = sv
            count += 1
        out["berr"][j] = passes[-1]
        out["steps_all"].append(count); out["passes"].append(passes)
        out["X"][:, j] = np.array([float(v) for v in xr]) + (1j * np.array([float(v) for v in xi]) if c.z else 0)
    out["steps"] = out["steps_all"][-1]
    return out


def simulate(c, av=None, check=True):
    """the whole transposed run of case c (dict as rx.simulate: berr, steps, steps_all, passes, X, ...); `av`: other values on the same pattern"""
    if c.kind == "diag":
        return rx.simulate(op_case(c, av), check=check)
    assert av is None
    return _simulate_sweep(c, check)


def untransposed_steps(c):
    """steps_all of the attached matrix run UNTRANSPOSED on the same factors and data (kind "diag"; no bounds: that run is not designed)"""
    r = rx.RCase(c.name, c.kind, c.z, c.pc, (c.rp, c.ci, c.av), c.B, c.X0, d=c.d)
    return rx.simulate(r, check=False)["steps_all"]


@functools.lru_cache(maxsize=None)
def expected(name):
    return simulate(cases()[name])
