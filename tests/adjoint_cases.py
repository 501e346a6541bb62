"""Cases of the adjoint value gradient and of the differentiable solve, with their expected results in Python integers.

Kernel cases (KCase): a CSR pattern, integer (complex16: Gaussian integer) Lam and X, and the expected G for the three trans values computed entry by entry
in Python integers.  |Lam|, |X| <= 2^10 and nrhs <= 32, hence |G| <= 32 * 2^20 = 2^25 < 2^26: every product and every partial sum is an integer far below
2^53, so the fp64 sums of the kernel are exact in any order and with or without fusing, and the comparison is bitwise.

Exact solve cases (LUCase): A = L U with unit-lower L and U with a +-1 diagonal, entries in {0, +-1} (complex16: {0, +-1, +-i}).  L^-1, U^-1 and A^-1 are
integer matrices.  With perm_c = identity and no pivoting the factorisation reproduces L and U; every quantity the device forms is an integer, and the generator
asserts in integers that all of them stay below 2^30 whatever the order of summation: the entries of |L| |U| (they bound every partial Schur sum), of
|L| |U| |U^-1| and |L^-1| |L| |U| (the panel solves through the diagonal blocks' inverses, which are diagonal blocks of L^-1 and U^-1), and for every
triangular solve T s = r of the forward and adjoint sweeps |T^-1| (|r| + |T| |s|).  So x, b.grad and values.grad are compared bitwise with integers.

General data (gradcheck_case): small well-conditioned matrices for torch.autograd.gradcheck; tests/test_adjoint_cases_cpu.py vets them by a dense restatement."""
import numpy as np

TRANS = ("N", "T", "C")
BOUND_IN = 2 ** 10
BOUND_G = 2 ** 26
BOUND_LU = 2 ** 30


# ---- Gaussian integers as pairs (re, im) of object arrays of Python ints ----
def zint(a):
    a = np.asarray(a)
    return (np.array(np.real(a).astype(np.int64).tolist(), dtype=object).reshape(a.shape), np.array(np.imag(a).astype(np.int64).tolist(), dtype=object).reshape(a.shape))


def zmul(a, b):
    return (a[0].dot(b[0]) - a[1].dot(b[1]), a[0].dot(b[1]) + a[1].dot(b[0]))


def zconj(a):
    return (a[0], -a[1])


def zT(a):
    return (a[0].T, a[1].T)


def zabs1(a):
    """|re| + |im| entrywise, an upper bound of the modulus"""
    return np.abs(a[0]) + np.abs(a[1])


def to_np(a, z):
    re = np.array(a[0].tolist(), dtype=np.float64)
    return re + 1j * np.array(a[1].tolist(), dtype=np.float64) if z else re


# ---- kernel cases ----
class KCase:
    def __init__(self, name, n, rowptr, colind, nrhs, z, seed):
        self.name, self.n, self.nrhs, self.z = name, int(n), int(nrhs), bool(z)
        self.rowptr = np.asarray(rowptr, dtype=np.int32); self.colind = np.asarray(colind, dtype=np.int32)
        self.nnz = int(self.rowptr[-1])
        rng = np.random.default_rng(seed)
        lim = 700                                                     # 700 sqrt(2) < 2^10: the modulus of a Gaussian integer stays inside the bound
        draw = lambda: rng.integers(-lim, lim + 1, (self.n, self.nrhs))
        self.lam = draw() + (1j * draw() if z else 0)
        self.x = draw() + (1j * draw() if z else 0)
        self.rows = np.repeat(np.arange(self.n), np.diff(self.rowptr))

    def expected(self, trans):
        """G[e] in Python integers (pairs for complex16), by the three formulas of include/superlu_dist_amd.h"""
        L, X = zint(self.lam), zint(self.x)
        out = []
        for e in range(self.nnz):
            i, j = int(self.rows[e]), int(self.colind[e])
            re = im = 0
            for r in range(self.nrhs):
                if trans == "N":      # - Lam[i] conj(X[j])
                    p, q = (L[0][i, r], L[1][i, r]), (X[0][j, r], -X[1][j, r])
                elif trans == "T":    # - conj(X[i]) Lam[j]
                    p, q = (X[0][i, r], -X[1][i, r]), (L[0][j, r], L[1][j, r])
                else:                 # - X[i] conj(Lam[j])
                    p, q = (X[0][i, r], X[1][i, r]), (L[0][j, r], -L[1][j, r])
                re -= p[0] * q[0] - p[1] * q[1]
                im -= p[0] * q[1] + p[1] * q[0]
            out.append((re, im))
        return out

    def expected_np(self, trans):
        e = self.expected(trans)
        re = np.array([float(v[0]) for v in e]); im = np.array([float(v[1]) for v in e])
        return re + 1j * im if self.z else re

    def check(self):
        for a in (self.lam, self.x):
            assert np.all(np.real(a) ** 2 + np.imag(a) ** 2 <= BOUND_IN ** 2)
        assert self.nrhs <= 32
        for t in TRANS:
            e = self.expected(t)
            assert all(abs(v[0]) < BOUND_G and abs(v[1]) < BOUND_G for v in e)
            if not self.z:
                assert all(v[1] == 0 for v in e)
        if not self.z:
            assert self.expected("T") == self.expected("C")


def pattern(n, counts, seed, dup=False):
    """CSR of order n with counts[i] entries in row i, columns ascending and distinct inside a row (counts[i] <= n); dup: the first entry of the first
    non-empty row of two or more entries is stored twice in a row"""
    rng = np.random.default_rng(seed)
    rp = np.zeros(n + 1, dtype=np.int32); ci = []
    done = False
    for i, c in enumerate(counts):
        cols = np.sort(rng.choice(n, size=c, replace=False)) if c else np.zeros(0, dtype=np.int64)
        if dup and not done and c >= 2:
            cols[1] = cols[0]
            done = True
        ci.extend(int(v) for v in cols)
        rp[i + 1] = rp[i] + c
    assert not dup or done
    return rp, np.array(ci, dtype=np.int32)


def spread(n, nnz, empty=()):
    """nnz entries over the rows of an order-n matrix that are not in `empty`, as evenly as they go"""
    rows = [i for i in range(n) if i not in empty]
    counts = [0] * n
    for t in range(nnz):
        counts[rows[t % len(rows)]] += 1
    assert max(counts) <= n
    return counts


def kcases():
    """name -> (n, rowptr, colind, nrhs): the shapes of tests/test_gpu_adjoint_values.py"""
    out = {}
    for nnz in (255, 256, 257, 513):                                 # workgroup ends
        out[f"nnz{nnz}"] = (40,) + pattern(40, spread(40, nnz), nnz) + (3,)
    for nrhs in (1, 3, 4, 5, 16, 17):                                 # register groups and their remainder
        out[f"nrhs{nrhs}"] = (24,) + pattern(24, spread(24, 130), 100 + nrhs) + (nrhs,)
    out["empty_rows"] = (30,) + pattern(30, spread(30, 90, empty=(0, 7, 8, 29)), 5) + (2,)
    counts = spread(320, 40); counts[3] = 310                         # a row longer than one workgroup
    out["long_row"] = (320,) + pattern(320, counts, 6) + (2,)
    out["duplicate"] = (16,) + pattern(16, spread(16, 50), 7, dup=True) + (5,)
    out["n1"] = (1, np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), 4)
    return out


def kcase(name, z):
    n, rp, ci, nrhs = kcases()[name]
    return KCase(name, n, rp, ci, nrhs, z, seed=sum(map(ord, name)) + (1000 if z else 0))


def padded(a, ld, sentinel):
    """the n x nrhs block in a column-major array of leading dimension ld >= n whose other rows hold `sentinel`"""
    out = np.full((ld, a.shape[1]), sentinel, dtype=a.dtype, order="F")
    out[:a.shape[0], :] = a
    return out


def tridiag(n, z):
    """a diagonally dominant tridiagonal matrix: the handle the kernel cases attach their own patterns to (the entry reads only the attached pattern)"""
    rp = [0]; ci = []; v = []
    for i in range(n):
        for j in (i - 1, i, i + 1):
            if 0 <= j < n:
                ci.append(j); v.append(4.0 if i == j else -1.0)
        rp.append(len(ci))
    v = np.array(v)
    return n, np.array(rp, dtype=np.int32), np.array(ci, dtype=np.int32), v + (0.5j * v if z else 0)


# ---- exact solve cases ----
class LUCase:
    def __init__(self, n, z, nrhs, seed):
        self.n, self.z, self.nrhs = n, z, nrhs
        rng = np.random.default_rng(seed)
        units = np.array([1, -1, 1j, -1j]) if z else np.array([1, -1])
        L = np.eye(n, dtype=complex); U = np.diag(rng.choice([1, -1], n)).astype(complex)
        for i in range(1, n):
            for j in ({i - 1} if rng.random() < 0.5 else set()) | ({int(rng.integers(0, i))} if rng.random() < 0.3 else set()):
                L[i, j] = rng.choice(units)
        for i in range(n - 1):
            for j in ({i + 1} if rng.random() < 0.5 else set()) | ({int(rng.integers(i + 1, n))} if rng.random() < 0.3 else set()):
                U[i, j] = rng.choice(units)
        self.L, self.U = zint(L), zint(U)
        self.A = zmul(self.L, self.U)
        struct = zabs1(self.L).dot(zabs1(self.U)) != 0            # the pattern of |L| |U|: entries that cancel stay stored
        self.rows, self.cols = np.nonzero(struct)
        self.rowptr = np.concatenate([[0], np.cumsum(struct.sum(1))]).astype(np.int32)
        self.colind = self.cols.astype(np.int32)
        self.nnz = len(self.colind)
        self.values = to_np((self.A[0][self.rows, self.cols], self.A[1][self.rows, self.cols]), z)
        self.Linv, self.Uinv = self._tri_inv(self.L, True), self._tri_inv(self.U, False)
        self.Ainv = zmul(self.Uinv, self.Linv)
        draw = lambda: rng.integers(-3, 4, (n, nrhs))
        self.b = zint(draw() + (1j * draw() if z else 0))
        self.w = zint(draw() + (1j * draw() if z else 0))
        self.check()

    def _tri_inv(self, T, lower):
        n = self.n
        inv = (np.array([[int(i == j) for j in range(n)] for i in range(n)], dtype=object), np.array([[0] * n for _ in range(n)], dtype=object))
        order = range(n) if lower else range(n - 1, -1, -1)
        for i in order:
            ks = range(i) if lower else range(i + 1, n)
            re, im = inv[0][i, :].copy(), inv[1][i, :].copy()
            for k in ks:
                a, c = T[0][i, k], T[1][i, k]
                if a or c:
                    re, im = re - (a * inv[0][k, :] - c * inv[1][k, :]), im - (a * inv[1][k, :] + c * inv[0][k, :])
            d = T[0][i, i]                                          # +-1: its own inverse
            assert T[1][i, i] == 0 and d in (1, -1)
            inv[0][i, :], inv[1][i, :] = d * re, d * im
        return inv

    def op_inv(self, trans):
        return self.Ainv if trans == "N" else zT(self.Ainv) if trans == "T" else zconj(zT(self.Ainv))

    def expected(self, trans):
        """(x, b.grad, values.grad) of loss = Re sum(w x) in integers: Gbar = conj(w) under PyTorch's convention"""
        x = zmul(self.op_inv(trans), self.b)
        gbar = zconj(self.w)
        if trans == "N":
            lam = zmul(zconj(zT(self.Ainv)), gbar)                   # A^-H Gbar
        elif trans == "T":
            lam = zmul(zconj(self.Ainv), gbar)                       # conj(A)^-1 Gbar
        else:
            lam = zmul(self.Ainv, gbar)                              # A^-1 Gbar
        G = ([], [])
        for i, j in zip(self.rows, self.cols):
            if trans == "N":
                p, q = (lam[0][i], lam[1][i]), (x[0][j], -x[1][j])
            elif trans == "T":
                p, q = (x[0][i], -x[1][i]), (lam[0][j], lam[1][j])
            else:
                p, q = (x[0][i], x[1][i]), (lam[0][j], -lam[1][j])
            G[0].append(-sum(p[0] * q[0] - p[1] * q[1])); G[1].append(-sum(p[0] * q[1] + p[1] * q[0]))
        return x, lam, (np.array(G[0], dtype=object), np.array(G[1], dtype=object))

    def check(self):
        n = self.n
        eye = np.array([[int(i == j) for j in range(n)] for i in range(n)], dtype=object)
        for T, Ti in ((self.L, self.Linv), (self.U, self.Uinv)):
            p = zmul(T, Ti)
            assert np.array_equal(p[0], eye) and not p[1].any()
        p = zmul(self.A, self.Ainv)
        assert np.array_equal(p[0], eye) and not p[1].any()         # A^-1 is an integer matrix
        aL, aU, aLi, aUi = zabs1(self.L), zabs1(self.U), zabs1(self.Linv), zabs1(self.Uinv)
        schur = aL.dot(aU)
        assert schur.max() < BOUND_LU and schur.dot(aUi).max() < BOUND_LU and aLi.dot(schur).max() < BOUND_LU
        for trans in TRANS:
            x, lam, G = self.expected(trans)
            assert max(zabs1(x).max(), zabs1(lam).max(), zabs1(G).max()) < BOUND_LU
            # the sweeps of op(A) s = r: forward sweep through L (N) or U^T / U^H (T, C), then the other factor; the adjoint system swaps the roles
            for (first, fi, second, si), r, s in (((aL, aLi, aU, aUi) if trans == "N" else (aU.T, aUi.T, aL.T, aLi.T), self.b, x),
                                                 ((aU.T, aUi.T, aL.T, aLi.T) if trans == "N" else (aL, aLi, aU, aUi), self.w, lam)):
                mid = second.dot(zabs1(s))                          # the intermediate vector y = second s: |y| <= |second| |s|
                assert fi.dot(zabs1(r) + first.dot(mid)).max() < BOUND_LU
                assert si.dot(mid + mid).max() < BOUND_LU


LU_SEEDS = {(False, 1): 11, (False, 5): 12, (True, 1): 13, (True, 5): 14}


def lucase(z, nrhs, n=48):
    return LUCase(n, z, nrhs, LU_SEEDS[(z, nrhs)])


# ---- general data for gradcheck ----
def gradcheck_case(z, n=8, nrhs=2, seed=3):
    """a diagonally dominant matrix of order n <= 16 with nnz <= 60 (tridiagonal plus a few scattered entries), b of nrhs columns; cond_1 <= 100 is asserted
    by the CPU test from the dense matrix"""
    rng = np.random.default_rng(seed + (50 if z else 0))
    S = np.eye(n, dtype=bool)
    for i in range(n - 1):
        S[i, i + 1] = S[i + 1, i] = True
    for _ in range(8):
        i, j = rng.integers(0, n, 2)
        S[i, j] = True
    rows, cols = np.nonzero(S)
    rnd = lambda m: rng.uniform(-1, 1, m) + (1j * rng.uniform(-1, 1, m) if z else 0)
    v = rnd(len(rows))
    v[rows == cols] += 5.0
    rp = np.concatenate([[0], np.cumsum(S.sum(1))]).astype(np.int32)
    b = rnd(n * nrhs).reshape(n, nrhs)
    assert n <= 16 and len(v) <= 60
    return dict(n=n, rowptr=rp, colind=cols.astype(np.int32), rows=rows, cols=cols, values=v, b=b)


# ---- the cases of tests/test_gpu_autograd.py (bodies: tests/autograd_gpu_cases.py, which needs torch; the ids are here so that the test file does not) ----
AUTOGRAD_GRADCHECKS = [(False, "N", False), (False, "T", False), (True, "N", False), (True, "C", False), (False, "N", True)]      # (complex16, trans, equil)
AUTOGRAD_EXACT = [(z, nrhs, trans) for z in (False, True) for nrhs in (1, 5) for trans in TRANS]


def autograd_case_ids():
    """every case id, in running order"""
    return ([f"exact-{'z' if z else 'd'}-{nrhs}-{t}" for z, nrhs, t in AUTOGRAD_EXACT] + ["batched-d", "batched-z"] +
            [f"gradcheck-{'z' if z else 'd'}-{t}{'-equil' if e else ''}" for z, t, e in AUTOGRAD_GRADCHECKS] + ["bookkeeping", "singular", "only-b"])


class DevBuf:
    """device memory through the HIP runtime itself (the library has initialised it; no second framework in the process)"""
    hip = None

    def __init__(self, a):
        import ctypes as C, os
        if DevBuf.hip is None:
            DevBuf.hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.a = np.ascontiguousarray(a)
        self.ptr = C.c_void_p()
        assert DevBuf.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(max(self.a.nbytes, 1))) == 0
        assert DevBuf.hip.hipMemcpy(self.ptr, self.a.ctypes.data_as(C.c_void_p), C.c_size_t(self.a.nbytes), 1) == 0      # hipMemcpyHostToDevice

    def data_ptr(self):
        return self.ptr.value

    def host(self):
        import ctypes as C
        out = np.empty_like(self.a)
        assert DevBuf.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes), 2) == 0           # hipMemcpyDeviceToHost
        return out

    def free(self):
        DevBuf.hip.hipFree(self.ptr)
