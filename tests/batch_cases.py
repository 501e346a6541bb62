"""Batches of same-pattern systems (sluamd_dBatch*, sluamd_symb_replicate) -- test helper for test_gpu_batch.py and test_batch_cases_cpu.py; not a conftest.

Exact cases.  A_k = L_k U_k with L_k = I + S_k unit lower, U_k = D_k + T_k upper, all on ONE pattern:
  S_k: entries in {-2 .. 2} \\ {0} at (i, j), i odd > j even;   T_k: the same at (i, j), i even < j odd;   D_k: powers of two 1, 2, 4.
No index is both a source and a target of S (or of T), so S^2 = 0 and T D^-1 T = 0: inv(L) = I - S, inv(U) = D^-1 - D^-1 T D^-1, and the same holds for every
principal submatrix, i.e. for every diagonal block of every supernode partition under any symmetric permutation.  Every quantity a factorisation or a sweep
can form -- Schur partial sums, pivots, panel times inverse block, Linv / Uinv, the sweeps' partial sums for an integer solution -- is then an integer or a
dyadic rational with at most four fractional bits and a magnitude far below 2^40: exact in fp64 in ANY summation order and kernel form.  That matters because a
batch of more than one matrix has no single-supernode level, so it never takes the tail forms (SLUAMD_TRSM_TAIL, SLUAMD_DIAG_TAIL) a lone matrix takes:
floating-point results of the two paths cannot be compared bit for bit, exact ones can.
The pattern of A is that of D + T + S + S T (structural, matrix-independent), stored with explicit zeros where a product cancels; `dense_tail` adds the full
trailing block to the pattern (explicit zeros), which gives the symbolic factorisation one wide supernode there.

Float cases: the same pattern, off-diagonal values uniform in [-1, 1], diagonal = 2 (sum of the row's moduli) + 1: strictly diagonally dominant by rows,
cond_2 <= 100 checked on the dense blocks (test_batch_cases_cpu.py).

Singular case: D_k[c0] = 0 for one matrix: the leading principal minors of A_k are the products of D_k, so elimination without pivoting meets its first zero
pivot exactly at (permuted) column perm_c[c0]; `first_zero_pivot` finds it by a dense elimination in numpy."""
import functools
import numpy as np

# (m, count, maxsup, dense_tail): a matrix boundary inside a 256-thread block (40, 100), at one past it (257), past it (300), many matrices of one wave (64)
SHAPES = {"m40x7": (40, 7, 64, 0), "m100x5": (100, 5, 64, 0), "m257x3": (257, 3, 64, 0), "m300x2": (300, 2, 256, 80), "m64x33": (64, 33, 64, 0),
          "m100x1": (100, 1, 64, 0)}
NRHS = (1, 3, 17)


def _pattern(m, dense_tail, seed):
    """boolean masks of S (strictly lower, odd row, even column) and T (strictly upper, even row, odd column): a band of half-width 3 plus a few long links"""
    rng = np.random.default_rng(seed)
    i, j = np.indices((m, m))
    band = np.abs(i - j) <= 3
    far = rng.random((m, m)) < 2.0 / m
    tail = (i >= m - dense_tail) & (j >= m - dense_tail)
    keep = band | far | tail
    S = keep & (i > j) & (i % 2 == 1) & (j % 2 == 0)
    T = keep & (i < j) & (i % 2 == 0) & (j % 2 == 1)
    P = S | T | (i == j) | ((S.astype(np.int64) @ T.astype(np.int64)) > 0) | tail
    return S, T, P


def _csr_of(P):
    m = P.shape[0]
    rows, cols = np.nonzero(P)                       # row-major: ascending columns inside a row
    rp = np.zeros(m + 1, dtype=np.int32)
    np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp).astype(np.int32), cols.astype(np.int32), rows


class BatchCase:
    """count matrices of order m on one pattern; dense[k], values [count, nnz] in CSR order, the exact factors where the case has them"""

    def __init__(self, name, m, count, maxsup, rp, ci, rows, dense, L=None, U=None):
        self.name, self.m, self.count, self.maxsup = name, m, count, maxsup
        self.rp, self.ci, self.rows = rp, ci, rows
        self.nnz = int(rp[-1])
        self.dense = dense
        self.L, self.U = L, U
        self.values = np.ascontiguousarray(dense[:, rows, ci])

    def rhs(self, nrhs, seed=5):
        """integer solutions x [count, m, nrhs] in -3 .. 3 and b = A x (exact), bt = A^T x"""
        rng = np.random.default_rng(seed + 1000 * nrhs + self.m)
        x = rng.integers(-3, 4, size=(self.count, self.m, nrhs)).astype(np.float64)
        b = np.einsum("kij,kjr->kir", self.dense, x)
        bt = np.einsum("kji,kjr->kir", self.dense, x)
        return x, b, bt


def _exact_factors(m, count, S, T, seed, singular=None):
    rng = np.random.default_rng(seed)
    nz = np.array([-2, -1, 1, 2], dtype=np.float64)
    L = np.zeros((count, m, m)); U = np.zeros((count, m, m))
    for k in range(count):
        L[k] = np.eye(m) + np.where(S, rng.choice(nz, size=(m, m)), 0.0)
        U[k] = np.diag(2.0 ** rng.integers(0, 3, size=m)) + np.where(T, rng.choice(nz, size=(m, m)), 0.0)
    if singular is not None:
        k, c0 = singular
        U[k, c0, c0] = 0.0
    return L, U


@functools.lru_cache(maxsize=None)
def exact_case(name, seed=0, singular=None):
    """singular = (k, c0): matrix k gets D[c0] = 0; every other matrix is the one of the regular case with the same seed"""
    m, count, maxsup, tail = SHAPES[name]
    S, T, P = _pattern(m, tail, 11)
    rp, ci, rows = _csr_of(P)
    L, U = _exact_factors(m, count, S, T, 100 + seed, singular)
    dense = np.einsum("kij,kjl->kil", L, U)
    assert not np.any(dense[:, ~P])                  # the pattern holds all of every A_k
    c = BatchCase(name, m, count, maxsup, rp, ci, rows, dense, L, U)
    for a in (c.dense, c.values, c.L, c.U):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def float_case(name, seed=0):
    m, count, maxsup, tail = SHAPES[name]
    _, _, P = _pattern(m, tail, 11)
    rp, ci, rows = _csr_of(P)
    rng = np.random.default_rng(200 + seed)
    dense = np.where(P, rng.uniform(-1.0, 1.0, size=(count, m, m)), 0.0)
    i = np.arange(m)
    dense[:, i, i] = 0.0
    dense[:, i, i] = 2.0 * np.abs(dense).sum(axis=2) + 1.0
    c = BatchCase(name, m, count, maxsup, rp, ci, rows, dense)
    c.dense.setflags(write=False); c.values.setflags(write=False)
    return c


def first_zero_pivot(A, perm):
    """0-based column of the first exactly zero pivot of elimination without pivoting on A1 = Pc A Pc^T (perm[old] = new), or -1"""
    m = A.shape[0]
    inv = np.empty(m, dtype=np.int64); inv[np.asarray(perm)] = np.arange(m)
    W = np.array(A[np.ix_(inv, inv)], dtype=np.float64)
    for c in range(m):
        if W[c, c] == 0.0:
            return c
        W[c + 1:, c] /= W[c, c]
        W[c + 1:, c + 1:] -= np.outer(W[c + 1:, c], W[c, c + 1:])
    return -1


def block_diag_csr(c, values=None):
    """(n, rowptr, colind, values) of diag(A_0 .. A_{count-1}), matrix-major"""
    v = c.values if values is None else values
    rp = np.concatenate([c.rp[:-1] + k * c.nnz for k in range(c.count)] + [[c.count * c.nnz]]).astype(np.int32)
    ci = np.concatenate([c.ci + k * c.m for k in range(c.count)]).astype(np.int32)
    return c.m * c.count, rp, ci, np.ascontiguousarray(v[:, :c.nnz]).reshape(-1)
