"""Complex16 batches (sluamd_zBatch*) and transposed refinement on batches -- test helper for test_gpu_zbatch.py, test_gpu_batch_trans_refine.py and
test_zbatch_cases_cpu.py; not a conftest.  Built on batch_cases.py: its patterns, its SHAPES and NRHS, its BatchCase.

Exact cases.  A_k = L_k U_k, L_k = I + S_k, U_k = D_k + T_k on the patterns of batch_cases.py, where S^2 = 0 and T D^-1 T = 0 hold STRUCTURALLY (no index is
both a source and a target), hence for complex values too:
  S_k, T_k: Gaussian integers with parts in -2 .. 2, never 0 + 0i;   D_k: a power of two (1, 2, 4) times a unit (1, i, -1, -i).
A reciprocal of D is a power of two times a unit, a product of two such numbers a Gaussian integer or a dyadic Gaussian rational with at most four fractional
bits, every part of every product and partial sum an integer or such a rational far below 2^40: exact in fp64 in any order and any kernel form, including the
real embedding [re -im; im re] of the complex product on the MFMA path (its entries are the parts).
rhs: Gaussian-integer solutions x (parts in -3 .. 3), b = A x, bt = A^T x, bh = A^H x, all exact.

Float cases: batch_cases.float_case's construction with complex off-diagonal values (both parts uniform in [-1, 1]) and the real diagonal
2 (sum of the row's moduli) + 1: strictly diagonally dominant by rows.

Refinement cases (refine_case): the construction of test_gpu_batch._refine_case.  Factored F_k = diag(d_k) with d_k signed powers of two (complex16: powers of
two times units), attached A'_k = F_k (I + 2^-8 N_k) with N_k nilpotent, strictly upper triangular (NOT symmetric), entries +-1 (complex16: +-1, +-i).  The
refinement of op(A') x = b with the factors of F, started from x0 = op(F)^-1 b, has the error recurrence
  op = N:  e <- -2^-8 N e,      op = T:  e <- -2^-8 D^-1 N^T D e,      op = C:  e <- -2^-8 D^-H N^H D^H e,
all dyadic: it ends at the exact solution after p - 1 steps when N^p = 0.  Matrix 0 has N = 0, matrix 1 N^4 = 0 != N^3, matrix 2 N^2 = 0 and b of the order
2^-1000, below SAFE2, so that every row takes the (SAFE1 + |r|) / t branch.  `replay` runs the loop of pdgsrfs.c / pzgsrfs.c in numpy: every quantity but
the final quotient is exact, the quotient is one correctly rounded division on either side, so steps, berr and x are predicted bit for bit."""
import functools
import numpy as np
import batch_cases as bc

SHAPES, NRHS = bc.SHAPES, bc.NRHS
UNITS = np.array([1, 1j, -1, -1j])
EPS = 2.0 ** -53
SAFMIN = 2.0 ** -1022


class ZBatchCase(bc.BatchCase):
    def rhs(self, nrhs, seed=5):
        """Gaussian-integer solutions x [count, m, nrhs] (parts in -3 .. 3) and b = A x, bt = A^T x, bh = A^H x (exact)"""
        rng = np.random.default_rng(seed + 1000 * nrhs + self.m)
        shape = (self.count, self.m, nrhs)
        x = rng.integers(-3, 4, size=shape) + 1j * rng.integers(-3, 4, size=shape)
        b = np.einsum("kij,kjr->kir", self.dense, x)
        bt = np.einsum("kji,kjr->kir", self.dense, x)
        bh = np.einsum("kji,kjr->kir", self.dense.conj(), x)
        return x, b, bt, bh


def _gauss(rng, shape):
    """Gaussian integers with parts in -2 .. 2, never zero"""
    g = rng.integers(-2, 3, size=shape) + 1j * rng.integers(-2, 3, size=shape)
    return np.where(g == 0, 1 - 1j, g)


def _exact_factors(m, count, S, T, seed, singular=None):
    rng = np.random.default_rng(seed)
    L = np.zeros((count, m, m), dtype=np.complex128); U = np.zeros((count, m, m), dtype=np.complex128)
    for k in range(count):
        L[k] = np.eye(m) + np.where(S, _gauss(rng, (m, m)), 0)
        U[k] = np.diag(2.0 ** rng.integers(0, 3, size=m) * rng.choice(UNITS, size=m)) + np.where(T, _gauss(rng, (m, m)), 0)
    if singular is not None:
        k, c0 = singular
        U[k, c0, c0] = 0
    return L, U


@functools.lru_cache(maxsize=None)
def exact_case(name, seed=0, singular=None):
    """singular = (k, c0): matrix k gets D[c0] = 0; every other matrix is the one of the regular case with the same seed"""
    m, count, maxsup, tail = SHAPES[name]
    S, T, P = bc._pattern(m, tail, 11)
    rp, ci, rows = bc._csr_of(P)
    L, U = _exact_factors(m, count, S, T, 300 + seed, singular)
    dense = np.einsum("kij,kjl->kil", L, U)
    assert not np.any(dense[:, ~P])                  # the pattern holds all of every A_k
    c = ZBatchCase(name, m, count, maxsup, rp, ci, rows, dense, L, U)
    for a in (c.dense, c.values, c.L, c.U):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def float_case(name, seed=0):
    m, count, maxsup, tail = SHAPES[name]
    _, _, P = bc._pattern(m, tail, 11)
    rp, ci, rows = bc._csr_of(P)
    rng = np.random.default_rng(400 + seed)
    dense = np.where(P, rng.uniform(-1.0, 1.0, size=(count, m, m)) + 1j * rng.uniform(-1.0, 1.0, size=(count, m, m)), 0)
    i = np.arange(m)
    dense[:, i, i] = 0
    dense[:, i, i] = 2.0 * np.abs(dense).sum(axis=2) + 1.0
    c = ZBatchCase(name, m, count, maxsup, rp, ci, rows, dense)
    c.dense.setflags(write=False); c.values.setflags(write=False)
    return c


def first_zero_pivot(A, perm):
    """0-based column of the first exactly zero pivot of elimination without pivoting on A1 = Pc A Pc^T (perm[old] = new), or -1"""
    m = A.shape[0]
    inv = np.empty(m, dtype=np.int64); inv[np.asarray(perm)] = np.arange(m)
    W = np.array(A[np.ix_(inv, inv)], dtype=np.complex128)
    for c in range(m):
        if W[c, c] == 0:
            return c
        W[c + 1:, c] /= W[c, c]
        W[c + 1:, c + 1:] -= np.outer(W[c + 1:, c], W[c, c + 1:])
    return -1


# ---- refinement ----
RM = 100


@functools.lru_cache(maxsize=None)
def refine_case(z):
    """(m, count, d [count, m], A' [count, m, m], N [count, m, m], b [count, m, 2]); z: complex16"""
    m, count = RM, 3
    rng = np.random.default_rng(19 if z else 9)
    d = rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], size=(count, m))
    N = np.zeros((count, m, m), dtype=np.complex128 if z else np.float64)
    i = np.arange(m - 1)
    chain = i[(i % 4) != 3]
    ev = i[(i % 2) == 0]
    if z:
        d = d * rng.choice(UNITS, size=(count, m))
        N[1, chain, chain + 1] = rng.choice(UNITS, size=len(chain))
        N[2, ev, ev + 1] = rng.choice(UNITS, size=len(ev))
    else:
        N[1, chain, chain + 1] = rng.choice([-1.0, 1.0], size=len(chain))
        N[2, ev, ev + 1] = rng.choice([-1.0, 1.0], size=len(ev))
    A = np.stack([np.diag(d[k]) @ (np.eye(m) + N[k] / 256.0) for k in range(count)])
    b = rng.integers(1, 8, size=(count, m, 2)).astype(np.float64)
    if z:
        b = b + 1j * rng.integers(-3, 4, size=(count, m, 2))
    b[:, :, 0] *= 2.0
    b[2] *= 2.0 ** -1000
    for a in (d, A, N, b):
        a.setflags(write=False)
    return m, count, d, A, N, b


def op(A, trans):
    return A if trans == "N" else A.T if trans == "T" else A.conj().T


def abs1(v):
    """|re| + |im| (slud_z_abs1); |v| for real arrays"""
    return np.abs(v.real) + np.abs(v.imag) if np.iscomplexobj(v) else np.abs(v)


def replay(d, A, b, trans, safe_n):
    """The refinement loop of one matrix in numpy: factors of diag(d), attached matrix A, system op(A) x = b, one right-hand side b [m]; SAFE1 formed from
    safe_n.  Returns (x, berr, steps, took_safe1) -- took_safe1: every row of every sweep took the (SAFE1 + |r|) / t branch."""
    Ao, fo = op(A, trans), (d.conj() if trans == "C" else d)
    safe1 = (safe_n + 1) * SAFMIN; safe2 = safe1 / EPS
    x = b / fo
    lstres, steps, all_safe1 = 3.0, 0, True
    while True:
        r = b - Ao @ x
        t = abs1(Ao) @ abs1(x) + abs1(b)
        big = t > safe2
        all_safe1 &= not big.any()
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(big, abs1(r) / t, np.where(t != 0.0, (safe1 + abs1(r)) / t, 0.0))
        berr = q.max()
        if not (berr > EPS and berr * 2 <= lstres and steps < 20):
            return x, berr, steps, all_safe1
        x = x + r / fo
        lstres = berr
        steps += 1


def csr(A):
    rows, cols = np.nonzero(A)
    rp = np.zeros(A.shape[0] + 1, dtype=np.int32); np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp).astype(np.int32), cols.astype(np.int32), A[rows, cols]


def block_diag(A):
    count, m, _ = A.shape
    big = np.zeros((count * m, count * m), dtype=A.dtype)
    for k in range(count):
        big[k * m:(k + 1) * m, k * m:(k + 1) * m] = A[k]
    return big
