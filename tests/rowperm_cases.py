"""Cases for RowPerm = LargeDiag_MC64 (sluamd_[dz]LargeDiag) and a numpy restatement of the algorithm the header documents: logarithmic costs through
frexp, initial duals, proposal rounds on the tight entries, shortest augmenting paths with a binary heap.  Shared by test_rowperm_cases_cpu.py (properties
of the cases and of the restatement, no GPU) and test_gpu_rowperm.py.

Exact cases: every entry is +- a power of two (complex16: purely real or purely imaginary), so every cost and dual is an integer held in a double, every
scaling a power of two, and the certificate  |r a c| <= 1, == 1 on the matched entries  holds with zero tolerance."""
import heapq
import itertools
import numpy as np

INF = np.inf
BIG = np.iinfo(np.int64).max


def csr_from_dense(A):
    """CSR of the entries of A that are not exactly zero (ascending columns)"""
    A = np.asarray(A)
    n = A.shape[0]
    rows, cols = np.nonzero(A)
    rp = np.zeros(n + 1, dtype=np.int32); np.add.at(rp, rows + 1, 1); rp = np.cumsum(rp).astype(np.int32)
    return n, rp, cols.astype(np.int32), A[rows, cols].copy()


def dense_from_csr(n, rp, ci, v):
    A = np.zeros((n, n), dtype=np.asarray(v).dtype)
    A[np.repeat(np.arange(n), np.diff(rp)), ci] = v
    return A


# ---- the cases ----

def _cyclic(n):
    """a(i, i+1 mod n) = +-2^(i mod 5) dominates its row and its column; a(i, i) and a(i, i+7 mod n) are smaller than every shift entry"""
    A = np.zeros((n, n))
    for i in range(n):
        A[i, (i + 1) % n] = (-1.0) ** i * 2.0 ** (i % 5)
        A[i, i] = 2.0 ** (i % 5 - 6)
        A[i, (i + 7) % n] = -(2.0 ** -8)
    return A


def _blocks(B, copies, scale=False):
    B = np.asarray(B, dtype=float)
    m = B.shape[0]
    A = np.zeros((m * copies, m * copies))
    for k in range(copies):
        A[m * k:m * k + m, m * k:m * k + m] = B * (2.0 ** (k % 7 - 3) if scale else 1.0)
    return A


def _rand8():
    """n = 8, random sparse, powers of two; the seed is one for which the optimum is unique (test_rowperm_cases_cpu.py proves it by brute force)"""
    rng = np.random.default_rng(RAND8_SEED)
    A = np.zeros((8, 8))
    mask = rng.random((8, 8)) < 0.45
    mask[np.arange(8), rng.permutation(8)] = True            # structurally non-singular
    A[mask] = (rng.choice([-1.0, 1.0], size=(8, 8)) * 2.0 ** rng.integers(-6, 7, size=(8, 8)))[mask]
    return A


RAND8_SEED = 3
POSPATH3 = [[4, 0, 2], [4, 0, 1], [0, 2, 8]]     # rows 0 and 1 are tight to column 0 only, row 2 takes column 1: row 1's shortest path has length 2


def _to_z(A):
    """purely real or purely imaginary entries of the same moduli, by a checkerboard"""
    A = np.asarray(A, dtype=float)
    i, j = np.indices(A.shape)
    return np.where((i + 2 * j) % 3 == 0, 1j, 1.0) * A


EXACT = {
    "n1": lambda: np.array([[-4.0]]),
    "antidiag2": lambda: np.array([[0.0, 2.0], [-8.0, 0.0]]),
    "rand8": _rand8,
    "cyclic64": lambda: _cyclic(64),
    "cyclic65": lambda: _cyclic(65),
    "cyclic257": lambda: _cyclic(257),
    "blocks130": lambda: _blocks([[2, 2], [2, 0]], 65),
    "pospath3": lambda: np.array(POSPATH3, dtype=float),
    "pospath66": lambda: _blocks(POSPATH3, 22, scale=True),
    "z_antidiag2": lambda: _to_z([[0.0, 2.0], [-8.0, 0.0]]),
    "z_rand8": lambda: _to_z(_rand8()),
    "z_cyclic65": lambda: _to_z(_cyclic(65)),
    "z_blocks130": lambda: _to_z(_blocks([[2, 2], [2, 0]], 65)),
    "z_pospath66": lambda: _to_z(_blocks(POSPATH3, 22, scale=True)),
}
UNIQUE = ["n1", "antidiag2", "rand8", "cyclic64", "cyclic65", "cyclic257", "blocks130", "pospath3", "pospath66",
          "z_antidiag2", "z_rand8", "z_cyclic65", "z_blocks130", "z_pospath66"]      # cases whose optimal perm_r is unique
ALL_ON_DEVICE = ["cyclic64", "cyclic65", "cyclic257", "z_cyclic65"]                   # matched_device == n, augmentations == 0
POSITIVE_PATH = ["pospath3", "pospath66", "z_pospath66"]                             # at least one augmenting path of positive length


def case(name):
    return csr_from_dense(EXACT[name]())


def singular(name):
    """structurally singular inputs -> (n, rp, ci, v, expected info)"""
    if name == "shared_column":      # rows 0 and 1 share their only column
        return csr_from_dense(np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 1.0, 4.0]])) + (1,)
    if name == "empty_column":
        return csr_from_dense(np.array([[1.0, 2.0, 0], [0, 1.0, 0], [4.0, 0, 0]])) + (1,)
    if name == "stored_zero":        # the only entry of row 1 is a stored zero
        return 2, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([1.0, 0.0]), 1
    raise KeyError(name)


SINGULAR = ["shared_column", "empty_column", "stored_zero"]


def general300(seed=7):
    """n = 300, unsymmetric random pattern with a zero diagonal, normal values; a shifted cycle keeps it structurally non-singular"""
    n = 300
    rng = np.random.default_rng(seed)
    A = np.where(rng.random((n, n)) < 0.03, rng.standard_normal((n, n)), 0.0)
    A[np.arange(n), (np.arange(n) + 17) % n] = rng.standard_normal(n)
    A[np.arange(n), np.arange(n)] = 0.0
    return csr_from_dense(A)


# ---- the restatement ----

def lg(x):
    """log2 as exponent + log2(mantissa) through frexp; a power of two gives an exact integer"""
    m, e = np.frexp(x)
    with np.errstate(divide="ignore"):
        return np.where(m == 0.5, e - 1.0, e + np.log2(m))


def exp2_exact(x):
    x = np.asarray(x, dtype=float)
    whole = (x == np.floor(x)) & (np.abs(x) < 1000)
    return np.where(whole, np.ldexp(1.0, np.where(whole, x, 0).astype(np.int64)), np.exp2(x))


def modulus(v):
    v = np.asarray(v)
    return np.hypot(v.real, v.imag) if np.iscomplexobj(v) else np.abs(v)


def large_diag_ref(n, rp, ci, v, host_only=False, max_rounds=32):
    """dict(info, perm_r, r, c, u, v, cost, cmax, rounds, matched_device, augmentations, path_lengths)"""
    rp = np.asarray(rp, dtype=np.int64); ci = np.asarray(ci, dtype=np.int64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    mod = modulus(v)
    cmax = np.zeros(n); np.maximum.at(cmax, ci, mod)
    edge = mod > 0
    cost = np.full(len(ci), INF)
    cost[edge] = np.maximum(lg(cmax[ci[edge]]) - lg(mod[edge]), 0.0)
    u = np.full(n, INF); np.minimum.at(u, rows, cost)
    vv = np.full(n, INF)
    with np.errstate(invalid="ignore"):
        red0 = cost - u[rows]
    np.minimum.at(vv, ci[edge], red0[edge])
    rowmatch = np.full(n, -1, dtype=np.int64); colmatch = np.full(n, -1, dtype=np.int64)
    tight = edge & (red0 == vv[ci])
    rounds = matched = 0
    while not host_only and rounds < max_rounds and matched < n:
        free = tight & (rowmatch[rows] < 0) & (colmatch[ci] < 0)
        choice = np.full(n, BIG); np.minimum.at(choice, rows[free], ci[free])
        who = np.nonzero(choice < BIG)[0]
        prop = np.full(n, BIG); np.minimum.at(prop, choice[who], who)
        cols = np.nonzero(prop < BIG)[0]
        colmatch[cols] = prop[cols]; rowmatch[prop[cols]] = cols
        rounds += 1
        if len(cols) == 0:
            break
        matched += len(cols)
    out = dict(rounds=rounds, matched_device=matched, cost=cost, cmax=cmax)
    # shortest augmenting paths
    dist = np.full(n, INF); pred = np.full(n, -1, dtype=np.int64); done = np.zeros(n, dtype=bool)
    unmatched = paths = 0
    lengths = []
    for r0 in range(n):
        if rowmatch[r0] >= 0:
            continue
        heap, touched, settled = [], [], []
        row, drow, sink = r0, 0.0, -1
        while True:
            for e in range(rp[row], rp[row + 1]):
                j = ci[e]
                if not edge[e] or done[j]:
                    continue
                nd = drow + max((cost[e] - u[row]) - vv[j], 0.0)
                if nd < dist[j]:
                    if dist[j] == INF:
                        touched.append(j)
                    dist[j] = nd; pred[j] = row
                    heapq.heappush(heap, (nd, j))
            j = -1
            while heap:
                d, k = heapq.heappop(heap)
                if not done[k] and d == dist[k]:
                    j = k
                    break
            if j < 0:
                break
            done[j] = True; settled.append(j)
            if colmatch[j] < 0:
                sink = j
                break
            row, drow = colmatch[j], dist[j]
        if sink < 0:
            unmatched += 1
        else:
            dsink = dist[sink]
            for j in settled:
                d = dsink - dist[j]
                if j != sink:
                    u[colmatch[j]] += d
                vv[j] -= d
            u[r0] += dsink
            j = sink
            while j >= 0:
                i = pred[j]; jn = rowmatch[i]
                rowmatch[i] = j; colmatch[j] = i
                j = jn
            paths += 1; lengths.append(float(dsink))
        for j in touched:
            dist[j] = INF; pred[j] = -1; done[j] = False
    out.update(info=unmatched, augmentations=paths, path_lengths=lengths, u=u, v=vv)
    if unmatched:
        out.update(perm_r=None, r=None, c=None)
    else:
        out.update(perm_r=rowmatch.astype(np.int32), r=exp2_exact(u), c=exp2_exact(vv) / cmax)
    return out


# ---- what the tests measure ----

def matched_positions(n, rp, ci, perm_r):
    """index in the CSR arrays of the entry (i, perm_r[i]) of every row"""
    pos = np.empty(n, dtype=np.int64)
    for i in range(n):
        e = np.nonzero(np.asarray(ci[rp[i]:rp[i + 1]]) == perm_r[i])[0]
        assert len(e) == 1, f"row {i}: column {perm_r[i]} is not a stored entry"
        pos[i] = rp[i] + e[0]
    return pos


def objective(n, rp, ci, cost, perm_r):
    """sum of the costs on the matched entries (minimal <=> the product of the diagonal moduli is maximal)"""
    return float(np.sum(cost[matched_positions(n, rp, ci, perm_r)]))


def certificate(n, rp, ci, v, perm_r, r, c):
    """(max |r a c| - 1 over all entries, max | |r a c| - 1 | over the matched ones)"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    s = r[rows] * modulus(v) * c[ci]
    return float(s.max() - 1.0), float(np.abs(s[matched_positions(n, rp, ci, perm_r)] - 1.0).max())


def brute_force(A):
    """(minimal cost, the permutations cols[i] that reach it) over all n! assignments of the dense matrix A; exact for power-of-two entries"""
    n = A.shape[0]
    mod = modulus(A)
    with np.errstate(divide="ignore"):
        C = np.where(mod > 0, lg(mod.max(axis=0))[None, :] - lg(np.where(mod > 0, mod, 1.0)), INF)
    perms = np.array(list(itertools.permutations(range(n))))
    tot = C[np.arange(n)[None, :], perms].sum(axis=1)
    best = tot.min()
    return best, perms[tot == best]


def shuffled_poisson(N=8, seed=5):
    """7-point Poisson on N^3 with its rows shuffled by a fixed permutation: (n, rp, ci, v of the shuffled matrix, shuffle, the Poisson CSR).
    Row k of the shuffled matrix is row shuffle[k] of the Poisson matrix, so the matching must return perm_r = shuffle."""
    from superlu_dist_amd import matgen
    n, rp, ci, v = matgen.poisson3d(N)
    shuffle = np.random.default_rng(seed).permutation(n)
    rp = np.asarray(rp, dtype=np.int64)
    cnt = np.diff(rp)[shuffle]
    rp1 = np.zeros(n + 1, dtype=np.int64); np.cumsum(cnt, out=rp1[1:])
    pos = np.repeat(rp[:-1][shuffle] - rp1[:-1], cnt) + np.arange(rp1[n])
    return n, rp1.astype(np.int32), np.asarray(ci)[pos].astype(np.int32), np.asarray(v)[pos].copy(), shuffle.astype(np.int32), (n, rp.astype(np.int32), ci, v)


def child_main():
    """run in a child process (test_gpu_rowperm.py sets SLUAMD_ROWPERM_HOST=1 for it): one JSON line {case: {perm_r, info, counters}} over the exact cases
    and the general one"""
    import json
    from superlu_dist_amd import driver
    out = {}
    for name in list(EXACT) + ["general300"]:
        n, rp, ci, v = general300() if name == "general300" else case(name)
        perm_r, r, c, info = driver.large_diag(n, rp, ci, v)
        out[name] = dict(perm_r=[int(x) for x in perm_r], r=[float(x) for x in r], c=[float(x) for x in c], **info)
    print("ROWPERM_CHILD " + json.dumps(out))


if __name__ == "__main__":
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child_main()
