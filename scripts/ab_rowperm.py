"""A/B of RowPerm = LargeDiag_MC64 (sluamd_dLargeDiag): the hybrid -- device costs, duals and proposal rounds, host augmenting paths for the rows left -- against
SLUAMD_ROWPERM_HOST=1, where the host matches every row from the same device-computed costs and duals.  Two operators: 7-point Poisson N^3 with its rows
shuffled, and the audikw_1 stand-in (matgen.elasticity3d_like(M, drop=0.05, seed=1), the bench's configuration).  Wall clock of the whole call, median of
`reps` after a warm-up; the library's own per-phase line (SLUAMD_ROWPERM_VERBOSE=1, stderr) of the last repetition follows each row.
usage: ab_rowperm.py [N=100] [M=68] [reps=3]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from superlu_dist_amd import _lib, driver, matgen

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100
M = int(sys.argv[2]) if len(sys.argv) > 2 else 68
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
L = _lib.load()


def shuffled(n, rp, ci, v, seed=5):
    sh = np.random.default_rng(seed).permutation(n)
    pr = np.empty(n, dtype=np.int64); pr[sh] = np.arange(n)                     # row k of the result is row sh[k]
    return driver.permute_rows_csr(n, rp, ci, v, pr)[:3]


def run(tag, n, rp, ci, v):
    print(f"# {tag}: n={n} nnz={len(v)}", flush=True)
    res = {}
    for mode, host in (("hybrid", "0"), ("host", "1")):
        os.environ["SLUAMD_ROWPERM_HOST"] = host
        ts = []
        for it in range(reps + 1):
            os.environ["SLUAMD_ROWPERM_VERBOSE"] = "1" if it == reps else "0"
            sys.stderr.flush()
            L.sluamd_device_synchronize(); t = time.perf_counter()
            perm_r, r, c, info = driver.large_diag(n, rp, ci, v)
            ts.append(time.perf_counter() - t)
        res[mode] = (float(np.median(ts[1:])), perm_r, r, c, info)
        print(f"{tag} | {mode:6s} | {res[mode][0] * 1e3:9.1f} ms | rounds {info['rounds']} | matched_device / n = {info['matched_device'] / n:.4f} | "
              f"augmentations {info['augmentations']} | info {info['info']}", flush=True)
    a, b = res["hybrid"], res["host"]
    rows = np.repeat(np.arange(n), np.diff(rp))
    for mode, (_, perm_r, r, c, info) in res.items():
        s = r[rows] * np.abs(v) * c[ci]
        print(f"{tag} | {mode:6s} | max |r a c| - 1 = {s.max() - 1:.2e} | sum log2 |diag| = {np.log2(np.abs(v[ci == perm_r[rows]])).sum():.6f}")
    print(f"{tag} | speed-up hybrid over host: {b[0] / a[0]:.2f} x | same perm_r: {bool(np.array_equal(a[1], b[1]))}", flush=True)


n, rp, ci, v = matgen.poisson3d(N)
run(f"poisson {N}^3 shuffled", n, *shuffled(n, rp, ci, v))
n, rp, ci, v = matgen.elasticity3d_like(M, drop=0.05, seed=1)
run(f"audikw stand-in {M}", n, rp, ci, v)
