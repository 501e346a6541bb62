"""Cost of one GMRES iteration of sluamd_pdgsrfs3d_gmres_dev against one plain refinement step of sluamd_pdgsrfs3d_dev on ONE handle: the bench operator
(Poisson N^3, nested dissection, leaf 64, maxsup 256, one right-hand side), and solves-to-eps of both loops on a replace_tiny_pivot case.
Wall-clock around the device-pointer calls (they synchronise their stream before they return), medians of `reps` calls after a warm-up.
  plain   pass = a call with b = 0, x = 0 (one residual pass, no step); call = b = A xtrue, x = 0: K steps;  step = (call - pass) / K
  gmres   the attached matrix is A with its diagonal scaled by 1 + (i mod 5) / 20 -- lagged factors: the cycle does not converge in 20 iterations -- and
          inner_tol = 1e-300, restart = 20, so max_solves = S runs exactly S - 1 iterations and the end of the cycle:
          iteration (2..10) = (t(S = 11) - t(S = 2)) / 9, iteration (11..20) = (t(S = 21) - t(S = 11)) / 10 -- the later ones orthogonalise against more vectors
          (two passes of the Krylov kernels from the 9th basis vector on)
  tiny    n = 257, three cut-off pairs [[4, 4], [4, 4 + 2^-38]] in a diagonally dominant matrix, replace_tiny_pivot = 1, the true matrix attached, x from the
          solve: (berr, steps) of the plain loop, (berr, steps, solves) of the GMRES loop
usage: ab_gmres_refine.py [N [reps]]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.init()                              # before the library initialises the runtime
from superlu_dist_amd import driver, matgen

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 100
reps = int(args[1]) if len(args) > 1 else 7


def timed(h, d_b, d_x0, n, **kw):
    x = d_x0.clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = h.pdgsrfs3d_dev(d_b.data_ptr(), n, x.data_ptr(), n, 1, **kw)
    return (time.perf_counter() - t0) * 1e3, out


def med(f):
    return float(np.median([f() for _ in range(reps + 2)][2:]))


n, rp, ci, v = matgen.poisson3d(N)
symb = driver.Symbolic(n, rp, ci, matgen.nd_perm_grid3d(N, N, N, leaf=64), relax=64, maxsup=256)
h = driver.LUHandle.from_symbolic(symb, v)
assert h.pdgstrf3d(driver.pivot_thresh(n, rp, ci, v)) == 0
import scipy.sparse as sp
A = sp.csr_matrix((v, ci, rp), shape=(n, n))
xt = np.where((np.arange(n) % 2) == 1, 1.0, -1.0)
zero = torch.zeros(n, dtype=torch.float64, device="cuda")
h.attach_matrix(n, rp, ci, v, symb.perm_c)
d_b = torch.from_numpy(np.ascontiguousarray(A @ xt)).cuda()
p = med(lambda: timed(h, zero, zero, n)[0])
K = timed(h, d_b, zero, n)[1][1]
c = med(lambda: timed(h, d_b, zero, n)[0])
step = (c - p) / max(K, 1)
print(f"poisson3d {N}^3 n={n} | plain: pass {p:.3f} ms | call {c:.3f} ms K={K} | step {step:.3f} ms")
rows = np.repeat(np.arange(n), np.diff(rp))
v2 = np.where(rows == ci, v * (1.0 + (rows % 5) / 20.0), v)
h.attach_matrix(n, rp, ci, v2, symb.perm_c)
d_b2 = torch.from_numpy(np.ascontiguousarray(sp.csr_matrix((v2, ci, rp), shape=(n, n)) @ xt)).cuda()
t = {}
for S in (2, 11, 21):
    got = timed(h, d_b2, zero, n, method="gmres", restart=20, inner_tol=1e-300, max_solves=S)[1]
    assert int(got[2][0]) == S and got[1] == 1, (S, got)
    t[S] = med(lambda: timed(h, d_b2, zero, n, method="gmres", restart=20, inner_tol=1e-300, max_solves=S)[0])
it_a, it_b = (t[11] - t[2]) / 9, (t[21] - t[11]) / 10
print(f"poisson3d {N}^3 n={n} | gmres: t(S=2) {t[2]:.3f} ms  t(S=11) {t[11]:.3f} ms  t(S=21) {t[21]:.3f} ms | iteration 2..10 {it_a:.3f} ms ({it_a / step:.2f} x plain step) | "
      f"iteration 11..20 {it_b:.3f} ms ({it_b / step:.2f} x plain step)")
h.destroy(); symb.free()

# replaced tiny pivots
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import gmres_cases as gc
m, S = 257, (9, 100, 201)
T = gc._lu_matrix(m, False).tolil()
for q0 in S:
    for q in (q0, q0 + 1):
        T[q, :] = 0; T[:, q] = 0
    T[q0, q0] = 4.0; T[q0, q0 + 1] = 4.0; T[q0 + 1, q0] = 4.0; T[q0 + 1, q0 + 1] = 4.0 + 2.0 ** -38
T = T.tocsr(); T.eliminate_zeros(); T.sort_indices()
xs = (((3 * np.arange(m) + 7) % 11) - 5).astype(np.float64).reshape(m, 1)
b = np.asfortranarray(T @ xs)
trp, tci = T.indptr.astype(np.int32), T.indices.astype(np.int32)
x, info, st, h, symb = driver.pdgssvx3d(m, trp, tci, T.data, b, replace_tiny=True, keep=True)
h.attach_matrix(m, trp, tci, T.data, symb.perm_c)
_, pb, ps = h.pdgsrfs3d(b, x)
_, gb, gs, gsol = h.pdgsrfs3d(b, x, method="gmres")
print(f"tiny pivots n={m} t=3 | plain: berr {pb[0]:.2e} after {ps} steps ({ps} solves) | gmres: berr {gb[0]:.2e} after {gs} outer steps, {int(gsol[0])} solves")
h.destroy(); symb.free()
