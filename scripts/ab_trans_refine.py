"""Cost of a transposed refinement step against the untransposed one on ONE handle: the bench operator (Poisson N^3, nested dissection, leaf 64, maxsup 256,
one right-hand side) for trans = N and T, and the complex16 zgrid2d operator (M x M complex 5-point grid, maxsup 64) for N and C.
Per (operator, trans), wall-clock around the device-pointer call (it synchronises its stream before it returns), medians of `reps` calls after a warm-up:
  pass   a call with b = 0, x = 0: berr = 0 at the first pass, no step -- ONE residual / berr pass (kernel + the 8-byte maximum back to the host)
  call   a call with b = op(A) xtrue, x = 0: K steps = K solves + K updates + (K + 1) passes
  step   (call - pass) / K: one solve, one update, one pass
  share  pass / step: what the residual kernel (with its launch and its synchronisation) takes of a step
and the one-off build of the transposed index (sluamd_setup_times: refine.transposed_index), paid by the first transposed call.
usage: ab_trans_refine.py [N [M [reps]]] [--header]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.init()                              # before the library initialises the runtime
from superlu_dist_amd import driver, matgen

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 100
M = int(args[1]) if len(args) > 1 else 1000
reps = int(args[2]) if len(args) > 2 else 10


def timed(h, d_b, d_x0, n, trans, dt):
    x = d_x0.clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    berr, steps = h.pdgsrfs3d_dev(d_b.data_ptr(), n, x.data_ptr(), n, 1, trans=trans)
    return (time.perf_counter() - t0) * 1e3, steps, float(berr[0])


def measure(tag, n, rp, ci, v, perm, maxsup, transes):
    z = np.iscomplexobj(v)
    dt = torch.complex128 if z else torch.float64
    symb = driver.Symbolic(n, rp, ci, perm, relax=64, maxsup=maxsup)
    h = driver.LUHandle.from_symbolic(symb, v)
    assert h.pdgstrf3d(driver.pivot_thresh(n, rp, ci, v)) == 0
    h.attach_matrix(n, rp, ci, v, symb.perm_c)
    import scipy.sparse as sp
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    xt = np.where((np.arange(n) % 2) == 1, 1.0, -1.0).astype(v.dtype) * ((1 + 0.5j) if z else 1.0)
    zero = torch.zeros(n, dtype=dt, device="cuda")
    for trans in transes:
        opA = A if trans == "N" else (A.conj().T if trans == "C" else A.T)
        d_b = torch.from_numpy(np.ascontiguousarray(opA @ xt)).cuda()
        tp, tc, ks, be = [], [], [], []
        for it in range(reps + 2):
            tp.append(timed(h, zero, zero, n, trans, dt)[0])
            t, k, e = timed(h, d_b, zero, n, trans, dt)
            tc.append(t); ks.append(k); be.append(e)
        assert len(set(ks)) == 1 and ks[0] > 0, ks
        K = ks[0]
        p, c = float(np.median(tp[2:])), float(np.median(tc[2:]))
        step = (c - p) / K
        build = h.setup_times().get("refine.transposed_index", 0.0) * 1e3
        print(f"{tag} n={n} nnz={len(v)} trans={trans} | pass {p:8.3f} ms | call {c:8.3f} ms K={K} berr={be[-1]:.2e} | step {step:8.3f} ms | share {100 * p / step:5.1f} % | "
              f"index build {build:8.3f} ms" + (" (first call included it)" if trans != "N" and trans == transes[1] else ""))
    h.destroy(); symb.free()


if "--header" in sys.argv:
    print("# operator n nnz trans | one residual pass | a call of K steps | one step = (call - pass) / K | pass / step | one-off transposed index (host counting sort + upload)")
n, rp, ci, v = matgen.poisson3d(N)
measure(f"poisson3d {N}^3", n, rp, ci, v, matgen.nd_perm_grid3d(N, N, N, leaf=64), 256, ("N", "T"))
n, rp, ci, v = matgen.poisson3d(0, M, M, 1)
v = matgen.complex_shift(v, rp, ci, seed=20)
measure(f"zgrid2d {M}^2", n, rp, ci, v, matgen.nd_perm_grid3d(M, M, 1, leaf=64), 64, ("N", "C"))
