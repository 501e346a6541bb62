"""Transposed against untransposed GRID solves of one matrix (Poisson N^3, nested dissection, leaf 64, maxsup 256) on 1 x 1 x 1, 1 x 1 x 2 and 2 x 2 x 1,
the ranks as threads of this process on ONE GPU over the in-process transport (grid3d.local_comms) -- what the exchanges cost there is host staging, not xGMI.
Per grid and nrhs = 1, 4: `reps` replicated solves each way on a device-resident right-hand side after two warm-up solves; one table line with the median of
stats()["t_solve_ms"] (slowest rank), the DAG levels this rank 0 sweeps and the ratio.  Not a gate: the expectation is a ratio near 1 on the XY grids, where
both forms run two launches and two exchanges per level and sweep (on 1 x 1 layers the untransposed sweeps run their joined one-launch links).
usage: ab_trans_solve_grid.py N [reps]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
import torch
from superlu_dist_amd import _lib, driver, grid3d, matgen

torch.cuda.init()          # before the library initialises the HIP runtime in this process
N = int(sys.argv[1]); reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
n, rp, ci, v = matgen.poisson3d(N)
perm = matgen.nd_perm_grid3d(N, N, N, leaf=64)
symb = driver.Symbolic(n, rp, ci, perm, relax=64, maxsup=256)
fn = _lib.entry("sluamd_pdgstrs3d_trans_dev")
print("# grid nrhs | untransposed ms (median, slowest rank) | transposed ms | ratio T/N | levels (rank 0) | max |x_T - x_N| (symmetric operator: the same system)")
for grid in ((1, 1, 1), (1, 1, 2), (2, 2, 1)):
    Pr, Pc, Pz = grid
    P = Pr * Pc * Pz
    tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)
    for nrhs in (1, 4):
        b = torch.randn(nrhs, n, dtype=torch.float64, device="cuda")           # column-major n x nrhs
        torch.cuda.synchronize()

        def body(rank):
            h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], tree)
            try:
                assert h.pdgstrf3d(0.0) == 0
                h.plan_transposed()
                tn, tt = [], []
                for it in range(reps + 2):
                    xt = b.clone(); torch.cuda.synchronize()
                    _lib.check(fn(h._h, 1, C.c_void_p(xt.data_ptr()), n, nrhs), "trans"); tt.append(h.stats()["t_solve_ms"])
                    xn = b.clone(); torch.cuda.synchronize()
                    _lib.check(fn(h._h, 0, C.c_void_p(xn.data_ptr()), n, nrhs), "notrans"); tn.append(h.stats()["t_solve_ms"])
                return float(np.median(tn[2:])), float(np.median(tt[2:])), len(h.plan_table()), float((xt - xn).abs().max())
            finally:
                h.destroy()

        out = grid3d.run_ranks(P, body)
        mn, mt = max(o[0] for o in out), max(o[1] for o in out)
        print(f"{Pr}x{Pc}x{Pz} {nrhs:3d} | {mn:8.3f} | {mt:8.3f} | {mt / mn:5.2f} | {out[0][2]:4d} | {max(o[3] for o in out):.2e}")
symb.free()
