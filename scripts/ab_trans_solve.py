"""A/B of the transposed solve against the untransposed one on ONE handle of the bench operator (Poisson N^3, nested dissection, leaf 64, maxsup 256):
alternates pdgstrs3d and pdgstrs3d(trans="T") on a device-resident right-hand side, `reps` solves each after a warm-up, for nrhs = 1, 4, 16, and prints one
table line per (schedule, nrhs) with the medians of stats()["t_solve_ms"] and the launch counts.  The schedule of the UNTRANSPOSED sweeps is what the
environment selects when the handle is created (default: joined links; SLUAMD_SOLVE_JOIN=0: the two-launch links, the like-for-like comparator -- both then
read the factors once per block of right-hand sides, in two launches per level and sweep); the transposed path has one schedule.
usage: ab_trans_solve.py N [reps] [--header] [--profile-only]   (--profile-only: 3 transposed solves with nrhs = 1 and nothing else, for a kernel trace)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from superlu_dist_amd import driver, matgen

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]); reps = int(args[1]) if len(args) > 1 else 10
n, rp, ci, v = matgen.poisson3d(N)
perm = matgen.nd_perm_grid3d(N, N, N, leaf=64)
symb = driver.Symbolic(n, rp, ci, perm, relax=64, maxsup=256)
h = driver.LUHandle.from_symbolic(symb, v)
assert h.pdgstrf3d(0.0) == 0
sched = "join=" + os.environ.get("SLUAMD_SOLVE_JOIN", "1")
if "--header" in sys.argv:
    print("# schedule nrhs | untransposed ms (median of reps) launches | transposed ms (median) launches | ratio T/N | max |x_T - x_N| (symmetric operator: the same system)")
for nrhs in ((1,) if "--profile-only" in sys.argv else (1, 4, 16)):
    b = torch.randn(nrhs, n, dtype=torch.float64, device="cuda")           # column-major n x nrhs
    tn, tt = [], []
    for it in range(3 if "--profile-only" in sys.argv else reps + 2):
        xt = b.clone(); h.pdgstrs3d_dev(xt.data_ptr(), n, nrhs, trans="T"); st = h.stats(); tt.append(st["t_solve_ms"]); lt = st["solve_launches"]
        if "--profile-only" in sys.argv:
            continue
        xn = b.clone(); h.pdgstrs3d_dev(xn.data_ptr(), n, nrhs); st = h.stats(); tn.append(st["t_solve_ms"]); ln = st["solve_launches"]
    if "--profile-only" in sys.argv:
        print(f"# transposed solve, nrhs=1: {tt[-1]:.3f} ms, {lt} launches")
        continue
    mn, mt = float(np.median(tn[2:])), float(np.median(tt[2:]))
    print(f"{sched} {nrhs:3d} | {mn:8.3f} {ln:5d} | {mt:8.3f} {lt:5d} | {mt / mn:5.2f} | {float((xt - xn).abs().max()):.2e}")
h.destroy(); symb.free()
