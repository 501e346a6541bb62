"""Cost of Equil = YES on the bench operator (Poisson N^3, nested dissection, leaf 64, maxsup 256) and A/B of the solve phase of pdgssvx3d on ONE handle:
  1. handle creation (from_symbolic) against sluamd_dEquilibrate on that handle (wall clock, device synchronised) -- on a Poisson operator the outcome is
     N, so a second handle of the same operator under row / column scalings 2^+-20 is timed too (outcome B: scaling, gather and re-distribution run);
  2. the solve phase as the parent's driver does it -- xp[perm_c] = b in numpy, pdgstrs3d on the host vector, [perm_c] in numpy -- against gssvx_solve on the
     same host b, for nrhs = 1 and 16: wall clock of the whole phase, median of `reps` after a warm-up, and max |x_A - x_B|.
usage: ab_equil.py N [reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from superlu_dist_amd import _lib, driver, matgen

N = int(sys.argv[1]); reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
L = _lib.load()
n, rp, ci, v = matgen.poisson3d(N)
perm = matgen.nd_perm_grid3d(N, N, N, leaf=64)
symb = driver.Symbolic(n, rp, ci, perm, relax=64, maxsup=256)


def timed(f):
    L.sluamd_device_synchronize(); t = time.perf_counter(); out = f(); L.sluamd_device_synchronize()
    return out, time.perf_counter() - t


rng = np.random.default_rng(0)
rows = np.repeat(np.arange(n), np.diff(rp))
vs = (v * 2.0 ** rng.integers(-20, 21, n)[rows]) * 2.0 ** rng.integers(-20, 21, n)[ci]
print(f"# N={N} n={n} nnz={len(v)}")
for tag, vals in (("poisson", v), ("poisson scaled 2^+-20", vs)):
    h, t_create = timed(lambda: driver.LUHandle.from_symbolic(symb, vals))
    eq, t_eq = timed(lambda: h.equilibrate(n, rp, ci, vals, symb.perm_c))
    print(f"{tag}: create {t_create * 1e3:.1f} ms | equilibrate {t_eq * 1e3:.1f} ms ({100 * t_eq / t_create:.1f} % of creation) | equed {eq['equed']} "
          f"rowcnd {eq['rowcnd']:.3g} colcnd {eq['colcnd']:.3g} anorm {eq['anorm']:.6g}")
    if tag != "poisson":
        h.destroy()
        continue
    assert h.pdgstrf3d(0.5 * float(np.finfo(np.float32).eps) * eq["anorm"]) == 0
    print("# nrhs | parent solve phase ms (numpy permutations around pdgstrs3d) | gssvx_solve ms | ratio new/parent | max |x_new - x_parent|")
    for nrhs in (1, 16):
        b = np.asfortranarray(rng.standard_normal((n, nrhs)))
        ta, tb = [], []
        for it in range(reps + 2):
            def parent():
                xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b
                return np.asfortranarray(h.pdgstrs3d(xp)[symb.perm_c, :])
            xa, t = timed(parent); ta.append(t)
            xb, t = timed(lambda: h.gssvx_solve(b)); tb.append(t)
        ma, mb = float(np.median(ta[2:])) * 1e3, float(np.median(tb[2:])) * 1e3
        print(f"{nrhs:3d} | {ma:8.3f} | {mb:8.3f} | {mb / ma:5.2f} | {float(np.abs(xa - xb).max()):.2e}")
    h.destroy()
symb.free()
