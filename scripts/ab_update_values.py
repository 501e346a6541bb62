"""Cost of a same-pattern value update on the bench operator (Poisson N^3, nested dissection, leaf 64, maxsup 256): new values for a planned handle, then
pdgstrf3d, four ways on ONE process (wall clock, device synchronised before and after each phase, median of `reps` after two warm-ups):
  1. update_values(numpy array)   sluamd_dUpdateValues: staging copy + zero-fill + one pass over A's entries, then the factorisation
  2. update_values(torch tensor on the device)   sluamd_dUpdateValues_dev: no host copy
  3. destroy + from_symbolic(new values)   what a caller had to do before the entry point existed (the symbolic structure is kept), then the factorisation
  4. reset_values   sluamd_dResetValues on the same handle: the SAME values again -- the yardstick: the expectation to check is that 2. costs this plus one pass
     over A's entries
The values alternate between two perturbations of the operator (same pattern, diagonally dominant), so that no update is a no-op.
usage: ab_update_values.py N [reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.init()                                  # first: torch's HIP context must exist before the library initialises the runtime
from superlu_dist_amd import _lib, driver, matgen

N = int(sys.argv[1]); reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
L = _lib.load()
n, rp, ci, v = matgen.poisson3d(N)
perm = matgen.nd_perm_grid3d(N, N, N, leaf=64)
symb = driver.Symbolic(n, rp, ci, perm, relax=64, maxsup=256)
rows = np.repeat(np.arange(n), np.diff(rp))
vals = [np.where(rows == ci, v * (1.0 + 0.125 * ((rows + s) % 5)), v * (1.0 - 0.0625 * ((np.arange(len(v)) + 3 * s) % 7))) for s in (1, 2)]
dvals = [torch.from_numpy(a).cuda() for a in vals]
torch.cuda.synchronize()                           # the copies ran on torch's stream: complete before the handle's stream reads the tensors
thresh = [driver.pivot_thresh(n, rp, ci, a) for a in vals]


def timed(f):
    L.sluamd_device_synchronize(); t = time.perf_counter(); out = f(); L.sluamd_device_synchronize()
    return out, time.perf_counter() - t


def med(ts):
    return float(np.median(ts[2:])) * 1e3


print(f"# N={N} n={n} nnz={len(v)} reps={reps}")
h = driver.LUHandle.from_symbolic(symb, v)
res = {}
for tag, arrs in (("update host", vals), ("update _dev", dvals)):
    tu, tf = [], []
    for it in range(reps + 2):
        _, t = timed(lambda: h.update_values(arrs[it % 2])); tu.append(t)
        info, t = timed(lambda: h.pdgstrf3d(thresh[it % 2])); tf.append(t)
        assert info == 0
    res[tag] = (med(tu), med(tf))
tu, tf = [], []
for it in range(reps + 2):
    _, t = timed(lambda: h.reset_values()); tu.append(t)
    info, t = timed(lambda: h.pdgstrf3d(thresh[(reps + 1) % 2])); tf.append(t)
    assert info == 0
res["reset (same values)"] = (med(tu), med(tf))
tu, tf = [], []
for it in range(reps + 2):
    def recreate():
        global h
        h.destroy()
        h = driver.LUHandle.from_symbolic(symb, vals[it % 2])
    _, t = timed(recreate); tu.append(t)
    info, t = timed(lambda: h.pdgstrf3d(thresh[it % 2])); tf.append(t)
    assert info == 0
res["destroy + create"] = (med(tu), med(tf))
# the last factorisation holds vals[(reps + 1) % 2]: one solve as a check of the whole loop
k = (reps + 1) % 2
xt = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)[:, None]
b = np.asfortranarray(matgen.csr_matvec(n, rp, ci, vals[k], xt))
xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b
x = h.pdgstrs3d(xp)[symb.perm_c, :]
print(f"# residual of the last system {float(np.linalg.norm(b - matgen.csr_matvec(n, rp, ci, vals[k], x)) / np.linalg.norm(b)):.2e}")
print("# way | new values ms | pdgstrf3d ms | sum ms")
for tag, (a, f) in res.items():
    print(f"{tag:22s} | {a:9.3f} | {f:9.3f} | {a + f:9.3f}")
r, d = res["reset (same values)"][0], res["update _dev"][0]
print(f"# update _dev - reset = {d - r:.3f} ms for one pass over {len(v)} entries ({len(v) * 8 / 1e6:.1f} MB of values)")
h.destroy(); symb.free()
