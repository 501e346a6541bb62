#!/usr/bin/env python3
"""A/B timing (not a test): `count` same-pattern systems as ONE batched handle (driver.BatchHandle) against a loop of `count` LUHandles, on the same build and
in the same process: creation, factorisation, solve.  Shifted 3-D Poisson operators A_k = A + (k / 4) I of order N^3.

    python scripts/ab_batch.py [--cases 12x256,8x512,16x64] [--reps 7] [--warmup 2] [--nrhs 1]

Method: both sides share one ordering and (for the loop) one symbolic factorisation per handle, as a user would pay them; every timed region ends with a
device synchronisation (the library's factor and solve calls synchronise themselves, creation is host-synchronous); `warmup` untimed repetitions first
(code objects, the device pool, clocks), then `reps` timed ones, alternating A and B inside every repetition so that drift hits both alike; the table gives
the median and the minimum - maximum range of the wall-clock times in milliseconds and the ratio of the medians.  The numbers include the host side (planning,
table uploads, launches): that is the point of the comparison.  Results belong in NOTEBOOK.md with the device and build they were taken on."""
import argparse, os, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from superlu_dist_amd import _lib, driver, matgen


def timed(fn):
    _lib.load().sluamd_device_synchronize()
    t0 = time.perf_counter()
    out = fn()
    _lib.load().sluamd_device_synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def case(N, count, reps, warmup, nrhs):
    n, rp, ci, v = matgen.poisson3d(N)
    rows = np.repeat(np.arange(n), np.diff(rp))
    vals = np.stack([v + np.where(rows == ci, 0.25 * k, 0.0) for k in range(count)])
    b = np.random.default_rng(0).uniform(-1, 1, size=(count, n, nrhs))
    perm = driver.order_nd(n, rp, ci)
    t = {k: [] for k in ("create_batch", "create_loop", "factor_batch", "factor_loop", "solve_batch", "solve_loop")}
    for rep in range(warmup + reps):
        def mk_batch():
            s = driver.Symbolic(n, rp, ci, perm)
            h = driver.BatchHandle.create(s, vals)
            s.free()
            return h

        def mk_loop():
            hs = []
            for k in range(count):
                s = driver.Symbolic(n, rp, ci, perm)
                hs.append((driver.LUHandle.from_symbolic(s, vals[k]), s.perm_c.copy()))
                s.free()
            return hs
        tb, bh = timed(mk_batch)
        tl, hs = timed(mk_loop)
        fb, info = timed(bh.factor)
        fl, _ = timed(lambda: [h.pdgstrf3d() for h, _ in hs])
        assert not info.any()
        sb, (x, _, _) = timed(lambda: bh.solve(b))

        def solve_loop():
            out = []
            for k, (h, pc) in enumerate(hs):
                xp = np.zeros((n, nrhs), order="F"); xp[pc, :] = b[k]
                out.append(h.pdgstrs3d(xp)[pc, :])
            return out
        sl, xs = timed(solve_loop)
        assert max(np.abs(x[k] - xs[k]).max() for k in range(count)) < 1e-10
        bh.destroy()
        for h, _ in hs:
            h.destroy()
        if rep >= warmup:
            for key, val in zip(t, (tb, tl, fb, fl, sb, sl)):
                t[key].append(val)
    print(f"N = {N} (n = {n}), count = {count}, nrhs = {nrhs}, {reps} repetitions after {warmup} warm-up")
    print(f"{'phase':8s} {'batch median [min - max] ms':>34s} {'loop median [min - max] ms':>34s} {'loop / batch':>13s}")
    for ph in ("create", "factor", "solve"):
        a, l = t[ph + "_batch"], t[ph + "_loop"]
        ma, ml = statistics.median(a), statistics.median(l)
        print(f"{ph:8s} {ma:12.3f} [{min(a):9.3f} - {max(a):9.3f}] {ml:12.3f} [{min(l):9.3f} - {max(l):9.3f}] {ml / ma:13.2f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="12x256,8x512,16x64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nrhs", type=int, default=1)
    a = ap.parse_args()
    if _lib.load().sluamd_device_count() < 1:
        sys.exit("no HIP device")
    for c in a.cases.split(","):
        N, count = (int(q) for q in c.split("x"))
        case(N, count, a.reps, a.warmup, a.nrhs)
