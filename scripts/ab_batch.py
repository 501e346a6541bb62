#!/usr/bin/env python3
"""A/B timing (not a test): `count` same-pattern systems as ONE batched handle (driver.BatchHandle) against a loop of `count` LUHandles, on the same build and
in the same process: creation, factorisation, solve.  Shifted 3-D Poisson operators A_k = A + (k / 4) I of order N^3.

    python scripts/ab_batch.py [--cases 12x256,8x512,16x64] [--reps 7] [--warmup 2] [--nrhs 1] [--complex] [--trefine]

--complex: the same comparison for complex16 (driver.ZBatchHandle against a loop of complex16 LUHandles) with complex shifts A_k = A + (k / 4)(1 + i) I: the
frequency sweep of one discretisation.
--trefine: one batch (double, or complex16 with --complex); per repetition the solve without and with refinement, of A_k x = b and of the transposed system
(A_k^T x = b; complex16: A_k^H x = b).  The table gives the four medians, the largest step count s of a matrix, and per system the cost of one refinement
sweep, (refined - unrefined) / (s + 1): a refined solve makes s + 1 residual passes, s of them followed by a correction and an update.

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


def systems(N, count, nrhs, z):
    n, rp, ci, v = matgen.poisson3d(N)
    rows = np.repeat(np.arange(n), np.diff(rp))
    shift = 0.25 * (1 + 1j) if z else 0.25
    vals = np.stack([v + np.where(rows == ci, shift * k, 0.0) for k in range(count)])
    rng = np.random.default_rng(0)
    b = rng.uniform(-1, 1, size=(count, n, nrhs))
    if z:
        b = b + 1j * rng.uniform(-1, 1, size=(count, n, nrhs))
    return n, rp, ci, vals, b, driver.order_nd(n, rp, ci)


def case(N, count, reps, warmup, nrhs, z):
    n, rp, ci, vals, b, perm = systems(N, count, nrhs, z)
    Batch = driver.ZBatchHandle if z else driver.BatchHandle
    t = {k: [] for k in ("create_batch", "create_loop", "factor_batch", "factor_loop", "solve_batch", "solve_loop")}
    for rep in range(warmup + reps):
        def mk_batch():
            s = driver.Symbolic(n, rp, ci, perm)
            h = Batch.create(s, vals)
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
                xp = np.zeros((n, nrhs), dtype=b.dtype, order="F"); xp[pc, :] = b[k]
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
    print(f"{'complex16' if z else 'double'}: N = {N} (n = {n}), count = {count}, nrhs = {nrhs}, {reps} repetitions after {warmup} warm-up")
    print(f"{'phase':8s} {'batch median [min - max] ms':>34s} {'loop median [min - max] ms':>34s} {'loop / batch':>13s}")
    for ph in ("create", "factor", "solve"):
        a, l = t[ph + "_batch"], t[ph + "_loop"]
        ma, ml = statistics.median(a), statistics.median(l)
        print(f"{ph:8s} {ma:12.3f} [{min(a):9.3f} - {max(a):9.3f}] {ml:12.3f} [{min(l):9.3f} - {max(l):9.3f}] {ml / ma:13.2f}")


def trefine_case(N, count, reps, warmup, nrhs, z):
    n, rp, ci, vals, b, perm = systems(N, count, nrhs, z)
    s = driver.Symbolic(n, rp, ci, perm)
    bh = (driver.ZBatchHandle if z else driver.BatchHandle).create(s, vals)
    s.free()
    assert not bh.factor().any()
    tt = "C" if z else "T"
    keys = [(tr, rf) for tr in ("N", tt) for rf in (False, True)]
    t = {k: [] for k in keys}
    steps = {}
    for rep in range(warmup + reps):
        for k in keys:                                  # the four solves alternate inside every repetition
            ms, (_, _, st) = timed(lambda: bh.solve(b, trans=k[0], refine=k[1]))
            steps[k] = int(st.max())
            if rep >= warmup:
                t[k].append(ms)
    bh.destroy()
    print(f"{'complex16' if z else 'double'}: N = {N} (n = {n}), count = {count}, nrhs = {nrhs}, {reps} repetitions after {warmup} warm-up")
    print(f"{'system':8s} {'solve median [min - max] ms':>34s} {'refined median [min - max] ms':>34s} {'steps':>6s} {'ms / sweep':>11s}")
    per = {}
    for tr in ("N", tt):
        a, r = t[(tr, False)], t[(tr, True)]
        ma, mr, st = statistics.median(a), statistics.median(r), steps[(tr, True)]
        per[tr] = (mr - ma) / (st + 1)
        print(f"{tr:8s} {ma:12.3f} [{min(a):9.3f} - {max(a):9.3f}] {mr:12.3f} [{min(r):9.3f} - {max(r):9.3f}] {st:6d} {per[tr]:11.3f}")
    print(f"one {tt} sweep / one N sweep: {per[tt] / per['N']:.2f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="12x256,8x512,16x64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nrhs", type=int, default=1)
    ap.add_argument("--complex", action="store_true", help="complex16 systems (ZBatchHandle)")
    ap.add_argument("--trefine", action="store_true", help="refinement of the transposed system against the untransposed one, on one batch")
    a = ap.parse_args()
    if _lib.load().sluamd_device_count() < 1:
        sys.exit("no HIP device")
    for c in a.cases.split(","):
        N, count = (int(q) for q in c.split("x"))
        (trefine_case if a.trefine else case)(N, count, a.reps, a.warmup, a.nrhs, a.complex)
