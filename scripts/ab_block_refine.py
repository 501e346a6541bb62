#!/usr/bin/env python3
"""A/B timing (not a test): the blocked refinement sluamd_pdgsrfs3d_block_dev of this build against the column form sluamd_pdgsrfs3d_dev of ANOTHER build of
the library (the parent commit's, given as --parent-lib and loaded through SLUAMD_LIB, as scripts/ab.sh compares two builds), for nrhs = 1, 4, 16, 32 on the
7-point Poisson operator of order N^3.

    python scripts/ab_block_refine.py [N = 100] [--parent-lib PATH/libsluamd.so] [--nrhs 1,4,16,32] [--rounds 3] [--reps 5] [--warmup 2]

Without --parent-lib the column form of this build stands in for the parent (labelled so).  A process loads one build, so every side runs in child
processes of its own, and the two sides ALTERNATE: `rounds` times a column child, then a block child, so that drift of a shared machine hits both sides
alike; the repetitions of all rounds of a side are pooled.  Per child and nrhs: X from the plain solve of random right-hand sides (the same seed everywhere),
copied to the device; a timed call refines a fresh copy of that X in place, between two device synchronisations; `warmup` untimed calls first, then `reps`
timed ones.  The table gives the median and the minimum - maximum range over rounds x reps, the ratio of the medians, and the step counts: for the column
form the count of the LAST right-hand side (all that entry point returns), for the block form the LARGEST of the per-column counts.  The spread to compare a
difference with is the parent's own range.  Results belong in NOTEBOOK.md with the device and build."""
import argparse, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(N, nrhs_list, reps, warmup, block):
    import ctypes as C
    import numpy as np
    from superlu_dist_amd import _lib, driver, matgen
    L = _lib.load()
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    n, rp, ci, v = matgen.poisson3d(N)
    perm = matgen.nd_perm_grid3d(N, N, N, leaf=27) if N <= 20 else driver.order_nd(n, rp, ci)
    rng = np.random.default_rng(0)
    out = {}
    x, info, st, h, symb = driver.pdgssvx3d(n, rp, ci, v, rng.standard_normal((n, 1)), perm, keep=True)
    assert info == 0
    h.attach_matrix(n, rp, ci, v, symb.perm_c)
    for nrhs in nrhs_list:
        b = np.asfortranarray(rng.standard_normal((n, nrhs)))
        xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b
        x0 = np.asfortranarray(h.pdgstrs3d(xp)[symb.perm_c, :])
        dB, dX = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(dB), C.c_size_t(b.nbytes)) == 0 and hip.hipMalloc(C.byref(dX), C.c_size_t(b.nbytes)) == 0
        assert hip.hipMemcpy(dB, b.ctypes.data_as(C.c_void_p), C.c_size_t(b.nbytes), 1) == 0
        ts, steps, berr = [], None, None
        for rep in range(warmup + reps):
            assert hip.hipMemcpy(dX, x0.ctypes.data_as(C.c_void_p), C.c_size_t(b.nbytes), 1) == 0
            hip.hipDeviceSynchronize()
            t0 = time.perf_counter()
            berr, steps = h.pdgsrfs3d_dev(dB.value, n, dX.value, n, nrhs, block=True) if block else h.pdgsrfs3d_dev(dB.value, n, dX.value, n, nrhs)
            hip.hipDeviceSynchronize()
            if rep >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        hip.hipFree(dB); hip.hipFree(dX)
        out[nrhs] = dict(ms=ts, steps=np.atleast_1d(steps).tolist(), berr_max=float(np.max(berr)))
    h.destroy(); symb.free()
    print("RESULT " + json.dumps(out))


def run_side(lib, N, a, block):
    env = dict(os.environ)
    if lib:
        env["SLUAMD_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(N), "--nrhs", a.nrhs, "--reps", str(a.reps), "--warmup", str(a.warmup), "--child",
                        "block" if block else "column"], capture_output=True, text=True, env=env, cwd=ROOT)
    if r.returncode != 0:
        sys.exit(r.stdout[-2000:] + r.stderr[-2000:])
    return {int(k): v for k, v in json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]).items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("N", nargs="?", type=int, default=100)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--nrhs", default="1,4,16,32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    nrhs_list = [int(q) for q in a.nrhs.split(",")]
    if a.child:
        child(a.N, nrhs_list, a.reps, a.warmup, a.child == "block")
        sys.exit(0)
    col, blk = {}, {}
    for rnd in range(a.rounds):                                 # the sides alternate
        for acc, res in ((col, run_side(a.parent_lib, a.N, a, False)), (blk, run_side(None, a.N, a, True))):
            for k, v in res.items():
                if k in acc:
                    acc[k]["ms"] += v["ms"]                     # (the step counts shown are the first round's)
                else:
                    acc[k] = v
    print(f"Poisson {a.N}^3, {a.rounds} alternating rounds of {a.reps} repetitions after {a.warmup} warm-up; column form: "
          + (a.parent_lib or "THIS build (no --parent-lib given)"))
    print(f"{'nrhs':>5s} {'column median [min - max] ms':>36s} {'steps (last)':>13s} {'block median [min - max] ms':>36s} {'steps (max)':>12s} {'column / block':>15s}")
    for k in nrhs_list:
        c, b = col[k]["ms"], blk[k]["ms"]
        mc, mb = statistics.median(c), statistics.median(b)
        print(f"{k:5d} {mc:14.3f} [{min(c):9.3f} - {max(c):9.3f}] {col[k]['steps'][-1]:13d} {mb:14.3f} [{min(b):9.3f} - {max(b):9.3f}] {max(blk[k]['steps']):12d} {mc / mb:15.2f}")
