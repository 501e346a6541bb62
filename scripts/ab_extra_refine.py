#!/usr/bin/env python3
"""A/B timing (not a test): the extra-precise refinement on the 7-point Poisson operator of order N^3, nrhs = 1.

    python scripts/ab_extra_refine.py [N = 100] [--parent-lib PATH/libsluamd.so] [--rounds 3] [--reps 5] [--warmup 2]

Two comparisons.  (1) One residual pass of THIS build, sluamd_dResidual_dev with extra = 0 against extra = 1: the same launch shape, gathers and
reduction, the doubled accumulation on top.  (2) A whole refinement: sluamd_pdgsrfs3d_extra_dev of this build against sluamd_pdgsrfs3d_dev of ANOTHER build
(the parent commit's, given as --parent-lib and loaded through SLUAMD_LIB; without it the plain form of this build stands in, labelled so).  A process
loads one build, so every side runs in child processes of its own and the sides ALTERNATE, `rounds` times, so that drift of a shared machine hits both
alike; the repetitions of all rounds of a side are pooled.  A timed call runs between two device synchronisations on a fresh copy of the solve's X; the
table gives the median and the minimum - maximum range, and for the refinements the steps taken (the two loops stop by different rules, so the per-step
time is the figure to compare).  Results belong in NOTEBOOK.md with the device and build."""
import argparse, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(N, reps, warmup, side):
    import ctypes as C
    import numpy as np
    from superlu_dist_amd import driver, matgen
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    n, rp, ci, v = matgen.poisson3d(N)
    perm = matgen.nd_perm_grid3d(N, N, N, leaf=27) if N <= 20 else driver.order_nd(n, rp, ci)
    rng = np.random.default_rng(0)
    b = np.asfortranarray(rng.standard_normal((n, 1)))
    x0, info, st, h, symb = driver.pdgssvx3d(n, rp, ci, v, b, perm, keep=True)
    assert info == 0
    h.attach_matrix(n, rp, ci, v, symb.perm_c)
    dB, dX, dR = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for d in (dB, dX, dR):
        assert hip.hipMalloc(C.byref(d), C.c_size_t(b.nbytes)) == 0
    assert hip.hipMemcpy(dB, b.ctypes.data_as(C.c_void_p), C.c_size_t(b.nbytes), 1) == 0
    runs = {"plain": [("refine_plain", lambda: h.pdgsrfs3d_dev(dB.value, n, dX.value, n, 1))],
            "extra": [("pass_plain", lambda: h.residual_dev(dB.value, n, dX.value, n, 1, dR.value, n)),
                      ("pass_extra", lambda: h.residual_dev(dB.value, n, dX.value, n, 1, dR.value, n, extra=True)),
                      ("refine_extra", lambda: h.pdgsrfs3d_dev(dB.value, n, dX.value, n, 1, method="extra"))]}[side]
    out = {}
    for name, call in runs:
        ts, res = [], None
        for rep in range(warmup + reps):
            assert hip.hipMemcpy(dX, x0.ctypes.data_as(C.c_void_p), C.c_size_t(b.nbytes), 1) == 0
            hip.hipDeviceSynchronize()
            t0 = time.perf_counter()
            res = call()
            hip.hipDeviceSynchronize()
            if rep >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(ms=ts)
        if name.startswith("refine"):
            out[name].update(steps=int(np.atleast_1d(res[1])[0]), berr=float(res[0][0]))
        if name == "refine_extra":
            out[name].update(dxrel=float(res[2][0]), state=int(res[3][0]))
    for d in (dB, dX, dR):
        hip.hipFree(d)
    h.destroy(); symb.free()
    print("RESULT " + json.dumps(out))


def run_side(lib, N, a, side):
    env = dict(os.environ)
    if lib:
        env["SLUAMD_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(N), "--reps", str(a.reps), "--warmup", str(a.warmup), "--child", side], capture_output=True,
                       text=True, env=env, cwd=ROOT)
    if r.returncode != 0:
        sys.exit(r.stdout[-2000:] + r.stderr[-2000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("N", nargs="?", type=int, default=100)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.N, a.reps, a.warmup, a.child)
        sys.exit(0)
    acc = {}
    for rnd in range(a.rounds):                                 # the sides alternate
        for res in (run_side(a.parent_lib, a.N, a, "plain"), run_side(None, a.N, a, "extra")):
            for k, v in res.items():
                if k in acc:
                    acc[k]["ms"] += v["ms"]
                else:
                    acc[k] = v
    print(f"Poisson {a.N}^3, nrhs = 1, {a.rounds} alternating rounds of {a.reps} repetitions after {a.warmup} warm-up; refine_plain: "
          + (a.parent_lib or "THIS build (no --parent-lib given)"))
    print(f"{'':>14s} {'median [min - max] ms':>36s} {'steps':>6s} {'ms / step':>10s} {'berr':>10s}")
    for k in ("pass_plain", "pass_extra", "refine_plain", "refine_extra"):
        t = acc[k]["ms"]
        m = statistics.median(t)
        tail = ""
        if "steps" in acc[k]:
            s = acc[k]["steps"]
            tail = f" {s:6d} {m / max(s, 1):10.3f} {acc[k]['berr']:10.2e}"
        print(f"{k:>14s} {m:14.3f} [{min(t):9.3f} - {max(t):9.3f}]" + tail)
    print(f"pass_extra / pass_plain = {statistics.median(acc['pass_extra']['ms']) / statistics.median(acc['pass_plain']['ms']):.2f}")
