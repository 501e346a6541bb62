"""Timing of the adjoint value gradient on the Poisson problem N^3 (default 100^3), nrhs 1 and 16; one step per process:
  --step a   the values kernel against one residual pass (sluamd_dResidual_dev, one column) of the same build on the same matrix
  --step b   the values kernel against the torch formulation a caller would write: expanded row index, two index_select, multiply, sum
  --step c   the whole backward of autograd.SparseLU.solve (adjoint solve + values kernel) against one forward solve
Every figure is the wall clock of a complete call between device synchronisations (both library entries synchronise their stream before returning, the
torch formulation is followed by torch.cuda.synchronize()): launch and synchronisation overheads are inside every number.  Median and minimum of --reps
calls after --warmup calls.  Prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, sync, warmup, reps):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e6)
    out.sort()
    return dict(median_us=round(out[len(out) // 2], 1), min_us=round(out[0], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices="abc", required=True)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    from superlu_dist_amd import driver, matgen
    from superlu_dist_amd.autograd import SparseLU
    N = a.N
    n, rp, ci, v = matgen.poisson3d(N)
    perm = matgen.nd_perm_grid3d(N, N, N, leaf=27)
    nnz = len(ci)
    res = dict(step=a.step, N=N, n=int(n), nnz=int(nnz))
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(0)
    if a.step in "ab":
        symb = driver.Symbolic(n, rp, ci, perm)
        h = driver.LUHandle.from_symbolic(symb, v)
        h.attach_matrix(n, rp, ci, v, symb.perm_c)
        for nrhs in (1, 16):
            lam = torch.from_numpy(rng.standard_normal((nrhs, n))).cuda(); x = torch.from_numpy(rng.standard_normal((nrhs, n))).cuda()      # column-major n x nrhs
            g = torch.empty(nnz, dtype=torch.float64, device="cuda")
            sync()
            kern = lambda: h.adjoint_values_dev(lam.data_ptr(), n, x.data_ptr(), n, nrhs, g.data_ptr())
            r = dict(values_kernel=timed(kern, sync, a.warmup, a.reps))
            if a.step == "a":
                rr = torch.empty(n, dtype=torch.float64, device="cuda")
                sync()
                r["residual_pass_1col"] = timed(lambda: h.residual_dev(lam.data_ptr(), n, x.data_ptr(), n, 1, rr.data_ptr(), n), sync, a.warmup, a.reps)
            else:
                rows = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.from_numpy(np.diff(rp).astype(np.int64)).cuda())
                cols = torch.from_numpy(ci.astype(np.int64)).cuda()
                lt, xt = lam.t().contiguous(), x.t().contiguous()      # (n, nrhs) row-major: the layout a torch caller holds
                ref = lambda: -(lt.index_select(0, rows) * xt.index_select(0, cols)).sum(1)
                r["torch_formulation"] = timed(ref, sync, a.warmup, a.reps)
                kern(); sync()
                d = (g - ref()).abs().max().item() / max(g.abs().max().item(), 1e-300)
                r["max_rel_diff"] = d
            res[f"nrhs{nrhs}"] = r
        h.destroy(); symb.free()
    else:
        lu = SparseLU(n, rp, ci, perm_c=perm)
        values = torch.from_numpy(v).cuda().requires_grad_()
        for nrhs in (1, 16):
            b = torch.from_numpy(rng.standard_normal((n, nrhs))).cuda().requires_grad_()
            w = torch.from_numpy(rng.standard_normal((n, nrhs))).cuda()
            lu.solve(values, b)                                        # factors once; later calls find the same tensor at the same version
            fwd = timed(lambda: lu.solve(values, b), sync, 2, 10)

            def back():
                x = lu.solve(values, b)
                sync()
                t0 = time.perf_counter()
                (w * x).sum().backward()
                sync()
                return (time.perf_counter() - t0) * 1e6
            ts = sorted(back() for _ in range(12))[:10]
            res[f"nrhs{nrhs}"] = dict(forward_solve=fwd, backward=dict(median_us=round(ts[len(ts) // 2], 1), min_us=round(ts[0], 1)), generation=lu.generation)
        lu.destroy()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
