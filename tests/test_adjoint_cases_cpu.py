"""The adjoint value gradient without a device: the new entry points of the cross-built library, the argument checks of the Python layer, the cases of
tests/adjoint_cases.py checked against themselves, and the formulas of include/superlu_dist_amd.h checked against torch on dense matrices."""
import os, re
import numpy as np
import pytest
import adjoint_cases as ac
from superlu_dist_amd import _lib, driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sluamd_dAdjointValues", "sluamd_dAdjointValues_dev", "sluamd_zAdjointValues", "sluamd_zAdjointValues_dev",
       "sluamd_dBatchAdjointValues", "sluamd_dBatchAdjointValues_dev", "sluamd_zBatchAdjointValues", "sluamd_zBatchAdjointValues_dev"]


def test_library_exports_binding_header_and_map_list_the_new_entry_points():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "superlu_dist_amd.h")).read()
    vmap = open(os.path.join(ROOT, "superlu_dist_amd", "csrc", "sluamd.map")).read()
    for s in NEW:
        assert hasattr(L, s), s
        assert s in _lib.EXPORTS, s
        assert len(getattr(L, s).argtypes) == (11 if "Batch" in s else 8), s
        assert re.search(r"\bint " + s + r"\(", hdr), s
        assert re.search(r"\b" + s + ";", vmap), s


def test_adjoint_values_refuses_its_arguments_without_a_device():
    h = driver.LUHandle(None)
    h.n, h.nnz = 4, 6
    ok = np.zeros((4, 2))
    for lam, x, kw in ((ok.astype(np.float32), ok, {}), (ok, ok.astype(np.complex128), {}), (np.zeros((5, 2)), np.zeros((5, 2)), {}), (ok, np.zeros((4, 3)), {}),
                       (np.zeros((4, 2, 1)), np.zeros((4, 2, 1)), {}), (np.zeros((8, 4))[::2, ::2], ok, {}), (ok, ok, dict(trans="H"))):
        with pytest.raises(ValueError):
            h.adjoint_values(lam, x, **kw)
    with pytest.raises(ValueError):
        h.adjoint_values_dev(0, 4, 0, 4, 1, 0, trans="X")
    hz = driver.LUHandle(None)
    hz.n, hz.nnz, hz.z = 4, 6, True
    with pytest.raises(ValueError):
        hz.adjoint_values(ok, ok)
    for cls, dt in ((driver.BatchHandle, np.float64), (driver.ZBatchHandle, np.complex128)):
        b = cls(None, 4, 6, 3)
        good = np.zeros((3, 4, 2), dtype=dt)
        for lam, x, kw in ((np.zeros((3, 4, 2), dtype=np.float32), good, {}), (np.zeros((2, 4, 2), dtype=dt), np.zeros((2, 4, 2), dtype=dt), {}),
                           (good, np.zeros((3, 4), dtype=dt), {}), (good, good, dict(trans="Q"))):
            with pytest.raises(ValueError):
                b.adjoint_values(lam, x, **kw)


def _torch():
    """torch, imported by the tests that need it and after the library: a module-level import would put torch's bundled ROCm runtime into every pytest process
    that merely collects this file"""
    _lib.load()
    import torch
    return torch


@pytest.mark.parametrize("name", ["SparseLU", "BatchedSparseLU"])
def test_solve_refuses_its_arguments_without_a_device(name):
    torch = _torch()
    from superlu_dist_amd import autograd
    cls = getattr(autograd, name)
    n, rp, ci = 3, np.array([0, 1, 3, 4]), np.array([0, 0, 1, 2])
    with pytest.raises(ValueError):
        cls(n, rp, ci, dtype=torch.float32)
    with pytest.raises(ValueError):
        cls(n, rp[:-1], ci)
    lu = cls(n, rp, ci)
    lead = () if cls is autograd.SparseLU else (2,)
    v = torch.zeros(lead + (4,), dtype=torch.float64); b = torch.zeros(lead + (3,), dtype=torch.float64)
    bad = [(v.float(), b, {}),                                                    # dtype
           (v.to(torch.complex128), b, {}),
           (v, b.float(), {}),
           (torch.zeros(lead + (5,), dtype=torch.float64), b, {}),                # shape
           (torch.zeros(lead + (4, 1), dtype=torch.float64), b, {}),
           (v, torch.zeros(lead + (4,), dtype=torch.float64), {}),                # b of the wrong length
           (v, torch.zeros(lead + (3, 2, 1), dtype=torch.float64), {}),
           (torch.zeros(lead + (8,), dtype=torch.float64)[..., ::2], b, {}),      # contiguity
           (v, torch.zeros(lead + (3, 4), dtype=torch.float64)[..., ::2], {}),
           (v, b, dict(trans="X")),                                               # trans
           (v.numpy(), b, {}),
           (v, b, {})]                                                            # not on a device
    for vv, bb, kw in bad:
        with pytest.raises(ValueError):
            lu.solve(vv, bb, **kw)
    if cls is autograd.SparseLU:
        with pytest.raises(ValueError, match="refine"):
            lu.solve(v, b, trans="T", refine=True)
    assert lu.generation == 0 and lu.stats() == {"generation": 0}


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_kernel_cases_prove_themselves(z):
    names = list(ac.kcases())
    for want in ("nnz255", "nnz256", "nnz257", "nnz513", "nrhs1", "nrhs3", "nrhs4", "nrhs5", "nrhs16", "nrhs17", "empty_rows", "long_row", "duplicate", "n1"):
        assert want in names
    for name in names:
        c = ac.kcase(name, z)
        c.check()
        assert np.array_equal(np.repeat(np.arange(c.n), np.diff(c.rowptr)), c.rows) and c.colind.min() >= 0 and c.colind.max() < c.n
        # the formulas against numpy on the same integers (exact in fp64 by the bound)
        li, xj = c.lam[c.rows, :], c.x[c.colind, :]
        lj, xi = c.lam[c.colind, :], c.x[c.rows, :]
        assert np.array_equal(c.expected_np("N"), -(li * np.conj(xj)).sum(1))
        assert np.array_equal(c.expected_np("T"), -(np.conj(xi) * lj).sum(1))
        assert np.array_equal(c.expected_np("C"), -(xi * np.conj(lj)).sum(1))
    for nnz in (255, 256, 257, 513):
        assert ac.kcase(f"nnz{nnz}", z).nnz == nnz
    c = ac.kcase("empty_rows", z)
    d = np.diff(c.rowptr)
    assert d[0] == 0 and d[-1] == 0 and d[7] == 0 and d[8] == 0
    assert np.diff(ac.kcase("long_row", z).rowptr).max() >= 300
    c = ac.kcase("duplicate", z)
    pairs = list(zip(c.rows.tolist(), c.colind.tolist()))
    dup = [e for e in range(1, c.nnz) if pairs[e] == pairs[e - 1]]
    assert len(dup) == 1 and all(c.expected(t)[dup[0]] == c.expected(t)[dup[0] - 1] != (0, 0) for t in ac.TRANS)


@pytest.mark.parametrize("z,nrhs", [(False, 1), (False, 5), (True, 1), (True, 5)])
def test_exact_solve_cases_prove_themselves(z, nrhs):
    c = ac.lucase(z, nrhs)                                           # (the constructor asserts the integer bounds)
    assert 40 <= c.n <= 100
    A = ac.to_np(c.A, z)
    dense = np.zeros((c.n, c.n), dtype=A.dtype); dense[c.rows, c.cols] = c.values
    assert np.array_equal(dense, A)
    for trans in ac.TRANS:
        x, lam, G = c.expected(trans)
        op = {"N": A, "T": A.T, "C": A.conj().T}[trans]
        assert np.array_equal(op @ ac.to_np(x, z), ac.to_np(c.b, z))
        assert np.abs(ac.to_np(G, z)).max() > 0
    if z:
        assert any(np.abs(ac.to_np(c.expected(t)[2], z).imag).max() > 0 for t in ac.TRANS)


def _dense_solve():
    torch = _torch()

    class DenseSolve(torch.autograd.Function):
        """the forward and backward of autograd.SparseLU restated densely: torch.linalg.solve on the CPU, the hand-written backward of the three formulas"""

        @staticmethod
        def forward(ctx, values, b, rows, cols, n, trans):
            A = torch.zeros((n, n), dtype=values.dtype).index_put((rows, cols), values.detach(), accumulate=True)
            x = torch.linalg.solve(_op(A, trans), b.detach())
            ctx.A, ctx.x, ctx.rows, ctx.cols, ctx.trans = A, x, rows, cols, trans
            return x

        @staticmethod
        def backward(ctx, g):
            A, x, rows, cols, trans = ctx.A, ctx.x, ctx.rows, ctx.cols, ctx.trans
            if trans == "N":
                lam = torch.linalg.solve(A.conj().T, g)
                G = -(lam[rows] * x[cols].conj()).sum(1)
            elif trans == "T":
                lam = torch.linalg.solve(A, g.conj()).conj()
                G = -(x[rows].conj() * lam[cols]).sum(1)
            else:
                lam = torch.linalg.solve(A, g)
                G = -(x[rows] * lam[cols].conj()).sum(1)
            return G, lam, None, None, None, None

    return DenseSolve


def _op(A, trans):
    return A if trans == "N" else A.T if trans == "T" else A.conj().T


def _dense_autograd(values, b, rows, cols, n, trans):
    torch = _torch()
    A = torch.zeros((n, n), dtype=values.dtype).index_put((rows, cols), values, accumulate=True)
    return torch.linalg.solve(_op(A, trans), b)


@pytest.mark.parametrize("trans", ac.TRANS)
@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_the_formulas_pass_gradcheck_on_the_matrices_of_the_gpu_test(z, trans):
    torch = _torch()
    DenseSolve = _dense_solve()
    c = ac.gradcheck_case(z)
    n = c["n"]
    rows, cols = torch.as_tensor(c["rows"]), torch.as_tensor(c["cols"])
    dense = np.zeros((n, n), dtype=c["values"].dtype); dense[c["rows"], c["cols"]] = c["values"]
    cond1 = np.linalg.norm(dense, 1) * np.linalg.norm(np.linalg.inv(dense), 1)
    print("cond_1 = %.2f" % cond1)
    assert cond1 <= 100
    v = torch.tensor(c["values"], requires_grad=True); b = torch.tensor(c["b"], requires_grad=True)
    assert torch.autograd.gradcheck(lambda vv, bb: DenseSolve.apply(vv, bb, rows, cols, n, trans), (v, b))
    # ... and torch's own autograd through the dense solve agrees, for a loss with a general gradient
    w = torch.tensor(ac.gradcheck_case(z, seed=9)["b"])

    def grads(fn):
        v.grad = b.grad = None
        out = (w * fn(v, b, rows, cols, n, trans)).sum()
        (out.abs() if z else out).backward()                         # a real loss of a complex sum
        return v.grad.clone(), b.grad.clone()

    for a, r in zip(grads(DenseSolve.apply), grads(_dense_autograd)):
        assert (a - r).abs().max() <= 1e-12 * r.abs().max()
