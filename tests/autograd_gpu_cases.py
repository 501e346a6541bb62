"""The bodies of tests/test_gpu_autograd.py.  They run in a CHILD process that imports torch first: torch.cuda reports no device once the library has
initialised the HIP runtime in a process (tests/test_gpu_update_values.py, tests/test_gpu_zrefine.py), so superlu_dist_amd.autograd cannot be exercised inside
the pytest process, which the other GPU tests have long since put the library into.  `python autograd_gpu_cases.py <repository root>` runs every case and
prints one line "RESULT {case id: "ok" | traceback}"; test_gpu_autograd.py runs it once and asserts case by case."""
import json, os, sys, traceback
import numpy as np
import torch                                   # first: torch's HIP context must exist before the library initialises the runtime

if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import adjoint_cases as ac
from superlu_dist_amd import _lib
from superlu_dist_amd.autograd import SparseLU, BatchedSparseLU

GRADCHECKS, EXACT = ac.AUTOGRAD_GRADCHECKS, ac.AUTOGRAD_EXACT


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(t, want, z):
    """bitwise up to the sign of a zero: the integers are exact in fp64"""
    return np.array_equal(t.detach().cpu().numpy(), ac.to_np(want, z).reshape(tuple(t.shape)))


def loss_of(w, x):
    s = (w * x).sum()
    return s.real if x.is_complex() else s


def raises(exc, match, fn):
    try:
        fn()
    except exc as e:
        assert match in str(e), str(e)
        return
    raise AssertionError(f"{exc.__name__} expected")


_exact = {}


def exact_lu(z, nrhs):
    """(case, SparseLU) per (z, nrhs): one symbolic factorisation and handle serves the three trans values"""
    if (z, nrhs) not in _exact:
        c = ac.lucase(z, nrhs)
        _exact[(z, nrhs)] = (c, SparseLU(c.n, c.rowptr, c.colind, dtype=torch.complex128 if z else torch.float64, perm_c=np.arange(c.n, dtype=np.int32),
                                         relax=2, maxsup=6))
    return _exact[(z, nrhs)]


def integer_system(z, nrhs, trans):
    c, lu = exact_lu(z, nrhs)
    values = dev(c.values).requires_grad_()
    b = dev(ac.to_np(c.b, z)[:, 0] if nrhs == 1 else ac.to_np(c.b, z)).requires_grad_()
    w = dev(ac.to_np(c.w, z)[:, 0] if nrhs == 1 else ac.to_np(c.w, z))
    x = lu.solve(values, b, trans=trans)
    assert x.shape == b.shape and x.device == b.device
    loss_of(w, x).backward()
    ex, elam, eG = c.expected(trans)
    assert lu.handle.stats()["num_levels"] > 2                       # several supernodes and levels
    assert same(x, ex, z), "x"
    assert same(b.grad, elam, z), "b.grad"
    assert values.grad.shape == (c.nnz,) and same(values.grad, eG, z), "values.grad"


def batched_integer_systems(z):
    """count = 3: the case's matrix, its negative and its double (the entries stay integers; the inverse of 2 A is exact in binary)"""
    c = ac.lucase(z, 5)
    lu = BatchedSparseLU(c.n, c.rowptr, c.colind, dtype=torch.complex128 if z else torch.float64, perm_c=np.arange(c.n, dtype=np.int32), relax=2, maxsup=6)
    scale = np.array([1.0, -1.0, 2.0])
    values = dev(scale[:, None] * c.values[None, :]).requires_grad_()
    b0, w0 = ac.to_np(c.b, z), ac.to_np(c.w, z)
    b = dev(np.stack([b0, b0, 2 * b0])).requires_grad_()              # x_k = +x, -x, +x
    w = dev(np.stack([w0, w0, w0]))
    for trans in ac.TRANS:
        values.grad = b.grad = None
        x = lu.solve(values, b, trans=trans)
        loss_of(w, x).backward()
        ex, elam, eG = (ac.to_np(v, z) for v in c.expected(trans))
        assert np.array_equal(x.detach().cpu().numpy(), np.stack([ex, -ex, ex]))
        assert np.array_equal(b.grad.cpu().numpy(), np.stack([elam, -elam, elam / 2]))
        assert values.grad.shape == (3, c.nnz) and np.array_equal(values.grad.cpu().numpy(), np.stack([eG, eG, eG / 2]))
    assert lu.generation == 1
    lu.destroy()


def gradcheck_general(z, trans, equil):
    """torch's defaults (eps 1e-6, atol 1e-5, rtol 1e-3) on the matrix vetted by the dense restatement of tests/test_adjoint_cases_cpu.py.  gradcheck
    evaluates the function once, then many times at perturbed inputs, and only then runs the backward of the first evaluation: on one SparseLU that backward
    would meet the factors of the last perturbation and be refused, as it must.  Every evaluation therefore gets a factorisation of its own (and with it the
    attach / equilibrate path of first values); gradcheck also perturbs through .data, which leaves _version alone"""
    c = ac.gradcheck_case(z)

    def fn(v, bb):
        lu = SparseLU(c["n"], c["rowptr"], c["colind"], dtype=torch.complex128 if z else torch.float64, equil=equil, relax=2, maxsup=4)
        return lu.solve(v, bb, trans=trans)

    values = dev(c["values"]).requires_grad_(); b = dev(c["b"]).requires_grad_()
    assert torch.autograd.gradcheck(fn, (values, b))


def factors_follow_the_tensor_and_its_version():
    c = ac.gradcheck_case(False)
    lu = SparseLU(c["n"], c["rowptr"], c["colind"])
    values = dev(c["values"]).requires_grad_(); b = dev(c["b"])
    x1 = lu.solve(values, b)
    assert lu.generation == 1 and lu.stats()["generation"] == 1
    x2 = lu.solve(values, b, trans="T")                               # the same tensor at the same version: no factorisation
    assert lu.generation == 1
    with torch.no_grad():
        values.mul_(2.0)                                              # modified in place: the version moves
    x3 = lu.solve(values, b)
    assert lu.generation == 2
    assert torch.allclose(x3, x1.detach() / 2, rtol=1e-12, atol=0)
    raises(RuntimeError, "factors", lambda: x1.sum().backward())      # x1 and x2 belong to generation 1
    raises(RuntimeError, "factors", lambda: x2.sum().backward())
    x3.sum().backward()
    assert values.grad is not None
    other = values.detach().clone()
    lu.solve(other, b)                                                # another tensor object of equal content factors too
    assert lu.generation == 3
    lu.destroy()


def singular_matrix_names_the_column():
    n, rp, ci = 3, np.array([0, 1, 2, 3]), np.array([0, 1, 2])
    lu = SparseLU(n, rp, ci, perm_c=np.arange(3, dtype=np.int32))
    raises(RuntimeError, "column 2", lambda: lu.solve(dev(np.array([1.0, 0.0, 3.0])), dev(np.ones(3))))
    assert lu.generation == 0
    lu.destroy()


def only_b_needs_a_gradient():
    """the entry -> row array is allocated by the first values kernel: without one, the backward allocates nothing through the library"""
    count = lambda: int(_lib.load().sluamd_device_alloc_count())
    c = ac.gradcheck_case(False)
    lu = SparseLU(c["n"], c["rowptr"], c["colind"])
    values = dev(c["values"]); b = dev(c["b"]).requires_grad_()
    lu.solve(values, b).sum().backward()                              # warm: the solve's own work vectors exist now
    b.grad = None
    x = lu.solve(values, b)
    before = count()
    x.sum().backward()
    assert count() == before and b.grad is not None
    v2 = values.clone().requires_grad_()
    x = lu.solve(v2, b)
    before = count()
    x.sum().backward()
    assert count() == before + 1 and v2.grad is not None             # the entry -> row array, once
    lu.destroy()


def cases():
    fns = ([lambda a=a: integer_system(*a) for a in EXACT] + [lambda: batched_integer_systems(False), lambda: batched_integer_systems(True)] +
           [lambda a=a: gradcheck_general(*a) for a in GRADCHECKS] + [factors_follow_the_tensor_and_its_version, singular_matrix_names_the_column, only_b_needs_a_gradient])
    return list(zip(ac.autograd_case_ids(), fns))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "torch sees no HIP device"
    torch.cuda.init()
    out = {}
    for name, fn in cases():
        try:
            fn()
            out[name] = "ok"
        except Exception:
            out[name] = traceback.format_exc()[-1500:]
    print("RESULT " + json.dumps(out))
