"""Differentiable sparse solves on the resident factors: x = op(A)^-1 b as a torch.autograd.Function whose backward is one solve with the adjoint operator and
the sampled outer product of sluamd_[dz]AdjointValues on A's pattern (formulas per trans: include/superlu_dist_amd.h).

    lu = SparseLU(n, rowptr, colind)                     # symbolic factorisation and plan, once
    x = lu.solve(values, b)                              # values: the nnz stored values as a device tensor, b: (n,) or (n, nrhs)
    loss(x).backward()                                   # values.grad: (nnz,), b.grad: the shape of b

torch is imported here, not by the package.  Import torch (or this module) BEFORE the first call into the library in a process: torch.cuda reports no device
once the library has initialised the HIP runtime on its own.  All numerics run in the library; Python only keeps the books: which tensor, at which version, the factors belong
to.  Gradients follow PyTorch's convention for complex tensors.  Not here: double backward and torch.func transforms (the backward is once_differentiable),
process grids, row permutations, gradients through the extra-precise and GMRES refinements."""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import driver

_ADJ_REAL = {"N": "T", "T": "N", "C": "N"}
_ADJ_CPLX = {"N": "C", "T": "N", "C": "N"}        # "T": conjugate in, conjugate out around the untransposed solve


def _torch_dtype(dtype):
    if dtype not in (torch.float64, torch.complex128):
        raise ValueError(f"dtype must be torch.float64 or torch.complex128, not {dtype!r}")
    return dtype


def _check_pattern(n, rowptr, colind):
    n = int(n)
    rp = np.ascontiguousarray(rowptr, dtype=np.int32); ci = np.ascontiguousarray(colind, dtype=np.int32)
    if n < 1 or rp.shape != (n + 1,) or rp[0] != 0 or ci.shape != (int(rp[-1]),):
        raise ValueError(f"rowptr must have {n + 1} entries starting at 0 and colind rowptr[n] entries, got shapes {rp.shape} and {ci.shape}")
    return n, rp, ci


def _check_trans(trans, refine):
    driver._trans_code(trans)
    t = str(trans).upper()
    if refine and t != "N":
        raise ValueError("refine=True belongs to trans='N': the expert solve refines the untransposed system only")
    return t


def _check_tensor(who, what, t, dtype, shapes, device):
    """dtype, shape, contiguity, then the device: ValueError before any library call"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: {what} must be a torch tensor, not {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{who}: the factorisation holds {dtype} values, {what} is {t.dtype}")
    if tuple(t.shape) not in shapes and not any(len(s) == t.dim() and s[-1] is None and tuple(t.shape[:-1]) == s[:-1] for s in shapes):
        raise ValueError(f"{who}: {what} must have one of the shapes {[tuple('nrhs' if v is None else v for v in s) for s in shapes]}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {what} is not contiguous")
    if t.device.type != "cuda":
        raise ValueError(f"{who}: {what} is on {t.device}, the factors live on a HIP device")
    if device is not None and t.device.index != device:
        raise ValueError(f"{who}: {what} is on {t.device}, the factorisation on device {device}")


def _sync(device):
    torch.cuda.current_stream(device).synchronize()      # the library reads and writes on its own stream


class _Base:
    def __init__(self, n, rowptr, colind, dtype, perm_c, equil, relax, maxsup, device):
        self.dtype = _torch_dtype(dtype)
        self.z = dtype == torch.complex128
        self.n, self.rowptr, self.colind = _check_pattern(n, rowptr, colind)
        self.nnz = int(self.rowptr[-1])
        self.equil = bool(equil)
        self.device = None if device is None else torch.device(device).index
        self._symb_args = (perm_c, int(relax), int(maxsup))
        self.symb = None
        self.generation = 0            # factorisations so far; a backward belongs to the generation of its forward
        self._of = None                # (values tensor, its _version) of the resident factors; the reference keeps the tensor alive and its id unique

    def _symbolic(self):
        if self.symb is None:
            perm_c, relax, maxsup = self._symb_args
            self.symb = driver.Symbolic(self.n, self.rowptr, self.colind, perm_c, relax, maxsup)
        return self.symb

    def _current(self, values):
        return self._of is not None and self._of[0] is values and self._of[1] == values._version

    def _claim_device(self, values):
        if self.device is None:
            self.device = values.device.index

    def _factored(self, values):
        self.generation += 1
        self._of = (values, values._version)


class SparseLU(_Base):
    """The factorisation of one sparsity pattern for values that change: the symbolic factorisation, the plan and the handle are made once
    (driver.Symbolic, LUHandle.from_symbolic), the first values attach (or, with equil=True, equilibrate) the matrix, later values go through update_values
    and pdgstrf3d.  dtype torch.float64 or torch.complex128; perm_c None: the natural order is what Symbolic makes of it; device None: the device of the
    first values."""

    def __init__(self, n, rowptr, colind, dtype=torch.float64, perm_c=None, equil=False, relax=32, maxsup=256, device=None):
        super().__init__(n, rowptr, colind, dtype, perm_c, equil, relax, maxsup, device)
        self.handle = None

    def _factor(self, values):
        """the factors of `values`: nothing when they are the resident ones (the same tensor object at the same _version)"""
        if self._current(values):
            return
        self._of = None
        self._claim_device(values)
        _sync(values.device)
        if self.handle is None:
            symb = self._symbolic()
            v0 = values.detach().cpu().numpy()
            with torch.cuda.device(self.device):
                h = driver.LUHandle.from_symbolic(symb, v0, device=self.device)
                if self.equil:
                    h.equilibrate(self.n, self.rowptr, self.colind, v0, symb.perm_c)
                else:
                    h.attach_matrix(self.n, self.rowptr, self.colind, v0, symb.perm_c)
            self.handle = h
        else:
            self.handle.update_values(values.detach())
        info = self.handle.pdgstrf3d(0.0)
        if info != 0:
            raise RuntimeError(f"SparseLU: the matrix is singular to working precision: zero pivot in column {info} (1-based, after perm_c)")
        self._factored(values)

    def solve(self, values, b, trans="N", refine=False):
        """x = op(A)^-1 b for the matrix whose stored values are `values` (1-D device tensor of nnz entries, the order of rowptr / colind); b (n,) or
        (n, nrhs) on the same device; trans "N" / "T" / "C": A x = b, A^T x = b, A^H x = b.  Refactors when `values` is not the tensor object, at the
        _version, of the resident factors.  refine=True (trans "N"): iterative refinement in the forward; the gradient is that of the exact solution.
        Differentiable with respect to values and b (once).  ValueError, before any library call: wrong dtype, shape, contiguity, device, trans.
        RuntimeError: a zero pivot; a backward after the handle was refactored with other values."""
        t = _check_trans(trans, refine)
        _check_tensor("SparseLU.solve", "values", values, self.dtype, [(self.nnz,)], self.device)
        _check_tensor("SparseLU.solve", "b", b, self.dtype, [(self.n,), (self.n, None)], values.device.index)
        self._factor(values)
        return _Solve.apply(values, b, self, t, bool(refine))

    def stats(self):
        """the handle's stats plus `generation`, the number of factorisations so far"""
        st = {} if self.handle is None else self.handle.stats()
        st["generation"] = self.generation
        return st

    def destroy(self):
        if self.handle is not None:
            self.handle.destroy()
            self.handle = None
        if self.symb is not None:
            self.symb.free()
            self.symb = None
        self._of = None


def _cols(t, lead):
    """[..lead.., n(, nrhs)] -> a contiguous [..lead.., nrhs, n]: every matrix's block column-major with ld = n"""
    t = t.detach().resolve_conj()
    return (t.unsqueeze(-1) if t.dim() == lead + 1 else t).transpose(-1, -2).contiguous()


def _rows(tc, like):
    """the inverse of _cols: back to the shape of `like`"""
    out = tc.transpose(-1, -2)
    return out.reshape(like.shape).contiguous()


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, b, lu, trans, refine):
        n = lu.n
        bc = _cols(b, 0)
        xc = torch.empty_like(bc)
        nrhs = bc.shape[0]
        _sync(b.device)
        lu.handle.gssvx_solve_dev(bc.data_ptr(), n, xc.data_ptr(), n, nrhs, trans=trans, refine=refine)
        ctx.lu, ctx.trans, ctx.generation, ctx.xc = lu, trans, lu.generation, xc
        return _rows(xc, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        lu, trans, xc = ctx.lu, ctx.trans, ctx.xc
        if ctx.generation != lu.generation:
            raise RuntimeError("SparseLU: the factors were replaced since this solve (another values tensor, or the same one modified in place, was "
                               "factored): its backward would differentiate against the wrong factors")
        n, nrhs = lu.n, xc.shape[0]
        flip = lu.z and trans == "T"                      # conj(A)^-1 g = conj(A^-1 conj(g))
        gc = _cols(gx.conj() if flip else gx, 0)
        lam = torch.empty_like(gc)
        _sync(gx.device)
        lu.handle.gssvx_solve_dev(gc.data_ptr(), n, lam.data_ptr(), n, nrhs, trans=(_ADJ_CPLX if lu.z else _ADJ_REAL)[trans])
        if flip:
            lam = lam.conj().resolve_conj()
        gv = gb = None
        if ctx.needs_input_grad[0]:
            gv = torch.empty(lu.nnz, dtype=lu.dtype, device=gx.device)
            _sync(gx.device)
            lu.handle.adjoint_values_dev(lam.data_ptr(), n, xc.data_ptr(), n, nrhs, gv.data_ptr(), trans=trans)
        if ctx.needs_input_grad[1]:
            gb = _rows(lam, gx)
        return gv, gb, None, None, None


class BatchedSparseLU(_Base):
    """SparseLU for `count` matrices of one pattern (driver.BatchHandle / ZBatchHandle: one block-diagonal factorisation): values [count, nnz],
    b [count, n] or [count, n, nrhs]; the gradients have the shapes of values and b.  count is that of the first values."""

    def __init__(self, n, rowptr, colind, dtype=torch.float64, perm_c=None, equil=False, relax=32, maxsup=256, device=None):
        super().__init__(n, rowptr, colind, dtype, perm_c, equil, relax, min(int(maxsup), 256), device)
        self.batch = None
        self.count = None

    def _factor(self, values):
        if self._current(values):
            return
        self._of = None
        self._claim_device(values)
        _sync(values.device)
        if self.batch is None:
            symb = self._symbolic()
            cls = driver.ZBatchHandle if self.z else driver.BatchHandle
            with torch.cuda.device(self.device):
                self.batch = cls.create(symb, values.detach().cpu().numpy(), device=self.device)
                self.count = self.batch.count
                if self.equil:
                    self.batch.equilibrate()
        else:
            self.batch.update_values(values.detach())
        info = self.batch.factor()
        if info.any():
            k = int(np.flatnonzero(info)[0])
            raise RuntimeError(f"BatchedSparseLU: matrix {k} is singular to working precision: zero pivot in column {int(info[k])} (1-based, after perm_c)")
        self._factored(values)

    def solve(self, values, b, trans="N"):
        """x_k = op(A_k)^-1 b_k: values [count, nnz], b [count, n] or [count, n, nrhs] device tensors; as SparseLU.solve, without refinement"""
        t = _check_trans(trans, False)
        who = "BatchedSparseLU.solve"
        count = self.count if self.count is not None else (values.shape[0] if isinstance(values, torch.Tensor) and values.dim() == 2 else 0)
        _check_tensor(who, "values", values, self.dtype, [(count, self.nnz)], self.device)
        _check_tensor(who, "b", b, self.dtype, [(count, self.n), (count, self.n, None)], values.device.index)
        self._factor(values)
        return _BatchSolve.apply(values, b, self, t)

    def stats(self):
        st = {} if self.batch is None else self.batch.stats()
        st["generation"] = self.generation
        return st

    def destroy(self):
        if self.batch is not None:
            self.batch.destroy()
            self.batch = None
        if self.symb is not None:
            self.symb.free()
            self.symb = None
        self._of = None


class _BatchSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, b, lu, trans):
        n = lu.n
        bc = _cols(b, 1)                                  # [count, nrhs, n]
        xc = torch.empty_like(bc)
        nrhs = bc.shape[1]
        _sync(b.device)
        lu.batch.solve_dev(bc.data_ptr(), n, n * nrhs, xc.data_ptr(), n, n * nrhs, nrhs, trans=trans)
        ctx.lu, ctx.trans, ctx.generation, ctx.xc = lu, trans, lu.generation, xc
        return _rows(xc, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        lu, trans, xc = ctx.lu, ctx.trans, ctx.xc
        if ctx.generation != lu.generation:
            raise RuntimeError("BatchedSparseLU: the factors were replaced since this solve: its backward would differentiate against the wrong factors")
        n, nrhs = lu.n, xc.shape[1]
        flip = lu.z and trans == "T"
        gc = _cols(gx.conj() if flip else gx, 1)
        lam = torch.empty_like(gc)
        _sync(gx.device)
        lu.batch.solve_dev(gc.data_ptr(), n, n * nrhs, lam.data_ptr(), n, n * nrhs, nrhs, trans=(_ADJ_CPLX if lu.z else _ADJ_REAL)[trans])
        if flip:
            lam = lam.conj().resolve_conj()
        gv = gb = None
        if ctx.needs_input_grad[0]:
            gv = torch.empty((lu.count, lu.nnz), dtype=lu.dtype, device=gx.device)
            _sync(gx.device)
            lu.batch.adjoint_values_dev(lam.data_ptr(), n, n * nrhs, xc.data_ptr(), n, n * nrhs, nrhs, gv.data_ptr(), lu.nnz, trans=trans)
        if ctx.needs_input_grad[1]:
            gb = _rows(lam, gx)
        return gv, gb, None, None
