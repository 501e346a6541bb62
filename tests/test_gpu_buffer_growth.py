"""The grow-only device buffers of a handle (DevBuf::reserve in sluamd_devmem.h) through the files the CPU test build does not link -- sluamd_tsolve.cpp,
sluamd_trefine.cpp, sluamd_equil.cpp, sluamd_update.cpp, sluamd_batch.cpp: ONE handle takes the host-pointer and the device-pointer form of every call
with nrhs 1, then 5 with the leading dimension grown by 3, then 1 again, so every buffer is allocated, freed for a larger one while the stream may still
hold work that used the old one, and then reused at a smaller size.  Every result is compared bit for bit with the same call on a FRESH handle, and the
solves with the integer solution the cases are built around (tests/trans_cases.py "widths", "z_narrow" as the complex16 run; the smallest case of
tests/batch_cases.py).  Then the arena pool is trimmed, the handle re-created, and a solve gives the same bits.  No failure is injected on the GPU.

Each part runs in a child process under a time limit, once (the pattern of test_gpu_grid_trans_exact.py)."""
import ctypes as C
import os, subprocess, sys
import numpy as np
import pytest
import batch_cases as bc
import trans_cases as tc
import update_cases as uc
from superlu_dist_amd import _lib, driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 120
STEPS = ((1, 0), (5, 3), (1, 0))            # (nrhs, rows added to the leading dimension)
I64 = C.c_int64


def _child(fn, *args):
    code = ("import os, sys\nsys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\n"
            "import test_gpu_buffer_growth as t\ngetattr(t, %r)(*%r)\nprint('RESULT ok')\n" % (fn, tuple(args)))
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=CHILD_LIMIT_S, cwd=ROOT)
    sys.stdout.write(r.stdout[-3000:])
    assert r.returncode == 0 and "RESULT ok" in r.stdout, "child exit %d\n" % r.returncode + r.stdout[-1500:] + r.stderr[-2500:]


class _Dev:
    """device memory through the HIP runtime itself (the library has initialised it)"""
    hip = None

    def __init__(self, a):
        if _Dev.hip is None:
            _Dev.hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.a = np.asfortranarray(a)
        self.ptr = C.c_void_p()
        assert _Dev.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(max(self.a.nbytes, 8))) == 0
        assert _Dev.hip.hipMemcpy(self.ptr, self.a.ctypes.data_as(C.c_void_p), C.c_size_t(self.a.nbytes), 1) == 0

    def host(self):
        out = np.empty_like(self.a, order="F")
        assert _Dev.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        _Dev.hip.hipFree(self.ptr)


def _pad(a, pad):
    """a (n x nrhs) on top of `pad` rows of ones, column-major: the leading dimension is n + pad"""
    out = np.ones((a.shape[0] + pad, a.shape[1]), dtype=a.dtype, order="F")
    out[:a.shape[0]] = a
    return out


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _entry(name):
    """the library's entry point; numpy arrays and raw pointers are passed as whatever pointer type its binding declares (void * where it declares none)"""
    fn = _lib.entry(name)

    def call(*args):
        conv = []
        for i, a in enumerate(args):
            if isinstance(a, np.ndarray): a = _vp(a)
            if isinstance(a, C.c_void_p) and fn.argtypes and issubclass(fn.argtypes[i], C._Pointer): a = C.cast(a, fn.argtypes[i])
            conv.append(a)
        _lib.check(fn(*conv), name)
    return call


class _Sys:
    """one case: its CSR, its integer right-hand sides, and handles on it"""

    def __init__(self, name):
        self.name = name
        self.c, self.n, self.rp, self.ci, self.v = uc.csr_case(name)
        self.z = bool(self.c.z)
        self.pc = np.arange(self.n, dtype=np.int32)
        self.symb = driver.Symbolic(self.n, self.rp, self.ci, self.pc, relax=1, maxsup=self.c.maxsup, unsym=True)
        self.tt = "C" if self.z else "T"

    def handle(self):
        """factored with the exact factors (the untransposed integer solve is asserted by the first call of every sequence), the matrix attached"""
        h = driver.LUHandle.from_symbolic(self.symb, self.v)
        assert h.z == self.z and h.pdgstrf3d(0.0) == 0
        h.attach_matrix(self.n, self.rp, self.ci, self.v, self.pc)
        return h

    def rhs(self, nrhs, trans):
        """(x, b) with op(A) x = b, integers"""
        return self.c.rhs(nrhs) if trans == "N" else tc.rhs_t(self.c, nrhs, trans == "C")


def _name(z, base):
    return base.replace("pd", "pz", 1) if z else base


def _call(S, h, op, dev, nrhs, pad):
    """one call of `op` in its host (dev = False) or device-pointer form on handle h: a dict of result arrays"""
    n, z = S.n, S.z
    kind, trans = op
    x, b = S.rhs(nrhs, trans)
    t = driver._trans_code(trans)
    ld = n + pad
    berr = np.zeros(nrhs); steps = C.c_int32(0)
    if kind == "update":            # new values (the same ones: the factors stay the exact ones), factor, solve
        if dev:
            d = _Dev(S.v)
            try:
                _entry("sluamd_zUpdateValues_dev" if z else "sluamd_dUpdateValues_dev")(h._h, d.ptr, None)
                info = h.pdgstrf3d(0.0)
            finally:
                d.free()
        else:
            assert h.update_values(S.v.copy()) is None
            info = h.pdgstrf3d(0.0)
        B = _pad(b, pad)
        _entry(_name(z, "sluamd_pdgstrs3d"))(h._h, B, I64(ld), nrhs)
        assert info == 0 and np.array_equal(B[:n], x), (S.name, op, dev, nrhs)
        return {"x": B[:n].copy(), "pad": B[n:].copy()}
    if kind == "strs":
        B = _pad(b, pad)
        if dev:
            d = _Dev(B)
            try:
                h.pdgstrs3d_dev(d.ptr.value, ld, nrhs, trans=trans)
                B = d.host()
            finally:
                d.free()
        elif t:
            _entry(_name(z, "sluamd_pdgstrs3d_trans"))(h._h, t, B, I64(ld), nrhs)
        else:
            _entry(_name(z, "sluamd_pdgstrs3d"))(h._h, B, I64(ld), nrhs)
        assert np.array_equal(B[:n], x), (S.name, op, dev, nrhs, int(np.count_nonzero(B[:n] != x)))
        return {"x": B[:n].copy(), "pad": B[n:].copy()}
    # the expert solve (refine = 0) and the refinements: B stays, X comes back.  The refinement starts from X = 0: its first residual is b itself and its
    # first correction the case's own exact solve, so one step lands on the integer x and the second pass finds a zero residual
    B = _pad(b, pad)
    X = _pad(np.zeros_like(x), pad)
    if dev:
        dB, dX = _Dev(B), _Dev(X)
        try:
            if kind == "ssvx":
                h.gssvx_solve_dev(dB.ptr.value, ld, dX.ptr.value, ld, nrhs, trans=trans)
            else:
                berr, st = h.pdgsrfs3d_dev(dB.ptr.value, ld, dX.ptr.value, ld, nrhs, trans=trans)
                steps = C.c_int32(st)
            X = dX.host()
            assert np.array_equal(dB.host(), B)
        finally:
            dB.free(); dX.free()
    elif kind == "ssvx":
        _entry(_name(z, "sluamd_pdgssvx3d_solve"))(h._h, t, B, I64(ld), X, I64(ld), nrhs, 0, berr, C.byref(steps))
    elif t:
        _entry(_name(z, "sluamd_pdgsrfs3d_trans"))(h._h, t, B, I64(ld), X, I64(ld), nrhs, berr, C.byref(steps))
    else:
        _entry(_name(z, "sluamd_pdgsrfs3d"))(h._h, B, I64(ld), X, I64(ld), nrhs, berr, C.byref(steps))
    assert np.array_equal(X[:n], x), (S.name, op, dev, nrhs, int(np.count_nonzero(X[:n] != x)))
    if kind == "rfs":
        assert steps.value == 1 and not np.asarray(berr).any(), (S.name, op, dev, nrhs, steps.value, np.asarray(berr).tolist())
    return {"x": X[:n].copy(), "pad": X[n:].copy(), "berr": np.asarray(berr, dtype=np.float64).copy(), "steps": np.array([steps.value])}


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def _ops(S):
    return [("strs", "N"), ("strs", S.tt), ("ssvx", "N"), ("rfs", "N"), ("rfs", S.tt), ("update", "N")]


def _handle_child(name):
    S = _Sys(name)
    ops = _ops(S)
    # the reference: every distinct call on a handle of its own that has taken no other call
    fresh = {}
    for op in ops:
        for dev in (False, True):
            for nrhs, pad in STEPS[:2]:
                h = S.handle()
                try:
                    fresh[op, dev, nrhs, pad] = _call(S, h, op, dev, nrhs, pad)
                finally:
                    h.destroy()
    # one handle takes them all: small, grown, small again
    h = S.handle()
    try:
        for op in ops:
            for dev in (False, True):
                for nrhs, pad in STEPS:
                    _same(_call(S, h, op, dev, nrhs, pad), fresh[op, dev, nrhs, pad], (name, op, dev, nrhs, pad))
    finally:
        h.destroy()
    # what the pool holds goes back to the driver; a handle created afterwards solves as before
    assert _lib.load().sluamd_device_pool_trim(-1) >= 0
    h = S.handle()
    try:
        _same(_call(S, h, ("strs", "N"), False, 5, 3), fresh[("strs", "N"), False, 5, 3], (name, "after the trim"))
    finally:
        h.destroy()
    S.symb.free()


def _batch_call(c, bh, dev, nrhs, pad, trans):
    x, b, bt = c.rhs(nrhs)
    rhs = b if trans == "N" else bt
    m, ld = c.m, c.m + pad
    B = np.ones((c.count, nrhs, ld)); B[:, :, :m] = rhs.transpose(0, 2, 1)          # every matrix's block column-major, leading dimension ld
    X = np.ones_like(B)
    berr = np.zeros((c.count, nrhs)); steps = np.zeros(c.count, dtype=np.int32)
    args = lambda pb, px: (bh._b, driver._trans_code(trans), pb, I64(ld), I64(ld * nrhs), px, I64(ld), I64(ld * nrhs), nrhs, 0, berr,
                           steps)
    if dev:
        dB, dX = _Dev(B.reshape(-1)), _Dev(X.reshape(-1))
        try:
            _entry("sluamd_dBatchSolve_dev")(*args(dB.ptr, dX.ptr))
            X = dX.host().reshape(X.shape)
        finally:
            dB.free(); dX.free()
    else:
        _entry("sluamd_dBatchSolve")(*args(B, X))
    assert np.array_equal(X[:, :, :m].transpose(0, 2, 1), x), (c.name, dev, nrhs, pad, trans)
    return {"x": X.copy()}


def _batch_child():
    name = min(bc.SHAPES, key=lambda k: bc.SHAPES[k][0] * bc.SHAPES[k][1])
    c = bc.exact_case(name)
    symb = driver.Symbolic(c.m, c.rp, c.ci, None, relax=8, maxsup=c.maxsup)

    def batch():
        bh = driver.BatchHandle.create(symb, c.values)
        assert not bh.factor().any()
        return bh

    fresh = {}
    for trans in ("N", "T"):
        for dev in (False, True):
            for nrhs, pad in STEPS[:2]:
                bh = batch()
                try:
                    fresh[trans, dev, nrhs, pad] = _batch_call(c, bh, dev, nrhs, pad, trans)
                finally:
                    bh.destroy()
    bh = batch()
    try:
        for trans in ("N", "T"):
            for dev in (False, True):
                for nrhs, pad in STEPS:
                    _same(_batch_call(c, bh, dev, nrhs, pad, trans), fresh[trans, dev, nrhs, pad], (name, trans, dev, nrhs, pad))
    finally:
        bh.destroy()
    assert _lib.load().sluamd_device_pool_trim(-1) >= 0
    bh = batch()
    try:
        _same(_batch_call(c, bh, False, 5, 3, "N"), fresh["N", False, 5, 3], (name, "after the trim"))
    finally:
        bh.destroy()
    symb.free()


@pytest.mark.parametrize("name", ["widths", "z_narrow"])
def test_one_handle_small_grown_small_equals_fresh_handles(name):
    _child("_handle_child", name)


def test_one_batch_small_grown_small_equals_fresh_batches():
    _child("_batch_child")
