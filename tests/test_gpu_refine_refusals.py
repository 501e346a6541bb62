"""What the twenty refinement entry points sluamd_p[dz]gsrfs3d{,_trans,_block,_gmres,_extra}{,_dev} and the four residual entry points
sluamd_[dz]Residual{,_dev} refuse, in which order, and what they do with nrhs == 0: the entry frame of sluamd_refine.h (rfs_frame and the RfsMethod of
every method), pinned through the C ABI.  Return codes, the distinguishing words of sluamd_last_error(), and which refusal wins where two apply.

Nothing here reaches a kernel: every call is refused, or has nothing to do, before a launch -- so the block pointers of the _dev forms are host arrays that
are never read, and the handles are not even factored.  A tridiagonal matrix of order 5 in both precisions, nrhs 0, 1, 2.

Recorded as the library behaves, not as one might wish:
  * nrhs == 0 without an attached matrix: the HOST form of the untransposed plain call (also reached through the _trans entry with SLUAMD_NOTRANS) returns 0
    and writes *steps = 0 before it asks for the matrix; its _dev form and every other entry refuse with "no matrix attached".
  * nrhs == 0 with a matrix: plain, transposed and GMRES write *steps = 0; the blocked and the extra-precise form write nothing at all.
  * the handle of a batch always has the batch's own block-diagonal matrix attached, so a batch handle cannot show which of "does not run on batches" and
    "no matrix attached" comes first; a grid handle without a matrix shows that "needs a 1 x 1 x 1 handle" comes before "no matrix attached"."""
import ctypes as C
import os, subprocess, sys
import numpy as np
import pytest
from superlu_dist_amd import _lib, driver, grid3d

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5
KINDS = ("plain", "trans", "block", "gmres", "extra", "residual")
NOUN = {"block": "blocked", "gmres": "GMRES", "extra": "extra-precise"}
BAD_OPTIONS = [(dict(restart=0), "restart must lie in [1, 64]"), (dict(restart=65), "restart must lie in [1, 64]"),
               (dict(max_solves=0), "max_solves must be at least 1"), (dict(inner_tol=0.0), "inner_tol must lie in (0, 1)"),
               (dict(inner_tol=1.0), "inner_tol must lie in (0, 1)")]


def _name(kind, z, dev):
    p = "z" if z else "d"
    base = "sluamd_%sResidual" % p if kind == "residual" else "sluamd_p%sgsrfs3d%s" % (p, "" if kind == "plain" else "_" + kind)
    return base + ("_dev" if dev else "")


ENTRIES = [(kind, z, dev) for kind in KINDS for z in (False, True) for dev in (False, True)]
assert len(ENTRIES) == 24 and len({_name(*e) for e in ENTRIES}) == 24


def _tridiag(z):
    """CSR of tridiag(-1, 4, -1) of order N (complex16: every value times 1 + 0.5i)"""
    rows = [[j for j in (i - 1, i, i + 1) if 0 <= j < N] for i in range(N)]
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    ci = np.array([j for r in rows for j in r], dtype=np.int32)
    v = np.array([4.0 if j == i else -1.0 for i, r in enumerate(rows) for j in r])
    return rp, ci, (v * (1 + 0.5j) if z else v)


def _symbolic():
    rp, ci, _ = _tridiag(False)
    return driver.Symbolic(N, rp, ci, np.arange(N, dtype=np.int32), relax=1, maxsup=64, unsym=True)


class _Call:
    """one call of an entry point on sentinel-filled arrays: rc, the error text, and what the call left in its outputs"""

    def __init__(self, kind, z, dev, h, nrhs, trans=0, opt=None, n=N):
        """n: the order of the handle (a batch of two: 2 N)"""
        self.kind, self.name = kind, _name(kind, z, dev)
        dt = np.complex128 if z else np.float64
        self.B = np.full((n, 2), 3.0, dtype=dt, order="F"); self.X = np.full((n, 2), 7.0, dtype=dt, order="F"); self.R = np.full((n, 2), 9.0, dtype=dt, order="F")
        self.berr = np.full(2, -1.0); self.steps = np.full(2, -7, dtype=np.int32); self.solves = np.full(2, -7, dtype=np.int32)
        self.out = (_lib.XRefine * 2)()
        for o in self.out:
            o.dxrel, o.rho, o.steps, o.state = -1.0, -1.0, -7, -7
        fn = _lib.entry(self.name)
        typed = kind == "plain" and not z and not dev                     # sluamd_pdgsrfs3d alone is bound with double pointers
        p = (lambda a: a.ctypes.data_as(_lib.P_dbl)) if typed else (lambda a: a.ctypes.data_as(C.c_void_p))
        pb, ps = self.berr.ctypes.data_as(_lib.P_dbl), self.steps.ctypes.data_as(_lib.P_int)
        blocks = (p(self.B), n, p(self.X), n, nrhs)
        if kind == "plain":
            self.rc = fn(h, *blocks, pb, ps)
        elif kind in ("trans", "block"):
            self.rc = fn(h, trans, *blocks, pb, ps)
        elif kind == "gmres":
            o = None
            if opt is not None:
                o = _lib.Gmres()
                _lib.entry("sluamd_default_gmres")(C.byref(o))
                for k, val in opt.items():
                    setattr(o, k, val)
            self.rc = fn(h, trans, *blocks, None if o is None else C.byref(o), pb, ps, self.solves.ctypes.data_as(_lib.P_int))
        elif kind == "extra":
            self.rc = fn(h, trans, *blocks, pb, self.out)
        else:
            self.rc = fn(h, trans, 0, *blocks, p(self.R), n, pb)
        self.err = _lib.load().sluamd_last_error().decode() if self.rc else ""

    def refused(self, *words):
        assert self.rc == -1 and all(w in self.err for w in words), (self.name, self.rc, self.err, words)
        self.untouched()

    def untouched(self, steps=None):
        """B, X, R, berr, the GMRES solves and the extra-precise records keep their sentinels; steps: None = every entry of steps[] too, else steps[0]"""
        assert np.all(self.B == 3.0) and np.all(self.X == 7.0) and np.all(self.R == 9.0) and np.all(self.berr == -1.0), (self.name, "a block or berr was written")
        assert self.steps.tolist() == ([-7, -7] if steps is None else [steps, -7]), (self.name, self.steps.tolist())
        assert self.solves.tolist() == [-7, -7] and all((o.steps, o.state, o.dxrel, o.rho) == (-7, -7, -1.0, -1.0) for o in self.out), self.name


def _handle(z, symb, attach):
    rp, ci, v = _tridiag(z)
    h = driver.LUHandle.from_symbolic(symb, v)
    assert h.z == z
    if attach:
        h.attach_matrix(N, rp, ci, v, symb.perm_c)
    return h


@pytest.fixture(scope="module")
def handles():
    """(z, attached) -> an unfactored handle of the tridiagonal matrix"""
    symb = _symbolic()
    hs = {(z, a): _handle(z, symb, a) for z in (False, True) for a in (False, True)}
    yield hs
    for h in hs.values():
        h.destroy()
    symb.free()


@pytest.mark.parametrize("kind,z,dev", ENTRIES, ids=lambda v: v if isinstance(v, str) else None)
def test_the_other_precision_and_a_missing_matrix_are_refused(handles, kind, z, dev):
    name = _name(kind, z, dev)
    twin = name[:7] + ("d" if z else "z") + name[8:] if kind == "residual" else name[:8] + ("d" if z else "z") + name[9:]
    assert twin == _name(kind, not z, dev)
    for trans in (0,) if kind == "plain" else (0, 1, 2):
        for nrhs in (0, 1, 2):                                              # the precision comes before nrhs == 0 and before the matrix
            for attached in (False, True):
                _Call(kind, z, dev, handles[(not z, attached)]._h, nrhs, trans).refused(
                    name + ": " + ("double" if z else "complex16") + " handle: call " + twin)
        for nrhs in (1, 2):
            _Call(kind, z, dev, handles[(z, False)]._h, nrhs, trans).refused("no matrix attached: call sluamd_%sAttachMatrix first" % ("z" if z else "d"))


@pytest.mark.parametrize("kind,z,dev", ENTRIES, ids=lambda v: v if isinstance(v, str) else None)
def test_nrhs_zero(handles, kind, z, dev):
    """with a matrix: 0 from every entry, *steps = 0 from plain, transposed and GMRES, nothing written by block, extra and the residual.  Without one: the host
    form of the untransposed plain call returns 0 with *steps = 0, every other entry asks for the matrix first"""
    writes_steps = kind in ("plain", "trans", "gmres")
    for trans in (0,) if kind == "plain" else (0, 1, 2):
        c = _Call(kind, z, dev, handles[(z, True)]._h, 0, trans)
        assert c.rc == 0, (c.name, trans, c.err)
        c.untouched(steps=0 if writes_steps else None)
        c = _Call(kind, z, dev, handles[(z, False)]._h, 0, trans)
        if kind in ("plain", "trans") and trans == 0 and not dev:
            assert c.rc == 0, (c.name, c.err)
            c.untouched(steps=0)
        else:
            c.refused("no matrix attached")


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_gmres_options_are_checked_after_the_precision_and_before_the_matrix(handles, z):
    for dev in (False, True):
        for opt, words in BAD_OPTIONS:
            for trans in (0, 1):
                for nrhs in (0, 1):
                    for attached in (False, True):
                        _Call("gmres", z, dev, handles[(z, attached)]._h, nrhs, trans, opt).refused(_name("gmres", z, dev) + ": " + words)
                    _Call("gmres", z, dev, handles[(not z, True)]._h, nrhs, trans, opt).refused("handle: call " + _name("gmres", not z, dev))
        c = _Call("gmres", z, dev, handles[(z, True)]._h, 0, 0, dict(restart=64, max_solves=1, inner_tol=0.5))       # the ends of the ranges pass
        assert c.rc == 0, c.err


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_the_handle_of_a_batch(z):
    """count 2: block, extra and GMRES refuse it by name ("does not run on batches"), GMRES after its options; the batch has attached its own block-diagonal
    matrix, which the plain entry with nrhs == 0 shows by returning 0"""
    symb = _symbolic()
    v = _tridiag(z)[2]
    bh = (driver.ZBatchHandle if z else driver.BatchHandle).create(symb, np.stack([v, 2 * v]))
    try:
        h = bh.handle()
        for dev in (False, True):
            for kind in ("block", "extra", "gmres"):
                for nrhs in (0, 1, 2):
                    for trans in (0, 1):
                        _Call(kind, z, dev, h, nrhs, trans, n=2 * N).refused(_name(kind, z, dev) + ": the handle belongs to a batch (sluamd_BatchHandle): the " + NOUN[kind] +
                                                                     " refinement does not run on batches")
            _Call("gmres", z, dev, h, 1, 0, dict(restart=0), n=2 * N).refused("restart must lie in [1, 64]")
            _Call("extra", not z, dev, h, 1, n=2 * N).refused("handle: call " + _name("extra", z, dev))
            c = _Call("plain", z, dev, h, 0, n=2 * N)
            assert c.rc == 0, c.err                                        # (a handle without a matrix refuses the _dev form: test_nrhs_zero)
            c.untouched(steps=0)
    finally:
        bh.destroy(); symb.free()


def _grid_child():
    """both ranks of a 1 x 1 x 2 grid (threads; handle creation is the only collective step, nothing is factored), no matrix attached: extra and GMRES refuse
    the grid before they ask for the matrix and GMRES after its options; block, plain, transposed and the residual run on grids and ask for the matrix"""
    symb = _symbolic()
    tree = symb.partition(2)
    comms = grid3d.local_comms(1, 1, 2)

    def body(rank):
        done = 0
        for z in (False, True):
            h = grid3d.GridHandle.from_symbolic(symb, _tridiag(z)[2], comms[rank], tree)
            try:
                for dev in (False, True):
                    for kind in ("extra", "gmres"):
                        for nrhs in (0, 1, 2):
                            _Call(kind, z, dev, h._h, nrhs).refused(_name(kind, z, dev) + ": the " + NOUN[kind] + " refinement needs a 1 x 1 x 1 handle")
                            done += 1
                    for opt, words in BAD_OPTIONS:
                        _Call("gmres", z, dev, h._h, 1, 0, opt).refused(words)
                    _Call("gmres", not z, dev, h._h, 1).refused("handle: call " + _name("gmres", z, dev))
                    for kind in ("plain", "trans", "block", "residual"):
                        _Call(kind, z, dev, h._h, 1).refused("no matrix attached")
                        done += 1
            finally:
                h.destroy()
        return done

    out = grid3d.run_ranks(2, body)
    symb.free()
    assert out == [40, 40], out
    print("RESULT ok")


def test_a_grid_handle():
    """in a child process under a time limit, like every test that creates grid handles"""
    code = ("import os, sys\nsys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\nimport test_gpu_refine_refusals as t\n"
            "t._grid_child()\n")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
