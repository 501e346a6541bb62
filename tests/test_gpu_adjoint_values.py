"""sluamd_[dz]AdjointValues[_dev] and the batch forms on the device, bitwise against the integer expectations of tests/adjoint_cases.py.  The entry reads only
the attached pattern, so the cases attach their own CSR to a small tridiagonal handle of the same order; nothing is factored."""
import ctypes as C
import numpy as np
import pytest
import adjoint_cases as ac
from superlu_dist_amd import _lib, driver, grid3d

pytestmark = pytest.mark.gpu
EINVAL = -1


def make_handle(n, z, attach=None):
    """a handle of order n (tridiagonal) with the CSR `attach` = (rowptr, colind) attached in its place (values: ones)"""
    n, rp, ci, v = ac.tridiag(n, z)
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32))
    h = driver.LUHandle.from_symbolic(symb, v)
    if attach is not None:
        arp, aci = attach
        h.attach_matrix(n, arp, aci, np.ones(len(aci), dtype=np.complex128 if z else np.float64), symb.perm_c)
    return h, symb


def alloc_count():
    return int(_lib.load().sluamd_device_alloc_count())


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(name, z):
        if (name, z) not in made:
            c = ac.kcase(name, z)
            made[(name, z)] = (c,) + make_handle(c.n, z, (c.rowptr, c.colind))
        return made[(name, z)]

    yield get
    for c, h, symb in made.values():
        h.destroy(); symb.free()


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
@pytest.mark.parametrize("name", list(ac.kcases()))
def test_host_form_is_exact_for_every_trans_and_repeats_without_allocating(handles, name, z):
    c, h, _ = handles(name, z)
    for trans in ac.TRANS:
        want = c.expected_np(trans)
        g1 = h.adjoint_values(c.lam.astype(want.dtype), c.x.astype(want.dtype), trans=trans)
        before = alloc_count()
        g2 = h.adjoint_values(c.lam.astype(want.dtype), c.x.astype(want.dtype), trans=trans)
        assert alloc_count() == before
        assert g1.shape == (c.nnz,) and np.array_equal(g1, want), (name, trans, np.flatnonzero(g1 != want)[:8])
        assert g1.tobytes() == g2.tobytes()


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
@pytest.mark.parametrize("name", ["nnz257", "nrhs5", "nrhs17", "empty_rows", "n1"])
def test_device_form_with_padded_leading_dimensions(handles, name, z):
    """ldl, ldx > n: the rows beyond n hold a sentinel that no entry may read; G is preset to a sentinel the call must overwrite"""
    c, h, _ = handles(name, z)
    dt = np.complex128 if z else np.float64
    ldl, ldx = c.n + 3, c.n + 7
    d_lam = ac.DevBuf(ac.padded(c.lam.astype(dt), ldl, 2.0 ** 40).T)       # [nrhs, ld] row-major: the column-major block
    d_x = ac.DevBuf(ac.padded(c.x.astype(dt), ldx, 2.0 ** 41).T)
    for trans in ac.TRANS:
        d_g, d_g2 = ac.DevBuf(np.full(c.nnz, 7.0, dtype=dt)), ac.DevBuf(np.full(c.nnz, 9.0, dtype=dt))
        h.adjoint_values_dev(d_lam.data_ptr(), ldl, d_x.data_ptr(), ldx, c.nrhs, d_g.data_ptr(), trans=trans)
        before = alloc_count()
        h.adjoint_values_dev(d_lam.data_ptr(), ldl, d_x.data_ptr(), ldx, c.nrhs, d_g2.data_ptr(), trans=trans)
        assert alloc_count() == before
        got = d_g.host()
        assert np.array_equal(got, c.expected_np(trans)), (name, trans)
        assert got.tobytes() == d_g2.host().tobytes()
        d_g.free(); d_g2.free()
    d_lam.free(); d_x.free()


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_nrhs_zero_gives_zeros(handles, z):
    c, h, _ = handles("nnz257", z)
    dt = np.complex128 if z else np.float64
    g = h.adjoint_values(np.zeros((c.n, 0), dtype=dt), np.zeros((c.n, 0), dtype=dt))
    assert g.shape == (c.nnz,) and not g.any()
    d = ac.DevBuf(np.full(c.nnz, 5.0, dtype=dt))
    h.adjoint_values_dev(d.data_ptr(), c.n, d.data_ptr(), c.n, 0, d.data_ptr())
    assert not d.host().any()
    d.free()


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_an_equilibrated_handle_gives_the_same_bits(z):
    n, rp, ci, v = ac.tridiag(40, z)
    v = v * np.repeat(2.0 ** np.arange(n), np.diff(rp))                  # rows of very different size: the equilibration scales
    c = ac.KCase("equil", n, rp, ci, 5, z, seed=77)
    dt = np.complex128 if z else np.float64
    out = []
    for equil in (False, True):
        symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32))
        h = driver.LUHandle.from_symbolic(symb, v)
        if equil:
            assert h.equilibrate(n, rp, ci, v, symb.perm_c)["equed"] != "N"
        else:
            h.attach_matrix(n, rp, ci, v, symb.perm_c)
        out.append([h.adjoint_values(c.lam.astype(dt), c.x.astype(dt), trans=t) for t in ac.TRANS])
        h.destroy(); symb.free()
    for t, a, b in zip(ac.TRANS, *out):
        assert a.tobytes() == b.tobytes() and np.array_equal(a, c.expected_np(t))


def _rc(h, z, n, nrhs=1, trans=0, ld=None, null=False, other=False):
    dt = np.complex128 if (z != other) else np.float64
    a = np.zeros((max(n, 1), max(nrhs, 1)), dtype=dt, order="F")
    g = np.zeros(4096, dtype=dt)
    fn = _lib.entry("sluamd_zAdjointValues" if (z != other) else "sluamd_dAdjointValues")
    p = a.ctypes.data_as(C.c_void_p)
    return fn(h._h if h is not None else None, trans, None if null else p, n if ld is None else ld, p, n if ld is None else ld, nrhs, g.ctypes.data_as(C.c_void_p))


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_refusals_return_einval_with_a_message(handles, z):
    L = _lib.load()
    c, h, _ = handles("nrhs3", z)
    err = lambda: L.sluamd_last_error().decode()
    assert _rc(None, z, c.n) == EINVAL
    assert _rc(h, z, c.n, null=True) == EINVAL
    assert _rc(h, z, c.n, nrhs=-1) == EINVAL
    assert _rc(h, z, c.n, ld=c.n - 1) == EINVAL
    assert _rc(h, z, c.n, trans=3) == EINVAL and "trans" in err()
    assert _rc(h, z, c.n, other=True) == EINVAL and ("sluamd_zAdjointValues" if z else "sluamd_dAdjointValues") in err()
    bare, symb = make_handle(c.n, z)                                       # no attached matrix
    assert _rc(bare, z, c.n) == EINVAL and "AttachMatrix" in err()
    n, rp, ci, v = ac.tridiag(c.n, z)
    bare.attach_matrix(n, rp, ci, v, symb.perm_c)
    assert _rc(bare, z, c.n) == 0
    bare.set_row_perm(np.arange(n, dtype=np.int32))                        # a row permutation, even the identity
    assert _rc(bare, z, c.n) == EINVAL and "row permutation" in err()
    bare.destroy(); symb.free()


def test_a_grid_handle_is_refused():
    n, rp, ci, v = ac.tridiag(24, False)
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=4, maxsup=8)
    comms = grid3d.local_comms(2, 1, 1)

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], None)
        try:
            h.attach_matrix(n, rp, ci, v, symb.perm_c)
            rc = _rc(h, False, n)
            return rc, _lib.load().sluamd_last_error().decode()
        finally:
            h.destroy()

    for rc, msg in grid3d.run_ranks(2, body):
        assert rc == EINVAL and "1 x 1 x 1" in msg
    symb.free()


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
@pytest.mark.parametrize("count", [1, 3])
def test_batch_form_with_strides_larger_than_the_minimum(z, count):
    n, rp, ci, v = ac.tridiag(20, z)
    nnz, nrhs = len(ci), 5
    dt = np.complex128 if z else np.float64
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=4, maxsup=8)
    bh = (driver.ZBatchHandle if z else driver.BatchHandle).create(symb, np.stack([v * (k + 1) for k in range(count)]))
    cases = [ac.KCase(f"batch{k}", n, rp, ci, nrhs, z, seed=200 + k) for k in range(count)]
    lam = np.stack([c.lam.astype(dt) for c in cases]); x = np.stack([c.x.astype(dt) for c in cases])
    for trans in ac.TRANS:
        want = np.stack([c.expected_np(trans) for c in cases])
        got = bh.adjoint_values(lam, x, trans=trans)                                        # host form, minimal strides
        assert got.shape == (count, nnz) and np.array_equal(got, want)
        # device form: ld > n, strides beyond a block, sentinels in every gap
        ldl, ldx, sl, sx, sg = n + 2, n + 5, (n + 2) * nrhs + 11, (n + 5) * nrhs + 3, nnz + 9
        L = np.full((count, sl), 2.0 ** 40, dtype=dt); X = np.full((count, sx), 2.0 ** 41, dtype=dt)
        for k in range(count):
            L[k, :ldl * nrhs] = ac.padded(lam[k], ldl, 2.0 ** 40).T.reshape(-1)
            X[k, :ldx * nrhs] = ac.padded(x[k], ldx, 2.0 ** 41).T.reshape(-1)
        dL, dX, dG = ac.DevBuf(L), ac.DevBuf(X), ac.DevBuf(np.full((count, sg), 7.0, dtype=dt))
        bh.adjoint_values_dev(dL.data_ptr(), ldl, sl, dX.data_ptr(), ldx, sx, nrhs, dG.data_ptr(), sg, trans=trans)
        G = dG.host()
        assert np.array_equal(G[:, :nnz], want) and np.all(G[:, nnz:] == 7.0)
        dL.free(); dX.free(); dG.free()
    bh.destroy(); symb.free()
