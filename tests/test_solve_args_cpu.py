"""The argument checks shared by the solve and refinement entry points (check_solve_args), on the CPU test build of the library's host sources
(oracle/libsluamd_emul.so, the `emul` fixture) and therefore over the entry points that build exports: sluamd_pdgstrs3d, sluamd_pdgstrs3d_dev,
sluamd_pzgstrs3d, sluamd_pdgsrfs3d, sluamd_pdgsrfs3d_dev.  Each of them refuses a handle of the other precision (naming its twin), a null pointer,
nrhs < 0 and a leading dimension below n with SLUAMD_EINVAL before it touches anything, and returns 0 for nrhs == 0 with every array unchanged.
(On that build a "device" pointer is host memory, so the _dev forms take numpy arrays.)"""
import ctypes as C
import numpy as np
import pytest

EINVAL = -1


@pytest.fixture()
def handles(emul):
    from superlu_dist_amd import driver, matgen
    n, rp, ci, vd = matgen.poisson3d(4)
    vz = matgen.complex_shift(vd, rp, ci, seed=1)
    _, info_d, _, hd, sd = driver.pdgssvx3d(n, rp, ci, vd, np.ones((n, 1)), relax=8, maxsup=16, keep=True)
    _, info_z, _, hz, sz = driver.pzgssvx3d(n, rp, ci, vz, np.ones((n, 1), dtype=np.complex128), relax=8, maxsup=16, keep=True)
    assert info_d == 0 and info_z == 0 and hz.z and not hd.z
    hd.attach_matrix(n, rp, ci, vd, sd.perm_c)
    yield emul, n, hd, hz
    hd.destroy(); hz.destroy(); sd.free(); sz.free()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


SOLVES = [("sluamd_pdgstrs3d", False, _dp, "sluamd_pzgstrs3d"), ("sluamd_pdgstrs3d_dev", False, _vp, "sluamd_pzgstrs3d_dev"),
          ("sluamd_pzgstrs3d", True, _vp, "sluamd_pdgstrs3d")]
REFINES = [("sluamd_pdgsrfs3d", _dp, "sluamd_pzgsrfs3d"), ("sluamd_pdgsrfs3d_dev", _vp, "sluamd_pzgsrfs3d_dev")]


@pytest.mark.parametrize("name,z,ptr,twin", SOLVES)
def test_solve_entry_points_refuse_bad_arguments_before_touching_anything(handles, name, z, ptr, twin):
    L, n, hd, hz = handles
    fn = getattr(L, name)
    own, other = (hz, hd) if z else (hd, hz)
    x0 = (np.arange(2 * n) + 1.0).astype(np.complex128 if z else np.float64).reshape((n, 2), order="F")
    x = x0.copy(order="F")
    err = lambda: L.sluamd_last_error().decode()
    assert fn(other._h, ptr(x), n, 2) == EINVAL
    assert err().startswith(name + ": ") and ("double handle" if z else "complex16 handle") in err() and err().endswith("call " + twin), err()
    for args in ((None, ptr(x), n, 2), (own._h, None, n, 2), (own._h, ptr(x), n, -1), (own._h, ptr(x), n - 1, 2)):
        assert fn(*args) == EINVAL, args
        assert err().startswith(name + ": ") and "solve" in err(), err()
    assert fn(own._h, ptr(x), n, 0) == 0
    assert np.array_equal(x, x0)
    assert fn(own._h, ptr(x), n, 2) == 0 and not np.array_equal(x, x0)                      # ... and the same arguments with nrhs = 2 solve


@pytest.mark.parametrize("name,ptr,twin", REFINES)
def test_refinement_entry_points_refuse_bad_arguments_before_touching_anything(handles, name, ptr, twin):
    L, n, hd, hz = handles
    fn = getattr(L, name)
    B0, X0 = np.ones((n, 2), order="F"), np.full((n, 2), 0.5, order="F")
    B, X, berr = B0.copy(order="F"), X0.copy(order="F"), np.full(2, -1.0)
    steps = C.c_int32(7)
    ps = C.byref(steps)
    err = lambda: L.sluamd_last_error().decode()
    assert fn(hz._h, ptr(B), n, ptr(X), n, 2, _dp(berr), ps) == EINVAL
    assert err().startswith(name + ": ") and "complex16 handle" in err() and err().endswith("call " + twin), err()
    for args in ((None, ptr(B), n, ptr(X), n, 2, _dp(berr), ps), (hd._h, None, n, ptr(X), n, 2, _dp(berr), ps), (hd._h, ptr(B), n, None, n, 2, _dp(berr), ps),
                 (hd._h, ptr(B), n, ptr(X), n, 2, None, ps), (hd._h, ptr(B), n, ptr(X), n, -1, _dp(berr), ps), (hd._h, ptr(B), n - 1, ptr(X), n, 2, _dp(berr), ps),
                 (hd._h, ptr(B), n, ptr(X), n - 1, 2, _dp(berr), ps)):
        assert fn(*args) == EINVAL, args
        assert err().startswith(name + ": ") and "refinement" in err(), err()
    assert steps.value == 7
    assert fn(hd._h, ptr(B), n, ptr(X), n, 0, _dp(berr), ps) == 0 and steps.value == 0
    assert np.array_equal(B, B0) and np.array_equal(X, X0) and np.all(berr == -1.0)
    assert fn(hd._h, ptr(B), n, ptr(X), n, 2, _dp(berr), ps) == 0 and np.all(berr >= 0.0) and np.array_equal(B, B0)      # ... and with nrhs = 2 they refine
