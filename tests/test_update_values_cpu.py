"""update_values without a GPU: the Python argument checks raise ValueError before any library call (the library's entry points are replaced by a
recorder), the accepted forms reach the right entry point, and the numpy restatement of the scaled values that test_gpu_update_values.py compares the
device against (update_cases.scaled_values) reproduces equil_cases' own expected scaled values -- existing, tested data, not the new code."""
import numpy as np
import pytest
import equil_cases as ec
import update_cases as uc
from superlu_dist_amd import _lib, driver, grid3d

NNZ = 12


@pytest.fixture
def calls(monkeypatch):
    """every library call of update_values goes through _lib.entry: record the names, return success"""
    made = []

    def entry(name):
        def fn(*args):
            made.append(name)
            return 0
        return fn
    monkeypatch.setattr(_lib, "entry", entry)
    return made


def _stubs(z=False):
    """handles that own nothing (a null library handle: destroy() and __del__ do nothing)"""
    h = driver.LUHandle(None)
    h.z, h.n, h.nnz, h.device = z, 4, NNZ, 0
    g = grid3d.GridHandle(None, None, 4, z)
    g.nnz, g.device = NNZ, 0
    return h, g


def test_bad_arguments_raise_before_any_library_call(calls):
    import torch
    good = np.arange(NNZ, dtype=np.float64)
    bad = [good[:-1], np.zeros(NNZ + 1), good.astype(np.float32), good.astype(np.int64), good.astype(np.complex128), np.zeros(2 * NNZ)[::2],
           good.reshape(3, 4), good.reshape(NNZ, 1),
           torch.zeros(NNZ - 1, dtype=torch.float64), torch.zeros(NNZ, dtype=torch.float32), torch.zeros(NNZ, dtype=torch.complex128),
           torch.zeros(2 * NNZ, dtype=torch.float64)[::2], torch.zeros(3, 4, dtype=torch.float64),
           torch.empty(NNZ, dtype=torch.float64, device="meta")]                     # a tensor on another device
    for h in _stubs():
        for a in bad:
            with pytest.raises(ValueError, match="update_values"):
                h.update_values(a)
            with pytest.raises(ValueError, match="update_values"):
                h.update_values(a, want_norm=True)
    for h in _stubs(z=True):                                                            # a complex16 handle refuses float64
        for a in (good, torch.zeros(NNZ, dtype=torch.float64), np.zeros(NNZ - 1, dtype=np.complex128)):
            with pytest.raises(ValueError, match="update_values"):
                h.update_values(a)
    assert calls == []


def test_accepted_forms_reach_the_host_entry_point(calls):
    import torch
    good = np.arange(NNZ, dtype=np.float64)
    ro = good.copy(); ro.setflags(write=False)
    for h in _stubs():
        assert h.update_values(good) is None
        assert h.update_values(ro) is None
        assert h.update_values(list(good)) is None                                      # a list of Python floats is a float64 array
        assert h.update_values(torch.from_numpy(good.copy())) is None                   # a tensor on the CPU takes the host form
        assert h.update_values(good, want_norm=True) == {"anorm": 0.0, "equed": "N"}    # (what the recorder leaves in sluamd_update_t)
    assert calls == ["sluamd_dUpdateValues"] * 10
    del calls[:]
    for h in _stubs(z=True):
        assert h.update_values(good.astype(np.complex128)) is None
    assert calls == ["sluamd_zUpdateValues"] * 2


@pytest.mark.parametrize("name", ["diag63_R", "neg257_C", "dense65_B", "clamp1030", "z_abs1", "z_rows1_R", "z_dense64_C", "rows7_64_N"])
def test_scaled_values_restatement_reproduces_the_equilibration_cases(name):
    """(a r[i]) c[j] with the case's own R and C (all ones where a side is not scaled) IS the scaled copy equil_cases.equilibrate returns, bit for bit"""
    n, rp, ci, v = ec.case(name)
    e = ec.equilibrate(n, rp, ci, v)
    got = uc.scaled_values(n, rp, ci, v, e["R"], e["C"])
    assert got.dtype == e["vals"].dtype and np.array_equal(got.view(np.uint64), e["vals"].view(np.uint64))


def test_the_equilibrated_update_case_and_its_second_values():
    """the case test_gpu_update_values.py equilibrates: equed = B, R and C not powers of two; the second values keep the pattern (no entry becomes zero),
    differ from the first everywhere off the k = 0 positions, and the order of the two scalings matters for them (so the bitwise store check can tell)"""
    n, rp, ci, v1 = ec.case(uc.EQUIL_CASE)
    e = ec.equilibrate(n, rp, ci, v1)
    assert e["equed"] == "B"
    assert not np.all(np.frexp(e["R"])[0] == 0.5) and not np.all(np.frexp(e["C"])[0] == 0.5)
    v2 = uc.second_values(n, rp, ci, v1)
    k = np.rint((v2 / v1 - 1.0) * 8).astype(int)
    assert set(k.tolist()) == {0, 1, 2, 3} and np.all(v2 != 0) and np.array_equal(v2[k == 0], v1[k == 0])
    rows = ec.rows_of(n, rp)
    s2 = uc.scaled_values(n, rp, ci, v2, e["R"], e["C"])
    other = v2 * (e["R"][rows] * e["C"][ci])
    assert np.count_nonzero(s2 != other) > 0


def test_wrong_values_differ_everywhere():
    rp = np.array([0, 2, 4], dtype=np.int32); ci = np.array([0, 1, 0, 1], dtype=np.int32)
    v = np.array([1.0, 2.0, -3.0, 4.0])
    assert uc.wrong_values(2, rp, ci, v).tolist() == [6.0, 6.0, -9.0, 24.0]
