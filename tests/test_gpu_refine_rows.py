"""The branches of the shared residual row on batches (sluamd_[dz]BatchSolve with refine): the cases of refine_rows_cases.py -- a structurally empty row of
op(A), a row in the SAFE1 branch, rows above safe2, waves that span many matrices (m = 3) or two (m = 65) and a partial last wave -- for double and
complex16 and op = N, T, C.  X, berr and steps are compared bitwise with the numpy prediction, which test_refine_rows_cases_cpu.py proves exact."""
import numpy as np
import pytest
import refine_rows_cases as rr
import zbatch_cases as zc
from superlu_dist_amd import driver

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("z,trans", rr.FORMS)
@pytest.mark.parametrize("name", list(rr.SHAPES))
def test_batch_rows_bit_for_bit(name, z, trans):
    m, count, d, A, b = rr.case(name, z, trans)
    xe, berr_e, steps_e, _ = rr.predict(name, z, trans)
    drp, dci = np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32)
    s = driver.Symbolic(m, drp, dci, None, relax=8, maxsup=64)
    perm = s.perm_c.copy()
    bh = (driver.ZBatchHandle if z else driver.BatchHandle).create(s, d if z else d.real.copy())
    try:
        assert not bh.factor().any()
        rp, ci, v = zc.csr(zc.block_diag(A))
        driver._attach_matrix(bh.handle(), z, count * m, rp, ci, v, np.concatenate([perm + k * m for k in range(count)]))
        x, berr, steps = bh.solve(b, trans=trans, refine=True)
    finally:
        bh.destroy(); s.free()
    assert np.array_equal(steps, steps_e)
    assert np.array_equal(berr, berr_e)
    assert np.array_equal(x, xe)
