"""The batch refinement cases of refine_rows_cases.py on the CPU: the exact replay agrees with the float64 prediction within the bounds the module states, and
every case reaches the branches it was built for."""
import numpy as np
import pytest
import refine_rows_cases as rr


@pytest.mark.parametrize("z,trans", rr.FORMS)
@pytest.mark.parametrize("name", list(rr.SHAPES))
def test_prediction_is_exact_and_reaches_every_branch(name, z, trans):
    rr.verify(name, z, trans)
    m, count, d, A, b = rr.case(name, z, trans)
    x, berr, steps, census = rr.predict(name, z, trans)
    safe_row, empty_row = rr.rows_of(name, trans)
    special = [k for k in range(count) if rr.is_special(name, k)]
    assert special and len(special) < count
    for k in range(count):
        for j in range(rr.NRHS):
            for zero, mid, big in census[k][j]:                   # every pass
                if k in special:
                    assert list(zero) == [empty_row] and list(mid) == [safe_row] and len(big) == m - 2
                else:
                    assert len(zero) == 0 and len(mid) == 0 and len(big) == m
    assert len(set(steps)) > 1 and steps.max() >= 2               # the matrices of a batch stop at different sweeps
    for k in special:                                               # the run ends on the SAFE1 floor, formed from m
        t = rr.zc.abs1(rr.zc.op(A[k], trans)[safe_row]) @ rr.zc.abs1(x[k][:, -1]) + rr.zc.abs1(b[k][safe_row, -1])
        assert berr[k, -1] == (m + 1) * rr.SAFMIN / t and berr[k, -1] != (m * count + 1) * rr.SAFMIN / t
