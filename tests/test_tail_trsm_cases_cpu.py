"""The cases of tests/tail_trsm_cases.py on the CPU: their structure against the symbolic factorisation, their bounds, the restated launch rules and the
CPU oracle on them -- so that a failure of test_gpu_tail_trsm.py on the device is the library's, not the cases'."""
import functools
import numpy as np
import pytest
import oracle as orc
import panel_cases as pn
import schur_cases as sc
import sweep_cases as sw
import tail_trsm_cases as tt
from superlu_dist_amd import driver


@functools.lru_cache(maxsize=None)
def _prepared(w):
    c = tt.CASES[w]()
    n, rp, ci = c.pattern_csr()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    perm, xsup = symb.perm_c.copy(), symb.xsup().tolist()
    fs = symb.flat_store(values=False)
    symb.free()
    assert np.array_equal(perm, np.arange(n)) and xsup == c.xsup.tolist(), (w, xsup)
    expL, expU = c.fill(fs)
    srcs = sc.sources(fs)
    return c, fs, expL, expU, srcs, sw.levels_of(srcs)


@pytest.mark.parametrize("w", tt.WIDTHS)
def test_structure(w):
    """four single-supernode levels; a: 5 rows, 85 columns with every designed lead; b: 85 rows and columns at full height; a's level is split, b's is not"""
    c, fs, _, _, srcs, lev = _prepared(w)
    tab = pn.level_table(srcs, lev)
    assert [(nn, mx) for nn, mx, _ in tab] == [(1, 1), (1, w), (1, w), (1, tt.TOP)]
    a, b = srcs[tt.A], srcs[tt.B]
    assert (pn.rows_below(a), pn.ucols(a)) == (5, 85) and (pn.rows_below(b), pn.ucols(b)) == (85, 85)
    assert [g for g, _ in a["lblocks"]] == [tt.B] and [(g, len(cols)) for g, cols in a["ublocks"]] == [(tt.B, 20), (tt.T, 65)]
    leads = [ld for _, cols in a["ublocks"] for ld in cols.values()]
    assert set(leads) == set(tt.lead_set(w)) and min(leads.count(ld) for ld in set(leads)) >= 17 // len(set(leads))
    assert {ld for _, cols in b["ublocks"] for ld in cols.values()} == {0}
    parts = [pn.split_parts(tab[l], lev, pn.DEFAULTS, l, len(tab)) for l in range(len(tab))]
    assert parts == [None, [(0, 1, 1), (1, 0, 1)], None, None], parts
    for form, (_, st) in tt.FORMS.items():
        pl = [x for x in pn.predicted_lines(srcs, lev, False, dict(pn.DEFAULTS, **st)) if x[0] == "panel"]
        assert {x[1] for x in pl} == {"trsm64"}                                              # every level is a tail level
        want = [(0, 1, 1, "whole"), (1, 1, 1, "0"), (1, 0, 1, "1"), (2, 2, 2, "whole")] if form == "split" else [(0, 1, 1, "whole"), (1, 1, 2, "whole"), (2, 2, 2, "whole")]
        assert sorted((x[2], x[5], x[6], x[7]) for x in pl) == sorted(want), (form, pl)


@pytest.mark.parametrize("w", tt.WIDTHS)
def test_bounds_and_oracle(w):
    """the bounds of both panel forms (asserted in Python integers by the fill); the CPU oracle returns L0 and U0 at every stored position and the integer x"""
    c, fs0, expL, expU, srcs, lev = _prepared(w)
    assert len(c.bounds) == 4 and all(isinstance(v, int) and v * pn.MARGIN < pn.LIMIT for v in c.bounds.values()) and c.bound * pn.MARGIN < pn.LIMIT
    o = orc.LUStore(fs0.n, fs0.xsup, fs0.Lrowind_off, fs0.Lrowind, fs0.Lnzval_off, fs0.Lnzval.copy(), fs0.Ufstnz_off, fs0.Ufstnz, fs0.Unzval_off, fs0.Unzval.copy())
    assert orc.dfactor(o)[0] == 0
    assert np.array_equal(o.Lnzval, expL) and np.array_equal(o.Unzval, expU)
    for nrhs in (1, 3):
        x, b = c.rhs(nrhs)
        assert np.array_equal(orc.dsolve(o, b.copy(order="F")), x)
