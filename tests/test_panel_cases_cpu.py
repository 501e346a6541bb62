"""The cases of tests/panel_cases.py on the CPU: their structure against the symbolic factorisation, their bounds, and the CPU oracle on them -- so that a
failure of test_gpu_panel_forms.py on the device is the library's, not the cases'."""
import functools
import numpy as np
import pytest
import oracle as orc
import panel_cases as pn
import schur_cases as sc
import sweep_cases as sw
from superlu_dist_amd import driver


@functools.lru_cache(maxsize=None)
def _prepared(name):
    c = pn.CASES[name]()
    n, rp, ci = c.pattern_csr()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    perm, xsup = symb.perm_c.copy(), symb.xsup().tolist()
    fs = symb.flat_store(values=False)
    symb.free()
    assert np.array_equal(perm, np.arange(n)) and xsup == c.xsup.tolist(), (name, xsup)
    expL, expU = c.fill(fs)
    srcs = sc.sources(fs)
    return c, fs, expL, expU, srcs, sw.levels_of(srcs)


def _levels(name):
    c, fs, _, _, srcs, lev = _prepared(name)
    return [(nn, mx) for nn, mx, _ in pn.level_table(srcs, lev)]


def test_chain_wide_structure():
    c, fs, _, _, srcs, lev = _prepared("chain_wide")
    assert _levels("chain_wide") == [(2, 1), (2, 17), (1, 33), (1, 65), (1, 129), (1, 200), (1, 256), (1, 256)]
    chain = srcs[4:]
    assert [pn.rows_below(s) for s in chain] == [1, 63, 64, 65, 130, 0] and [pn.ucols(s) for s in chain] == [1, 63, 64, 65, 130, 0]
    for s in chain[1:5]:                                                                    # an empty column between the segments
        (g, cols), = s["ublocks"]
        assert set(range(min(cols), max(cols) + 1)) - set(cols)
    # ragged leads: the symbolic factorisation stores the U rows of a supernode behind a wide predecessor at full height, so the chain members carry none;
    # the leaves here (multi-supernode level) and the guarded 129-column member of `rs32` and 48-column member of `split` (single-supernode levels) do
    assert all(len({ld for _, cols in srcs[k]["ublocks"] for ld in cols.values()}) >= 3 for k in (1, 3))
    for name, k, cnt in (("rs32", 1, 7), ("split", 1, 4)):
        assert len({ld for _, cols in _prepared(name)[4][k]["ublocks"] for ld in cols.values()}) >= cnt
    for tail, want in ((2, [6, 7]), (0, []), (64, list(range(2, 8)))):
        cfg = dict(pn.DEFAULTS, trsm_tail=tail)
        got = sorted(x[2] for x in pn.predicted_lines(srcs, lev, False, cfg) if x[0] == "full_inv" and x[8] == "bulk")
        assert got == want, (tail, got)


def test_tail_boundary_structure():
    lv = _levels("tail_boundary")
    assert len(lv) == 73 and all(nn == 1 for nn, _ in lv) and {mx for _, mx in lv} == set(range(1, 9)) and _prepared("tail_boundary")[0].n == 326
    srcs, lev = _prepared("tail_boundary")[4:]
    pl = pn.predicted_lines(srcs, lev, False, pn.DEFAULTS)
    assert sorted(x[2] for x in pl if x[1] == "gemm16") == list(range(9)) and sorted(x[2] for x in pl if x[1] == "trsm64") == list(range(9, 72))


def test_mixed_level_structure():
    c, fs, _, _, srcs, lev = _prepared("mixed_level")
    assert _levels("mixed_level") == [(3, 64), (3, 128), (3, 200), (3, 256), (1, 70)]
    for l, (nn, mx, per) in enumerate(pn.level_table(srcs, lev)[:4]):
        assert sorted(s["w"] for s in per) == [3, 17, mx]
        assert [pn.rows_below(s) for s in sorted(per, key=lambda s: s["w"])][:2] == [1, 65]


def test_rs32_structure():
    c, fs, _, _, srcs, lev = _prepared("rs32")
    assert _levels("rs32") == [(1, 1), (1, 129), (1, 160), (1, 200), (1, 256), (1, 129)]
    assert [pn.rows_below(s) for s in srcs[1:5]] == [31, 32, 33, 97] and [pn.ucols(s) for s in srcs[1:5]] == [31, 32, 33, 97]
    pl = pn.predicted_lines(srcs, lev, False, dict(pn.DEFAULTS, rs32=True))
    assert [(x[5], x[6]) for x in pl if x[1] == "trsm32"] == [(1, 1), (1, 1), (2, 2), (4, 4)]


def test_split_structure():
    c, fs, _, _, srcs, lev = _prepared("split")
    assert _levels("split") == [(1, 1), (1, 48), (1, 48), (1, 48), (1, 130), (1, 130), (1, 200)]
    big = [sc.source_is_big(s) for s in srcs]
    assert big == [False, False, False, False, True, True, False]
    urg = [tuple(sorted(u) for u in pn.urgent_units(s, lev)) for s in srcs[1:6]]
    assert urg == [([0], [0]), ([], []), ([0], [0]), ([0, 1], [0, 1]), ([0, 1, 2, 3], [0, 1, 2, 3])], urg
    # d: the block of the next level alone (60 rows) would reach strip 0 only; the merged 128-row tile that starts in it makes strip 1 urgent
    assert [len(r) for _, r in srcs[4]["lblocks"]] == [60, 196]
    tab = pn.level_table(srcs, lev)
    parts = [pn.split_parts(tab[l], lev, pn.DEFAULTS, l, len(tab)) for l in range(len(tab))]
    assert parts == [None, None, None, [(0, 1, 1), (1, 1, 1)], [(0, 2, 2), (1, 2, 2)], None, None]


def test_z_chain_structure():
    c, fs, _, _, srcs, lev = _prepared("z_chain")
    side = [3, 8, 9, 16, 17, 32, 33, 64, 65, 200, 256]
    assert _levels("z_chain") == [(2, w) for w in side] and c.z
    tab = pn.level_table(srcs, lev)
    assert sorted(s["w"] for s in tab[9][2]) == [17, 200] and sorted(s["w"] for s in tab[8][2]) == [3, 65] and sorted(s["w"] for s in tab[10][2]) == [3, 256]


@pytest.mark.parametrize("name", list(pn.CASES))
def test_bounds_and_oracle(name):
    """the bounds of both panel forms (asserted in Python integers by the fill); the CPU oracle returns L0 and U0 at every stored position and the integer x"""
    c, fs0, expL, expU, srcs, lev = _prepared(name)
    assert c.bounds and all(isinstance(v, int) and v * pn.MARGIN < pn.LIMIT for v in c.bounds.values()) and c.bound * pn.MARGIN < pn.LIMIT
    assert len(c.bounds) == (2 if c.z else 4)
    o = orc.LUStore(fs0.n, fs0.xsup, fs0.Lrowind_off, fs0.Lrowind, fs0.Lnzval_off, fs0.Lnzval.copy(), fs0.Ufstnz_off, fs0.Ufstnz, fs0.Unzval_off, fs0.Unzval.copy())
    assert orc.dfactor(o)[0] == 0                                                           # (the complex oracle behind the same entry on a complex store)
    assert np.array_equal(o.Lnzval, expL) and np.array_equal(o.Unzval, expU)
    for nrhs in (1, 3):
        x, b = c.rhs(nrhs)
        assert np.array_equal(orc.dsolve(o, b.copy(order="F")), x)
    # off-diagonal panels are dense: at most the zeros of the value pattern (one residue in seven)
    off = sum(pn.rows_below(s) * s["w"] for s in srcs)
    below = np.tril(c.L0, -1) * (1 - pn._blockdiag_mask(c.xsup).toarray())
    assert off == 0 or np.count_nonzero(below) * 7 >= off * 5


def test_the_variants_reach_every_form_of_the_table():
    """the restated rules over all cases and variants name every form of the launch line (the device test compares them with the lines themselves)"""
    seen = set()
    for name in pn.CASES:
        c, _, _, _, srcs, lev = _prepared(name)
        for v in pn.VARIANTS:
            for ln in pn.predicted_lines(srcs, lev, c.z, pn.settings(v)):
                seen.add((ln[0], ln[1]))
    need = {("diag_lu", f) for f in ("wave", "lu2_1", "lu2_2", "v1_128", "v1_256", "zwave_small8", "zwave_small16", "zwave_small32", "zwave", "zwave4", "zlu")}
    need |= {("full_inv", "inv64"), ("full_inv", "inv")} | {("panel", f) for f in ("gemm16", "gemm32", "gemm64", "trsm32", "trsm64", "zquad4", "zquad8", "zquad16", "ztrsm")}
    assert need <= seen, sorted(need - seen)
