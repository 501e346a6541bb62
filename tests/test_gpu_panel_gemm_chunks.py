"""The product form of the panel solves (k_panel_gemm<16 | 32 | 64>: L(:,k) <- L(:,k) Uinv_kk and U(k,:) <- Linv_kk U(k,:)) against EXACT factors at the
places its chunk loop can go wrong: the 32-column chunks of the triangular K range (supernode widths on both sides of every multiple of 32 and at the
limits of each instantiation), the first and the last chunk of the two-buffer stage pipeline (one-block and many-block supernodes), the choice between the
16-byte loads of even-width supernodes and the predicated loads of odd widths and ragged last blocks (an odd and an even width on ONE level, so one launch
takes both), and workgroups whose waves are partly or wholly idle (panels of 1 .. 130 rows / skyline columns).

The matrices are panel_cases.PanelCase designs (dense exactly known inverses of the diagonal blocks, dense panels, every bound of the product form asserted
below 2^53 / 64 by panel_bounds), so every comparison is numpy.array_equal: factors at every stored position, Linv / Uinv of every diagonal block, the
integer solution for 1 and 3 right-hand sides.  One design serves all of them (`fan`):

    guard_i -> source_i (i < K, all on one level, the widths under test) -> d (48 columns) -> top (140 columns)

source i holds `cnt` rows below its diagonal block and `cnt` skyline columns with the ragged leads of panel_cases._leads: the first 40 of them in d, the
rest in the top -- or all of them in the top (the middle one of three sources), so that a level has urgent and other 64-row units and the default schedule
launches it in the `units` form (build_panel_split), while a panel of at most 64 rows that reaches d is all urgent and stays whole.

Schedules: the default one (look-ahead, split panel solves), SLUAMD_PANEL_SPLIT=0 (look-ahead, whole launches) and SLUAMD_NO_LOOKAHEAD=1 (serial).  A level
of ONE supernode near the top of so short a DAG is a tail level and would take the substitution form, so the single-supernode cases switch the tail rule off
(SLUAMD_TRSM_TAIL=0) in all three; levels of three supernodes take the product form as they are.  Which form a level takes is read off the restated rules of
panel_cases.predicted_lines (that the device launches what they say is asserted by test_gpu_panel_forms.py on the launch lines themselves)."""
import numpy as np
import pytest
import panel_cases as pn
import schur_cases as sc
import sweep_cases as sw
from superlu_dist_amd import driver

pytestmark = pytest.mark.gpu
WIDTHS = {16: [31, 32, 33, 63, 64], 32: [65, 95, 96, 97, 127, 128], 64: [129, 160, 161, 191, 192, 193, 223, 224, 255, 256]}
ROWS = [1, 15, 16, 17, 63, 64, 65, 130]
CLASS = {w: nq for nq, ws in WIDTHS.items() for w in ws}
WD, WTOP, IN_D = 48, 140, 40
NRHS = (1, 3)
# three sources per level: the outer two have the width under test and, over the four levels of a width, every panel height; the middle one has the
# neighbouring width of the other parity (same instantiation) and reaches the top only
TRIPLES = [(1, 17, 15), (16, 65, 17), (63, 1, 64), (65, 64, 130)]
SCHEDULES = {"default": {}, "panel_split0": {"SLUAMD_PANEL_SPLIT": "0"}, "no_lookahead": {"SLUAMD_NO_LOOKAHEAD": "1"}}


def partner(w):
    """the neighbouring width of the other parity inside the same instantiation (supernodes of at most 4 NQ columns)"""
    return w + 1 if w < 4 * CLASS[w] else w - 1


def fan(widths, counts):
    """numbered in the postorder of the elimination tree: the sources that reach d (each behind its guard), d, the source that reaches the top only, the top"""
    K = len(widths)
    order = [i for i in range(K) if not (K == 3 and i == 1)] + ([1] if K == 3 else [])      # sources in the order they are numbered
    w, pos, guards = [], {}, []
    for i in order:
        if K == 3 and i == 1:
            d = len(w); w.append(WD)
        guards.append(len(w)); w.append(1)
        pos[i] = len(w); w.append(widths[i])
    if K != 3:
        d = len(w); w.append(WD)
    top = len(w); w.append(WTOP)
    L, U = {}, {}
    for i, (ws, cnt) in enumerate(zip(widths, counts)):
        s, g = pos[i], pos[i] - 1
        L[g], U[g] = {s: [0]}, {s: {0: 0}}
        nd = 0 if s > d else min(cnt, IN_D)
        leads = pn._leads(i + ws, cnt)
        offs = sorted(leads)
        assert len(offs) == cnt
        L[s], U[s] = {}, {}
        if nd:
            L[s][d] = list(range(1, 1 + nd))
            U[s][d] = {o: min(leads[o], ws - 1) for o in offs[:nd]}
        if cnt > nd:
            L[s][top] = list(range(1, 1 + cnt - nd))
            U[s][top] = {j + 1: min(leads[o], ws - 1) for j, o in enumerate(offs[nd:])}
    pn._link(L, U, d, top, range(1, WTOP), {c: c % 2 for c in range(1, WTOP)}, WD)
    name = "fan_" + "_".join("%dx%d" % (a, b) for a, b in zip(widths, counts))
    return pn.PanelCase(name, "k_panel_gemm chunks", w, L, U, guards=guards)


def _prepare(c):
    n, rp, ci = c.pattern_csr()
    assert n <= 1000
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    assert np.array_equal(symb.perm_c, np.arange(n))
    assert symb.xsup().tolist() == c.xsup.tolist(), symb.xsup().tolist()
    fs = symb.flat_store(values=False)
    symb.free()
    expL, expU = c.fill(fs)                          # (asserts the bounds of the product form: panel_bounds)
    return fs, expL, expU


def _copy(fs):
    return driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind.copy(), fs.Lnzval_off, fs.Lnzval.copy(), fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off,
                            fs.Unzval.copy())


def _exact(c, fs0, expL, expU, tag):
    fs = _copy(fs0)
    h = driver.LUHandle.from_store(fs)
    try:
        assert h.pdgstrf3d(0.0) == 0, (c.name, tag)
        h.copy_to_host(fs)
        for which, got, exp in (("L", fs.Lnzval, expL), ("U", fs.Unzval, expU)):
            assert np.array_equal(got, exp), (c.name, tag, which, int(np.count_nonzero(got != exp)), int(np.flatnonzero(got != exp)[0]))
        for k, w in enumerate(c.widths):
            a = int(c.xsup[k])
            li, ui = h.diag_inv(k, w)
            assert np.array_equal(li, c.Linv[a:a + w, a:a + w]), (c.name, tag, "Linv", k, w)
            assert np.array_equal(ui, c.Uinv[a:a + w, a:a + w]), (c.name, tag, "Uinv", k, w)
        for nrhs in NRHS:
            x, b = c.rhs(nrhs)
            got = h.pdgstrs3d(b.copy(order="F"))
            assert np.array_equal(got, x), (c.name, tag, nrhs, int(np.count_nonzero(got != x)))
    finally:
        h.destroy()


def _forms(fs, base, sched):
    """the panel lines of the source level under one schedule, by the restated rules: [(form, part, nl, nu)]"""
    srcs = sc.sources(fs)
    lev = sw.levels_of(srcs)
    cfg = dict(pn.DEFAULTS, **base)
    if sched == "panel_split0":
        cfg["panel_split"] = 0
    if sched == "no_lookahead":
        cfg["no_lookahead"] = True
    return [(x[1], x[7], x[5], x[6]) for x in pn.predicted_lines(srcs, lev, False, cfg) if x[0] == "panel" and x[2] == lev[1]]


def _run(widths, counts, monkeypatch, single):
    c = fan(widths, counts)
    fs, expL, expU = _prepare(c)
    want = "gemm%d" % (16 if max(widths) <= 64 else 32 if max(widths) <= 128 else 64)
    seen = set()
    for sched, env in SCHEDULES.items():
        for k, v in dict(env, **({"SLUAMD_TRSM_TAIL": "0"} if single else {})).items():
            monkeypatch.setenv(k, v)
        forms = _forms(fs, {"trsm_tail": 0} if single else {}, sched)
        assert forms and all(f[0] == want for f in forms), (c.name, sched, forms)       # the level under test runs the instantiation it is meant for
        assert sum(f[2] for f in forms) == sum(-(-n // 64) for n in counts) == sum(f[3] for f in forms), (c.name, sched, forms)
        seen |= {(sched, f[1]) for f in forms}
        _exact(c, fs, expL, expU, sched)
        for k in env:
            monkeypatch.delenv(k)
    assert {("panel_split0", "whole"), ("no_lookahead", "whole")} <= seen and all(p == "whole" for s, p in seen if s != "default"), seen
    return seen


@pytest.mark.parametrize("cnt", ROWS)
@pytest.mark.parametrize("w", sorted(CLASS))
def test_single_supernode_level(w, cnt, monkeypatch):
    """one supernode of the width under test on its level, a panel of `cnt` rows and `cnt` skyline columns; panels of more than 64 rows are split into
    urgent and other units by the default schedule (the `units` form of the launch), the others stay whole"""
    seen = _run([w], [cnt], monkeypatch, single=True)
    assert (("default", "0") in seen and ("default", "1") in seen) == (cnt > 64), seen


@pytest.mark.parametrize("triple", TRIPLES, ids=lambda t: "%d_%d_%d" % t)
@pytest.mark.parametrize("w", sorted(CLASS))
def test_three_supernode_level(w, triple, monkeypatch):
    """three supernodes on one level -- the width under test twice and the neighbouring width of the other parity between them, so ONE launch takes the
    16-byte and the predicated stage loads -- at the defaults: the level is split (the middle source reaches the top only: nothing of it is urgent)"""
    seen = _run([w, partner(w), w], list(triple), monkeypatch, single=False)
    assert ("default", "0") in seen and ("default", "1") in seen, seen


def test_the_widths_cover_the_chunk_boundaries():
    """every instantiation sees a last block of 1, 31 and 32 columns and block counts on both sides of its limit; both parities sit in every class"""
    for nq, ws in WIDTHS.items():
        assert max(ws) == 4 * nq and {w % 32 for w in ws} >= {0, 1, 31}, nq
        assert all(nq < partner(w) <= 4 * nq and (partner(w) - w) % 2 for w in ws)
    assert sorted(set(t[0] for t in TRIPLES) | set(t[2] for t in TRIPLES)) == ROWS
