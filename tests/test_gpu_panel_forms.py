"""The panel chain of the factorisation (diagonal LU -> Linv / Uinv -> L and U panel solves; pdgstrf3d / pzgstrf3d) against EXACT factors over the forms it
takes at run time: product and substitution panels, tail and non-tail levels, 32- and 64-row strips, split panel solves, the inverse kernels on and off the
chain, the diagonal LU kernels, the complex16 kernels of every width class, narrow supernodes on levels of wide ones, process grids.  tests/panel_cases.py
builds the matrices and restates the decision rules; the `[sluamd panel]` launch lines of SLUAMD_FACTOR_DEBUG prove which form ran.  No tolerance appears
in this file: every comparison of values is numpy.array_equal (the rule for the sign of a stored zero is in schur_cases.py)."""
import functools, json, os, subprocess, sys
import numpy as np
import pytest
import panel_cases as pn
import pivot_cases as pc
import schur_cases as sc
import sweep_cases as sw
from superlu_dist_amd import driver, grid3d

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = "emul" in os.path.basename(os.environ.get("SLUAMD_LIB", ""))
NRHS = (1, 3)


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """(case, flat store holding B, expected Lnzval, expected Unzval, sources, DAG levels): built once per case"""
    c = pn.CASES[name]()
    n, rp, ci = c.pattern_csr()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    assert np.array_equal(symb.perm_c, np.arange(n))
    assert symb.xsup().tolist() == c.xsup.tolist(), symb.xsup().tolist()
    fs = symb.flat_store(values=False)
    symb.free()
    expL, expU = c.fill(fs)
    srcs = sc.sources(fs)
    return c, fs, expL, expU, srcs, sw.levels_of(srcs)


def _copy(fs):
    return driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind.copy(), fs.Lnzval_off, fs.Lnzval.copy(), fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off,
                            fs.Unzval.copy())


def _factor_exact(name, h, fs, tag=""):
    """one factorisation of the values the handle holds: info == 0, L0 and U0 at every stored position of `fs` after the copy back"""
    expL, expU = _prepared(name)[2:4]
    assert h.pdgstrf3d(0.0) == 0, (name, tag)
    h.copy_to_host(fs)
    for which, got, exp in (("L", fs.Lnzval, expL), ("U", fs.Unzval, expU)):
        assert np.array_equal(got, exp), (name, tag, which, int(np.count_nonzero(got != exp)), int(np.flatnonzero(got != exp)[0]))


def _demand_exact(name, h, tag=""):
    """Linv / Uinv of every diagonal block (double) and the integer x for 1 and 3 right-hand sides"""
    c = _prepared(name)[0]
    if not c.z:
        for k, w in enumerate(c.widths):
            a = int(c.xsup[k])
            li, ui = h.diag_inv(k, w)
            assert np.array_equal(li, c.Linv[a:a + w, a:a + w]), (name, tag, "Linv", k, w)
            assert np.array_equal(ui, c.Uinv[a:a + w, a:a + w]), (name, tag, "Uinv", k, w)
    for nrhs in NRHS:
        x, b = c.rhs(nrhs)
        got = h.pdgstrs3d(b.copy(order="F"))
        assert np.array_equal(got, x), (name, tag, nrhs, int(np.count_nonzero(got != x)))


def _run(name, tag="", again=False, mark=None, **opts):
    fs = _copy(_prepared(name)[1])
    h = driver.LUHandle.from_store(fs, **opts)
    if mark:
        mark("factor")
    _factor_exact(name, h, fs, tag)
    if mark:
        mark("demand")
    _demand_exact(name, h, tag)
    if again:                                        # new values into the factored handle, a second factorisation
        fs2 = _copy(_prepared(name)[1])
        h.set_values(fs2)
        _factor_exact(name, h, fs2, tag + " second")
        _demand_exact(name, h, tag + " second")
    h.destroy()


@pytest.mark.parametrize("name", list(pn.CASES))
def test_defaults_are_exact(name):
    """every case at the defaults: L0 and U0 at every stored position, Linv and Uinv of every diagonal block (double), the integer x for 1 and 3 right-hand
    sides; on `chain_wide` and `split` a second factorisation after set_values"""
    _run(name, again=name in ("chain_wide", "split"))


@pytest.mark.parametrize("name", list(pn.CASES))
@pytest.mark.parametrize("variant", [v for v in pn.PER_HANDLE if v != "default"])
def test_switches_read_per_handle_are_exact(variant, name, monkeypatch):
    """the switches a handle reads when it is created (and the deterministic option): every case returns the values of the default run -- the exact ones.
    SLUAMD_TRSM_PANELS: the factorisation leaves no Linv / Uinv (inv_ready is false); they are ABSENT, not refused -- the first demand (sluamd_dGetDiagInv,
    a solve) computes them (ensure_inv), and they are the exact ones; test_the_forms_that_ran_are_the_restated_ones sees those launches with where=demand."""
    env, st = pn.VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _run(name, tag=variant, deterministic=bool(st.get("deterministic")))


# ---------------------------------------------------------------------------------------------------------------------------------------
# Child processes: SLUAMD_FACTOR_DEBUG (and SLUAMD_NO_FULL_INV64, SLUAMD_ZLU4_MAX_NODES, SLUAMD_NO_ZTRSM_QUAD) are read when the library is loaded
# ---------------------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_panel_forms as t
print("RESULT " + json.dumps(t.child_body(sys.argv[2].split(","), sys.argv[3].split(","))))
"""


def child_body(variants, names):
    out = {}
    for v in variants:
        env, st = pn.VARIANTS[v]
        os.environ.update(env)                       # (the variables read at load are set by the parent already)
        for name in names:
            def mark(phase):
                sys.stderr.write("[case] %s %s %s\n" % (name, v, phase)); sys.stderr.flush()
            try:
                _run(name, tag=v, mark=mark, deterministic=bool(st.get("deterministic")))
                out["%s:%s" % (v, name)] = True
            except AssertionError as e:
                out["%s:%s" % (v, name)] = repr(e)[:300]
        for k in env:
            os.environ.pop(k)
    return out


GRID_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_panel_forms as t
t._grid_exact(sys.argv[2], (2, 1, 1))
print("RESULT ok")
"""


@functools.lru_cache(maxsize=None)
def _grid_child(name):
    """case `name` on a 2 x 1 x 1 thread grid in a child process that prints the launch lines (of both ranks, interleaved line by line); run once, never retried"""
    r = subprocess.run([sys.executable, "-c", GRID_CHILD, ROOT, name], env=dict(os.environ, SLUAMD_FACTOR_DEBUG="1"), capture_output=True, text=True, timeout=600, cwd=ROOT)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("name", ["chain_wide", "mixed_level"])
def test_the_forms_of_an_xy_layer(name):
    """2 x 1 x 1: exact under the launch lines, and BOTH ranks launch, on every level, the diagonal LU the restated rule names, k_diag_inv on the diagonal blocks
    they hold after the exchange (family diag_inv), the full inverses on the chain, and the product form of the panel solves (gemm16 / 32 / 64 by the widest
    supernode; no substitution form, no tail level, nothing deferred: run_factor_sched sets trsm_tail = 0 on an XY layer)"""
    rc, out, err = _grid_child(name)
    assert rc == 0 and "RESULT ok" in out, out[-1500:] + err[-1500:]
    if EMUL:
        pytest.skip("the emulation engine has no forms")
    c, _, _, _, srcs, lev = _prepared(name)
    got = pn.parse_lines(err)
    assert all(x[8] == "chain" and x[7] == "whole" and not x[1].startswith("trsm") for x in got), [x for x in got if x[8] != "chain" or x[1].startswith("trsm")][:4]
    want = pn.predicted_grid_forms(srcs, lev)
    fixed = sorted((x[0], x[1], x[2], x[3], x[7], x[8]) for x in got if x[0] != "panel")
    assert fixed == sorted(2 * [w for w in want if w[0] != "panel"]), (name, fixed[:6])
    # panels: a rank launches where it owns strips or chunks of the level -- every level with panels on at least one rank, always the restated form
    panels = {(x[0], x[1], x[2], x[3], x[7], x[8]) for x in got if x[0] == "panel"}
    assert panels == {w for w in want if w[0] == "panel"}, (name, sorted(panels)[:6])
    tab = pn.level_table(srcs, lev)
    for l, (nn, mx, per) in enumerate(tab):          # the two ranks' strips together are at least the level's (a supernode's rows are dealt over both)
        lines = [x for x in got if x[0] == "panel" and x[2] == l]
        assert sum(x[5] for x in lines) >= sum(pn._ceil(pn.rows_below(s), 64) for s in per) and sum(x[6] for x in lines) == sum(pn._ceil(pn.ucols(s), 64) for s in per if s["k"] >= 0), (name, l, lines)


def _names(variant):
    return ["z_chain"] if variant in ("zlu4", "no_ztrsm_quad") else [n for n in pn.CASES if n != "z_chain"] if variant == "no_full_inv64" else list(pn.CASES)


@functools.lru_cache(maxsize=None)
def _child(group):
    """one child process per group of variants -- the per-handle ones share one, each variable read at load has its own; run once, never retried"""
    variants = pn.PER_HANDLE if group == "per_handle" else [group]
    env = dict(os.environ, SLUAMD_FACTOR_DEBUG="1")
    if group != "per_handle":
        env.update(pn.VARIANTS[group][0])
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, ",".join(variants), ",".join(_names(group))], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    return r.returncode, r.stdout, r.stderr


def _group(variant):
    return variant if variant in pn.AT_LOAD else "per_handle"


def _lines(variant):
    """{(case, phase): [launch lines]} of one variant from its child's stderr"""
    rc, out, err = _child(_group(variant))
    assert rc == 0, out[-1500:] + err[-1500:]
    key, per = None, {}
    for ln in err.splitlines():
        if ln.startswith("[case] "):
            _, name, v, phase = ln.split()
            key = (name, phase) if v == variant else None
            if key:
                per[key] = []
        elif key and ln.startswith("[sluamd panel] "):
            per[key] += pn.parse_lines(ln)
    return per


@pytest.mark.parametrize("variant", pn.AT_LOAD)
def test_switches_read_at_load_are_exact(variant):
    """SLUAMD_NO_FULL_INV64 (double cases), SLUAMD_ZLU4_MAX_NODES = 2^30 and SLUAMD_NO_ZTRSM_QUAD (complex16): exact factors, inverses and solutions"""
    rc, out, err = _child(variant)
    assert rc == 0, out[-1500:] + err[-1500:]
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == len(_names(variant)) and all(v is True for v in res.values()), res


def test_every_variant_is_exact_under_the_launch_lines():
    """the child that prints the launch lines runs every per-handle variant on every case: all exact there too (the lines change nothing)"""
    rc, out, err = _child("per_handle")
    assert rc == 0, out[-1500:] + err[-1500:]
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == len(pn.PER_HANDLE) * len(pn.CASES) and all(v is True for v in res.values()), {k: v for k, v in res.items() if v is not True}


@pytest.mark.parametrize("variant", list(pn.VARIANTS))
def test_the_forms_that_ran_are_the_restated_ones(variant):
    """per case: the `[sluamd panel]` lines of the factorisation ARE the lines the restated rules give (family, form, level, supernodes, widest supernode,
    strips, chunks, part, stream role); the first demand for inverses and solutions launches nothing of the chain -- except under SLUAMD_TRSM_PANELS,
    where it computes the inverses of every level after the factorisation (where=demand)"""
    if EMUL:
        pytest.skip("the emulation engine has no forms")
    per = _lines(variant)
    cfg = pn.settings(variant)
    for name in _names(variant):
        c, _, _, _, srcs, lev = _prepared(name)
        want = pn.predicted_lines(srcs, lev, c.z, cfg)
        got = sorted(per[(name, "factor")])
        assert got == want, (name, [x for x in got if x not in want][:6], [x for x in want if x not in got][:6])
        later = per[(name, "demand")]
        if cfg["trsm_panels"] and not c.z:
            tab = pn.level_table(srcs, lev)
            assert sorted(later) == sorted(("full_inv", "inv64" if mx <= 64 else "inv", l, nn, mx, 0, 0, "whole", "demand") for l, (nn, mx, _) in enumerate(tab)), name
            assert not any(x[0] == "full_inv" for x in got)
        else:
            assert later == [], (name, later[:4])


def test_named_forms_ran():
    """the assertions the forms were built for, read off the lines themselves"""
    if EMUL:
        pytest.skip("the emulation engine has no forms")
    def of(variant, name):
        return _lines(variant)[(name, "factor")]
    t2 = of("trsm_tail2", "chain_wide")             # levels 2 .. 5 (33, 65, 129, 200 columns) are not tail levels, 6 and 7 (256) are
    assert {(x[1], x[2]) for x in t2 if x[0] == "panel" and x[3] == 1 and x[2] >= 2} == {("gemm16", 2), ("gemm32", 3), ("gemm64", 4), ("gemm64", 5), ("trsm64", 6)}
    assert {(x[2], x[8]) for x in t2 if x[0] == "full_inv"} == {(l, "chain") for l in range(6)} | {(6, "bulk"), (7, "bulk")}
    assert all(x[8] == "chain" for x in of("trsm_tail0", "chain_wide")) and sum(x[8] == "bulk" for x in of("default", "chain_wide")) == 6
    d2 = of("diag_tail2", "chain_wide")
    assert {(x[1], x[2]) for x in d2 if x[0] == "diag_lu" and x[4] > 64} == {("lu2_2", 3), ("lu2_2", 4), ("lu2_2", 5), ("lu2_1", 6), ("lu2_1", 7)}
    tb = of("default", "tail_boundary")             # the rule l >= nlevels - 64 crossed at the defaults
    assert {x[2] for x in tb if x[1] == "gemm16"} == set(range(9)) and {x[2] for x in tb if x[1] == "trsm64"} == set(range(9, 72))
    assert {x[2] for x in tb if x[0] == "full_inv" and x[8] == "chain"} == set(range(9)) and {x[2] for x in tb if x[8] == "bulk"} == set(range(9, 73))
    sp_ = [x for x in of("default", "split") if x[0] == "panel"]
    assert [(x[2], x[7], x[5], x[6]) for x in sorted(sp_, key=lambda x: (x[2], x[7])) if x[7] != "whole"] == [(3, "0", 1, 1), (3, "1", 1, 1), (4, "0", 2, 2), (4, "1", 2, 2)]
    assert {x[1] for x in sp_ if x[7] != "whole"} == {"trsm64"}
    assert {x[1] for x in of("trsm_tail0", "split") if x[7] != "whole"} == {"gemm16", "gemm64"}
    for name in pn.CASES:
        assert all(x[7] == "whole" for v in ("panel_split0", "no_lookahead", "deterministic") for x in of(v, name)), name
    assert [(x[2], x[5], x[6]) for x in sorted(of("rs32", "rs32")) if x[1] == "trsm32"] == [(1, 1, 1), (2, 1, 1), (3, 2, 2), (4, 4, 4)]
    zf = {x[1] for v in ("default", "zlu4", "no_ztrsm_quad") for x in of(v, "z_chain")}
    assert zf == {"zwave_small8", "zwave_small16", "zwave_small32", "zwave", "zwave4", "zlu", "zquad4", "zquad8", "zquad16", "ztrsm"}, zf


@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 2, 1), (2, 2, 1)])
@pytest.mark.parametrize("name", ["chain_wide", "mixed_level", "z_chain"])
def test_thread_grids_return_the_exact_solution(name, grid):
    """Pr x Pc x 1 thread grids: the peers of a diagonal block invert the copy they receive (k_diag_inv), k_pack_diag packs the blocks, the panels go through
    k_panel_gemm on XY layers (the complex twins substitute on the received block): info == 0 and the integer x from every rank, 1 and 3 right-hand sides.
    (Values only: which forms ran on an XY layer is what test_the_forms_of_an_xy_layer reads off the launch lines.)"""
    _grid_exact(name, grid)


def _grid_exact(name, grid):
    c, fs0 = _prepared(name)[:2]
    # the matrix handed over is B on the STORED pattern (the designed one closed under fill -- the symbolic factorisation lowers leads, and B holds values there)
    (lr, lc), (ur, uc) = pc.store_positions(fs0)
    mask = np.zeros((c.n, c.n), dtype=bool)
    mask[lr[lr >= 0], lc[lr >= 0]] = True
    mask[ur[ur >= 0], uc[ur >= 0]] = True
    n, rows, ci = c.n, *np.nonzero(mask)
    rp = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    ci = ci.astype(np.int32)
    v = c.B[rows, ci].copy()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    assert np.array_equal(symb.perm_c, np.arange(n)) and symb.xsup().tolist() == c.xsup.tolist()
    Pr, Pc, Pz = grid
    comms = grid3d.local_comms(Pr, Pc, Pz)
    rhs = [c.rhs(r) for r in NRHS]

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], None)
        info = h.pdgstrf3d(0.0)
        ys = [h.pdgstrs3d(b.copy(order="F")) for _, b in rhs]
        h.destroy()
        return info, ys

    out = grid3d.run_ranks(Pr * Pc * Pz, body)
    symb.free()
    for rank, (info, ys) in enumerate(out):
        assert info == 0
        for (x, _), y in zip(rhs, ys):
            assert np.array_equal(y, x), (rank, x.shape[1], int(np.count_nonzero(y != x)))


def test_the_cases_cover_every_form():
    """Coverage recomputed from the exported structure and the restated rules, never from the kernels: the tags (family, form, part, single / multi-supernode
    level, narrow supernode on a wide level) of all cases under all variants, and of the 2 x 1 x 1 layer, contain the table of the launch line.  The tags come
    from the RESTATED rules: that the device launches what they say is what test_the_forms_that_ran_are_the_restated_ones and test_the_forms_of_an_xy_layer
    assert on the lines themselves -- on the CPU build, where those skip, this test checks the restatement against the table only."""
    seen = set()
    for name in pn.CASES:
        c, fs0, _, _, srcs, lev = _prepared(name)
        h = driver.LUHandle.from_store(_copy(fs0))
        pt = h.plan_table()
        h.destroy()
        tab = pn.level_table(srcs, lev)
        assert pt[:, 2].astype(int).tolist() == [nn for nn, _, _ in tab] and pt[:, 3].astype(int).tolist() == [mx for _, mx, _ in tab], name      # the restated levels are the library's
        for v in pn.VARIANTS:
            if name in _names(v):
                lines = pn.predicted_lines(srcs, lev, c.z, pn.settings(v))
                seen |= pn.tags(lines, srcs, lev)
                seen |= {("where", x[0], x[8]) for x in lines}
        if name in ("chain_wide", "mixed_level"):
            seen |= {("xy", f, form, "single" if nn == 1 else "multi") for f, form, l, nn, part, where in pn.predicted_grid_forms(srcs, lev)}
    P, S, M, N, W = "plain", "single", "multi", "narrow-in-wide", "whole"
    need = {("diag_lu", "wave", W, S, P), ("diag_lu", "wave", W, M, P), ("diag_lu", "lu2_1", W, S, P), ("diag_lu", "lu2_2", W, S, P), ("diag_lu", "lu2_2", W, M, N),
            ("diag_lu", "v1_128", W, S, P), ("diag_lu", "v1_128", W, M, N), ("diag_lu", "v1_256", W, S, P), ("diag_lu", "v1_256", W, M, N),
            ("full_inv", "inv64", W, S, P), ("full_inv", "inv64", W, M, P), ("full_inv", "inv", W, S, P), ("full_inv", "inv", W, M, N),
            ("where", "full_inv", "chain"), ("where", "full_inv", "bulk"),
            ("panel", "gemm16", W, S, P), ("panel", "gemm16", W, M, P), ("panel", "gemm32", W, S, P), ("panel", "gemm32", W, M, N), ("panel", "gemm32", "0", M, N),
            ("panel", "gemm32", "1", M, N), ("panel", "gemm64", W, S, P), ("panel", "gemm64", W, M, N), ("panel", "gemm64", "0", S, P), ("panel", "gemm64", "1", S, P),
            ("panel", "gemm64", "0", M, N), ("panel", "gemm16", "0", S, P), ("panel", "gemm16", "1", S, P),
            ("panel", "trsm64", W, S, P), ("panel", "trsm64", W, M, N), ("panel", "trsm64", "0", S, P), ("panel", "trsm64", "1", S, P), ("panel", "trsm32", W, S, P),
            ("panel", "trsm32", W, M, N)}
    need |= {("xy", "diag_inv", "inv", S), ("xy", "diag_inv", "inv", M), ("xy", "panel", "gemm16", M), ("xy", "panel", "gemm32", S), ("xy", "panel", "gemm32", M),
             ("xy", "panel", "gemm64", S), ("xy", "panel", "gemm64", M), ("xy", "full_inv", "inv", M), ("xy", "full_inv", "inv64", M), ("xy", "diag_lu", "lu2_1", S)}
    need |= {("diag_lu", f, W, M, P) for f in ("zwave_small8", "zwave_small16", "zwave_small32", "zwave", "zwave4")} | {("diag_lu", "zlu", W, M, N)}
    need |= {("panel", f, W, M, P) for f in ("zquad4", "zquad8", "zquad16")} | {("panel", "ztrsm", W, M, N), ("panel", "ztrsm", W, M, P)}
    assert need <= seen, sorted(need - seen)
