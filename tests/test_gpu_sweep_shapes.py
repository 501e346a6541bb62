"""The triangular sweeps (pdgstrs3d / pzgstrs3d) against EXACT solutions, over the forms they take at run time: the builds of the sweep kernels, blocks
of four right-hand sides, right-hand-side chunks, ldx > n, joined and two-launch links and their mixtures, the complex16 fused links and the in-place pair,
process grids, the distributed entry point.  tests/sweep_cases.py builds B = L0 U0 whose diagonal blocks have DENSE exact inverses, so that an indexing
error in a diagonal strip, a 64 x 64 inverse block or a substitution multiplies non-zeros.  No tolerance appears in this file: every comparison of values
is numpy.array_equal (the rule for the sign of a stored zero is in schur_cases.py)."""
import ctypes as C
import functools, json, os, subprocess, sys
import numpy as np
import pytest
import oracle as orc
import schur_cases as sc
import sweep_cases as sw
from superlu_dist_amd import _lib, driver, grid3d

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NRHS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17)
EMUL = "emul" in os.path.basename(os.environ.get("SLUAMD_LIB", ""))


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """(case, flat store holding B, expected Lnzval, expected Unzval, sources, DAG levels): built once per case"""
    c = sw.CASES[name]()
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


def _factored(name, profile=False):
    """a handle holding the exact factors of case `name` (asserted); profile: factored under sluamd_set_profile(h, 1), which the solves then follow"""
    c, fs0, expL, expU = _prepared(name)[:4]
    fs = _copy(fs0)
    h = driver.LUHandle.from_store(fs)
    if profile:
        h.set_profile(True)
    assert h.pdgstrf3d(0.0) == 0
    h.copy_to_host()
    for which, got, exp in (("L", fs.Lnzval, expL), ("U", fs.Unzval, expU)):
        assert np.array_equal(got, exp), (name, which, int(np.count_nonzero(got != exp)))
    return h


def _solve_exact(name, h, nrhs_list):
    c = _prepared(name)[0]
    for nrhs in nrhs_list:
        x, b = c.rhs(nrhs)
        got = h.pdgstrs3d(b.copy(order="F"))
        bad = np.flatnonzero((got != x).any(axis=0))
        assert np.array_equal(got, x), (name, nrhs, "columns", bad.tolist()[:8], "first row", int(np.flatnonzero(got[:, bad[0]] != x[:, bad[0]])[0]))


@pytest.mark.parametrize("name", list(sw.CASES))
def test_factors_inverses_and_solution_are_exact(name):
    """every case at the defaults: the CPU oracle returns L0, U0 and x; the library returns L0 and U0 at every stored position, Linv and Uinv of every
    diagonal block (double; the complex path keeps none) and the integer x for 1 to 17 right-hand sides, every column a different vector: the blocks of
    four right-hand sides (nrhs >= 2) with 1, 2 and 3 surplus columns, and the two-launch links on every level (nrhs >= 4)"""
    c, fs0, expL, expU = _prepared(name)[:4]
    o = orc.LUStore(fs0.n, fs0.xsup, fs0.Lrowind_off, fs0.Lrowind, fs0.Lnzval_off, fs0.Lnzval.copy(), fs0.Ufstnz_off, fs0.Ufstnz, fs0.Unzval_off, fs0.Unzval.copy())
    assert orc.dfactor(o)[0] == 0
    assert np.array_equal(o.Lnzval, expL) and np.array_equal(o.Unzval, expU)
    x, b = c.rhs(5)
    assert np.array_equal(orc.dsolve(o, b.copy(order="F")), x)
    h = _factored(name)
    if not c.z:
        for k, w in enumerate(c.widths):
            a = int(c.xsup[k])
            li, ui = h.diag_inv(k, w)
            assert np.array_equal(li, c.Linv[a:a + w, a:a + w]), (name, "Linv", k, w)
            assert np.array_equal(ui, c.Uinv[a:a + w, a:a + w]), (name, "Uinv", k, w)
    _solve_exact(name, h, NRHS)
    h.destroy()


def test_chunks_of_right_hand_sides_are_exact():
    """run_solve_local cuts the right-hand sides into chunks of max_rhs_chunk columns (48 at 256 columns): 48, 49 and 97 on the 256-column case; 300
    right-hand sides on a case of at most 64 columns (one chunk; dynamic LDS above 64 KiB) -- every column exact"""
    h = _factored("widths")
    sizes = sw.level_sizes(_prepared("widths")[5])
    for nrhs, parts in ((48, (48,)), (49, (48, 1)), (97, (48, 48, 1))):                      # the launches of all chunks: the chunk is 48 columns wide
        _solve_exact("widths", h, (nrhs,))
        assert h.stats()["solve_launches"] == sum(sw.predicted_launches(sizes, r) for r in parts), nrhs
    h.destroy()
    h = _factored("narrow")
    _solve_exact("narrow", h, (300,))
    h.destroy()


@pytest.mark.parametrize("name", ["widths", "z_wide"])
def test_profiled_in_place_sweeps_are_the_unprofiled_ones_bitwise(name):
    """a handle factored under sluamd_set_profile(h, 1) solves with the plain in-place level loop (diagonal, then update, per level; no second vector) until
    the profile is switched off: on one handle the profiled and the unprofiled solutions are the same bits, and both are the integer x.  1 and 3
    right-hand sides, and one more than a chunk (48 at 256 columns, 30 at 200 complex16 columns): two chunks.  The in-place loop counts no launches."""
    c = _prepared(name)[0]
    chunk = (96 * 1024) // (max(c.widths) * (16 if c.z else 8))
    assert chunk == (30 if c.z else 48)
    h = _factored(name, profile=True)
    rhs = [c.rhs(nrhs) for nrhs in (1, 3, chunk + 1)]
    prof = []
    for x, b in rhs:
        prof.append(h.pdgstrs3d(b.copy(order="F")))
        assert h.stats()["solve_launches"] == 0, (name, x.shape[1])
    h.set_profile(False)                                                                    # takes effect at once; switching it on again would need a factorisation
    for (x, b), p in zip(rhs, prof):
        plain = h.pdgstrs3d(b.copy(order="F"))
        if not c.z:
            assert h.stats()["solve_launches"] > 0, (name, x.shape[1])                      # the links with the second vector ran
        assert np.array_equal(np.ascontiguousarray(p).view(np.uint64), np.ascontiguousarray(plain).view(np.uint64)), (name, x.shape[1])
        assert np.array_equal(p, x), (name, x.shape[1])
    h.destroy()


@pytest.mark.parametrize("name", ["widths", "z_narrow"])
def test_leading_dimension_larger_than_n(name):
    """ldx = n + 3 through the C ABI: the solution rows are exact, and the three padding rows of every column -- NaNs with a payload that tells the
    position -- come back bitwise unchanged"""
    c = _prepared(name)[0]
    h = _factored(name)
    n = c.n
    L = _lib.load()
    for nrhs in (1, 5, 49):
        x, b = c.rhs(nrhs)
        vs = 2 if c.z else 1
        buf = np.zeros(((n + 3) * vs, nrhs), dtype=np.uint64, order="F")
        for q in range(nrhs):
            buf[:n * vs, q] = np.ascontiguousarray(b[:, q]).view(np.uint64)
        pad = 0x7FF8000000000000 + 1 + np.arange(3 * vs, dtype=np.uint64)[:, None] + 16 * np.arange(nrhs, dtype=np.uint64)[None, :]
        buf[n * vs:, :] = pad
        if c.z:
            _lib.check(L.sluamd_pzgstrs3d(h._h, buf.ctypes.data_as(C.c_void_p), n + 3, nrhs), "sluamd_pzgstrs3d")
            got = np.stack([np.ascontiguousarray(buf[:n * vs, q]).view(np.complex128) for q in range(nrhs)], axis=1)
        else:
            _lib.check(L.sluamd_pdgstrs3d(h._h, buf.ctypes.data_as(_lib.P_dbl), n + 3, nrhs), "sluamd_pdgstrs3d")
            got = np.stack([np.ascontiguousarray(buf[:n, q]).view(np.float64) for q in range(nrhs)], axis=1)
        assert np.array_equal(got, x), (name, nrhs)
        assert np.array_equal(buf[n * vs:, :], pad), (name, nrhs)
    h.destroy()


@pytest.mark.parametrize("maxn", [2 ** 30, 32, 4, 1])
@pytest.mark.parametrize("join", [1, 0])
def test_link_forms_are_exact_and_scheduled_as_restated(join, maxn, monkeypatch):
    """SLUAMD_SOLVE_JOIN x SLUAMD_JOIN_MAX_NODES on `levels` (levels of 66, 1, 33, 4, 2 and 1 supernodes): joined and two-launch links in every mixture; the
    solutions are exact and the number of launches is what the restatement of level_joined (sweep_cases.predicted_launches) gives for the level sizes"""
    monkeypatch.setenv("SLUAMD_SOLVE_JOIN", str(join)); monkeypatch.setenv("SLUAMD_JOIN_MAX_NODES", str(maxn))
    c, _, _, _, srcs, lev = _prepared("levels")
    sizes = sw.level_sizes(lev)
    h = _factored("levels")
    assert h.plan_table()[:, 2].astype(int).tolist() == sizes
    for nrhs in (1, 3, 4, 9):
        _solve_exact("levels", h, (nrhs,))
        assert h.stats()["solve_launches"] == sw.predicted_launches(sizes, nrhs, maxn, bool(join)), (join, maxn, nrhs)
    h.destroy()


CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_sweep_shapes as t
out = {}
for name in ("widths", "levels", "wide_launch"):
    h = t._factored(name)
    c = t._prepared(name)[0]
    for nrhs in (1, 3, 4, 9):
        x, b = c.rhs(nrhs)
        sys.stderr.write("[case] %s %d\n" % (name, nrhs)); sys.stderr.flush()
        got = h.pdgstrs3d(b.copy(order="F"))
        out["%s:%d" % (name, nrhs)] = bool(t.np.array_equal(got, x))
    h.destroy()
print("RESULT " + json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def _build_child(v):
    """one child process per build (SLUAMD_SWEEP_WIDE_V and SLUAMD_SWEEP_WIDE_MIN are read when the library is loaded); run once, never retried"""
    env = dict(os.environ, SLUAMD_SWEEP_WIDE_V=str(v), SLUAMD_SWEEP_WIDE_MIN="1", SLUAMD_SOLVE_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("v", [0, 1, 5])
def test_sweep_builds_are_exact(v):
    """the builds of the sweep kernels (SLUAMD_SWEEP_WIDE_V = 0 / 1 / 5 with SLUAMD_SWEEP_WIDE_MIN=1): `widths`, `levels` and `wide_launch` with 1, 3, 4 and 9
    right-hand sides are exact under each"""
    rc, out, err = _build_child(v)
    assert rc == 0, out[-1500:] + err[-1500:]
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == 12 and all(res.values()), res


@pytest.mark.parametrize("v", [0, 1, 5])
def test_sweep_builds_ran(v):
    """the SLUAMD_SOLVE_DEBUG lines of the launch wrappers prove which build ran in the child of test_sweep_builds_are_exact: the wide launches run build v,
    blocks of right-hand sides turn 5 into 1 (except in the joined units, which have no blocked form), narrow launches run the narrow build (10)"""
    if EMUL:
        pytest.skip("the emulation engine has no builds")
    rc, out, err = _build_child(v)
    assert rc == 0, out[-1500:] + err[-1500:]
    case, seen = None, {}
    for ln in err.splitlines():
        if ln.startswith("[case] "):
            case = ln.split()[1]
        elif ln.startswith("[sluamd sweep] "):
            f = dict(tok.split("=") for tok in ln.split()[2:])
            mx, nrhs, build = int(f["mx"]), int(f["nrhs"]), int(f["build"])
            want = 10 if mx <= 64 else 1 if (v == 5 and nrhs >= 2 and f["family"] != "sweep_join") else v
            assert build == want, ln
            seen.setdefault((case, f["family"], nrhs >= 2), set()).add(build)
    for case in ("widths", "levels", "wide_launch"):
        for fam in ("fwd_update", "bwd_update", "sweep_step"):
            assert (1 if v == 5 else v) in seen.get((case, fam, True), set()), (case, fam, seen)
        assert v in seen.get((case, "sweep_join", False), set()), (case, seen)
    assert 10 in seen.get(("levels", "sweep_step", False), set()) and 10 in seen.get(("levels", "sweep_step", True), set())      # its lowest level is narrow


@pytest.mark.parametrize("groups", [0, 1])
def test_merged_chain_groups_are_exact(groups, monkeypatch):
    """SLUAMD_SOLVE_GROUPS 0 / 1 on `groups` (k_grp_gather, k_gemm_batched, the strips of the group's inverse, dead rows and columns): exact; fewer launches
    with the group; 30 right-hand sides (240 x 30 doubles > 48 KiB: groups_fit refuses) run the ungrouped schedule on the handle that has the group"""
    monkeypatch.setenv("SLUAMD_SOLVE_GROUPS", str(groups))
    sizes = sw.level_sizes(_prepared("groups")[5])
    assert sizes == [2, 2, 1, 1, 1, 1, 1]
    h = _factored("groups")
    for nrhs in (1, 3, 5, 30):
        _solve_exact("groups", h, (nrhs,))
        la, plain = h.stats()["solve_launches"], sw.predicted_launches(sizes, nrhs)
        if groups and nrhs < 30:
            assert la < plain, (nrhs, la, plain)
            # the contracted schedule: levels 2, 2, group, top; the group's level keeps the two-launch form
            assert la == sw.predicted_launches([2, 2, 4, 1], nrhs, has_group=[0, 0, 1, 0]), (nrhs, la)
        elif not groups:
            assert la == plain, (nrhs, la, plain)
        else:                                                                               # refused: not the contracted schedule (18 launches at nrhs >= 4)
            assert la > sw.predicted_launches([2, 2, 4, 1], nrhs, has_group=[0, 0, 1, 0]), (nrhs, la)
    h.destroy()


@pytest.mark.parametrize("env", [{}, {"SLUAMD_ZFUSE_MAX_NODES": "0"}, {"SLUAMD_ZFUSE_MAX_NODES": str(2 ** 30)}, {"SLUAMD_NO_ZTRSM_QUAD": "1"}],
                         ids=["default", "never-fused", "always-fused", "no-quad"])
def test_complex16_sweeps_are_exact(env):
    """complex16: fused links (kz_fwd_fused / kz_bwd_fused with tickets) against the in-place pair across SLUAMD_ZFUSE_MAX_NODES = 0 / 16 / 2^30, and
    kz_solve_diag[_wave] on supernodes of up to 200 columns, with 1, 2 and 5 right-hand sides.  SLUAMD_NO_ZTRSM_QUAD is read when the library is loaded:
    every variant runs in a child process of its own."""
    code = ("import os, sys\nsys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\nimport test_gpu_sweep_shapes as t\n"
            "for name in ('z_narrow', 'z_wide', 'z_levels'):\n    h = t._factored(name)\n    t._solve_exact(name, h, (1, 2, 5))\n"
            "    print('LAUNCHES', name, h.stats()['solve_launches'])\n    h.destroy()\nprint('RESULT ok')\n")
    r = subprocess.run([sys.executable, "-c", code, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    la = {ln.split()[1]: int(ln.split()[2]) for ln in r.stdout.splitlines() if ln.startswith("LAUNCHES")}
    sizes = sw.level_sizes(_prepared("z_levels")[5])
    zf = int(env.get("SLUAMD_ZFUSE_MAX_NODES", "16"))
    if zf > 0:                                                                              # zsolve_fused: one launch per fused level and sweep, two otherwise
        assert la["z_levels"] == 2 * sum(1 if s <= zf else 2 for s in sizes), (la, sizes)
    assert la["z_wide"] == 0                                                                # wider than 64 columns: the fused links do not engage (the level loop counts nothing)
    if "SLUAMD_ZFUSE_MAX_NODES" not in env:
        assert any(s <= 16 for s in sizes) and any(s > 16 for s in sizes)                  # the levels straddle the default


@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 2, 1), (1, 1, 2), (2, 2, 2)])
@pytest.mark.parametrize("name", ["widths", "z_narrow"])
def test_process_grids_return_the_exact_solution(name, grid):
    """the grid sweeps (k_solve_diag with its 64-column block skipping, k_fwd_update / k_bwd_update through find_node_wave; the complex twins) on
    Pr x Pc x Pz thread grids: the integer x back from every rank, 1 and 5 right-hand sides"""
    c = _prepared(name)[0]
    n, rp, ci = c.pattern_csr()
    rows = np.repeat(np.arange(n), np.diff(rp))
    v = c.B[rows, ci].copy()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    Pr, Pc, Pz = grid
    tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)
    rhs = [c.rhs(1), c.rhs(5)]

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], tree)
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


def test_distributed_entry_point_is_exact():
    """sluamd_pdgstrs3d_dist on one rank (identity permutations): 1, 3 and 60 right-hand sides (60 > one chunk of 48 on the 256-column case)"""
    c = _prepared("widths")[0]
    h = _factored("widths")
    for nrhs in (1, 3, 60):
        x, b = c.rhs(nrhs)
        got = h.pdgstrs3d_dist(b.copy(order="F"))
        assert np.array_equal(got, x), nrhs
    h.destroy()


def test_the_cases_cover_every_decision():
    """Coverage recomputed from the exported structure (xsup, L row lists, Ufstnz), plan_table() and the restated schedule, never from the kernels"""
    seen = set()
    for name in sw.CASES:
        c, fs0, _, _, srcs, lev = _prepared(name)
        sizes = sw.level_sizes(lev)
        h = driver.LUHandle.from_store(_copy(fs0))
        pt = h.plan_table()
        h.destroy()
        assert pt[:, 2].astype(int).tolist() == sizes, name                                # the restated DAG levels are the library's
        widest = [max(s["w"] for s in srcs if lev[s["k"]] == l) for l in range(len(sizes))]
        assert pt[:, 3].astype(int).tolist() == widest, name
        pre = "z:" if c.z else ""
        for s in srcs:
            seen.add(f"{pre}w:{s['w']}")
            l = lev[s["k"]]
            for nr, nnear in sw.strips(s, lev):
                seen.add(f"{pre}strip:{nr}")
                if 0 < nnear < nr:
                    seen.add(pre + "strip:near-and-far-rows")
            if any(ld > 0 for _, cols in s["ublocks"] for ld in cols.values()):
                seen.add(pre + "u:skyline-leads")
            nc = sw.near_columns(s, lev)
            mx = max(widest[l], widest[l - 1] if l else 0)
            if nc > 64 and mx <= 64:
                seen.add(pre + "near-columns:>64:narrow")
            if nc > 256 and 64 < mx <= 256:
                seen.add(pre + "near-columns:>256:wide")
            if lev[s["k"]] > 0:
                for cnt in sw.forward_sources(srcs, lev, s, fs0.xsup):
                    seen.add(f"{pre}sources:{'>=6' if cnt >= 6 else cnt}")
        for per in [sorted(len(r) for g2, r in s["lblocks"]) for s in srcs]:
            for nr in per:
                seen.add(f"{pre}rows-per-destination:{nr}")
        if name == "levels":
            for s_ in sizes:
                seen.add("level-size:" + (">=64" if s_ >= 64 else str(s_)))
            for maxn in (2 ** 30, 32, 4, 1):
                J = [sw.joined(sizes, m, 1, maxn) for m in range(len(sizes))]
                for a, b in zip(J[:-1], J[1:]):
                    seen.add(f"links:{'joined' if a else 'two-launch'}->{'joined' if b else 'two-launch'}")
    for nrhs in NRHS:
        if nrhs >= 2 and nrhs % 4:
            seen.add(f"rk-surplus:{4 - nrhs % 4}")
    # (the chunk boundary is pinned by the launch counts of test_chunks_of_right_hand_sides_are_exact)
    need = {f"w:{w}" for w in sw.WIDTHS} | {f"z:w:{w}" for w in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 200)}
    need |= {f"rows-per-destination:{r}" for r in (1, 63, 64, 65, 130)} | {f"strip:{r}" for r in (1, 63, 64)} | {"strip:near-and-far-rows", "u:skyline-leads", "z:u:skyline-leads"}
    need |= {"level-size:1", "level-size:4", "level-size:33", "level-size:>=64", "links:joined->joined", "links:two-launch->joined", "links:joined->two-launch",
             "links:two-launch->two-launch"}
    need |= {"sources:1", "sources:3", "sources:4", "sources:>=6", "near-columns:>64:narrow", "near-columns:>256:wide", "rk-surplus:1", "rk-surplus:2", "rk-surplus:3"}
    assert need <= seen, sorted(need - seen)
