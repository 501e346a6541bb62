"""The transposed and conjugate-transposed solves, their refinement and the expert solve on XY process grids (sluamd_tsolve.cpp: tsweep_fwd_z / tsweep_bwd_z over
LevelSched::xt_*, the four xseg_exchange calls per level; sluamd_trefine.cpp) against integer systems whose solution is known EXACTLY
(tests/grid_trans_exact_cases.py: the cases, the bounds, what each (case, grid) pair exercises -- asserted by test_grid_trans_exact_cases_cpu.py).

Every comparison of values is numpy.array_equal, on every rank, with one exception that is stated where it is made (the expert solve under equilibration,
whose scalings round).  Every test first asserts info == 0 and that the UNTRANSPOSED solve of the same handles returns its integer x: that proves the factors
before anything is asked of the transposed path.  Ranks are threads over grid3d.local_comms; every test runs them in a child process under a time limit, once
and never retried (the pattern of test_gpu_refine_exact._grid_child), so ranks that fall out of step end the test and do not hang it."""
import ctypes as C
import os, pickle, subprocess, sys
import numpy as np
import pytest
import grid_trans_exact_cases as gx
import trans_cases as tc
from superlu_dist_amd import _lib, driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 240
EPS = 2.0 ** -53
_gid = lambda g: "%dx%dx%d" % tuple(g)


def _child(fn, *args, torch_first=False):
    """run test_gpu_grid_trans_exact.<fn>(*args) in a child process; the child asserts and prints RESULT ok"""
    code = ("import os, sys\n" + ("import torch\n" if torch_first else "") + "sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\n"
            "import test_gpu_grid_trans_exact as t\ngetattr(t, %r)(*%r)\nprint('RESULT ok')\n" % (fn, tuple(args)))
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=CHILD_LIMIT_S, cwd=ROOT)
    sys.stdout.write(r.stdout[-3000:])
    assert r.returncode == 0 and "RESULT ok" in r.stdout, "child exit %d\n" % r.returncode + r.stdout[-1500:] + r.stderr[-2500:]


def _proved(name, grid, out):
    """info == 0 and the untransposed integer x on every rank: the factors on this grid are the exact ones"""
    x5 = gx.prepared(name)[0].rhs(5)[0]
    assert len(out) == grid[0] * grid[1] * grid[2]
    for rank, (info, y, _, _) in enumerate(out):
        assert info == 0 and np.array_equal(y, x5), (name, grid, rank, "untransposed", int(np.count_nonzero(y != x5)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _exact(got, x, what):
    assert got.shape == x.shape and np.array_equal(got, x), (what, int(np.count_nonzero(got != x)), np.argwhere(got != x)[:4].tolist())


# ---- 1. transposed and conjugate-transposed solves ----

def _solves_child(name, grid):
    z = gx.is_z(name)
    reqs, want = [], []
    for nrhs in gx.NRHS:
        xT, bT = gx.rhs_t(name, nrhs, False)
        xC, bC = gx.rhs_t(name, nrhs, True)                       # double: the same system
        reqs += [("T", bT), ("C", bC)]
        want += [(nrhs, "T", xT), (nrhs, "C", xC)]
        assert np.array_equal(xT, xC) and np.array_equal(bT, bC) != z
    out = gx.solve_exact(name, grid, reqs)
    _proved(name, grid, out)
    for rank, (_, _, _, res) in enumerate(out):
        for (nrhs, trans, x), got in zip(want, res):
            _exact(got, x, (name, grid, rank, nrhs, trans))
        if not z:                                                  # "C" on a double handle: the same bits as "T"
            assert np.array_equal(res[0], res[1]) and np.array_equal(res[2], res[3])


@pytest.mark.parametrize("grid", gx.GRIDS, ids=_gid)
@pytest.mark.parametrize("name", gx.CASES)
def test_transposed_and_conjugate_transposed_solves_are_exact(name, grid):
    """every case on every grid, nrhs 1 (RK = 1 kernels) and 5 (RK = 4 with a remainder) in one set of handles: double cases under "T" and under "C" (the same
    bits), complex16 cases under "T" and "C" against their own right-hand sides (two different systems with one x)"""
    _child("_solves_child", name, grid)


# ---- 2. more right-hand sides than one chunk ----

def _chunks_child(name, grid, nrhs):
    c = gx.prepared(name)[0]
    trans = ("T", "C") if c.z else ("T",)
    sys_ = [gx.rhs_t(name, nrhs, t == "C") for t in trans]
    out = gx.solve_exact(name, grid, [(t, b) for t, (_, b) in zip(trans, sys_)])
    _proved(name, grid, out)
    for rank, (_, _, widest, res) in enumerate(out):
        assert widest == max(c.widths) and tc.max_rhs_chunk(widest, z=c.z) == nrhs - 1, (widest, nrhs)
        for t, (x, _), got in zip(trans, sys_, res):
            _exact(got, x, (name, grid, rank, nrhs, t))


@pytest.mark.parametrize("name,grid,nrhs", gx.CHUNK_RUNS, ids=["%s-%s-%d" % (n, _gid(g), r) for n, g, r in gx.CHUNK_RUNS])
def test_more_right_hand_sides_than_one_chunk(name, grid, nrhs):
    """one right-hand side more than max_rhs_chunk (asserted from the widest supernode of every rank's plan): the second chunk runs the whole exchange sequence
    again on accumulators the first chunk used"""
    _child("_chunks_child", name, grid, nrhs)


# ---- 3. no state carried between solves ----

def _sequence_child(name, grid):
    c = gx.prepared(name)[0]
    first = "C" if c.z else "T"
    x1, b1 = gx.rhs_t(name, 5, first == "C")
    x0, b0 = c.rhs(5)
    xa, ba = gx.rhs_t(name, 5, False)
    x2, b2 = xa[:, 3:4], ba[:, 3:4]                                # one right-hand side, not the first column of b1
    out = gx.solve_exact(name, grid, [(first, b1), ("N", b0), ("T", b2), (first, b1)])
    _proved(name, grid, out)
    for rank, (_, _, _, res) in enumerate(out):
        for what, x, got in zip(("first", "untransposed", "one rhs", "last"), (x1, x0, x2, x1), res):
            _exact(got, x, (name, grid, rank, what))
        assert np.array_equal(_bits(res[3]), _bits(res[0])), (name, grid, rank)


@pytest.mark.parametrize("grid", [(2, 2, 1), (2, 2, 2)], ids=_gid)
@pytest.mark.parametrize("name", ["widths", "z_narrow", "mixed_level"])
def test_no_state_is_carried_between_solves(name, grid):
    """T(b1), N(b0), T(b2), T(b1) on ONE set of handles (complex16: b1 under "C"), nrhs 5, 5, 1, 5: every solve returns its own integer x and the last is
    bitwise the first -- the accumulator rows the forward reduce packed and cleared and the backward sweep reused, across calls, sweeps of the other
    direction and another nrhs"""
    _child("_sequence_child", name, grid)


# ---- 4. leading dimension and padding ----

def _padded(b, pad_rows, tag):
    """column-major uint64 image of b with pad_rows rows of position-tagged NaN payloads under every column"""
    n, nrhs = b.shape
    vs = 2 if np.iscomplexobj(b) else 1
    buf = np.zeros(((n + pad_rows) * vs, nrhs), dtype=np.uint64, order="F")
    for q in range(nrhs):
        buf[:n * vs, q] = np.ascontiguousarray(b[:, q]).view(np.uint64)
    buf[n * vs:, :] = 0x7FF8000000000000 + 256 * tag + 1 + np.arange(pad_rows * vs, dtype=np.uint64)[:, None] + 16 * np.arange(nrhs, dtype=np.uint64)[None, :]
    return buf


def _unpadded(buf, n, z):
    vs = 2 if z else 1
    return np.stack([np.ascontiguousarray(buf[:n * vs, q]).view(np.complex128 if z else np.float64) for q in range(buf.shape[1])], axis=1)


def _ld_child(name, grid):
    c = gx.prepared(name)[0]
    n, vs = c.n, 2 if c.z else 1
    fn = _lib.entry("sluamd_pzgstrs3d_trans" if c.z else "sluamd_pdgstrs3d_trans")
    todo = [(nrhs, t) for nrhs in gx.NRHS for t in (("T", "C") if c.z else ("T",))]

    def request(nrhs, t):
        def run(h, rank):
            buf = _padded(gx.rhs_t(name, nrhs, t == "C")[1], 3, 1 + rank)
            pad = buf[n * vs:, :].copy()
            rc = fn(h._h, driver._trans_code(t), buf.ctypes.data_as(C.c_void_p), n + 3, nrhs)
            return rc, _unpadded(buf, n, c.z), bool(np.array_equal(buf[n * vs:, :], pad))
        return run

    out = gx.solve_exact(name, grid, [request(*a) for a in todo])
    _proved(name, grid, out)
    for rank, (_, _, _, res) in enumerate(out):
        for (nrhs, t), (rc, got, pad_ok) in zip(todo, res):
            assert rc == 0, (name, rank, nrhs, t, rc)
            _exact(got, gx.rhs_t(name, nrhs, t == "C")[0], (name, grid, rank, nrhs, t))
            assert pad_ok, (name, rank, nrhs, t, "padding rows changed")


@pytest.mark.parametrize("name", ["widths", "z_narrow"])
def test_leading_dimension_larger_than_n_on_a_grid(name):
    """ldx = n + 3 through sluamd_p[dz]gstrs3d_trans on 2 x 1 x 1: exact x on every rank and the padding rows -- NaNs whose payload tells rank, row and column --
    bitwise unchanged (complex16: the exchanges address the vector as doubles with leading dimension 2 ldx)"""
    _child("_ld_child", name, (2, 1, 1))


# ---- 5. device-pointer forms ----

def _dev_child(name, grid):
    import torch
    assert torch.cuda.is_available(), "torch sees no HIP device"
    c = gx.prepared(name)[0]
    n, vs = c.n, 2 if c.z else 1
    fn = _lib.entry("sluamd_pzgstrs3d_trans_dev" if c.z else "sluamd_pdgstrs3d_trans_dev")
    todo = [(nrhs, t) for nrhs in gx.NRHS for t in (("T", "C") if c.z else ("T",))]

    def request(nrhs, t):
        def run(h, rank):
            buf = _padded(gx.rhs_t(name, nrhs, t == "C")[1], 2, 1 + rank)
            d = torch.from_numpy(np.ascontiguousarray(buf.T).view(np.int64)).cuda()          # [nrhs, (n + 2) vs]: the column-major image
            torch.cuda.synchronize()
            rc = fn(h._h, driver._trans_code(t), C.c_void_p(d.data_ptr()), n + 2, nrhs)
            torch.cuda.synchronize()
            got = d.cpu().numpy().view(np.uint64).T
            return rc, _unpadded(got, n, c.z), bool(np.array_equal(got[n * vs:, :], buf[n * vs:, :]))
        return run

    out = gx.solve_exact(name, grid, [request(*a) for a in todo])
    _proved(name, grid, out)
    for rank, (_, _, _, res) in enumerate(out):
        for (nrhs, t), (rc, got, pad_ok) in zip(todo, res):
            assert rc == 0, (name, rank, nrhs, t, rc)
            _exact(got, gx.rhs_t(name, nrhs, t == "C")[0], (name, grid, rank, nrhs, t))
            assert pad_ok, (name, rank, nrhs, t, "padding rows changed")


@pytest.mark.parametrize("name", ["widths", "z_narrow"])
def test_device_pointer_forms_on_a_grid(name):
    """sluamd_pdgstrs3d_trans_dev / sluamd_pzgstrs3d_trans_dev on 1 x 2 x 1 with torch device tensors (the child imports torch before the library initialises
    the HIP runtime), ldx = n + 2: exact x on both ranks, the padding rows unchanged"""
    _child("_dev_child", name, (1, 2, 1), torch_first=True)


# ---- 6. transposed refinement with an exact trajectory ----

def _refine_names(kind):
    return [f"sw_{run}_{t}_{kind}" for t in (("t", "c") if gx.is_z(kind) else ("t",)) for run in ("nil", "rhs3")]


def _refine_child(kind, grid, path):
    with open(path, "rb") as f:
        todo = pickle.load(f)                                      # [(name, attached data, the simulator's run)]: nothing is simulated twice

    def request(d):
        def run(h, rank):
            h.attach_matrix(d["n"], d["rp"], d["ci"], d["av"], d["pc"])
            return h.pdgsrfs3d(d["B"].copy(order="F"), d["X0"].copy(order="F"), trans=d["trans"])
        return run

    out = gx.solve_exact(kind, grid, [request(d) for _, d, _ in todo])
    _proved(kind, grid, out)
    for rank, (_, _, _, res) in enumerate(out):
        for (name, _, r), (X, berr, steps) in zip(todo, res):
            print(name, _gid(grid), "rank", rank, "steps", steps, "expected", r["steps_all"], "berr", np.asarray(berr).tolist(), "expected", r["berr"].tolist())
            assert steps == r["steps"], (name, grid, rank, steps, r["steps_all"])
            assert np.array_equal(_bits(berr), _bits(r["berr"])), (name, grid, rank, np.asarray(berr).tolist(), r["berr"].tolist())
            bad = np.flatnonzero(_bits(X) != _bits(r["X"]))
            assert bad.size == 0, (name, grid, rank, "X differs at", bad[:8].tolist())


@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 1), (1, 1, 2)], ids=_gid)
@pytest.mark.parametrize("kind", ["narrow", "z_narrow"])
def test_transposed_refinement_follows_the_exact_trajectory_on_every_rank(kind, grid, tmp_path):
    """refine_trans_cases' runs through the real sweeps -- sw_nil_* (three steps to berr = 0) and sw_rhs3_* (three right-hand sides of 0, 2 and 1 steps), under
    "T" and, complex16, under "C" -- with GridHandle.pdgsrfs3d(trans=): every rank returns the simulator's X and berr bitwise and its step count.  The
    corrections are exact in any summation order (the simulator asserts the bounds of the transposed sweeps on every one), so the step count is not left open
    as it is for the floating-point system of test_gpu_grid_trans.py"""
    import refine_trans_cases as rt
    todo = []
    for name in _refine_names(kind):
        c, r = rt.cases()[name], rt.expected(name)
        assert c.kind == kind
        todo.append((name, dict(n=c.n, rp=c.rp, ci=c.ci, av=c.av, pc=c.pc, B=c.B, X0=c.X0, trans=c.trans),
                     dict(steps=r["steps"], steps_all=r["steps_all"], berr=r["berr"], X=r["X"])))
    assert [t[2]["steps_all"] for t in todo[:2]] == [[3], [0, 2, 1]]
    path = str(tmp_path / "runs.pkl")
    with open(path, "wb") as f:
        pickle.dump(todo, f)
    _child("_refine_child", kind, grid, path)


# ---- 7. expert solve ----

def _expert_child(name, grid, trans):
    c = gx.prepared(name)[0]
    n, rp, ci, vB = gx.csr(name)
    rows = np.repeat(np.arange(n), np.diff(rp))
    rng = np.random.default_rng(11)
    Dr, Dc = 2.0 ** rng.choice([-100, 100], n), 2.0 ** rng.choice([-100, 100], n)
    v = (vB * Dr[rows]) * Dc[ci]
    x_int, b_t = gx.rhs_t(name, 2, trans == "C")
    b = np.asfortranarray(Dc[:, None] * b_t)
    xtrue = x_int / Dr[:, None]
    x, info, st = driver.pdgssvx3d(n, rp, ci, v, b, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, equil=True, trans=trans, grid=grid)
    assert info == 0 and st["equed"] == "B", (info, st["equed"])
    bound = 8 * n * EPS * (np.abs(np.linalg.inv(c.B)).T @ (np.abs(c.U0).T @ (np.abs(c.L0).T @ np.abs(x_int)))) / Dr[:, None]
    ratio = float((np.abs(x - xtrue) / bound).max())
    print(name, _gid(grid), trans, "max error / bound", ratio, "max relative error", float((np.abs(x - xtrue) / np.abs(xtrue)).max()))
    assert np.all(np.isfinite(x)) and ratio <= 1.0, ratio


def test_expert_solve_under_power_of_two_scalings_on_a_grid():
    """driver.pdgssvx3d(grid=(2, 2, 1), equil=True, trans="T") on A = Dr B Dc, B = L0 U0 of "narrow", Dr and Dc powers of two (2^+-100): the construction and
    the bar of test_gpu_equil.py::test_exact_transposed_cases_under_power_of_two_scalings.  NOT bitwise: R and C are reciprocals of maxima, so the scaled
    values round; what holds is the componentwise forward bound of an LU solve, invariant under diagonal scalings,
        |x^ - x| <= 8 n 2^-53 (1 / Dr) o (|B^-T| |U0|^T |L0|^T |x_int|)
    (derived there).  R and C swapped around the transposed grid solve, or one of them left out, moves x by factors of 2^100; the bound allows < 2^20."""
    _child("_expert_child", "narrow", (2, 2, 1), "T")
