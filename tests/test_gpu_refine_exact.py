"""The refinement kernels (k_rfs_residual / k_rfs_update of both precisions) and the driver loop of sluamd_refine.h against trajectories
known EXACTLY: tests/refine_exact_cases.py attaches a matrix that is not the factored one to handles holding exact factors and predicts berr of every pass,
every stop decision, the step count and the final X in integers (bitwise equal to the oracle's restatement: test_refine_exact_cases_cpu.py).  Every
comparison of values in this file is numpy.array_equal on bit patterns: X, berr and the padding rows; the step counts are compared as integers."""
import json, os, subprocess, sys
import numpy as np
import pytest
import refine_exact_cases as rx
import trans_cases as tc
from superlu_dist_amd import driver, grid3d

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = "emul" in os.path.basename(os.environ.get("SLUAMD_LIB", ""))
CASES = rx.cases()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _no_z(c):
    if EMUL and c.z:
        pytest.skip("the emulation library has no complex16 refinement (its engine restates k_rfs_residual / k_rfs_update only)")


def _copy(fs):
    return driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind.copy(), fs.Lnzval_off, fs.Lnzval.copy(), fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off,
                            fs.Unzval.copy())


def _factored(kind, n, z, **kw):
    """a handle holding the exact factors of a case kind (asserted)"""
    fs0, expL, expU = rx.diag_store(n, z) if kind == "diag" else tc.prepared(kind)[1:4]
    fs = _copy(fs0)
    h = driver.LUHandle.from_store(fs, **kw)
    assert h.z == z and h.pdgstrf3d(0.0) == 0
    h.copy_to_host()
    assert np.array_equal(fs.Lnzval, expL) and np.array_equal(fs.Unzval, expU), kind
    return h


def _check(name, got, what=""):
    X, berr, steps = got
    r = rx.expected(name)
    print(name, what, "steps", steps, "expected", r["steps_all"], "berr", np.asarray(berr).tolist(), "expected", r["berr"].tolist())
    assert steps == r["steps"], (name, what, steps, r["steps_all"])
    assert np.array_equal(_bits(berr), _bits(r["berr"])), (name, what, np.asarray(berr).tolist(), r["berr"].tolist())
    bad = np.flatnonzero(_bits(X) != _bits(r["X"]))
    assert bad.size == 0, (name, what, "X differs at", bad[:8].tolist())


def _run(h, c):
    h.attach_matrix(c.n, c.rp, c.ci, c.av, c.pc)
    return h.pdgsrfs3d(c.B.copy(order="F"), c.X0.copy(order="F"))


def _groups():
    """the cases by handle: (kind, n, z) -> names"""
    g = {}
    for k, c in CASES.items():
        g.setdefault((c.kind, c.n, c.z), []).append(k)
    return g


@pytest.mark.parametrize("key", list(_groups()), ids=lambda k: "%s-n%d-%s" % (k[0], k[1], "z" if k[2] else "d"))
def test_host_form_follows_the_exact_trajectory(key):
    """pdgsrfs3d / pzgsrfs3d on host arrays, every case: X, berr and the step count of the simulator, bitwise.  The cases of one factored system share its handle,
    so every case but the first also runs behind another matrix's work vectors and maximum."""
    kind, n, z = key
    _no_z(CASES[_groups()[key][0]])
    h = _factored(kind, n, z)
    for name in _groups()[key]:
        c = CASES[name]
        B0, X0 = c.B.copy(), c.X0.copy()
        _check(name, _run(h, c))
        assert np.array_equal(_bits(c.B), _bits(B0)) and np.array_equal(_bits(c.X0), _bits(X0))
    h.destroy()


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_reattaching_carries_nothing_over(z):
    """two matrices in turn on one handle, twice: the trajectory is the attached matrix's, and the second run of each is bitwise its first"""
    p = "z_" if z else "d_"
    _no_z(CASES[p + "half_long"])
    h = _factored("diag", 65, z)
    for name in (p + "half_long", p + "rhs3", p + "half_long", p + "nilpotent", p + "rhs3", p + "safe1_stop_n65", p + "half_stop"):
        _check(name, _run(h, CASES[name]), "re-attached")
    h.destroy()
    kind = "z_narrow" if z else "narrow"
    h = _factored(kind, CASES[f"sw_nil_{kind}"].n, z)
    for name in (f"sw_rhs3_{kind}", f"sw_nil_{kind}", f"sw_rhs3_{kind}"):
        _check(name, _run(h, CASES[name]), "re-attached")
    h.destroy()


@pytest.mark.parametrize("name", ["d_max_n513_r255", "z_max_n513_r512", "sw_rhs3_narrow", "sw_nil_z_wide", "d_half_long"])
def test_a_deterministic_handle_follows_the_same_trajectory(name):
    c = CASES[name]
    _no_z(c)
    h = _factored(c.kind, c.n, c.z, deterministic=True)
    _check(name, _run(h, c), "deterministic")
    h.destroy()


def _dev_child(expected):
    """every case through the _dev forms on device memory, ldb = n + 3 and ldx = n + 5, the padding rows holding position-tagged NaN payloads.  On the emulation library device
    memory is host memory: numpy buffers take the place of the torch tensors"""
    rx.preload_expected(expected)                                                           # the parent's trajectories: nothing is simulated twice
    emul = EMUL
    if not emul:
        import torch
        assert torch.cuda.is_available(), "torch sees no HIP device"
    out = {}
    handles = {}
    for name in CASES:
        c = CASES[name]
        if emul and c.z:
            continue
        key = (c.kind, c.n, c.z)
        if key not in handles:
            handles[key] = _factored(*key)
        h = handles[key]
        h.attach_matrix(c.n, c.rp, c.ci, c.av, c.pc)
        n, vs, nrhs = c.n, 2 if c.z else 1, c.nrhs
        bufs = []
        for a, pad_rows, tag in ((c.B, 3, 1), (c.X0, 5, 2)):
            buf = np.zeros(((n + pad_rows) * vs, nrhs), dtype=np.uint64, order="F")
            for q in range(nrhs):
                buf[:n * vs, q] = np.ascontiguousarray(a[:, q]).view(np.uint64)
            pad = 0x7FF8000000000000 + 256 * tag + 1 + np.arange(pad_rows * vs, dtype=np.uint64)[:, None] + 16 * np.arange(nrhs, dtype=np.uint64)[None, :]
            buf[n * vs:, :] = pad
            bufs.append(buf)
        if emul:
            dB, dX = (np.ascontiguousarray(b.T) for b in bufs)
            berr, steps = h.pdgsrfs3d_dev(dB.ctypes.data, n + 3, dX.ctypes.data, n + 5, nrhs)
            gB, gX = dB.T, dX.T
        else:
            dB, dX = (torch.from_numpy(np.ascontiguousarray(b.T).view(np.int64)).cuda() for b in bufs)
            torch.cuda.synchronize()
            berr, steps = h.pdgsrfs3d_dev(dB.data_ptr(), n + 3, dX.data_ptr(), n + 5, nrhs)
            torch.cuda.synchronize()
            gB, gX = (t.cpu().numpy().view(np.uint64).T for t in (dB, dX))
        r = rx.expected(name)
        out[name] = dict(steps=[int(steps), int(r["steps"])], berr=bool(np.array_equal(_bits(berr), _bits(r["berr"]))),
                         X=bool(np.array_equal(gX[:n * vs, :], np.stack([_bits(r["X"][:, q]) for q in range(nrhs)], axis=1))),
                         padX=bool(np.array_equal(gX[n * vs:, :], bufs[1][n * vs:, :])), B=bool(np.array_equal(gB, bufs[0])), berr_got=np.asarray(berr).tolist())
    for h in handles.values():
        h.destroy()
    print("RESULT " + json.dumps(out))


def test_dev_forms_with_padded_leading_dimensions(tmp_path):
    """every case through sluamd_pdgsrfs3d_dev / sluamd_pzgsrfs3d_dev from a child process that imports torch first (torch.cuda reports no device once the library has
    initialised the HIP runtime in the process): X, berr, steps bitwise; the padding rows of X and the whole of B come back bitwise unchanged"""
    code = ("import os, sys\n" + ("" if EMUL else "import torch\n") + "sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\n"
            "import test_gpu_refine_exact as t\nt._dev_child(sys.argv[2])\n")
    want = [k for k in CASES if not (EMUL and CASES[k].z)]
    rx.dump_expected(str(tmp_path / "expected.pkl"), want)
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(tmp_path / "expected.pkl")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert sorted(res) == sorted(want) and len(want) == (len(CASES) if not EMUL else sum(1 for c in CASES.values() if not c.z))
    for k, v in res.items():
        assert v["steps"][0] == v["steps"][1] and v["berr"] and v["X"] and v["padX"] and v["B"], (k, v)


def _grid_child(kind, Pr, Pc, Pz, expected):
    rx.preload_expected(expected)
    s = tc.prepared(kind)[0]
    n, rp, ci = s.pattern_csr()
    v = s.B[np.repeat(np.arange(n), np.diff(rp)), ci].copy()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=s.maxsup, unsym=True)
    tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)
    todo = [f"sw_nil_{kind}", f"sw_rhs3_{kind}"]
    x5, b5 = s.rhs(5)

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], tree)
        try:
            info = h.pdgstrf3d(0.0)
            y = h.pdgstrs3d(b5.copy(order="F"))
            res = []
            for name in todo:
                c = CASES[name]
                h.attach_matrix(c.n, c.rp, c.ci, c.av, c.pc)
                res.append(h.pdgsrfs3d(c.B.copy(order="F"), c.X0.copy(order="F")))
        finally:
            h.destroy()
        return info, y, res

    out = grid3d.run_ranks(Pr * Pc * Pz, body)
    symb.free()
    for rank, (info, y, res) in enumerate(out):
        assert info == 0 and np.array_equal(y, x5), rank                                    # the factors are the exact ones
        for name, got in zip(todo, res):
            _check(name, got, "rank %d of %s" % (rank, (Pr, Pc, Pz)))
    print("RESULT ok %d" % len(out))


@pytest.mark.parametrize("grid", [(1, 1, 2), (2, 1, 1)], ids=["1x1x2", "2x1x1"])
@pytest.mark.parametrize("kind", ["narrow", "z_narrow"])
def test_grid_handles_follow_the_exact_trajectory_on_every_rank(kind, grid, tmp_path):
    """replicated form on thread grids (grid3d.local_comms / run_ranks) in a child process under a time limit, so that ranks that split into unmatched
    collective solves end the test instead of hanging it: handles from the integer values of the sweep case; a continuing case and the three right-hand
    sides; every rank returns the simulator's X, berr and steps"""
    _no_z(CASES[f"sw_nil_{kind}"])
    code = ("import os, sys\nsys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\nimport test_gpu_refine_exact as t\n"
            "t._grid_child(%r, %d, %d, %d, sys.argv[2])\n" % ((kind,) + grid))
    rx.dump_expected(str(tmp_path / "expected.pkl"), [f"sw_nil_{kind}", f"sw_rhs3_{kind}"])
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(tmp_path / "expected.pkl")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "RESULT ok 2" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
