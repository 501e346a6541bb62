"""Blocks of 16 right-hand sides in the triangular sweeps: the fp64 MFMA form (rk = 16) of the forward-update, backward-update and diagonal-strip units,
chosen by the launch wrappers when nrhs >= SLUAMD_SWEEP_MFMA_MIN (default 16).  The exact cases of tests/sweep_cases.py (every partial sum of any order is
an exact double) are compared with numpy.array_equal; the SLUAMD_SOLVE_DEBUG lines of the launch wrappers prove which form ran; a real-arithmetic pair
compares a block solve with sixteen single solves."""
import functools, json, os, subprocess, sys
import numpy as np
import pytest
import sweep_cases as sw
import test_gpu_sweep_shapes as shapes
from superlu_dist_amd import _lib, driver, grid3d, matgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = "emul" in os.path.basename(os.environ.get("SLUAMD_LIB", ""))
MFMA_MIN = 16                                            # the default of SLUAMD_SWEEP_MFMA_MIN
CASES = ("widths", "levels", "wide_launch", "groups")
NRHS = (8, 15, 16, 17, 31, 32, 33, 48, 49, 97)           # whole blocks, 1 / 15 / 2 surplus columns, the 48-column chunk of the 256-column cases and one past it
SMALL = (1, 2, 3, 4, 7)                                  # below the threshold: rk = 1 and rk = 4
CONFIGS = {"default": {},
           "wide0": {"SLUAMD_SWEEP_WIDE_V": "0", "SLUAMD_SWEEP_WIDE_MIN": "1"},
           "wide1": {"SLUAMD_SWEEP_WIDE_V": "1", "SLUAMD_SWEEP_WIDE_MIN": "1"},
           "off": {"SLUAMD_SWEEP_MFMA_MIN": "0"},
           "min2": {"SLUAMD_SWEEP_MFMA_MIN": "2"}}      # the form from two right-hand sides on: lone partial blocks (2 .. 15) and the joined links' `chk` rules (nrhs < 4)
THRESHOLD = {"default": MFMA_MIN, "wide0": MFMA_MIN, "wide1": MFMA_MIN, "off": None, "min2": 2}

CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_sweep_shapes as t
out = {}
for name in sys.argv[2].split(","):
    h = t._factored(name)
    c = t._prepared(name)[0]
    for nrhs in [int(a) for a in sys.argv[3].split(",")]:
        x, b = c.rhs(nrhs)
        sys.stderr.write("[case] %s %d\n" % (name, nrhs)); sys.stderr.flush()
        got = h.pdgstrs3d(b.copy(order="F"))
        out["%s:%d" % (name, nrhs)] = bool(t.np.array_equal(got, x))
    h.destroy()
print("RESULT " + json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def _child(cfg):
    """one child process per setting (the switches are read when the library is loaded); run once, never retried: a child that met its time limit is a
    cached failure too (lru_cache keeps no exceptions)"""
    env = dict(os.environ, SLUAMD_SOLVE_DEBUG="1", **CONFIGS[cfg])
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, ",".join(CASES), ",".join(str(a) for a in SMALL + NRHS)], env=env, capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        txt = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")
        return -1, txt(e.stdout), txt(e.stderr) + "\n[child %s met its time limit of 600 s]" % cfg
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_blocks_of_sixteen_are_exact(cfg):
    """`widths`, `levels`, `wide_launch` and `groups` (default schedule) with 8 .. 97 right-hand sides return the integer x in every column: at the
    defaults, under the 1024- and 512-thread builds on every wide launch (SLUAMD_SWEEP_WIDE_V = 0 / 1 with SLUAMD_SWEEP_WIDE_MIN=1), with the form off, and with
    the form from two right-hand sides on (SLUAMD_SWEEP_MFMA_MIN=2: 2 .. 15 right-hand sides as ONE partial block, and the units next to joined links)"""
    rc, out, err = _child(cfg)
    assert rc == 0, out[-1500:] + err[-1500:]
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == len(CASES) * len(SMALL + NRHS) and all(res.values()), sorted(k for k, ok in res.items() if not ok)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_form_that_ran(cfg):
    """every fwd_update / bwd_update / sweep_step line of the children carries rk=16 from SLUAMD_SWEEP_MFMA_MIN right-hand sides on (narrow and wide launches
    alike), rk=4 for two or more below it, rk=1 for one; with SLUAMD_SWEEP_MFMA_MIN=0 no line carries rk=16, with SLUAMD_SWEEP_MFMA_MIN=2 every line from two
    right-hand sides on does.  Every case meets every family in the MFMA form."""
    if EMUL:
        pytest.skip("the emulation engine has no builds")
    rc, out, err = _child(cfg)
    assert rc == 0, out[-1500:] + err[-1500:]
    case, seen = None, {}
    for ln in err.splitlines():
        if ln.startswith("[case] "):
            case = ln.split()[1]
        elif ln.startswith("[sluamd sweep] "):
            f = dict(tok.split("=") for tok in ln.split()[2:])
            if f["family"] not in ("fwd_update", "bwd_update", "sweep_step"):
                continue
            nrhs, rk = int(f["nrhs"]), int(f["rk"])
            th = THRESHOLD[cfg]
            assert rk == (16 if th and nrhs >= th else 4 if nrhs >= 2 else 1), ln
            seen.setdefault((case, f["family"]), set()).add((rk, int(f["mx"]) <= 64))
    for case in CASES:
        for fam in ("fwd_update", "bwd_update", "sweep_step"):
            assert any(rk == 16 for rk, _ in seen.get((case, fam), set())) == (cfg != "off"), (case, fam, seen)
    if cfg != "off":
        assert (16, True) in seen[("levels", "sweep_step")] and (16, False) in seen[("levels", "sweep_step")]      # narrow and wide launches


def test_leading_dimension_larger_than_n():
    """ldx = n + 3 through the C ABI on `widths`: the solution rows are exact and the padding rows (NaNs whose payload tells the position) come back
    bitwise unchanged"""
    c = shapes._prepared("widths")[0]
    h = shapes._factored("widths")
    n = c.n
    L = _lib.load()
    for nrhs in NRHS:
        x, b = c.rhs(nrhs)
        buf = np.zeros((n + 3, nrhs), dtype=np.uint64, order="F")
        for q in range(nrhs):
            buf[:n, q] = np.ascontiguousarray(b[:, q]).view(np.uint64)
        pad = 0x7FF8000000000000 + 1 + np.arange(3, dtype=np.uint64)[:, None] + 16 * np.arange(nrhs, dtype=np.uint64)[None, :]
        buf[n:, :] = pad
        _lib.check(L.sluamd_pdgstrs3d(h._h, buf.ctypes.data_as(_lib.P_dbl), n + 3, nrhs), "sluamd_pdgstrs3d")
        got = np.stack([np.ascontiguousarray(buf[:n, q]).view(np.float64) for q in range(nrhs)], axis=1)
        assert np.array_equal(got, x), nrhs
        assert np.array_equal(buf[n:, :], pad), nrhs
    h.destroy()


@pytest.mark.parametrize("name", ["widths", "levels"])
def test_launch_counts_are_unchanged(name):
    """the MFMA form is another build of the same units: stats()["solve_launches"] is what the restated schedule predicts at 16 and 48 right-hand sides"""
    sizes = sw.level_sizes(shapes._prepared(name)[5])
    h = shapes._factored(name)
    for nrhs in (16, 48):
        shapes._solve_exact(name, h, (nrhs,))
        assert h.stats()["solve_launches"] == sw.predicted_launches(sizes, nrhs), (name, nrhs)
    h.destroy()


@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 2, 1), (1, 1, 2), (2, 2, 2)])
@pytest.mark.parametrize("name", ["widths", "z_narrow"])
def test_process_grids_return_the_exact_solution(name, grid):
    """the grid sweeps (k_fwd_update / k_bwd_update through find_node_wave) on Pr x Pc x Pz thread grids with 16 and 20 right-hand sides: the integer x
    back from every rank (the complex16 twins are unchanged and ride along)"""
    c = shapes._prepared(name)[0]
    n, rp, ci = c.pattern_csr()
    rows = np.repeat(np.arange(n), np.diff(rp))
    v = c.B[rows, ci].copy()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    Pr, Pc, Pz = grid
    tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)
    rhs = [c.rhs(16), c.rhs(20)]

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
    """sluamd_pdgstrs3d_dist on one rank (identity permutations) with 16 right-hand sides"""
    c = shapes._prepared("widths")[0]
    h = shapes._factored("widths")
    x, b = c.rhs(16)
    got = h.pdgstrs3d_dist(b.copy(order="F"))
    assert np.array_equal(got, x)
    h.destroy()


def _poisson20():
    N = 20
    n, rp, ci, v = matgen.poisson3d(N)
    return n, rp, ci, v, matgen.nd_perm_grid3d(N, N, N, leaf=27), 16, 256


def _unsym700():
    n, rp, ci, v = matgen.random_unsym(700, 0.01, seed=8)
    return n, rp, ci, v, None, 8, 48


@pytest.mark.parametrize("problem", [_poisson20, _unsym700], ids=["poisson20", "unsym700"])
def test_block_of_sixteen_against_sixteen_single_solves(problem):
    """real arithmetic: one solve of 16 right-hand sides against sixteen solves of one on the same handle.  Both meet the residual bound of
    test_gpu_edge_cases.py (1e-10 relative to |b|), and the largest difference between the two solutions stays below the same 1e-10 (absolute; the
    entries of x are standard normal).  The difference is part of the assertion message."""
    n, rp, ci, v, perm, relax, maxsup = problem()
    rng = np.random.default_rng(1)
    xt = rng.standard_normal((n, 16))
    b = np.asfortranarray(matgen.csr_matvec(n, rp, ci, v, xt))
    x16, info, _, h, symb = driver.pdgssvx3d(n, rp, ci, v, b, perm, relax=relax, maxsup=maxsup, keep=True)
    assert info == 0
    xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b
    y16 = np.zeros_like(b, order="F"); y16[symb.perm_c, :] = x16                          # the driver's solve, in the order of the factored system
    y1 = np.column_stack([h.pdgstrs3d(np.asfortranarray(xp[:, q:q + 1].copy()))[:, 0] for q in range(16)])
    h.destroy()
    pc = symb.perm_c.copy()
    symb.free()
    diff = float(np.abs(y16 - y1).max())
    for tag, y in (("nrhs=16", y16), ("16 x nrhs=1", y1)):
        x = y[pc, :]
        res = float(np.linalg.norm(b - matgen.csr_matvec(n, rp, ci, v, x)) / np.linalg.norm(b))
        print(f"{problem.__name__} {tag}: residual {res:.3e}")
        assert res <= 1e-10, (tag, res)
    print(f"{problem.__name__}: max |x(nrhs=16) - x(16 x nrhs=1)| = {diff:.3e}")
    assert diff <= 1e-10, f"largest difference between the block solve and the single solves: {diff:.3e}"
