"""The small factorisations whose issue order tests/golden/factor_trace.json pins (test_factor_trace_cpu.py) and whose launch counters the
device build must reproduce (test_gpu_factor_counts.py): one table of configurations, one runner."""
import contextlib
import ctypes
import os
import numpy as np
from superlu_dist_amd import _lib, driver, grid3d, matgen

# name -> what differs from the base case.  The base is the deep DAG of test_stream_order.py: poisson3d(10), perturbed values,
# nd_perm_grid3d(leaf=8), relax=4, maxsup=16 on one rank in double.
#   env: switches read at handle creation; N / leaf / relax / maxsup: the matrix, its ordering and the supernode limits; z: complex16 values; grid: (Pr, Pc, Pz) over the
#   stream-ordered in-process transport; second: the traced factorisation is the handle's second one (tile records already built)
CASES = {
    "lookahead": {},
    "deterministic": {"deterministic": True},
    "no_lookahead": {"env": {"SLUAMD_NO_LOOKAHEAD": "1"}},
    "profiled": {"profile": True},
    "trsm_panels": {"env": {"SLUAMD_TRSM_PANELS": "1"}},
    "trsm_tail_0": {"env": {"SLUAMD_TRSM_TAIL": "0"}},
    "diag_tail_0": {"env": {"SLUAMD_DIAG_TAIL": "0"}},
    "panel_split_0": {"env": {"SLUAMD_PANEL_SPLIT": "0"}},
    "no_tile_maps": {"env": {"SLUAMD_NO_TILE_MAPS": "1"}},
    "no_fuse": {"env": {"SLUAMD_NO_FUSE": "1"}},
    "ksplit_1": {"env": {"SLUAMD_KSPLIT": "1"}},
    "solve_groups_1": {"env": {"SLUAMD_SOLVE_GROUPS": "1"}},
    "second_factorisation": {"second": True},
    "wide": {"N": 14, "maxsup": 200},
    "wide_no_lookahead": {"N": 14, "maxsup": 200, "env": {"SLUAMD_NO_LOOKAHEAD": "1"}},
    "wide_balanced": {"N": 14, "maxsup": 200, "env": {"SLUAMD_BALANCE_MIN_TILES": "1"}},
    "wide_balanced_no_lookahead": {"N": 14, "maxsup": 200, "env": {"SLUAMD_BALANCE_MIN_TILES": "1", "SLUAMD_NO_LOOKAHEAD": "1"}},
    "big_tiles": {"N": 14, "maxsup": 200, "env": {"SLUAMD_BIG_UTIL_PCT": "1"}},
    "big_tiles_no_lookahead": {"N": 14, "maxsup": 200, "env": {"SLUAMD_NO_LOOKAHEAD": "1", "SLUAMD_BIG_UTIL_PCT": "1"}},
    "big_tiles_z": {"N": 14, "maxsup": 200, "z": True, "env": {"SLUAMD_BIG_UTIL_PCT": "1"}},
    "groups": {"N": 12, "leaf": 27, "relax": 16, "maxsup": 64, "env": {"SLUAMD_SOLVE_GROUPS": "1"}},
    "groups_no_lookahead": {"N": 12, "leaf": 27, "relax": 16, "maxsup": 64, "env": {"SLUAMD_SOLVE_GROUPS": "1", "SLUAMD_NO_LOOKAHEAD": "1"}},
    "complex16": {"z": True},
    "grid_1x1x2": {"grid": (1, 1, 2)},
    "grid_2x1x1": {"grid": (2, 1, 1)},
    "grid_1x2x1": {"grid": (1, 2, 1)},
    "grid_1x2x1_complex16": {"grid": (1, 2, 1), "z": True},
}
SINGLE_RANK = [name for name, c in CASES.items() if "grid" not in c]
COUNTERS = ("num_launches", "schur_launches", "schur_tiles")
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_trace.json")


@contextlib.contextmanager
def _environment(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def matrix(case):
    """(n, rowptr, colind, values, perm, b) of a case"""
    N = case.get("N", 10)
    n, rp, ci, v = matgen.poisson3d(N)
    v = v * (1.0 + 0.2 * np.random.default_rng(5).random(v.size))
    if case.get("z"):
        v = matgen.complex_shift(v, rp, ci, seed=9)
    perm = matgen.nd_perm_grid3d(N, N, N, leaf=case.get("leaf", 8))
    xt = np.where(np.arange(n) % 2 == 1, 1.0, -1.0)[:, None] * np.ones((1, 2))
    return n, rp, ci, v, perm, matgen.csr_matvec(n, rp, ci, v, xt.astype(v.dtype))


def run(name, trace=False):
    """Factor and solve a case.  Per rank: {"stats": the counters after the traced factorisation, "x": the solution in the original order,
    "trace": the issue-order trace of that factorisation (emulation library only, trace=True)}; and the residual ||b - A x|| / ||b||."""
    case = CASES[name]
    n, rp, ci, v, perm, b = matrix(case)
    Pr, Pc, Pz = grid = case.get("grid", (1, 1, 1))
    L = _lib.load()
    if trace:
        L.sluamd_emul_trace.argtypes = [ctypes.c_int]
        L.sluamd_emul_trace_dump.restype = ctypes.c_char_p
    with _environment(case.get("env", {})):
        symb = driver.Symbolic(n, rp, ci, perm, relax=case.get("relax", 4), maxsup=case.get("maxsup", 16))
        sn_tree = symb.partition(Pz) if Pz > 1 else None
        comms = grid_comms(*grid) if "grid" in case else None
        xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b

        def rank_body(rank):
            opts = {"deterministic": bool(case.get("deterministic"))}
            h = (grid3d.GridHandle.from_symbolic(symb, v, comms[rank], sn_tree, **opts) if comms else driver.LUHandle.from_symbolic(symb, v, **opts))
            if case.get("profile"):
                h.set_profile(True)
            if case.get("second"):
                assert h.pdgstrf3d(0.0) == 0
                h.reset_values()
            if trace: L.sluamd_emul_trace(1)       # the ranks of a thread grid each switch on and read their own thread's trace
            info = h.pdgstrf3d(0.0)
            if trace: L.sluamd_emul_trace(0)
            out = {"stats": {k: int(h.stats()[k]) for k in COUNTERS}}
            if trace:
                out["trace"] = L.sluamd_emul_trace_dump().decode()
            assert info == 0
            out["x"] = h.pdgstrs3d(xp)[symb.perm_c, :]
            h.destroy()
            return out

        ranks = grid3d.run_ranks(Pr * Pc * Pz, rank_body) if comms else [rank_body(0)]
        symb.free()
    res = max(np.linalg.norm(b - matgen.csr_matvec(n, rp, ci, v, r["x"])) / np.linalg.norm(b) for r in ranks)
    return ranks, res


def grid_comms(Pr, Pc, Pz):
    import grid_cases
    return grid_cases.stream_ordered_comms(Pr, Pc, Pz)
