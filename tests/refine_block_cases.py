"""Multi-column refinement runs whose whole trajectory is known EXACTLY, for the blocked refinement sluamd_p[dz]gsrfs3d_block (test helper for
test_gpu_refine_block.py and test_refine_block_cases_cpu.py; not a conftest).  Builds on refine_exact_cases (rx) and refine_trans_cases (rt) by import: the
`_Diag` builder, the sweep kinds, and their simulators, which predict per COLUMN the berr of every pass, the step count (`steps_all`) and the final X in
integers and assert their own bounds.  The blocked form promises that every column runs exactly as it does alone, so the per-column simulators are its
reference unchanged.

Kind "diag" (F = diag(d), rx.diag_store).  ONE matrix A' per case; what a column does is decided by its b and x0 alone (`_mix`):
  zero    every row has r = 0: berr = 0, 0 steps
  safe1   the empty row holds b = safmin: berr = n + 2 from the SAFE1 branch, 0 steps (the stop at pass 0 of rx's safe1_stop), X untouched
  one     a row over a frozen column keeps a constant residual: the second pass does not halve, 1 step
  two     the same beside one wrong x0 that the first step repairs: 2 steps (rx's rhs3 column 1)
  long    rx's half_long: the error halves exactly at every step, ITMAX = 20 steps
  eps     rx's eps_stop: berr == eps exactly, 0 steps (rows 0, 3, 5 are `tight`, as there)
Order 1 knows "zero" and "one" only (the one row stalls or is exact).

The cases (both precisions; "N" for all, "T" and for complex16 "C" for those in TRANS_PATTERNS, attached as the transpose exactly as rt._from_rx does, so
that the same trajectory is predicted):
  cols_<k>       k = 1, 2, 3, 4, 5, 15, 16, 17, 33 columns of the rhs3 pattern (0, 2, 1 steps) repeated: one register group of the residual kernel, a group
                 boundary, an rk = 4 sweep block with a remainder, a full MFMA block, a panel boundary, three panels; n = 65
  ord_<n>        n in rx.ORDERS, 17 columns of that pattern (n = 1: 0, 1 steps alternating)
  first0_16      the first column stops at pass 0 (SAFE1), the others take 2 or 1 steps
  last_first_16  the last column stops first
  mid_first_17   a middle column stops first
  all_once_16    all columns stop at once (one step each)
  long_16        one `long` column beside 0-, 1- and 2-step columns: the panel shrinks 16 -> 10 -> 4 -> 1 and the last column goes on alone to 20
  eps_17         an `eps` column sits exactly on the boundary, in the first panel beside running columns
Through the real sweeps (sw_<kind>_<trans>_<k>): the design of rx._sweep_cases / rt._sweep_cases, A' = A M with M = I - e_m e_m^T, k columns of the kinds
zero / two / one; "narrow" and "z_narrow" with 17 columns under N, T (and C), "levels" and "z_wide" with 5 columns under N."""
import functools
import numpy as np
import scipy.sparse as sp
import refine_exact_cases as rx
import refine_trans_cases as rt
import trans_cases as tc

PANEL = 16
COLS = (1, 2, 3, 4, 5, 15, 16, 17, 33)
STEPS = dict(zero=0, safe1=0, one=1, two=2, long=rx.ITMAX, eps=0)
TRANS_PATTERNS = ("cols_5", "cols_17", "ord_1", "ord_64", "ord_257", "first0_16", "long_16", "eps_17")
# rows of _mix (orders >= 63)
R_P0, R_E, R_P3, R_T, R_F7, R_K, R_K2, R_A, R_M2, R_F = 0, 2, 3, 5, 7, 10, 30, 33, 45, 52


def _cycle(k, kinds=("safe1", "two", "one")):
    return [kinds[j % len(kinds)] for j in range(k)]


def patterns():
    """name -> (order, column kinds)"""
    p = {}
    for k in COLS:
        p[f"cols_{k}"] = (65, _cycle(k))
    for n in rx.ORDERS:
        p[f"ord_{n}"] = (n, _cycle(17, ("zero", "one")) if n == 1 else _cycle(17))
    p["first0_16"] = (65, ["safe1"] + _cycle(15, ("two", "one")))
    p["last_first_16"] = (65, _cycle(15, ("two", "one")) + ["zero"])
    p["mid_first_17"] = (65, _cycle(8, ("one", "two")) + ["safe1"] + _cycle(8, ("two", "one")))
    p["all_once_16"] = (65, ["one"] * 16)
    p["long_16"] = (65, ["zero", "one", "two", "safe1", "one"] * 3 + ["long"])
    p["eps_17"] = (65, _cycle(9, ("two", "one")) + ["eps"] + _cycle(7))
    return p


def _mix(name, n, z, kinds):
    """the kind-"diag" rx.RCase of order n whose column j is of kind kinds[j]"""
    g = 1j if z else 1.0
    D = rx._Diag(n, z, nrhs=len(kinds))
    if n == 1:
        x0 = D.zz(2 ** 20, 0)
        D.stall(0, x0, 0)
        for j, k in enumerate(kinds):
            assert k in ("zero", "one")
            D.B[0, j] = D.dp[0] * (2 * x0 + (D.zz(1, 0) if k == "one" else 0))
        return D.case(name)
    assert n >= 63
    D.rows[R_E] = []; D.X[R_E, :] = 0; D.B[R_E, :] = 0
    D.frozen(R_F7, D.zz(8, R_F7))
    D.off(R_F, [(R_F7, 3.0)], 0)
    c, e = D.zz(2.0 ** 21, 16), 2.0 ** 20
    D.half(R_K, c, 0); D.half(R_K2, c, 0)
    D.rows[R_M2] = [(R_K, g), (R_K2, -g)]; D.X[R_M2, :] = 0; D.B[R_M2, :] = 0
    if "eps" in kinds:
        D.rows[R_T] = [(R_P0, g), (R_P3, -g)]; D.X[R_T, :] = 0
        D.B[R_T, :] = g * (D.X[R_P0, 0] - D.X[R_P3, 0])
        D.tight = {R_P0, R_T, R_P3}
    for j, k in enumerate(kinds):
        if k == "safe1":
            D.B[R_E, j] = rx.SAFMIN * g
        elif k == "one":
            D.B[R_F, j] += D.zz(3, R_F + j) / 16
        elif k == "two":
            D.B[R_F, j] += D.zz(2, R_F + j) / 64
            D.X[R_A, j] += 2.0 ** 10
        elif k == "long":
            D.X[R_K, j] = 2 * c + e; D.X[R_K2, j] = 2 * c - e
        elif k == "eps":
            for i in (R_P0, R_P3):
                D.X[i, j] = rx.P53 - 1; D.B[i, j] = D.dp[i] * (rx.P53 - 1)
            D.B[R_T, j] = 2 * g
        else:
            assert k == "zero"
    return D.case(name)


class BCase:
    """one case: what the device gets (c.rp, c.ci, c.av, c.pc, c.B, c.X0), trans, the handle it runs on (kind, n, z) and the designed step counts"""

    def __init__(self, name, c, trans, kinds):
        self.name, self.c, self.trans, self.kinds = name, c, trans, list(kinds)
        self.kind, self.n, self.z, self.nrhs = c.kind, c.n, c.z, c.nrhs
        self.steps = [STEPS[k] for k in kinds]
        assert self.nrhs == len(kinds)

    def __repr__(self):
        return self.name


def _sweep(kind, trans, kinds):
    """k columns on the factors of sweep case `kind`: A' = (op(A) M)^op^-1, M = I - e_m e_m^T, b = op(A) c (rx._sweep_cases / rt._sweep_cases)"""
    s = tc.prepared(kind)[0]
    n, z = s.n, s.z
    pc = rx.perm(n)
    vt = np.complex128 if z else np.float64
    A16 = s.B16.tocsr()[pc, :][:, pc].tocsr().astype(vt)
    i = np.arange(n)
    xs = (((3 * i + 7) % 11) - 5).astype(vt)
    if z:
        xs = xs + 1j * (((5 * i + 1) % 7) - 3)
    a0, m = n // 7, n // 5
    opA16 = A16 if trans == "N" else (A16.conj().T if trans == "C" else A16.T).tocsr()
    M = sp.identity(n, dtype=vt, format="lil"); M[m, m] = 0; M = M.tocsr(); M.eliminate_zeros()
    opAp = (opA16 @ M).tocsr() / 16
    opAp.eliminate_zeros()
    Cm = np.stack([np.roll(xs, 3 * j) if j % 2 == 0 else np.roll(xs[::-1], j) for j in range(len(kinds))], axis=1).astype(vt)
    Cm[m, :] = [dict(zero=0, one=1 / 16, two=1 / 64)[k] for k in kinds]
    if z:
        Cm[m, :] *= (1 + 2j)
    B = (opA16 @ Cm) / 16
    X0 = Cm.copy()
    for j, k in enumerate(kinds):
        if k == "two":
            X0[a0, j] += 2.0 ** 10
    name = f"sw_{kind}_{trans}_{len(kinds)}"
    if trans == "N":
        return rx.RCase(name, kind, z, pc, opAp, B, X0)
    Ap = (opAp.conj().T if trans == "C" else opAp.T).tocsr()
    Ap.sort_indices()
    return rt.TCase(name, trans, kind, z, pc, (Ap.indptr, Ap.indices, Ap.data), B, X0, design=(M, Cm))


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for pname, (n, kinds) in patterns().items():
        for z in (False, True):
            r = _mix(pname, n, z, kinds)                                                    # r.name = d_<pname> / z_<pname>
            out[r.name + "_N"] = BCase(r.name + "_N", r, "N", kinds)
            if pname in TRANS_PATTERNS:
                for t in rt._from_rx(r):                                                     # t_<name>, and c_<name> for complex16
                    out[r.name + "_" + t.trans] = BCase(r.name + "_" + t.trans, t, t.trans, kinds)
    for kind, k, transes in (("narrow", 17, "NT"), ("z_narrow", 17, "NTC"), ("levels", 5, "N"), ("z_wide", 5, "N"), ("narrow", 16, "N")):
        kinds = _cycle(k, ("two", "one") if k == PANEL else ("zero", "two", "one"))         # (16 columns: every one takes a step -- ONE full MFMA block)
        for trans in transes:
            c = _sweep(kind, trans, kinds)
            out[c.name] = BCase(c.name, c, trans, kinds)
    return out


def names(kind=None, z=None, trans=None):
    return [k for k, b in cases().items() if (kind is None or (b.kind == "diag") == (kind == "diag")) and (z is None or b.z == z)
            and (trans is None or b.trans == trans)]


_PRELOADED = {}


@functools.lru_cache(maxsize=None)
def expected(name):
    """dict(berr[nrhs], steps_all[nrhs], passes, X) of the simulators: every column on its own"""
    if name in _PRELOADED:
        return _PRELOADED[name]
    b = cases()[name]
    return rx.simulate(b.c) if b.trans == "N" else rt.simulate(b.c)


def dump_expected(path, names_):
    import pickle
    with open(path, "wb") as f:
        pickle.dump({k: {q: expected(k)[q] for q in ("berr", "steps_all", "X")} for k in names_}, f)


def preload_expected(path):
    import pickle
    with open(path, "rb") as f:
        _PRELOADED.update(pickle.load(f))
