"""Tiny and zero pivots through every diagonal-LU branch (double and complex16), against the CPU oracle and against what the construction of
the matrices says must happen (tests/pivot_cases.py: B = L0 U0 with dyadic entries, every pivot exactly known): the tiny-pivot replacement
of pdgstrf2.c:544-560 / pzgstrf2.c:544-556 (ReplaceTinyPivot), the zero-pivot `info` (:568-571) under both rules, the grid reduction of
both, the diagonal inverses of wide blocks with replaced pivots, and static pivoting followed by iterative refinement (GESP)."""
import numpy as np
import pytest
import oracle as orc
import pivot_cases as pc
from pivot_cases import THRESH
from superlu_dist_amd import driver, grid3d, matgen

pytestmark = pytest.mark.gpu

CASES = list(pc.SPECS)


def _stores(c):
    """(symbolic, CSR of B, FlatStore with B distributed into it, (L, U) entry positions)"""
    n, rp, ci, v = c.csr()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=c.relax, maxsup=c.maxsup)
    assert np.array_equal(symb.perm_c, np.arange(n))                 # the construction order is the factored order
    assert symb.xsup().tolist() == c.expect["xsup"], symb.xsup().tolist()
    if c.z:                                                          # the distribution is linear in the values: real and imaginary parts apart
        symb.distribute_host(v.real); fr = symb.flat_store()
        symb.distribute_host(v.imag); fi = symb.flat_store()
        fs = driver.FlatStore(fr.n, fr.xsup, fr.Lrowind_off, fr.Lrowind, fr.Lnzval_off, fr.Lnzval + 1j * fi.Lnzval, fr.Ufstnz_off, fr.Ufstnz,
                              fr.Unzval_off, fr.Unzval + 1j * fi.Unzval)
    else:
        symb.distribute_host(v); fs = symb.flat_store()
    pos = pc.store_positions(fs)
    (lr, lc), (ur, uc) = pos
    assert np.array_equal(fs.Lnzval, c.B[lr, lc]) and np.array_equal(fs.Unzval, c.B[ur, uc])     # the store holds B, every entry
    return symb, (n, rp, ci, v), fs, pos


def _copy(fs, L=None, U=None):
    return driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind, fs.Lnzval_off, fs.Lnzval if L is None else L, fs.Ufstnz_off, fs.Ufstnz,
                            fs.Unzval_off, fs.Unzval if U is None else U)


def _oracle(fs, replace_tiny):
    o = orc.LUStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind, fs.Lnzval_off, fs.Lnzval, fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off, fs.Unzval)
    info, tiny, _ = orc.dfactor(o, None, replace_tiny, THRESH)
    return o, info, tiny


def _diag(fs, pos):
    (lr, lc), _ = pos
    on = lr == lc
    d = np.empty(fs.n, dtype=fs.Lnzval.dtype)
    d[lr[on]] = fs.Lnzval[on]
    return d


def _branches(c, pt, diag_tail=True):
    """the diagonal-LU kernel of every level from the plan's (supernodes, widest) columns.  A copy of the dispatch -- keep it in step with
    eng::diag_lu / eng::zdiag_lu (sluamd_kernels.hip) and the big_regs flag of FactorRun::panel_diag (sluamd_factor.cpp) -- at the defaults: k_diag_lu2<1>
    takes single-supernode levels among the last SLUAMD_DIAG_TAIL (64) levels, which every level of these cases is; kz_diag_lu_wave4 is off
    (SLUAMD_ZLU4_MAX_NODES); SLUAMD_DIAG_V1 is not set."""
    out = []
    for i, (cnt, mx) in enumerate((int(r[2]), int(r[3])) for r in pt):
        if c.z:
            out.append("kz_wave_small<8>" if mx <= 8 else "kz_wave_small<16>" if mx <= 16 else "kz_wave_small<32>" if mx <= 32 else
                       "kz_diag_lu_wave" if mx <= 64 else "kz_diag_lu")
        else:
            out.append("k_diag_lu_wave" if mx <= 64 else "k_diag_lu2<1>" if (diag_tail and cnt == 1) else "k_diag_lu2<2>")
    return out


def _kind(v, z):
    if z:
        return {(True, True): "(t,t)", (True, False): "(t,0)", (False, True): "(0,t)", (False, False): "(0,0)"}[(v.real != 0, v.imag != 0)] + \
            ("-re" if v.real < 0 else "") + ("=thresh" if abs(v.real) + abs(v.imag) == THRESH else "")
    if v == 0:
        return "-0.0" if np.signbit(v) else "0"
    return ("+" if v > 0 else "-") + ("thresh" if abs(v) == THRESH else "tiny")


def _check_plan(c, h, diag_tail=True):
    """the plan's levels are the case's, every column range sits on the level it says (supernode count and widest per level): returns the
    diagonal-LU branch of every level"""
    pt = h.plan_table()
    assert [(int(r[2]), int(r[3])) for r in pt] == c.expect["levels"], pt[:, :4]
    xs = np.asarray(c.expect["xsup"])
    cuts = sorted(set(xs.tolist()) | {r[0] for r in c.expect["ranges"]})      # a range boundary inside a supernode: a piece of its refinement
    per = {}
    for a, b in zip(cuts[:-1], cuts[1:]):
        per.setdefault(pc.level_of(c.name, a), []).append(b - a)
    assert [(len(per[l]), max(per[l])) for l in sorted(per)] == c.expect["levels"]
    return _branches(c, pt, diag_tail)


def test_the_cases_cover_every_branch_event_and_route():
    """Coverage proved from the plans, not assumed: every diagonal-LU branch meets a replaced pivot, every event kind and every route occurs,
    a replaced pivot and a zero pivot sit past column 256 of a refined supernode, and one arrives through a K-fused pair."""
    branches, kinds, routes = set(), set(), set()
    for name in CASES:
        c = pc.make(name)
        symb, _, fs, pos = _stores(c)
        h = driver.LUHandle.from_store(_copy(fs), replace_tiny=True)
        br = _check_plan(c, h)
        xs = np.asarray(c.expect["xsup"])
        for j, val, k in c.events:
            kinds.add((c.z, _kind(val, c.z)))
            routes.add(c.route(j, xs))
            if j in c.tiny_cols(True):
                branches.add(br[pc.level_of(name, j)])
        if name == "rc":
            assert h.stats()["reserved_i"] > 0                          # the two chain pieces are a K-fused pair ...
            assert any(c.route(j, xs) == "schur" and j >= 386 and j in c.tiny_cols(True) for j, _, _ in c.events)   # ... feeding a tiny pivot
            routes.add("schur-kfused")
        if name in ("rb", "zc"):
            assert any(j - 130 >= 256 for j in c.tiny_cols(True)) and any(j - 130 >= 256 for j in c.zero_cols(False))
        h.destroy(); symb.free()
    assert {"k_diag_lu_wave", "k_diag_lu2<1>", "k_diag_lu2<2>", "kz_wave_small<8>", "kz_wave_small<16>", "kz_wave_small<32>", "kz_diag_lu_wave",
            "kz_diag_lu"} <= branches, branches
    assert {(False, k) for k in ("0", "-0.0", "+tiny", "-tiny", "+thresh", "-thresh")} <= kinds, kinds
    assert {(True, k) for k in ("(t,t)", "(t,t)-re", "(t,0)", "(0,t)", "(0,0)", "(t,t)-re=thresh", "(t,t)=thresh")} <= kinds, kinds
    assert {"diag", "block", "schur", "schur-kfused"} <= routes


@pytest.mark.parametrize("name,diag_tail", [(n, True) for n in CASES] + [(n, False) for n in CASES if not pc.SPECS[n][1]])
def test_tiny_pivots_match_the_oracle_and_the_construction(name, diag_tail, monkeypatch):
    """ReplaceTinyPivot on: info and the number of replaced pivots equal the oracle's and the construction's; every L/U value within 1e-12 of
    the oracle; U's diagonal BITWISE what the construction says -- a replaced pivot is exactly (sign) thresh ((+-thresh, 0) in complex16, the sign
    of the real part), a pivot of exactly +-thresh (|re| + |im| = thresh) stays, and so do (t, 0) and (0, t) in complex16 (pzgstrf2.c:544-556 replaces
    only when both parts are non-zero; (0, 0) then sets info); in double an exact zero is replaced and info stays 0.
    diag_tail=False (SLUAMD_DIAG_TAIL=0): the single wide levels at the top go through k_diag_lu2<2> instead of k_diag_lu2<1>.
    complex16: the (0, 0) events are repaired here (a zero pivot makes the panel solves divide by zero, and what the NaNs then do to later pivots
    is nobody's contract); test_zero_pivots_without_replacement_report_info checks them with the replacement on and off."""
    c = pc.make(name, repair=pc.SPECS[name][1])
    if not diag_tail:
        monkeypatch.setenv("SLUAMD_DIAG_TAIL", "0")
    symb, _, fs, pos = _stores(c)
    o, info_o, tiny_o = _oracle(fs, True)
    dev = _copy(fs)
    h = driver.LUHandle.from_store(dev, replace_tiny=True)
    br = _check_plan(c, h, diag_tail)
    assert diag_tail or "k_diag_lu2<1>" not in br
    info = h.pdgstrf3d(THRESH)
    h.copy_to_host()
    zeros = c.zero_cols(True)
    assert info == (zeros[0] + 1 if zeros else 0)                      # the smallest column (the default rule) ...
    assert info_o == (zeros[-1] + 1 if zeros else 0)                   # ... the oracle keeps the last one met (pdgstrf2.c:568-571)
    assert h.stats()["tiny_pivots"] == tiny_o == len(c.tiny_cols(True)) > 0
    if not c.z:
        assert info == 0                                                # double: every exact zero was replaced
    scale = max(np.abs(c.B).max(), 1.0)
    assert np.abs(dev.Lnzval - o.Lnzval).max() <= 1e-12 * scale
    assert np.abs(dev.Unzval - o.Unzval).max() <= 1e-12 * scale
    # the construction's factors: a replaced pivot's column of L is scaled by the REPLACEMENT (L0[i, j] * value / thresh), every value exact
    Lx, Ux = c.expected_L(True), np.triu(c.U0, 1) + np.diag(c.expected_diag(True))
    for st in (dev, _copy(fs, o.Lnzval, o.Unzval)):
        L, U = pc.dense_factors(st, pos)
        assert np.abs(L - Lx).max() <= 1e-14 * np.abs(Lx).max() and np.abs(U - Ux).max() <= 1e-14 * np.abs(Ux).max()
    for j in c.tiny_cols(True):
        if np.any(c.L0[j + 1:, j] != 0):
            assert np.abs(L[j + 1:, j]).max() <= np.abs(c.L0[j + 1:, j]).max() * 2.0 ** -19     # not scaled by 1 / (the tiny value)
    assert sum(np.any(c.L0[j + 1:, j] != 0) for j in c.tiny_cols(True)) >= len(c.tiny_cols(True)) // 2
    want = c.expected_diag(True)
    got = _diag(dev, pos)
    assert np.array_equal(got.view(np.float64), want.view(np.float64)), np.nonzero(got != want)[0]     # bitwise, signs of zero included
    assert np.array_equal(_diag(_copy(fs, o.Lnzval, o.Unzval), pos).view(np.float64), want.view(np.float64))
    for j, val, _ in c.events:
        if j in c.tiny_cols(True):
            assert abs(got[j]) == THRESH and (got[j].imag == 0 if c.z else True)
        else:
            assert got[j] == val
    h.destroy(); symb.free()


def _zero_variants():
    out = []
    for name in CASES:
        for lv in sorted({r[2] for r in pc.SPECS[name][7]}):
            if pc.make(name, zero_level=lv).zero_cols(False):
                out.append((name, lv))
    return out


@pytest.mark.parametrize("name,level", _zero_variants())
def test_zero_pivots_without_replacement_report_info(name, level):
    """ReplaceTinyPivot off, exact zero pivots in one DAG level (= one dispatch branch) at a time: info is the smallest 1-based column under the
    default rule, the largest under info_rule = 1 (the oracle's: the last one met); refactoring the same handle with the zeros repaired gives
    info = 0.  (No values are compared after a zero pivot, and nothing is solved: the reference stops there too.)"""
    c = pc.make(name, zero_level=level)
    zeros = c.zero_cols(False)
    symb, _, fs, pos = _stores(c)
    _, info_o, tiny_o = _oracle(fs, False)
    assert info_o == zeros[-1] + 1 and tiny_o == 0
    runs = [(0, False, zeros[0] + 1), (1, False, zeros[-1] + 1)]
    if c.z:                                     # complex16 with the replacement ON: (0, 0) is not a tiny pivot (pzgstrf2.c:545-546), info as without it
        assert c.zero_cols(True) == zeros
        runs += [(0, True, zeros[0] + 1), (1, True, zeros[-1] + 1)]
    symb2, _, fs2, _ = _stores(pc.make(name, repair=True))
    symb2.free()
    for rule, replace, want in runs:
        h = driver.LUHandle.from_store(_copy(fs), info_rule=rule, replace_tiny=replace)
        assert h.pdgstrf3d(THRESH) == want, (rule, replace, zeros)
        if not replace:
            assert h.stats()["tiny_pivots"] == 0
        h.set_values(_copy(fs2))
        assert h.pdgstrf3d(THRESH) == 0
        h.destroy()
    symb.free()


@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 1, 2), (2, 2, 2)])
@pytest.mark.parametrize("name", ["ra", "rb", "za", "zb"])
def test_pivots_on_grids(name, grid):
    """The same cases on process grids: the per-rank tiny_pivots sum to the oracle's count, every rank returns the same info (MIN over the ranks,
    pdgstrf3d.c:388-392), and the solutions of the tiny-pivot factorisations are the oracle's."""
    Pr, Pc, Pz = grid
    P = Pr * Pc * Pz
    for replace in (True, False):
        c = pc.make(name, repair=replace and pc.SPECS[name][1])
        symb, (n, rp, ci, v), fs, pos = _stores(c)
        o, info_o, tiny_o = _oracle(fs, replace)
        sn_tree = symb.partition(Pz) if Pz > 1 else None
        comms = grid3d.local_comms(Pr, Pc, Pz)
        rng = np.random.default_rng(1)
        xp = np.asfortranarray(rng.standard_normal((n, 2)) + (1j * rng.standard_normal((n, 2)) if c.z else 0))
        want_info = (c.zero_cols(replace)[0] + 1) if c.zero_cols(replace) else 0

        def body(rank):
            h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], sn_tree, replace_tiny=replace)
            info = h.pdgstrf3d(THRESH)
            tiny = h.stats()["tiny_pivots"]
            y = h.pdgstrs3d(xp) if info == 0 else None
            h.destroy()
            return info, tiny, y

        out = grid3d.run_ranks(P, body)
        assert [r[0] for r in out] == [want_info] * P
        assert sum(r[1] for r in out) == tiny_o == len(c.tiny_cols(replace))
        if replace:
            assert tiny_o > 0 and want_info == 0
            xo = orc.dsolve(o, xp)
            for _, _, y in out:
                assert np.abs(y - xo).max() <= 1e-10 * np.abs(xo).max()
        symb.free()


@pytest.mark.parametrize("name", ["star", "ra"])
def test_diagonal_inverses_against_extended_precision(name):
    """Linv / Uinv of every diagonal block (k_full_inv64 for levels of <= 64 columns, k_full_inv above: widths 1, 31, 32, 33, 64, 65, 128, 129,
    200, 256), some with replaced pivots, against a triangular inversion in np.longdouble of the oracle's factored block,
    entrywise |dX| <= 16 ns eps (|X| |T| |X|) (X the exact inverse; at its exact zeros the same bound with the row and column maxima of |X|)."""
    if name == "star":
        root = pc.Block(16, [pc.Block(w) for w in (1, 31, 32, 33, 64, 65, 128, 129, 200, 256)] + [pc.Block(2)])
        offs = np.cumsum([0, 1, 31, 32, 33, 64, 65, 128, 129, 200, 256, 2])
        ev = [(int(offs[i] + min(w - 1, 30)), pc.TINY * (-1) ** i, None) for i, w in enumerate((1, 31, 32, 33, 64, 65, 128, 129, 200, 256))]
        c = pc.Case("star", root, ev, relax=256, maxsup=256, seed=7,
                    expect=dict(xsup=[int(x) for x in offs] + [int(offs[-1]) + 16], levels=[(11, 256), (1, 16)]))
    else:
        c = pc.make(name)
    symb, _, fs, pos = _stores(c)
    o, info_o, _ = _oracle(fs, True)
    assert info_o == 0
    h = driver.LUHandle.from_store(_copy(fs), replace_tiny=True)
    assert h.pdgstrf3d(THRESH) == 0 and h.stats()["tiny_pivots"] > 0
    L, U = pc.dense_factors(_copy(fs, o.Lnzval, o.Unzval), pos)
    xs = symb.xsup()
    eps = np.finfo(np.float64).eps
    for k in range(len(xs) - 1):
        f, ns = int(xs[k]), int(xs[k + 1] - xs[k])
        Li, Ui = h.diag_inv(k, ns)
        for T, X, lower in ((L[f:f + ns, f:f + ns], Li, True), (U[f:f + ns, f:f + ns], Ui, False)):
            R = _tri_inv_longdouble(T, lower)
            A = np.abs(R).astype(np.float64)
            bound = 16 * ns * eps * (A @ np.abs(T) @ A)
            # where the exact inverse has an exact zero the blocked inversion may leave roundoff (2^-63 seen): there, and only there, the same
            # bound taken with the row and column maxima of |X|
            zero = R == 0
            bound[zero] = (16 * ns * eps * np.outer(A.max(axis=1), A.max(axis=0)) * np.abs(T).max())[zero]
            err = np.abs(X.astype(np.longdouble) - R).astype(np.float64)
            assert np.all(err <= bound), (k, ns, lower, np.max(err - bound))
    h.destroy(); symb.free()


def _tri_inv_longdouble(T, lower):
    ns = T.shape[0]
    T = T.astype(np.longdouble)
    if not lower:
        return _upper_inv(T)
    X = np.zeros((ns, ns), dtype=np.longdouble)
    for i in range(ns):
        X[i] = -(T[i, :i] @ X[:i]) if i else 0
        X[i, i] += 1
        X[i] /= T[i, i]
    return X


def _upper_inv(T):
    ns = T.shape[0]
    X = np.zeros((ns, ns), dtype=np.longdouble)
    for i in range(ns - 1, -1, -1):
        X[i] = -(T[i, i + 1:] @ X[i + 1:]) if i < ns - 1 else 0
        X[i, i] += 1
        X[i] /= T[i, i]
    return X


@pytest.mark.parametrize("relax,maxsup,branch", [(4, 8, "k_diag_lu_wave"), (96, 96, "k_diag_lu2<1>")])
def test_static_pivoting_then_refinement(relax, maxsup, branch):
    """GESP (ReplaceTinyPivot + iterative refinement): a non-singular matrix whose unpivoted elimination meets exact zero pivots; factored with
    replacement, then pdgsrfs3d -- the replaced count is the oracle's, the refinement steps are the oracle's (orc.dgsrfs) to one step, berr is
    at roundoff, and x is the oracle's refined x.  The zero pivots arrive by elimination and are coupled (replacing them changes the rest of
    the factors), in narrow supernodes (k_diag_lu_wave) and inside one 96-column supernode (k_diag_lu2<1>)."""
    import scipy.sparse as sp
    n = 96
    A = sp.lil_matrix((n, n)); A.setdiag(2.0)
    for i in range(n - 1):
        A[i, i + 1] = -0.5; A[i + 1, i] = -0.7
    for z in (10, 41, 77):                 # u(z-1, z-1) = 2 exactly (no lower coupling into row z-1), then u(z, z) = 2 - (4 / 2) * 1 = 0 exactly
        A[z - 1, z - 2] = 0.0; A[z - 1, z - 1] = 2.0; A[z, z - 1] = 4.0; A[z - 1, z] = 1.0; A[z, z] = 2.0
    A = A.tocsr(); A.sort_indices(); A.eliminate_zeros()
    rp, ci, v = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    xt, b = matgen.xtrue_rhs(n, rp, ci, v, 1)
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=relax, maxsup=maxsup)
    thresh = driver.pivot_thresh(n, rp, ci, v)
    h = driver.LUHandle.from_symbolic(symb, v, replace_tiny=True)
    assert h.pdgstrf3d(thresh) == 0
    tiny = h.stats()["tiny_pivots"]
    pt = h.plan_table()
    if branch == "k_diag_lu_wave":
        assert max(int(r[3]) for r in pt) <= 64
    else:
        assert [(int(r[2]), int(r[3])) for r in pt] == [(1, 96)]      # one wide supernode on a single level: k_diag_lu2<1>
    xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b
    x0 = h.pdgstrs3d(xp)[symb.perm_c, :]
    h.attach_matrix(n, rp, ci, v, symb.perm_c)
    x, berr, steps = h.pdgsrfs3d(b, x0)
    symb.distribute_host(v)
    fs = symb.flat_store()
    o = orc.LUStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind, fs.Lnzval_off, fs.Lnzval, fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off, fs.Unzval)
    info_o, tiny_o, _ = orc.dfactor(o, None, True, thresh)
    assert info_o == 0 and tiny == tiny_o >= 3
    xo0 = orc.dsolve(o, xp)[symb.perm_c, :]
    xo, berr_o, steps_o = orc.dgsrfs(o, rp, ci, v, symb.perm_c, b, xo0)
    # pdgsrfs3d stops once berr <= eps or berr no longer halves: the last step is decided by a berr within a few ulp of eps, and the device's
    # solve (fp64 atomics, inverse-based diagonal solves) and the oracle's substitution land on either side of it -- one step apart at most
    assert steps_o >= 1 and abs(steps - steps_o) <= 1, (steps, steps_o, berr, berr_o)
    assert berr.max() <= 4 * np.finfo(np.float64).eps and berr_o.max() <= 4 * np.finfo(np.float64).eps
    assert np.abs(x - xo).max() <= 1e-10 * np.abs(xo).max()
    assert np.abs(x - xt).max() <= 1e-8 * np.abs(xt).max()
    h.destroy(); symb.free()


# ---- exponent range: the factorisation commutes with power-of-two row and column scaling ----------------------------------------------------

def _scaling_matrix(kind, z):
    """(symbolic, FlatStore of the factored matrix M, its entry positions): a Poisson nested-dissection case whose plan runs 128 x 128 tiles and
    K-fused groups, or a ragged unsymmetric structure (the reference's symbolic rules); unsymmetric values, complex16 on request"""
    rng = np.random.default_rng(11)
    if kind == "poisson":
        N = 24
        n, rp, ci, v = matgen.poisson3d(N)
        v = v * (1.0 + 0.3 * rng.random(v.size))
        perm = matgen.nd_perm_grid3d(N, N, N, leaf=64)
        symb = driver.Symbolic(n, rp, ci, perm, relax=64, maxsup=256)
    else:
        n, rp, ci, v = matgen.stencil3d_unsym(12, drop=0.3, seed=4)
        symb = driver.Symbolic(n, rp, ci, matgen.nd_perm_grid3d(12, 12, 12, leaf=27), relax=24, maxsup=96, unsym=True)
    if z:
        v = matgen.complex_shift(v, rp, ci, seed=3)
        symb.distribute_host(v.real); fr = symb.flat_store()
        symb.distribute_host(v.imag); fi = symb.flat_store()
        fs = _copy(fr, fr.Lnzval + 1j * fi.Lnzval, fr.Unzval + 1j * fi.Unzval)
    else:
        symb.distribute_host(v); fs = symb.flat_store()
    return symb, fs, pc.store_positions(fs)


def _pow2(e):
    return np.ldexp(1.0, np.asarray(e, dtype=np.int64))


def _scale_store(fs, pos, er, ec):
    """M' = D_r M D_c on the store (M(i, j) -> 2^(er[i] + ec[j]) M(i, j)): exact, every product is a power-of-two shift"""
    (lr, lc), (ur, uc) = pos
    return _copy(fs, fs.Lnzval * _pow2(er[lr] + ec[lc]), fs.Unzval * _pow2(er[ur] + ec[uc]))


def _unscale_factors(fs, pos, er, ec):
    """the factors of M' = D_r M D_c are L' = D_r L D_r^-1 and U' = D_r U D_c: back to those of M (exact shifts)"""
    (lr, lc), (ur, uc) = pos
    el = np.where(lr > lc, er[lr] - er[np.maximum(lc, 0)], er[lr] + ec[np.maximum(lc, 0)])
    return _copy(fs, fs.Lnzval * _pow2(-el), fs.Unzval * _pow2(-(er[ur] + ec[uc])))


def _normal(a):
    """every entry finite and zero or normal (no subnormal part)"""
    parts = (a.real, a.imag) if np.iscomplexobj(a) else (a,)
    tiny = np.finfo(np.float64).tiny
    return all(np.all(np.isfinite(p)) and np.all((p == 0) | (np.abs(p) >= tiny)) for p in parts)


def _factor_store(st, deterministic):
    h = driver.LUHandle.from_store(st, deterministic=deterministic)
    assert h.pdgstrf3d(0.0) == 0
    h.copy_to_host()
    return h


@pytest.mark.parametrize("z", [False, True], ids=["double", "complex16"])
@pytest.mark.parametrize("kind", ["poisson", "ragged"])
def test_power_of_two_scaling_is_exact_across_the_exponent_range(kind, z):
    """A' = D_r A D_c with power-of-two diagonals, exponents drawn from [-300, 300], and A scaled as a whole by 2^900 and by 2^-900, applied to
    the rows and columns of the permuted store.  With no subnormal or infinite entry anywhere in the oracle's factors of A' (checked first: the
    range where scaling by powers of two is exact), every operation of the factorisation -- the pivot reciprocals (v_rcp_f64 + Newton steps,
    z_recip), the diagonal inverses, the MFMA Schur tiles, the panel products -- commutes with the scaling: in deterministic mode the unscaled
    factors of A' equal the deterministic factors of A BITWISE; in the default mode (fp64 atomics, K-fused groups) they agree within 1e-12 of the
    largest entry of each supernode; the solution of A' y = D_r b is D_c^-1 x within 1e-12."""
    symb, fs, pos = _scaling_matrix(kind, z)
    n = fs.n
    rng = np.random.default_rng(5)
    base = _copy(fs, fs.Lnzval.copy(), fs.Unzval.copy())
    h0 = _factor_store(base, True)
    b = np.asfortranarray(rng.standard_normal((n, 1)) + (1j * rng.standard_normal((n, 1)) if z else 0))
    x = h0.pdgstrs3d(b)
    h0.destroy()
    xs = fs.xsup
    zero = np.zeros(n, dtype=np.int64)
    for label, er, ec in (("random", rng.integers(-300, 301, n), rng.integers(-300, 301, n)), ("2^900", zero + 900, zero), ("2^-900", zero - 900, zero)):
        sc = _scale_store(fs, pos, er, ec)
        o = orc.LUStore(n, sc.xsup, sc.Lrowind_off, sc.Lrowind, sc.Lnzval_off, sc.Lnzval, sc.Ufstnz_off, sc.Ufstnz, sc.Unzval_off, sc.Unzval)
        assert orc.dfactor(o)[0] == 0
        assert _normal(sc.Lnzval) and _normal(sc.Unzval) and _normal(o.Lnzval) and _normal(o.Unzval), label
        modes = (True, False) if label == "random" else (True,)
        for det in modes:
            st = _copy(sc, sc.Lnzval.copy(), sc.Unzval.copy())
            h = _factor_store(st, det)
            if not det and kind == "poisson" and not z:
                assert h.stats()["reserved_i"] > 0                    # K-fused groups ran
            un = _unscale_factors(st, pos, er, ec)
            if det:
                bad = np.nonzero(un.Lnzval != base.Lnzval)[0]
                assert bad.size == 0 and np.array_equal(un.Unzval, base.Unzval), (label, bad[:5], un.Lnzval[bad[:5]], base.Lnzval[bad[:5]])
            else:
                for k in range(len(xs) - 1):
                    l0, l1, u0, u1 = int(fs.Lnzval_off[k]), int(fs.Lnzval_off[k + 1]), int(fs.Unzval_off[k]), int(fs.Unzval_off[k + 1])
                    ref = np.concatenate([base.Lnzval[l0:l1], base.Unzval[u0:u1]])
                    got = np.concatenate([un.Lnzval[l0:l1], un.Unzval[u0:u1]])
                    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (label, k)
            y = h.pdgstrs3d(b * _pow2(er)[:, None])
            assert np.abs(y * _pow2(ec)[:, None] - x).max() <= 1e-12 * np.abs(x).max(), (label, det)
            h.destroy()
    symb.free()
