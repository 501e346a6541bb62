"""RowPerm = LargeDiag_MC64 on the device (sluamd_[dz]LargeDiag, sluamd_[dz]EquilibrateWith, sluamd_SetRowPerm, driver.p[dz]gssvx3d(rowperm=...)) against
the numpy restatement and the cases of rowperm_cases.py (their properties are proved in test_rowperm_cases_cpu.py).
Bars: the exact cases hold with ZERO tolerance; the general case with SLACK_BOUND (below); residuals and solutions with the project's 1e-10 parity bound."""
import functools
import json
import os
import subprocess
import sys
import numpy as np
import pytest
import rowperm_cases as rc
from superlu_dist_amd import _lib, driver, matgen

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))

# Certificate slack of the general case, max |r a c| - 1 and | |matched r a c| - 1 |: measured 4.44e-16 on the restatement and 4.44e-16 on the device
# (NOTEBOOK.md, "LargeDiag_MC64"); the bar is 8 x the larger of the two -- the margin covers the libm differences in log2 / exp2 between builds -- and is in
# no case above 1e-10.
SLACK_BOUND = min(8 * 4.440892098500626e-16, 1e-10)


@functools.lru_cache(maxsize=None)
def _dev(name):
    n, rp, ci, v = rc.general300() if name == "general300" else rc.case(name)
    return n, rp, ci, v, driver.large_diag(n, rp, ci, v)


@functools.lru_cache(maxsize=None)
def _ref(name):
    n, rp, ci, v = rc.general300() if name == "general300" else rc.case(name)
    return rc.large_diag_ref(n, rp, ci, v)


@functools.lru_cache(maxsize=None)
def _host_child():
    """every case once more in a child process with SLUAMD_ROWPERM_HOST=1: the host matches every row"""
    env = dict(os.environ, SLUAMD_ROWPERM_HOST="1")
    p = subprocess.run([sys.executable, os.path.join(TESTS, "rowperm_cases.py")], env=env, capture_output=True, text=True, timeout=120,
                       cwd=os.path.dirname(TESTS))
    assert p.returncode == 0, p.stdout + p.stderr
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWPERM_CHILD ")][-1]
    return json.loads(line[len("ROWPERM_CHILD "):])


# ---- exact cases ----

@pytest.mark.parametrize("name", sorted(rc.EXACT))
def test_exact_certificate(name):
    n, rp, ci, v, (perm_r, r, c, info) = _dev(name)
    d = _ref(name)
    print(name, info)
    assert info["info"] == 0 and sorted(perm_r) == list(range(n))
    assert np.all(np.frexp(r)[0] == 0.5) and np.all(np.frexp(c)[0] == 0.5)                 # powers of two
    assert rc.certificate(n, rp, ci, v, perm_r, r, c) == (0.0, 0.0)
    assert rc.objective(n, rp, ci, d["cost"], perm_r) == rc.objective(n, rp, ci, d["cost"], d["perm_r"])
    # the restatement follows the same rules: the same matching, duals and counters, bit for bit
    assert np.array_equal(perm_r, d["perm_r"]) and np.array_equal(r, d["r"]) and np.array_equal(c, d["c"])
    assert {k: info[k] for k in ("rounds", "matched_device", "augmentations")} == {k: d[k] for k in ("rounds", "matched_device", "augmentations")}


def test_unique_optimum_rand8():
    for name in ("rand8", "z_rand8"):
        perm_r = _dev(name)[4][0]
        best, perms = rc.brute_force(rc.EXACT[name]())
        assert len(perms) == 1 and np.array_equal(perm_r, perms[0])


@pytest.mark.parametrize("name", rc.ALL_ON_DEVICE)
def test_cyclic_all_on_device(name):
    n, rp, ci, v, (perm_r, r, c, info) = _dev(name)
    assert info["matched_device"] == n and info["augmentations"] == 0
    assert np.array_equal(perm_r, (np.arange(n) + 1) % n)


@pytest.mark.parametrize("name", ["blocks130", "z_blocks130"])
def test_blocks_counters(name):
    n, rp, ci, v, (perm_r, r, c, info) = _dev(name)
    assert info["matched_device"] == 65 and info["augmentations"] == 65
    assert np.array_equal(perm_r, np.arange(n) ^ 1)


@pytest.mark.parametrize("name", rc.POSITIVE_PATH)
def test_positive_path(name):
    n, rp, ci, v, (perm_r, r, c, info) = _dev(name)
    d = _ref(name)
    assert max(d["path_lengths"]) > 0 and info["augmentations"] == d["augmentations"] > 0
    assert np.array_equal(r, d["r"]) and np.array_equal(c, d["c"])                          # the duals the host moved


@pytest.mark.parametrize("name", rc.SINGULAR)
def test_singular(name):
    n, rp, ci, v, expect = rc.singular(name)
    perm_r, r, c, info = driver.large_diag(n, rp, ci, v)
    assert info["info"] == expect and perm_r is None and r is None and c is None


def test_host_only_child():
    child = _host_child()
    for name in sorted(rc.EXACT):
        n, rp, ci, v, (perm_r, r, c, info) = _dev(name)
        h = child[name]
        cost = _ref(name)["cost"]
        assert (h["info"], h["rounds"], h["matched_device"], h["augmentations"]) == (0, 0, 0, n)
        assert rc.objective(n, rp, ci, cost, np.array(h["perm_r"])) == rc.objective(n, rp, ci, cost, perm_r)
        assert rc.certificate(n, rp, ci, v, np.array(h["perm_r"]), np.array(h["r"]), np.array(h["c"])) == (0.0, 0.0)
        if name in rc.UNIQUE:
            assert h["perm_r"] == list(perm_r)


@pytest.mark.parametrize("name", ["rand8", "blocks130", "z_pospath66", "general300"])
def test_two_calls_bitwise_equal(name):
    n, rp, ci, v, (p1, r1, c1, i1) = _dev(name)
    p2, r2, c2, i2 = driver.large_diag(n, rp, ci, v)
    assert np.array_equal(p1, p2) and r1.tobytes() == r2.tobytes() and c1.tobytes() == c2.tobytes() and i1 == i2


def test_bad_arguments():
    n, rp, ci, v = rc.case("rand8")
    bad = ci.copy(); bad[3] = n
    with pytest.raises(RuntimeError, match="column index outside"):
        driver.large_diag(n, rp, bad, v)
    with pytest.raises(RuntimeError, match="rowptr is not ascending"):
        driver.large_diag(3, np.array([0, 2, 1, 3]), np.array([0, 1, 2]), np.ones(3))


# ---- general values ----

def test_general300():
    """objective against the restatement's optimum, certificate slack against SLACK_BOUND.
    Objective: the device's matching is optimal for the device's cost array, the restatement's for its own; the two arrays differ by the rounding of two
    log2 and a subtraction per entry, <= 4 units in the last place of the largest cost, so two optima evaluated on one array differ by <= 2 n x that."""
    n, rp, ci, v, (perm_r, r, c, info) = _dev("general300")
    d = _ref("general300")
    assert info["info"] == 0 and sorted(perm_r) == list(range(n)) and 0 < info["matched_device"] < n
    o_dev, o_ref = rc.objective(n, rp, ci, d["cost"], perm_r), rc.objective(n, rp, ci, d["cost"], d["perm_r"])
    s_dev = rc.certificate(n, rp, ci, v, perm_r, r, c)
    s_ref = rc.certificate(n, rp, ci, v, d["perm_r"], d["r"], d["c"])
    print("general300:", info, "objective", o_dev, o_ref, "slack device", s_dev, "restatement", s_ref)
    cmaxfin = d["cost"][np.isfinite(d["cost"])].max()
    assert abs(o_dev - o_ref) <= 2 * n * 4 * 2.0 ** -52 * max(cmaxfin, 1.0)
    assert s_dev[0] <= SLACK_BOUND and s_dev[1] <= SLACK_BOUND
    h = _host_child()["general300"]
    assert abs(rc.objective(n, rp, ci, d["cost"], np.array(h["perm_r"])) - o_ref) <= 2 * n * 4 * 2.0 ** -52 * max(cmaxfin, 1.0)


# ---- end to end ----

def test_shuffled_poisson_recovered_on_the_device():
    n, rp, ci, v, shuffle, (pn, prp, pci, pv) = rc.shuffled_poisson()
    perm_r, r, c, info = driver.large_diag(n, rp, ci, v)
    assert np.array_equal(perm_r, shuffle) and info["matched_device"] == n and info["augmentations"] == 0
    rp1, ci1, v1, _ = driver.permute_rows_csr(n, rp, ci, v, perm_r)
    assert np.array_equal(rp1, prp) and np.array_equal(ci1, pci) and np.array_equal(v1, pv)


def _factors(symb, h):
    fs = symb.flat_store(values=False)
    h.copy_to_host(fs)
    return fs.Lnzval.copy(), fs.Unzval.copy()


@functools.lru_cache(maxsize=None)
def _poisson_pair():
    """(x, L, U) of the unshuffled Poisson solve, twice, and of the shuffled one through rowperm, all with deterministic=True; plus xtrue"""
    n, rp, ci, v, shuffle, (pn, prp, pci, pv) = rc.shuffled_poisson()
    perm = matgen.nd_perm_grid3d(8, 8, 8, leaf=27)
    xt, b = matgen.xtrue_rhs(n, prp, pci, pv, 1)
    out = []
    for args, kw in (((prp, pci, pv, b), {}), ((prp, pci, pv, b), {}), ((rp, ci, v, b[shuffle]), dict(rowperm="LargeDiag_MC64", equil=False))):
        x, info, st, h, symb = driver.pdgssvx3d(n, *args, perm, relax=16, maxsup=128, deterministic=True, keep=True, **kw)
        assert info == 0
        out.append((x,) + _factors(symb, h))
        h.destroy(); symb.free()
    assert st["rowperm"]["matched_device"] == n
    return out, xt


def test_shuffled_poisson_factors_bitwise():
    """the shuffled system through rowperm is factored from the same store, bit for bit, as the unshuffled one"""
    (a, a2, c), xt = _poisson_pair()
    assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])
    assert np.abs(a[0] - xt.reshape(a[0].shape)).max() < 1e-10


def test_shuffled_poisson_solution_bitwise():
    """x of the shuffled system through rowperm (equil=False, deterministic=True) bitwise equal to x of the unshuffled solve -- and two unshuffled solves
    bitwise equal to each other: a deterministic handle runs every update unit of the sweeps as a launch of its own, so the fp64 atomics on shared rows of x
    arrive in one order (without the option two solves of one system differ in the last bits of some entries)."""
    (a, a2, c), xt = _poisson_pair()
    print("entries that differ: unshuffled twice", int((a[0] != a2[0]).sum()), "| shuffled vs unshuffled", int((c[0] != a[0]).sum()))
    assert a2[0].tobytes() == a[0].tobytes()
    assert c[0].tobytes() == a[0].tobytes()


@pytest.mark.parametrize("nrhs", [1, 3])
def test_deterministic_handle_repeats_its_solve(nrhs):
    """one deterministic handle, an unsymmetric operator, the same right-hand sides three times: bitwise equal solutions, equal to the default schedule's
    within the bar of repeated solves (1e-13 max|x|, test_gpu_edge_cases.py)"""
    n, rp, ci, v = matgen.stencil3d_unsym(6, seed=2)
    perm = matgen.nd_perm_grid3d(6, 6, 6, leaf=27)
    b = np.asfortranarray(np.random.default_rng(nrhs).standard_normal((n, nrhs)))
    xs = []
    for det in (True, False):
        symb = driver.Symbolic(n, rp, ci, perm, relax=8, maxsup=64)
        h = driver.LUHandle.from_symbolic(symb, v, deterministic=det)
        try:
            assert h.pdgstrf3d(driver.pivot_thresh(n, rp, ci, v)) == 0
            xp = np.zeros_like(b, order="F"); xp[symb.perm_c, :] = b
            xs.append([h.pdgstrs3d(xp.copy(order="F")) for _ in range(3 if det else 1)])
        finally:
            h.destroy(); symb.free()
    assert xs[0][1].tobytes() == xs[0][0].tobytes() == xs[0][2].tobytes()
    assert np.abs(xs[1][0] - xs[0][0]).max() <= 1e-13 * np.abs(xs[0][0]).max()


@functools.lru_cache(maxsize=None)
def _system(z):
    """an irregular unsymmetric operator whose rows arrive badly scaled and in another order; (n, rp, ci, v, dense A)"""
    n, rp, ci, v = matgen.stencil3d_unsym(5, seed=3)
    if z:
        v = matgen.complex_shift(v, rp, ci, seed=4)
    rng = np.random.default_rng(11)
    A = rc.dense_from_csr(n, rp, ci, v) * (10.0 ** rng.uniform(-3, 3, n))[:, None]
    A = A[rng.permutation(n)]
    return rc.csr_from_dense(A) + (A,)


@pytest.fixture(scope="module", params=[False, True], ids=["d", "z"])
def solved(request):
    """pdgssvx3d(rowperm, equil=True, keep=True) once per precision"""
    z = request.param
    n, rp, ci, v, A = _system(z)
    rng = np.random.default_rng(2)
    b = rng.standard_normal((n, 3)) + (1j * rng.standard_normal((n, 3)) if z else 0)
    x, info, st, h, symb = driver.pdgssvx3d(n, rp, ci, v, b, relax=8, maxsup=64, rowperm="LargeDiag_MC64", equil=True, keep=True)
    assert info == 0 and st["equed"] == "B"
    yield z, n, rp, ci, v, A, b, x, h, symb
    h.destroy(); symb.free()


def _op(A, trans):
    return {"N": A, "T": A.T, "C": A.conj().T}[trans]


def _check(A, trans, b, x):
    """relative residual and distance to the dense solve of the ORIGINAL system, both against 1e-10"""
    M = _op(A, trans)
    xd = np.linalg.solve(M, b)
    res = np.linalg.norm(b - M @ x) / np.linalg.norm(b)
    err = np.linalg.norm(x - xd) / np.linalg.norm(xd)
    print(f"trans {trans} nrhs {b.shape[1]}: residual {res:.2e}, |x - x_dense| / |x_dense| {err:.2e}")
    assert res <= 1e-10 and err <= 1e-10


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("trans,refine", [("N", False), ("N", True), ("T", False), ("C", False)])
def test_rowperm_equil_solves(solved, trans, refine, nrhs):
    """(refine with trans = T / C is not part of sluamd_p[dz]gssvx3d_solve, with or without a row permutation)"""
    z, n, rp, ci, v, A, b, x, h, symb = solved
    bb = np.asfortranarray(b[:, :nrhs])
    out = h.gssvx_solve(bb, trans=trans, refine=refine)
    if refine:
        out, berr, steps = out
        assert np.all(berr <= 4 * 2.0 ** -53)
    _check(A, trans, bb, out)
    if trans == "N" and not refine and nrhs == 3:
        assert np.abs(out - x).max() <= 1e-13 * np.abs(x).max()                # what the driver itself returned
    if z and trans == "C":
        assert np.abs(out - h.gssvx_solve(bb, trans="T")).max() > 1e-3 * np.abs(out).max()


def test_matching_scalings_in_the_handle(solved):
    """the handle holds the matching's scalings alone: R by the rows of Pr A, C by column; |R A1 C| has a unit diagonal and entries <= 1"""
    z, n, rp, ci, v, A, b, x, h, symb = solved
    perm_r, r, c, info = driver.large_diag(n, rp, ci, v)
    R, Cs = h.scalings()
    assert np.array_equal(R[perm_r], r) and np.array_equal(Cs, c)
    S = np.abs(r[:, None] * A * c[None, :])
    assert S.max() <= 1 + SLACK_BOUND and np.abs(S[np.arange(n), perm_r] - 1).max() <= SLACK_BOUND


def test_update_values_second_step(solved):
    """new values of the same pattern, given in A's order, go through the position map; R, C and perm_r are reused"""
    z, n, rp, ci, v, A, b, x, h, symb = solved
    rng = np.random.default_rng(9)
    v2 = v * (1.0 + 0.1 * rng.uniform(-1, 1, len(v)))
    A2 = rc.dense_from_csr(n, rp, ci, v2)
    d = h.update_values(np.ascontiguousarray(v2), want_norm=True)
    assert d["equed"] == "B"
    assert h.pdgstrf3d(0.5 * float(np.finfo(np.float32).eps) * d["anorm"]) == 0
    for trans in ("N", "T"):
        _check(A2, trans, b, h.gssvx_solve(b, trans=trans))


_TORCH_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch                                   # first: torch's HIP context must exist before the library initialises the runtime
assert torch.cuda.is_available(), "torch sees no HIP device"
torch.cuda.init()
import numpy as np
import rowperm_cases as rc
import test_gpu_rowperm as t
from superlu_dist_amd import driver
for z in (False, True):
    n, rp, ci, v, A = t._system(z)
    b = np.random.default_rng(2).standard_normal((n, 2)).astype(complex if z else float)
    x, info, st, h, symb = driver.pdgssvx3d(n, rp, ci, v, b, relax=8, maxsup=64, rowperm="LargeDiag_MC64", equil=True, keep=True)
    v2 = v * (1.0 + 0.1 * np.random.default_rng(9).uniform(-1, 1, len(v)))
    h.update_values(torch.from_numpy(np.ascontiguousarray(v2)).cuda())            # values in A's order, on the device
    assert h.pdgstrf3d(0.0) == 0
    t._check(rc.dense_from_csr(n, rp, ci, v2), "N", b, h.gssvx_solve(b))
    h.destroy(); symb.free()
print("TORCH_CHILD_OK")
"""


def test_update_values_device_tensor():
    """a torch tensor on the device, in A's order, goes through index_select with the position map and sluamd_[dz]UpdateValues_dev.  In a child process that
    initialises torch first (torch.cuda reports no device once the library has initialised the HIP runtime in the process)."""
    root = os.path.dirname(TESTS)
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, root], capture_output=True, text=True, timeout=300, cwd=root)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "TORCH_CHILD_OK" in p.stdout


def test_c_example_rowperm(tmp_path):
    """examples/pddrive3d_amd --rowperm --equil on the shuffled, badly scaled operator from a MatrixMarket file, and with a same-pattern step on Poisson"""
    root = os.path.dirname(TESTS)
    exe = os.path.join(root, "examples", "pddrive3d_amd")
    subprocess.check_call(["make", "-C", os.path.join(root, "examples")], stdout=subprocess.DEVNULL)
    n, rp, ci, v, A = _system(False)
    f = str(tmp_path / "shuffled.mtx")
    matgen.write_matrix_market(f, n, rp, ci, v)
    for args in ([f, "--rowperm", "--equil"], [f, "--rowperm"], ["6", "--rowperm", "--equil", "--steps", "1"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        print(r.stdout, r.stderr)
        assert r.returncode == 0 and "ROWPERM: rounds" in r.stdout


# ---- error cases ----

def _handle(n, rp, ci, v):
    symb = driver.Symbolic(n, rp, ci, None, relax=8, maxsup=64)
    return symb, driver.LUHandle.from_symbolic(symb, v)


def test_set_row_perm_errors():
    n, rp, ci, v = matgen.poisson3d(4)
    symb, h = _handle(n, rp, ci, v)
    try:
        ident = np.arange(n, dtype=np.int32)
        with pytest.raises(RuntimeError, match="no matrix attached"):
            h.set_row_perm(ident)
        h.attach_matrix(n, rp, ci, v, symb.perm_c)
        bad = ident.copy(); bad[1] = 0
        with pytest.raises(RuntimeError, match="not a permutation"):
            h.set_row_perm(bad)
        bad[1] = n
        with pytest.raises(RuntimeError, match="not a permutation"):
            h.set_row_perm(bad)
        with pytest.raises(ValueError, match="entries expected"):
            h.set_row_perm(ident[:-1])
        h.set_row_perm(ident)                                                  # the identity changes nothing
        assert h.pdgstrf3d(0.0) == 0
        b = np.random.default_rng(0).standard_normal((n, 2))
        x = h.gssvx_solve(b)
        assert np.linalg.norm(b - matgen.csr_matvec(n, rp, ci, v, x)) <= 1e-10 * np.linalg.norm(b)
        with pytest.raises(RuntimeError, match="holds factors"):
            h.set_row_perm(ident)
    finally:
        h.destroy(); symb.free()


def test_equilibrate_with_contract():
    n, rp, ci, v = matgen.stencil3d_unsym(4, seed=1)
    rng = np.random.default_rng(3)
    r = 2.0 ** rng.integers(-4, 5, n).astype(float); c = 2.0 ** rng.integers(-4, 5, n).astype(float)
    rows = np.repeat(np.arange(n), np.diff(rp))
    for rr, cc, equed in ((r, c, "B"), (r, None, "R"), (None, c, "C"), (None, None, "N")):
        symb, h = _handle(n, rp, ci, v)
        try:
            d = h.equilibrate_with(n, rp, ci, v, symb.perm_c, rr, cc)
            R, Cs = h.scalings()
            assert d["equed"] == equed and d["info"] == 0
            assert np.array_equal(R, np.ones(n) if rr is None else rr) and np.array_equal(Cs, np.ones(n) if cc is None else cc)
            assert d["rowcnd"] == (1.0 if rr is None else rr.min() / rr.max()) and d["colcnd"] == (1.0 if cc is None else cc.min() / cc.max())
            assert d["amax"] == np.abs(v).max()
            sv = (v * R[rows]) * Cs[ci]
            ref = np.bincount(ci, weights=np.abs(sv), minlength=n).max()
            assert abs(d["anorm"] - ref) <= n * 2.0 ** -52 * ref
            with pytest.raises(RuntimeError, match="equilibrated already"):
                h.equilibrate_with(n, rp, ci, v, symb.perm_c, rr, cc)
            with pytest.raises(RuntimeError, match="equilibrated already"):
                h.equilibrate(n, rp, ci, v, symb.perm_c)
            # the solve of the scaled handle, in the caller's scaling
            assert h.pdgstrf3d(0.5 * float(np.finfo(np.float32).eps) * d["anorm"]) == 0
            b = rng.standard_normal((n, 1))
            x = h.gssvx_solve(b)
            assert np.linalg.norm(b - matgen.csr_matvec(n, rp, ci, v, x)) <= 1e-10 * np.linalg.norm(b)
        finally:
            h.destroy(); symb.free()
    symb, h = _handle(n, rp, ci, v)
    try:
        bad = r.copy(); bad[5] = 0.0
        with pytest.raises(RuntimeError, match="not positive and finite"):
            h.equilibrate_with(n, rp, ci, v, symb.perm_c, bad, c)
        with pytest.raises(ValueError, match="must have shape"):
            h.equilibrate_with(n, rp, ci, v, symb.perm_c, r[:-1], c)
        assert h.equilibrate_with(n, rp, ci, v, symb.perm_c, r, c)["equed"] == "B"      # a refused call leaves the handle open
    finally:
        h.destroy(); symb.free()


def test_unknown_rowperm_name():
    n, rp, ci, v = matgen.poisson3d(3)
    with pytest.raises(ValueError, match="rowperm must be"):
        driver.pdgssvx3d(n, rp, ci, v, np.ones(n), rowperm="LargeDiag_HWPM")
