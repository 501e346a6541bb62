"""CPU checks behind tests/test_gpu_refine_exact.py: the designed edges of tests/refine_exact_cases.py hold (asserted from the simulator alone), the
exactness bounds hold for every pass of every case (`simulate` asserts them), and the simulator agrees BITWISE with the oracle's restatement of
pdgsrfs3d / pzgsrfs3d (oracle/slu_oracle_body.inc) run on the exact factors -- two independent statements of the reference, neither the code under test."""
import numpy as np
import pytest
import oracle as orc
import refine_exact_cases as rx

CASES = rx.cases()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_the_case_list_holds_every_edge():
    names = set(CASES)
    for p in ("d_", "z_"):
        for n in rx.ORDERS:
            assert any(k.startswith(f"{p}max_n{n}_r") for k in names), (p, n)
        for n in (257, 513):
            assert {f"{p}max_n{n}_r{m % n}" for m in rx.MAXPOS} <= names
        for k in ("rows_long", "rows_last", "empty_b", "safe1_stop_n5", "safe_mid_stop", "safe_mid_run", "safe2_eq", "safe2_above", "eps_stop", "eps_go", "half_long", "half_go",
                  "half_stop", "nilpotent", "rhs3"):
            assert p + k in names
    for k in rx.SWEEPS:
        assert {f"sw_nil_{k}", f"sw_rhs3_{k}"} <= names
    assert [m % 257 // 64 for m in rx.MAXPOS[:4]] == [0, 1, 2, 3]                           # one row in each wave of the first workgroup


@pytest.mark.parametrize("name", list(CASES))
def test_designed_edges_and_bounds(name):
    c = CASES[name]
    r = rx.expected(name)                                                                   # asserts the bounds of every pass
    ex = c.expect
    pc = c.pc
    assert sorted(pc.tolist()) == list(range(c.n))
    if c.n >= 3:                                                                            # (n = 1 has the identity only)
        assert not np.array_equal(pc, np.arange(c.n)) and not np.array_equal(pc[pc], np.arange(c.n))
    assert c.z == (name.startswith("z_") or c.kind in ("z_narrow", "z_wide"))
    assert r["steps"] == r["steps_all"][-1] and len(r["berr"]) == c.nrhs
    if "steps" in ex:
        assert r["steps_all"] == ex["steps"], r["steps_all"]
    if "berr" in ex:
        assert np.array_equal(r["berr"], np.array(ex["berr"])), r["berr"]
    if ex.get("untouched"):
        assert np.array_equal(_bits(r["X"]), _bits(c.X0))
    else:
        assert not np.array_equal(r["X"], c.X0)
    if "final" in ex:
        assert np.array_equal(r["X"], ex["final"])
    q, br, t = r["q"][-1], r["branch"][-1], r["t"][-1]                                      # of the last column: lists over its passes
    m = c.max_row
    if m is not None:
        assert int(np.argmax(q[-1])) == m and np.count_nonzero(q[-1] == q[-1][m]) == 1, (int(np.argmax(q[-1])), m)
        assert r["berr"][-1] == q[-1][m] and q[-1][m] > 0
    if ex.get("strict_max"):
        assert (c.n == 1 or np.sort(q[-1])[-2] < q[-1][m]) and np.count_nonzero(q[-1]) == c.n             # every other row is smaller, none is idle
    if "branch" in ex:
        assert br[0][m] == ex["branch"]
    if "first_t" in ex:
        assert t[0][m] == ex["first_t"] and br[0][m] == ex.get("first_branch", 1)
    if "first_branch" in ex:
        safe2 = (c.n + 1) * rx.SAFMIN / rx.EPS
        assert (t[0][m] == safe2) == (ex["first_branch"] == 2) and t[0][m] < safe2 * (1 + 2.0 ** -40)      # on, or just above, safe2
    if name.endswith("safe2_eq"):                                                           # the two branches give another quotient there: (safe1 + 2 u) / 6 u against 2 u / 6 u
        assert r["berr"][0] == q[0][m] != 1.0 / 3.0 and abs(r["berr"][0] - 1.0 / 3.0) < 1e-15
    if name.endswith("safe_mid_stop") or name.endswith("safe_mid_run"):
        assert (c.n + 1) * rx.SAFMIN < t[0][m] <= (c.n + 1) * rx.SAFMIN / rx.EPS and q[0][m] != round(q[0][m])
    p = r["passes"][-1]
    if "halves" in ex:
        assert all(p[k + 1] * 2 == p[k] for k in range(ex["halves"])) and r["steps"] >= 2
    if name.endswith("half_long"):
        assert r["steps"] == rx.ITMAX and len(p) == rx.ITMAX + 1 and r["berr"][0] > rx.EPS
    if ex.get("short_of_half"):
        assert p[0] < 2 * p[1] < 1.2 * p[0] and r["berr"][0] == p[1] > 0
    if name.endswith("eps_go"):
        assert p[0] == 2 * rx.EPS
    if ex.get("nonzero_berr"):
        assert r["berr"][1] > 0 and r["berr"][2] > 0 and r["berr"][1] != r["berr"][2] and r["berr"][0] != r["berr"][1]
    if "zero_t_row" in ex:
        i = ex["zero_t_row"]
        assert c.rp[i] == c.rp[i + 1] and r["t"][-1][0][i] == 0.0 and r["branch"][-1][0][i] == 0 and r["q"][-1][0][i] == 0.0
    if "lengths" in ex:
        ln = np.diff(c.rp)
        assert {0, 1, 2} <= set(ln.tolist()) and ln[m] == ln.max() >= 300
        assert any(np.any(np.diff(c.ci[c.rp[i]:c.rp[i + 1]]) < 0) for i in range(c.n))     # columns unsorted within a row
    if name.endswith("rows_last"):
        x = r["x"][-1][-1]
        e = range(c.rp[m], c.rp[m + 1])
        assert [bool(c.av[k] * x[c.ci[k]] != 0) for k in e] == [False] * (len(e) - 1) + [True]
    if c.z and c.kind == "diag" and m is not None and ("max_n" in name or "rows_" in name or "half" in name):
        x = r["x"][-1][-1]                                                                  # abs1 and the modulus give another t in the row of the maximum
        e = slice(c.rp[m], c.rp[m + 1])
        t_mod = float(np.sum(np.abs(c.av[e]) * np.abs(x[c.ci[e]])) + abs(c.B[m, -1]))
        assert abs(t_mod - t[-1][m]) > 1e-3 * t[-1][m]
        k = c.ci[e][-1]
        assert x[k].real != 0 and x[k].imag != 0 and abs(x[k].real) != abs(x[k].imag)


@pytest.mark.parametrize("name", ["z_rows_long", "z_max_n257_r71", "z_half_stop"])
def test_the_conjugate_matrix_gives_another_trajectory(name):
    c = CASES[name]
    assert np.any(c.av.imag != 0)
    r, rc = rx.expected(name), rx.simulate(c, av=c.av.conj(), check=False)
    assert not np.array_equal(r["berr"], rc["berr"]) and not np.array_equal(r["X"], rc["X"])


def _oracle_store(c):
    import trans_cases as tc
    if c.kind == "diag":
        fs, L, U = rx.diag_store(c.n, c.z)
    else:
        _, fs, L, U = tc.prepared(c.kind)[:4]
    return orc.LUStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind, fs.Lnzval_off, L.copy(), fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off, U.copy())


@pytest.mark.parametrize("name", list(CASES))
def test_simulator_equals_the_oracle_bitwise(name):
    c = CASES[name]
    r = rx.expected(name)
    X, berr, steps = orc.dgsrfs(_oracle_store(c), c.rp, c.ci, c.av, c.pc, c.B.copy(order="F"), c.X0.copy(order="F"))
    assert steps == r["steps"], (steps, r["steps_all"])
    assert np.array_equal(_bits(berr), _bits(r["berr"])), (berr.tolist(), r["berr"].tolist())
    assert np.array_equal(_bits(X), _bits(r["X"])), int(np.count_nonzero(X != r["X"]))
