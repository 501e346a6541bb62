"""The transposed refinement cases without a GPU: the numpy restatement of the library's counting sort against scipy, the simulator's own bounds on every
case, the properties the cases are designed to have, and the Python argument checks of LUHandle.pdgsrfs3d(trans=) / pdgsrfs3d_dev(trans=) (the library's
entry points replaced by a recorder, as in test_update_values_cpu.py)."""
import numpy as np
import pytest
import scipy.sparse as sp
import refine_exact_cases as rx
import refine_trans_cases as rt
from superlu_dist_amd import _lib, driver

CASES = rt.cases()


def _attached(c):
    return sp.csr_matrix((c.av, c.ci, c.rp), shape=(c.n, c.n))


@pytest.mark.parametrize("name", list(CASES))
def test_counting_sort_is_scipys_transpose(name):
    """(tcp, tri, av[tpos]) is A'.T.tocsr() with sorted indices, entry for entry; tpos is a permutation of the CSR positions"""
    c = CASES[name]
    tcp, tri, tpos = rt.transpose_index(c.n, c.rp, c.ci)
    T = _attached(c).T.tocsr()
    T.sort_indices()
    assert T.nnz == len(c.av) == len(tpos)                                                  # (no duplicates, no stored zeros summed away)
    assert np.array_equal(tcp, T.indptr) and np.array_equal(tri, T.indices) and np.array_equal(c.av[tpos], T.data)
    assert np.array_equal(np.sort(tpos), np.arange(len(tpos)))
    if c.n <= 65 and len(c.av) <= 4096:                                                     # the library's loop, entry by entry
        for a, b in zip(rt.counting_sort_loop(c.n, c.rp, c.ci), (tcp, tri, tpos)):
            assert np.array_equal(a, b)


def test_counting_sort_keeps_rows_ascending_for_unsorted_rows():
    """column indices in descending order inside the rows: the rows still ascend inside every column"""
    rp = np.array([0, 3, 5, 6, 8]); ci = np.array([3, 1, 0, 3, 0, 2, 3, 0])
    tcp, tri, tpos = rt.transpose_index(4, rp, ci)
    assert tcp.tolist() == [0, 3, 4, 5, 8] and tri.tolist() == [0, 1, 3, 0, 2, 0, 1, 3] and tpos.tolist() == [2, 4, 7, 1, 5, 0, 3, 6]
    for a, b in zip(rt.counting_sort_loop(4, rp, ci), (tcp, tri, tpos)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", list(CASES))
def test_simulator_bounds_and_designed_facts(name):
    """rt.expected runs the simulator with its assertions (every row of every pass, every correction); the designed step counts, berr and final X hold"""
    c = CASES[name]
    r = rt.expected(name)
    ex = c.expect
    if "steps" in ex:
        assert r["steps_all"] == ex["steps"], (name, r["steps_all"])
    if "berr" in ex:
        assert r["berr"].tolist() == ex["berr"]
    if "final" in ex:
        assert np.array_equal(r["X"], np.conj(ex["final"]) if name.startswith("c_") else ex["final"])
    if ex.get("untouched"):
        assert np.array_equal(r["X"], c.X0)
    if c.kind != "diag":
        assert len(r["bounds"]) == sum(r["steps_all"]) and all(max(b) < rt.tc.LIMIT for b in r["bounds"])
    if c.max_col is not None and c.kind == "diag":                                          # the designed column carries the last berr
        q = r["q"][-1][-1]
        assert q[c.max_col] == r["berr"][-1] and (not ex.get("strict_max") or np.count_nonzero(q == q.max()) == 1)


def test_every_order_and_every_position_of_the_maximum():
    for p in ("d", "z"):
        for t in ("t", "c") if p == "z" else ("t",):
            got = {(CASES[k].n, CASES[k].max_col) for k in CASES if k.startswith(f"{t}_{p}_max_n")}
            assert {n for n, _ in got} == set(rx.ORDERS)
            for n in (257, 513):
                assert {m for nn, m in got if nn == n} == {m % n for m in rx.MAXPOS}


def test_conjugate_cases_are_the_conjugate_runs():
    for k in rt.names(trans="C", kind="diag"):
        if not k.startswith("c_"):
            continue
        a, b = rt.expected(k), rt.expected("t_" + k[2:])
        assert a["steps_all"] == b["steps_all"] and np.array_equal(a["berr"], b["berr"]) and np.array_equal(a["X"], b["X"].conj()), k


def test_stop_reasons():
    for p in ("t_d_", "t_z_", "c_z_"):
        r = rt.expected(p + "eps_stop")                                                     # berr <= eps at the first pass
        assert r["steps_all"] == [0] and r["berr"][0] == rx.EPS
        r = rt.expected(p + "max_n257_r5")                                                  # 2 berr > lstres
        assert r["steps_all"] == [1] and r["passes"][0][1] * 2 > r["passes"][0][0] > rx.EPS
        r = rt.expected(p + "half_long")                                                    # count = 20
        ps = r["passes"][0]
        assert r["steps_all"] == [rx.ITMAX] and len(ps) == rx.ITMAX + 1 and ps[-1] > rx.EPS and ps[-1] * 2 <= ps[-2]


def test_transposition_shows_in_the_step_count():
    """the attached matrix run untransposed takes another number of steps: a kernel that ignored the transposition cannot pass"""
    for k in rt.ASYM:
        c = CASES[k]
        A = _attached(c)
        assert (A != A.T).nnz > 0
        assert rt.untransposed_steps(c) != rt.expected(k)["steps_all"], k


def test_structures():
    for p in ("d", "z"):
        c = CASES[f"t_{p}_dense_col"]                                                        # one column of n entries, the others of one
        cols = np.bincount(c.ci, minlength=c.n)
        assert cols.max() == c.n == 257 and np.count_nonzero(cols == c.n) == 1 and int(np.argmax(cols)) == c.max_col
        c = CASES[f"t_{p}_dense_row"]                                                        # one row of n entries; the columns hold it before and after their diagonal
        rows = np.diff(c.rp)
        assert rows.max() == c.n and np.count_nonzero(rows == c.n) == 1
        tcp, tri, _ = rt.transpose_index(c.n, c.rp, c.ci)
        m = int(np.argmax(rows))
        first = {int(tri[tcp[j]]) == m for j in range(c.n) if j != m}
        assert first == {True, False}
        c = CASES[f"t_{p}_rows_long"]                                                       # an empty column with b_j = 0: t == 0, q = 0 (branch 0)
        j = c.expect["zero_t_row"]
        assert np.count_nonzero(c.ci == j) == 0 and c.B[j, 0] == 0 and rt.expected(c.name)["branch"][0][0][j] == 0
        c = CASES[f"t_{p}_empty_b"]                                                         # ... and with b_j != 0: q = 1
        assert np.count_nonzero(c.ci == c.max_col) == 0 and c.B[c.max_col, 0] != 0 and rt.expected(c.name)["berr"][0] == 1.0
        assert rt.expected(f"t_{p}_rhs3")["steps_all"] == [0, 2, 1]


def test_t_and_c_differ_on_one_attached_matrix():
    t, c = CASES["z_split_T"], CASES["z_split_C"]
    assert np.array_equal(t.av, c.av) and np.array_equal(t.B, c.B) and np.array_equal(t.X0, c.X0)
    assert np.count_nonzero(t.av.imag) > 0
    assert np.all(t.X0.imag != 0) and np.all(t.B.imag != 0)
    assert rt.expected("z_split_T")["passes"][0][0] != rt.expected("z_split_C")["passes"][0][0]


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_update_pair(z):
    """the same-pattern update of the GPU test: both runs inside the simulator's bounds, the second an exact step to berr = 0, and a stale copy of the
    first values would show in berr"""
    u = rt.update_pair(z)
    f, s_ = u["first"], u["second"]
    assert np.array_equal(f.rp, s_.rp) and np.array_equal(f.ci, s_.ci) and len(f.av) == len(u["v0"]) and not np.array_equal(f.av, s_.av)
    A = _attached(f)
    assert (A != A.T).nnz > 0 and np.count_nonzero(u["v0"] == 0) == u["n"]
    r1, r2 = rt.simulate(f), rt.simulate(s_)
    assert r1["steps_all"] != [0] and r1["berr"][0] > rx.EPS
    assert r2["steps_all"] == [1] and r2["berr"][0] == 0.0
    stale = rt.simulate(u["stale"], check=False)
    assert stale["berr"][0] != r2["berr"][0] and not np.array_equal(stale["X"], r2["X"])


# ---- the Python argument checks ----

@pytest.fixture
def calls(monkeypatch):
    made = []

    def entry(name):
        def fn(*args):
            made.append((name, args[1]))
            return 0
        return fn
    monkeypatch.setattr(_lib, "entry", entry)
    return made


def _stub(z=False):
    h = driver.LUHandle(None)
    h.z, h.n = z, 4
    return h


def test_bad_arguments_raise_before_any_library_call(calls):
    for z in (False, True):
        h = _stub(z)
        dt = np.complex128 if z else np.float64
        good = np.ones(4, dtype=dt)
        for trans in ("X", "", "TT", 3, None):
            with pytest.raises(ValueError, match="trans"):
                h.pdgsrfs3d(good, good, trans=trans)
            with pytest.raises(ValueError, match="trans"):
                h.pdgsrfs3d_dev(0, 4, 0, 4, 1, trans=trans)
        other = np.ones(4, dtype=np.float64 if z else np.complex128)
        for b, x in ((other, good), (good, other), (np.ones(4, dtype=np.float32), good), (good, np.ones(4, dtype=np.int64)),
                     (good, np.ones(5, dtype=dt)), (np.ones(3, dtype=dt), np.ones(3, dtype=dt)), (np.ones((4, 2), dtype=dt), good),
                     (np.ones((4, 2), dtype=dt), np.ones((4, 3), dtype=dt)), (np.ones((4, 1, 1), dtype=dt), np.ones((4, 1, 1), dtype=dt)), (dt(1), dt(1))):
            for trans in ("T", "C"):
                with pytest.raises(ValueError, match="pdgsrfs3d"):
                    h.pdgsrfs3d(b, x, trans=trans)
    assert calls == []


def test_accepted_forms_reach_the_trans_entry_points_with_the_right_code(calls):
    for z, p in ((False, "d"), (True, "z")):
        h = _stub(z)
        dt = np.complex128 if z else np.float64
        for shape in ((4,), (4, 3)):
            b, x = np.ones(shape, dtype=dt), np.zeros(shape, dtype=dt)
            for trans, code in (("T", 1), ("t", 1), ("C", 2), ("c", 2)):
                del calls[:]
                xo, berr, steps = h.pdgsrfs3d(b, x, trans=trans)
                assert calls == [(f"sluamd_p{p}gsrfs3d_trans", code)] and xo.shape == (4, len(berr)) and steps == 0
                del calls[:]
                berr, steps = h.pzgsrfs3d_dev(0, 4, 0, 4, 2, trans=trans)
                assert calls == [(f"sluamd_p{p}gsrfs3d_trans_dev", code)] and len(berr) == 2
        del calls[:]
        h.pdgsrfs3d(np.ones(4, dtype=dt), np.ones(4, dtype=dt))                              # trans = "N": today's entry points, today's conversions
        h.pdgsrfs3d([1, 2, 3, 4], [0, 0, 0, 0], trans="N")
        h.pdgsrfs3d_dev(0, 4, 0, 4, 1)
        assert [c[0] for c in calls] == [f"sluamd_p{p}gsrfs3d"] * 2 + [f"sluamd_p{p}gsrfs3d_dev"]
