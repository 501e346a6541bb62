"""The inputs of test_gpu_refine_block.py mean what that test assumes: the designed facts of every case of tests/refine_block_cases.py, from the simulators
alone (rx.simulate / rt.simulate assert their own exactness bounds on every row of every pass while they run).  No GPU."""
import numpy as np
import pytest
import refine_block_cases as bc
import refine_exact_cases as rx

CASES = bc.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_every_column_takes_its_designed_steps(name):
    b, r = CASES[name], bc.expected(name)
    assert r["steps_all"] == b.steps and len(b.steps) == b.nrhs == b.c.B.shape[1] == r["X"].shape[1]
    for j, k in enumerate(b.kinds):
        p = r["passes"][j]
        assert len(p) == b.steps[j] + 1 and r["berr"][j] == p[-1]
        if b.steps[j] == 0:                                                                  # stopped at pass 0: X is the x0 it was given
            assert np.array_equal(r["X"][:, j], b.c.X0[:, j])
        if k == "safe1":
            assert p[0] == float(b.n + 2)
        if k == "eps":
            assert p[0] == rx.EPS
        if k == "zero":
            assert p[0] == 0.0
        if k == "long":
            assert all(p[i + 1] * 2 == p[i] for i in range(rx.ITMAX)) and p[-1] > rx.EPS   # halves exactly: only the count ends it
        if k in ("one", "two"):
            assert p[-1] > rx.EPS and p[-1] * 2 > p[-2]                                     # stopped because the last step did not halve


def test_the_patterns_cover_what_the_block_form_can_get_wrong():
    P = bc.patterns()
    assert tuple(len(P[f"cols_{k}"][1]) for k in bc.COLS) == (1, 2, 3, 4, 5, 15, 16, 17, 33)
    assert sorted(n for n, _ in (P[f"ord_{n}"] for n in rx.ORDERS)) == sorted(rx.ORDERS) and all(len(P[f"ord_{n}"][1]) == 17 for n in rx.ORDERS)
    st = lambda name: [bc.STEPS[k] for k in P[name][1]]
    s = st("first0_16"); assert s[0] == 0 and min(s[1:]) >= 1 and P["first0_16"][1][0] == "safe1"
    s = st("last_first_16"); assert s[-1] == 0 and min(s[:-1]) >= 1
    s = st("mid_first_17"); assert s[8] == 0 and min(s[:8] + s[9:]) >= 1
    assert set(st("all_once_16")) == {1}
    s = st("long_16")
    active = [sum(1 for v in s if v >= p) for p in range(4)]                                 # columns in pass p
    assert s.count(rx.ITMAX) == 1 and active == [16, 10, 4, 1] and {0, 1} <= set(s)
    k = P["eps_17"][1]; assert k.count("eps") == 1 and 0 < k.index("eps") < bc.PANEL - 1
    for k in (17, 33):                                                                       # the rhs3 pattern runs across the panel boundary
        assert st(f"cols_{k}")[bc.PANEL - 1:bc.PANEL + 1] == [[0, 2, 1][j % 3] for j in (bc.PANEL - 1, bc.PANEL)] == [0, 2]
    # both precisions, N / T / C, and the four sweep kinds
    assert {(b.z, b.trans) for b in CASES.values()} == {(False, "N"), (False, "T"), (True, "N"), (True, "T"), (True, "C")}
    assert {b.kind for b in CASES.values()} == {"diag"} | set(rx.SWEEPS)
    for t in bc.TRANS_PATTERNS:
        assert {"d_%s_N" % t, "d_%s_T" % t, "z_%s_N" % t, "z_%s_T" % t, "z_%s_C" % t} <= set(CASES)


def test_transposed_cases_predict_the_trajectory_of_their_untransposed_twin():
    for t in bc.TRANS_PATTERNS:
        for p in "dz":
            a, b = bc.expected(f"{p}_{t}_N"), bc.expected(f"{p}_{t}_T")
            assert a["steps_all"] == b["steps_all"] and np.array_equal(a["berr"], b["berr"]) and np.array_equal(a["X"], b["X"])
        a, c = bc.expected(f"z_{t}_N"), bc.expected(f"z_{t}_C")
        assert a["steps_all"] == c["steps_all"] and np.array_equal(a["berr"], c["berr"]) and np.array_equal(a["X"].conj(), c["X"])
