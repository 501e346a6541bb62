"""The numpy restatement of pdgsequ + pdlaqgs (equil_cases.py) checked on its own: against the reference's recorded scalings, its invariants, and
the outcome every case matrix of test_gpu_equil.py is built for.  No GPU."""
import numpy as np
import pytest
import equil_cases as ec
import refine_cases as rc


@pytest.mark.parametrize("name,rowcnd", [("unsym300", 0.199), ("unsym120_tiny", 0.242), ("z_unsym200", 0.279), ("g20_1x1x1", 1.0)])
def test_recorded_fixtures_are_not_scaled(golden, name, rowcnd):
    """The reference ran Equil = YES on these and pdlaqgs left them alone (R = 1): the restatement must say N on the recorded A."""
    g = golden(name)
    assert np.all(g["r0__R"] == 1.0)                # (r0__C carries the column scaling of the reference's MC64 step, which is not pdgsequ's)
    raw = dict(g); raw["r0__R"] = np.ones_like(g["r0__R"]); raw["r0__C"] = np.ones_like(g["r0__C"])
    n, rp, ci, v = rc.equilibrated_system(raw)[:4]    # the recorded A itself, assembled from the ranks' rows
    e = ec.equilibrate(n, rp, ci, v)
    print(name, e["rowcnd"], e["colcnd"], e["amax"])
    assert e["equed"] == "N" and e["info"] == 0
    assert np.all(e["R"] == 1.0) and np.all(e["C"] == 1.0) and np.array_equal(e["vals"], v)
    assert abs(e["rowcnd"] - rowcnd) < 5e-4 and abs(e["colcnd"] - 1.0) < 5e-4      # the figures of the issue, to their three digits


@pytest.mark.parametrize("name", sorted(ec.EXPECT))
def test_case_matrices_give_their_outcome(name):
    n, rp, ci, v = ec.case(name)
    assert np.all(np.isfinite(v)) and len(ci) == rp[n]
    e = ec.equilibrate(n, rp, ci, v)
    assert (e["equed"], e["info"]) == ec.EXPECT[name]
    assert np.iscomplexobj(v) == name.startswith("z_")
    if e["info"]:
        assert np.array_equal(e["vals"], v) and np.all(e["R"] == 1.0) and np.all(e["C"] == 1.0)


def test_all_four_outcomes_and_both_info_kinds_are_covered():
    assert {q[0] for q in ec.EXPECT.values()} == set("NRCB")
    infos = [q[1] for q in ec.EXPECT.values() if q[1]]
    assert any(i <= 257 for i in infos) and ec.EXPECT["zero_col"][1] > 64


def test_info_names_the_smallest_zero_index():
    n, rp, ci, v = ec.case("zero_row")
    r = np.zeros(n); np.maximum.at(r, ec.rows_of(n, rp), np.abs(v))
    assert np.flatnonzero(r == 0.0).tolist() == [40, 77, 200]           # stored -0.0 / 0.0, an empty row, stored zeros
    assert np.signbit(v[rp[40]:rp[41]]).any() and not np.signbit(v[rp[40]:rp[41]]).all()
    n, rp, ci, v = ec.case("zero_col")
    assert 30 not in ci and np.all(v[ci == 12] == 0.0) and ec.equilibrate(n, rp, ci, v)["info"] == n + 12 + 1


@pytest.mark.parametrize("name", ["dense65_B", "clamp1030", "z_abs1"])
def test_scaled_maxima_after_B(name):
    """after 'B' every row and column maximum of the scaled matrix is <= 1, and every row maximum of the row-scaled matrix is exactly 1 (where no clamp
    acted: x * (1 / x) rounds to 1 only up to one unit, so the claim is on the rows whose maximum is a power of two, and <= 1 + 2^-52 elsewhere)"""
    n, rp, ci, v = ec.case(name)
    e = ec.equilibrate(n, rp, ci, v)
    assert e["equed"] == "B"
    rows = ec.rows_of(n, rp)
    rmax = np.zeros(n); np.maximum.at(rmax, rows, ec.abs1(e["vals"]))
    cmax = np.zeros(n); np.maximum.at(cmax, ci, ec.abs1(e["vals"]))
    # x * fl(1 / x) = fl(1 + d), |d| <= 2^-53, is never above 1, and scaling is monotonic: <= 1 exactly for real values; abs1 of a complex value adds two
    # separately rounded parts: one unit more
    top = 1.0 + (2.0 ** -52 if np.iscomplexobj(v) else 0.0)
    assert rmax.max() <= top and cmax.max() <= top
    with np.errstate(over="ignore"):
        rs = np.zeros(n); np.maximum.at(rs, rows, ec.abs1(v) * e["R"][rows])
    raw = np.zeros(n); np.maximum.at(raw, rows, ec.abs1(v))
    clamped = (raw < ec.SMLNUM) | (raw > ec.BIGNUM)
    assert np.all(np.abs(rs[~clamped] - 1.0) <= 2.0 ** -52)
    pow2 = ~clamped & (np.frexp(raw)[0] == 0.5)
    assert np.all(rs[pow2] == 1.0)
    if name == "clamp1030":
        assert clamped.sum() == 2 and e["R"][5] == ec.BIGNUM and e["R"][9] == ec.SMLNUM


def test_abs1_and_modulus_order_two_entries_differently():
    n, rp, ci, v = ec.case("z_abs1")
    row0 = v[rp[0]:rp[1]]
    assert np.argmax(ec.abs1(row0)) != np.argmax(np.abs(row0))


def test_amax_outside_small_large_forces_the_row_branch():
    for name in ("tiny_amax_R", "huge_amax_R"):
        e = ec.equilibrate(*ec.case(name))
        assert e["rowcnd"] >= ec.THRESH and e["colcnd"] >= ec.THRESH and e["equed"] == "R"
        assert e["amax"] < ec.SMALL or e["amax"] > ec.LARGE


def test_end_to_end_systems_are_finite_and_in_range():
    for mode in "ab":
        n, rp, ci, v, perm, rs, cs = ec.scaled_operator(mode=mode)
        assert np.all(np.isfinite(v))
        e = ec.equilibrate(n, rp, ci, v)
        assert e["info"] == 0 and ec.SMALL <= e["amax"] <= ec.LARGE and e["equed"] in "RB"


@pytest.mark.parametrize("z,seed", [(False, 0), (True, 0), (False, 1), (True, 1)])
def test_end_to_end_systems_stay_safe_for_static_pivoting(z, seed):
    """The 2^+-40 systems the GPU tests factor without pivoting: after 'B' the diagonal of the scaled matrix is the largest entry of its column
    (abs1 >= 1 - 2^-52), so no pivot can fall below eps_single * anorm for a scaling reason.  Equilibration does not promise that for every scaling:
    with seed 2 a row whose columns are ALL scaled by 2^-40 takes over six column maxima and leaves diagonal entries of 3e-23 -- the reference's
    pdgsequ does the same; that system is not used."""
    n, rp, ci, v, perm, rs, cs = ec.scaled_operator(mode="a", z=z, seed=seed)
    e = ec.equilibrate(n, rp, ci, v)
    assert e["equed"] == "B"
    d = ec.abs1(e["vals"])[ec.rows_of(n, rp) == ci]
    assert len(d) == n and d.min() >= 1.0 - 2.0 ** -52
