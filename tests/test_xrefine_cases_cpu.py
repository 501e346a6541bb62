"""The helper of the extra-precise refinement tests checked against itself on the CPU (tests/xrefine_cases.py), the new entry points of the cross-built
library, and the argument checks of the Python layer that need no device."""
import ctypes, os
from fractions import Fraction
import numpy as np
import pytest
import xrefine_cases as xc
from superlu_dist_amd import _lib, driver, grid3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sluamd_pdgsrfs3d_extra", "sluamd_pdgsrfs3d_extra_dev", "sluamd_pzgsrfs3d_extra", "sluamd_pzgsrfs3d_extra_dev",
       "sluamd_dResidual", "sluamd_dResidual_dev", "sluamd_zResidual", "sluamd_zResidual_dev"]


def test_two_sum_and_the_product_error_are_exact():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        a, b = (float(v) for v in rng.standard_normal(2) * 2.0 ** rng.integers(-40, 40, 2))
        s, e = xc.two_sum(a, b)
        assert Fraction(s) + Fraction(e) == Fraction(a) + Fraction(b)
        s1, c1 = xc.sub_prod(b, 0.0, a, b)
        exact = Fraction(b) - Fraction(a) * Fraction(b)                                          # head + compensation: the one rounding of se - pe away from it
        assert abs(Fraction(s1) + Fraction(c1) - exact) <= Fraction(2) ** -104 * (abs(Fraction(b)) + abs(Fraction(a) * Fraction(b)))


def test_the_restatement_beats_the_plain_sum_on_random_rows():
    """rows of 7 and 70 entries of random data: the doubled accumulation meets the bound of a compensated sum, the plain sum misses it by far"""
    rng = np.random.default_rng(7)
    worse = 0
    for z in (False, True):
        for m in (7, 70):
            for _ in range(40):
                a = rng.standard_normal(m) + (1j * rng.standard_normal(m) if z else 0)
                x = rng.standard_normal(m) + (1j * rng.standard_normal(m) if z else 0)
                ent = list(zip(a, x))
                b = complex(np.dot(a, x)) if z else float(np.dot(a, x))                         # a residual that cancels
                re, im = xc.exact_row(ent, b, z)
                got, plain = complex(xc.xrow(ent, b, z)), complex(xc.plain_row(ent, b, z))
                t = Fraction(xc.weight(ent, b))
                for g, p, ex in ((got.real, plain.real, re), (got.imag, plain.imag, im)):
                    # the bound of a compensated sum: one rounding of the result, and (4 m eps)^2 of the weight (here 2^-90 t and less)
                    assert abs(Fraction(g) - ex) <= abs(ex) * Fraction(2) ** -52 + t * Fraction(2) ** -90
                    worse += abs(Fraction(p) - ex) > t * Fraction(2) ** -60
    assert worse > 50


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_one_pass_cases_are_exact_and_designed(z):
    """every case of test_gpu_xresidual.py: the restatement returns the exact residual, t does not depend on fusing, the maximum sits alone in its row,
    the plain pass differs; the cancelling row loses its answer in fp64"""
    for n, m in xc.xcase_list():
        c = xc.xcase(n, z, m)
        for tr in xc.TRANS[z]:
            xc.check_case(c, tr)
            e = c.expected(tr)
            if n > 1:
                assert e["plain"][11] == c.b[11] and e["extra"][11] == c.b[11] - c.x[0]          # 2^60 + 1 - 2^60 over x: lost / kept
                assert e["plain"][13] == 0 and e["extra"][13] != 0


def test_a_contracted_pass_would_return_twice_the_error():
    """the data of rows 13 / 14: with s - a x fused into one multiply-add (s' = the exact difference rounded) TwoSum reports no error and the compensation
    subtracts the product's error a second time"""
    a = x = xc.U30
    p = a * x
    pe = float(Fraction(a) * Fraction(x) - Fraction(p))
    assert pe != 0
    assert xc.xrow([(a, x)], p, False) == -pe
    s = float(Fraction(p) - Fraction(a) * Fraction(x))                                           # fma(-a, x, b)
    bb = s - p
    se = (p - (s - bb)) + (-p - bb)
    assert s + (0.0 + (se - pe)) == -2 * pe


def test_trajectories_end_in_the_designed_states():
    for name, (c, trans, want) in xc.trajectories().items():
        r = xc.expected(name)
        assert r["state"] == want["state"] and r["steps"] == want["steps"], name
        if "rho" in want:
            assert r["rho"] == want["rho"], name
        if "dxrel" in want:
            assert r["dxrel"] == want["dxrel"], name
        if "last_ndx" in want:                                                                  # the eps boundary, met exactly
            assert r["ndx"][0][-1] == want["last_ndx"] and want["last_ndx"] == xc.EPS * 2.0 ** 52
        if "dxrel_ratio" in want:
            assert r["ndx"][0][1] / r["ndx"][0][0] == want["dxrel_ratio"]
        for j, st in enumerate(r["state"]):
            if st == xc.LIMIT:
                assert all(b * 2 == a for a, b in zip(r["ndx"][j], r["ndx"][j][1:])), name      # ratio exactly 1 / 2
    r3 = xc.expected("d_rhs3")
    assert len(set(r3["state"])) == 3
    c = xc.trajectories()["d_noprog"][0]
    r = xc.expected("d_noprog")
    assert not np.array_equal(r["X"], c.X0) and r["X"][10, 0] == c.X0[10, 0] - 2.0 ** 18        # X after the first correction, before the dropped one


def test_the_ill_conditioned_case_meets_its_conditions():
    ic = xc.ill_case()
    assert 64 <= ic["n"] <= 300 and 1e9 < ic["cond"] < 1e13 and xc.EPS * ic["cond"] < 1
    assert np.array_equal(ic["A"], np.round(ic["A"])) and np.array_equal(ic["x_true"], np.round(ic["x_true"]))
    r = xc.ill_cpu_loops()
    print("cond %.3e" % ic["cond"], r)
    assert r["state"] == xc.CONVERGED
    assert r["err_plain"] >= 2.0 ** 10 * r["err_extra"] and r["err_plain"] > 0


def test_library_exports_and_binding_of_the_new_entry_points():
    L = _lib.load()
    for s in NEW:
        assert hasattr(L, s), s
        assert s in _lib.EXPORTS and getattr(L, s).argtypes is not None, s
    assert ctypes.sizeof(_lib.XRefine) == 24 and _lib.XR_STATES == ("CONVERGED", "NO_PROGRESS", "LIMIT")
    hdr = open(os.path.join(ROOT, "include", "superlu_dist_amd.h")).read()
    for k, v in (("SLUAMD_XR_CONVERGED", 0), ("SLUAMD_XR_NO_PROGRESS", 1), ("SLUAMD_XR_LIMIT", 2)):
        assert f"#define {k} {v}" in hdr


def test_method_extra_refuses_its_arguments_without_a_device():
    h = driver.LUHandle(None)
    h.n = 4
    b = x = np.zeros(4)
    for kw in (dict(block=True), dict(restart=5), dict(inner_tol=0.5), dict(max_solves=3)):
        with pytest.raises(ValueError):
            h.pdgsrfs3d(b, x, method="extra", **kw)
        with pytest.raises(ValueError):
            h.pdgsrfs3d_dev(0, 4, 0, 4, 1, method="extra", **kw)
    with pytest.raises(ValueError):
        h.pdgsrfs3d(b.astype(np.float32), x, method="extra")
    with pytest.raises(ValueError):
        h.pdgsrfs3d(np.zeros(5), np.zeros(5), method="extra")
    with pytest.raises(ValueError):
        h.residual(b, np.zeros(5))
    with pytest.raises(ValueError):
        h.pdgsrfs3d(b, x, method="doubled")
    g = grid3d.GridHandle.__new__(grid3d.GridHandle)
    with pytest.raises(ValueError, match="extra"):
        g.pdgsrfs3d(b, x, method="extra")


def test_the_driver_refuses_extra_with_grid_or_rowperm():
    n, rp, ci, v = 2, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.ones(2)
    with pytest.raises(ValueError, match="extra"):
        driver.pdgssvx3d(n, rp, ci, v, np.ones(2), refine="extra", grid=(2, 1, 1))
    with pytest.raises(ValueError, match="extra"):
        driver.pdgssvx3d(n, rp, ci, v, np.ones(2), refine="extra", rowperm="LargeDiag_MC64")
    with pytest.raises(ValueError):
        driver.pdgssvx3d(n, rp, ci, v, np.ones(2), refine="extra", trans="T")
    with pytest.raises(ValueError, match="'extra'"):
        driver.pdgssvx3d(n, rp, ci, v, np.ones(2), refine="quad")
