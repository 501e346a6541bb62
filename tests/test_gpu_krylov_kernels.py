"""The Krylov kernels of the GMRES refinement (sluamd_gkernels.inc: k_gm_dots, k_gm_sum, k_gm_axpys, k_gm_scale, k_gm_combine; both precisions, NV = 0 .. 8)
one operation at a time through sluamd_krylov_selftest, which runs them through the chunk loops gmres_cycle itself runs (basis_dots, basis_axpys,
basis_combine in sluamd_gmres.cpp) on vectors laid out as the cycle's workspace, with NaN in the partials slab, the result words and every vector that is only
written.  The data (tests/krylov_cases.py; proved by test_krylov_cases_cpu.py) are small integers, so every result is exact in fp64 in any order of summation
and is compared with integer arithmetic by numpy.array_equal: dense pseudo-random vectors, and probes w = e_i whose coefficients name the element that was
read, at the first and last value, on both sides of the wave, workgroup, k_gm_sum-loop and grid-wrap boundaries and beside the pad.

The library is built without any flag that relaxes fp64 division (csrc/Makefile: -O3 -munsafe-fp-atomics, which concerns atomic adds, and no -ffast-math or
reciprocal option), so k_gm_scale's quotient by 3.0 is asserted EQUAL to numpy's correctly rounded one, not within one unit in the last place.

The floating-point runs (uniform random doubles) check what the kernels' header claims -- results repeat bit for bit, and the order of a sum depends on n
alone: not on the stride, not on how many vectors share the launch -- and the textbook bound of a sum of m products in any order,
|got - ref| <= 2 m 2^-53 sum |v_i| |w_i| (gamma_m < 2 m u while m u < 1/2; fused multiply-adds only lower it; the factor 2 over m u also covers the
reference's own 2^-64 arithmetic), m = n for double and 2 n for either part of a complex16 dot product.  The reference is formed in numpy.longdouble, and in
fractions at the small order."""
import ctypes as C
from fractions import Fraction
import numpy as np
import pytest
import krylov_cases as kc
from superlu_dist_amd import _lib

pytestmark = pytest.mark.gpu

ZN = [(z, n) for z in (False, True) for n in kc.ORDERS[z]] + [(z, n) for z in (False, True) for n in kc.BIG_NV_ORDERS if n not in kc.ORDERS[z]]
IDS = [("z" if z else "d") + str(n) for z, n in ZN]
NRES = 2 * kc.MAX_NV + 1


def _p(a):
    return None if a is None else a.ctypes.data_as(_lib.P_dbl)


def _f(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def call(op, z, n, nv=0, vstride=None, V=None, x=None, coef=None, h=1.0, add=0):
    """(rc, xout [ns], res [2 * 64 + 1]); what the entry does not write stays NaN.  V, x, coef: float64, contiguous (V: at least nv vectors)"""
    xout, res = np.full(kc.ns_of(n, z) if n > 0 else 2, np.nan), np.full(NRES, np.nan)
    rc = _lib.entry("sluamd_krylov_selftest")(kc.OPS.get(op, op), int(z), n, nv, kc.ns_of(n, z) if vstride is None else vstride, _p(V), _p(x), _p(coef), h, add,
                                               _p(xout), _p(res))
    return rc, xout, res


def run(*a, **kw):
    rc, xout, res = call(*a, **kw)
    assert rc == 0, _lib.load().sluamd_last_error().decode()
    return xout, res


def _check_dots(res, nv, z, coef, nrm, what):
    m = nv * (2 if z else 1)
    got = res[:m + 1]
    assert not np.isnan(got).any(), (what, "a slot nothing wrote was read", got.tolist())
    assert np.array_equal(got[:m], np.asarray(coef, dtype=np.float64).reshape(-1)), (what, got[:m].tolist(), np.asarray(coef).reshape(-1).tolist())
    assert got[m] == float(nrm), (what, "norm", got[m], nrm)
    assert np.isnan(res[m + 1:]).all(), (what, "more results than asked for")


@pytest.mark.parametrize("z,n", ZN, ids=IDS)
def test_dots(z, n):
    """v_k^H w and ||w||^2 for every (order, nv, data kind, stride); w comes back untouched"""
    d = kc.dense(n, z)
    Vd, wd, Vc = _f(d["V"]), _f(d["w"]), _f(kc.coded_basis(n, z))
    e = np.zeros_like(wd)
    for nv in kc.nvs("dots", z, n):
        coef, nrm = kc.expected_dots(d["V"][:nv], d["w"], z)
        for vstride in kc.strides(n, z):
            xout, res = run("dots", z, n, nv, vstride, Vd, wd)
            _check_dots(res, nv, z, coef, nrm, ("dense", n, nv, vstride))
            assert np.array_equal(_bits(xout), _bits(kc.padded(wd, n, z)))
            for i in kc.probes(n, z):
                e.reshape(-1)[i * (2 if z else 1)] = 1.0
                xout, res = run("dots", z, n, nv, vstride, Vc, e)
                e.reshape(-1)[i * (2 if z else 1)] = 0.0
                pc, pn = kc.probe_expected(i, nv, z)
                _check_dots(res, nv, z, pc, pn, ("probe", n, nv, vstride, i))


@pytest.mark.parametrize("z,n", ZN, ids=IDS)
def test_axpys(z, n):
    """w -= sum_k v_k h_k with the coefficients in device memory, and ||w||^2 of the NEW w from the last launch's partials; the pad of an odd double vector
    stays 0.0"""
    d = kc.dense(n, z)
    Vd, wd, cd = _f(d["V"]), _f(d["w"]), _f(d["coef"])
    for nv in kc.nvs("axpys", z, n):
        w1, nrm = kc.expected_axpys(d["V"][:nv], d["w"], d["coef"][:nv], z)
        want = kc.padded(w1, n, z)
        for vstride in kc.strides(n, z):
            xout, res = run("axpys", z, n, nv, vstride, Vd, wd, cd)
            assert np.array_equal(xout, want), ("w", n, nv, vstride, np.flatnonzero(xout != want)[:8].tolist())
            assert res[0] == float(nrm), ("norm", n, nv, vstride, res[0], nrm)
            assert np.isnan(res[1:]).all()
            if not z and n & 1:
                assert xout[n] == 0.0


@pytest.mark.parametrize("z,n", ZN, ids=IDS)
def test_scale(z, n):
    """dst = src / h into a vector that held NaN: exact for h = +-2^k; the pad compares equal to 0.0 (0 / -h is -0.0: a zero all the same); the quotient by
    3.0 equals numpy's (no compile flag relaxes fp64 division: see the head of this file)"""
    wd = _f(kc.dense(n, z)["w"])
    src = kc.padded(wd, n, z)
    for k, sign in ((0, 1.0), (0, -1.0), (1, 1.0), (-3, -1.0), (40, 1.0), (-40, -1.0), (600, -1.0)):
        xout, _ = run("scale", z, n, x=wd, h=sign * 2.0 ** k)
        assert not np.isnan(xout).any(), ("a unit was not written", n, k)
        assert np.array_equal(xout, sign * np.ldexp(src, -k)), (n, k, sign)
        if not z and n & 1:
            assert xout[n] == 0.0
    xout, _ = run("scale", z, n, x=wd, h=3.0)
    assert np.array_equal(xout, src / 3.0), (n, np.flatnonzero(xout != src / 3.0)[:8].tolist())


@pytest.mark.parametrize("z,n", ZN, ids=IDS)
def test_combine(z, n):
    """u = (add ? u : 0) + sum_k v_k y_k on a nonzero u.  With nv > 8 and add = 0 the first launch must drop u and every later one must keep what the launches
    before it left; the pad stays 0.0"""
    d = kc.dense(n, z)
    Vd, ud, cd = _f(d["V"]), _f(d["u"]), _f(d["coef"])
    assert np.count_nonzero(ud) > ud.size // 2 or n < 4
    for nv in kc.nvs("combine", z, n):
        for add in (0, 1):
            want = kc.padded(kc.expected_combine(d["V"][:nv], d["u"], d["coef"][:nv], add, z), n, z)
            for vstride in kc.strides(n, z):
                xout, _ = run("combine", z, n, nv, vstride, Vd, ud, cd, add=add)
                assert np.array_equal(xout, want), (n, nv, add, vstride, np.flatnonzero(xout != want)[:8].tolist())
                if not z and n & 1:
                    assert xout[n] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# floating-point data: repeatability, independence of stride and of the company in the launch, the error bound of a sum
# ---------------------------------------------------------------------------------------------------------------------------------------
FLOAT_CASES = [(False, 513), (False, 524288 + 4097), (True, 257), (True, 262144 + 2049)]


def _float_data(z, n):
    rng = np.random.default_rng(12345 + n)
    nv = 9 if kc.small(n) else 8
    tail = (2,) if z else ()
    return nv, rng.uniform(-1.0, 1.0, size=(nv, n) + tail), rng.uniform(-1.0, 1.0, size=(n,) + tail), rng.uniform(-1.0, 1.0, size=(nv,) + tail)


def _sum_exactly(terms):
    return sum((Fraction(float(t)) for t in terms), Fraction(0))


def _ref_dots(V, w, z, exact):
    """per coefficient part: (reference value, sum of |products|, number of products), then the same for ||w||^2; longdouble, or fractions when `exact`"""
    L = np.longdouble
    out = []
    flat = lambda a: a.reshape(-1)
    def one(pairs):                                             # pairs: [(a, b, sign)]: sum of sign a_i b_i over all pairs
        m = sum(a.size for a, b, s in pairs)
        mag = float(sum((np.abs(a.astype(L)) * np.abs(b.astype(L))).sum() for a, b, s in pairs))
        if exact:
            ref = sum((s * _sum_exactly(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(flat(a), flat(b))) for a, b, s in pairs), Fraction(0))
        else:
            ref = sum(s * (a.astype(L) * b.astype(L)).sum() for a, b, s in pairs)
        return ref, mag, m
    for k in range(V.shape[0]):
        if z:
            vr, vi, wr, wi = V[k, :, 0], V[k, :, 1], w[:, 0], w[:, 1]
            out.append(one([(vr, wr, 1), (vi, wi, 1)])); out.append(one([(vr, wi, 1), (vi, wr, -1)]))
        else:
            out.append(one([(V[k], w, 1)]))
    out.append(one([(flat(w), flat(w), 1)]))
    return out


def _within(got, ref, mag, m, exact):
    err = abs(Fraction(float(got)) - ref) if exact else abs(np.longdouble(got) - ref)
    return float(err) <= 2.0 * m * 2.0 ** -53 * mag


@pytest.mark.parametrize("z,n", FLOAT_CASES, ids=[("z" if z else "d") + str(n) for z, n in FLOAT_CASES])
def test_floating_point_runs_repeat_and_meet_the_bound_of_a_sum(z, n):
    nv, V, w, h = _float_data(z, n)
    vs = 2 if z else 1
    s0, s1 = kc.strides(n, z)
    # dots: two calls, two strides
    _, a = run("dots", z, n, nv, s0, V, w)
    _, b = run("dots", z, n, nv, s0, V, w)
    _, c = run("dots", z, n, nv, s1, V, w)
    got = a[:nv * vs + 1]
    assert not np.isnan(got).any()
    assert np.array_equal(_bits(a), _bits(b)), "two calls differ"
    assert np.array_equal(_bits(a), _bits(c)), "the stride changed the bits"
    # which elements a thread sums depends on n alone: alone in the launch, first of a chunk or last of one, in the first chunk or the second -- the same bits
    for k in sorted({0, kc.GM_CHUNK - 1, nv - 1}):
        _, one = run("dots", z, n, 1, s0, np.ascontiguousarray(V[k:k + 1]), w)
        assert np.array_equal(_bits(one[:vs + 1]), _bits(np.concatenate([got[k * vs:(k + 1) * vs], got[-1:]]))), ("vector", k, "alone")
    _, none = run("dots", z, n, 0, s0, None, w)
    assert _bits(none[:1])[0] == _bits(got[-1:])[0]
    # accuracy of the sums
    exact = kc.small(n)
    for j, (ref, mag, m) in enumerate(_ref_dots(V, w, z, exact)):
        assert m == (2 * n if z else n)
        assert _within(got[j], ref, mag, m, exact), (n, z, j, float(got[j]), float(ref), mag)
    # axpys: the same for the updated vector and its norm; the norm is that of the vector that came back
    w1, r1 = run("axpys", z, n, nv, s0, V, w, h)
    w2, r2 = run("axpys", z, n, nv, s0, V, w, h)
    w3, r3 = run("axpys", z, n, nv, s1, V, w, h)
    assert not np.isnan(w1).any() and not np.isnan(r1[0])
    assert np.array_equal(_bits(w1), _bits(w2)) and _bits(r1[:1])[0] == _bits(r2[:1])[0], "two calls differ"
    assert np.array_equal(_bits(w1), _bits(w3)) and _bits(r1[:1])[0] == _bits(r3[:1])[0], "the stride changed the bits"
    if exact:
        ref, mag = _sum_exactly(Fraction(float(t)) ** 2 for t in w1), float((w1.astype(np.longdouble) ** 2).sum())
    else:
        ref = mag = (w1.astype(np.longdouble) ** 2).sum()
    assert _within(r1[0], ref, float(mag), 2 * n if z else n, exact), (n, z, "norm of the updated w", r1[0], float(ref))
    # ... and the update itself against longdouble: each element is a chain of nv (complex16: 2 nv) fused multiply-adds
    L = np.longdouble
    if z:
        Vc, hc, wc = V[..., 0].astype(L) + 1j * V[..., 1].astype(L), h[:, 0].astype(L) + 1j * h[:, 1].astype(L), w[:, 0].astype(L) + 1j * w[:, 1].astype(L)
        upd = wc - (Vc * hc[:, None]).sum(axis=0)
        refw = np.stack([upd.real, upd.imag], axis=-1).reshape(-1)
        magw = (np.abs(w).sum(axis=-1) + (np.abs(V).sum(axis=-1) * np.abs(h).sum(axis=-1)[:, None]).sum(axis=0)).repeat(2)
    else:
        refw = w.astype(L) - (V.astype(L) * h.astype(L)[:, None]).sum(axis=0)
        magw = np.abs(w) + (np.abs(V) * np.abs(h)[:, None]).sum(axis=0)
    terms = vs * nv + 1
    assert np.all(np.abs(w1[:refw.size].astype(L) - refw) <= 2.0 * terms * 2.0 ** -53 * magw), (n, z, "updated w")


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    n, z = 65, False
    d = kc.dense(513, z)
    V, w, c = _f(d["V"][:, :n]), _f(d["w"][:n]), _f(d["coef"])
    ns = kc.ns_of(n, z)

    def refused(word, *a, **kw):
        rc, xout, res = call(*a, **kw)
        msg = _lib.load().sluamd_last_error().decode()
        assert rc == -1 and msg.startswith("sluamd_krylov_selftest: ") and word in msg, (a, kw, rc, msg)          # SLUAMD_EINVAL
        assert np.isnan(xout).all() and np.isnan(res).all()

    refused("nv must lie in [0, 64]", "dots", z, n, -1, ns, V, w)
    refused("nv must lie in [0, 64]", "dots", z, n, 65, ns, V, w)
    for op in ("axpys", "combine"):
        refused("nv must lie in [1, 64]", op, z, n, 0, ns, V, w, c)
        refused("nv must lie in [1, 64]", op, z, n, 65, ns, V, w, c)
    for op in ("dots", "axpys", "combine"):
        refused("vstride", op, z, n, 2, ns + 1, V, w, c)                                                        # odd
        refused("vstride", op, z, n, 2, ns - 2, V, w, c)                                                        # shorter than a vector
        refused("vstride", op, True, n, 2, 2 * n - 2, V, w, c)
    for op in ("dots", "axpys", "scale", "combine"):
        refused("n must", op, z, 0, 1, ns, V, w, c)
        refused("n must", op, z, -5, 1, ns, V, w, c)
    refused("unknown operation", 4, z, n, 1, ns, V, w, c)
    refused("unknown operation", -1, z, n, 1, ns, V, w, c)
    refused("null pointer", "dots", z, n, 1, ns, None, w)
    refused("null pointer", "axpys", z, n, 1, ns, V, w, None)
    refused("null pointer", "scale", z, n, x=None)
    rc, xout, res = call("dots", z, n, 2, ns, V, w)                                                             # ... and the same arguments, legal, run
    assert rc == 0 and not np.isnan(res[:3]).any()
