"""Exact cases for the Krylov kernels of the GMRES refinement (superlu_dist_amd/csrc/sluamd_gkernels.inc: k_gm_dots, k_gm_sum, k_gm_axpys, k_gm_scale,
k_gm_combine) as sluamd_krylov_selftest runs them; test helper for test_krylov_cases_cpu.py and test_gpu_krylov_kernels.py, not a conftest.

Data.  Entries of V, w and u are integers in -3..3, complex16 entries Gaussian integers with both parts in -3..3, coefficients nonzero integers in -3..3
(a zero coefficient would hide its vector).  Every product, partial sum and result is then an integer far below 2^53 (test_krylov_cases_cpu.py asserts it
from the sums of absolute values, which bound every partial sum in every order), so fp64 gives the integer result whatever the order of summation, with or
without fused multiply-adds, and the comparisons are numpy.array_equal.  Expected values come from `expected_*` in integer arithmetic: dt = numpy.int64, or
dt = object, which makes numpy do the same arithmetic on Python integers.

Two kinds of data:
  dense   pseudo-random, seeded by (precision, order); the vectors of a smaller nv are the first of a larger one.
  probes  w = e_i against index-coded V, v_k[i] = ((i + 3 k) mod 7) - 3 (+ i ((2 i + k) mod 5 - 2) for complex16): coefficient k comes back as conj(v_k[i]) and
          so names the element that was read, and ||w||^2 = 1 says that it was read once.  The positions i: `probes`.

Arrays.  double: (n,) and (nv, n); complex16: (n, 2) and (nv, n, 2), last axis (re, im) -- as float64 that is the memory layout of the library's complex16.
One unit = 16 bytes = PER[z] values: two doubles or one complex16."""
import functools
import os
import re
import numpy as np

GM_BLOCK, GM_GRID, GM_CHUNK = 256, 1024, 8                      # restated from sluamd_gkernels.inc (test_krylov_cases_cpu.py compares)
WAVE = 64
MAX_NV = 64                                                     # GM_MAX_RESTART of sluamd_gmres.cpp
SWEEP = GM_GRID * GM_BLOCK                                      # units in one pass of the grid: beyond it the grid-stride loops wrap
PER = {False: 2, True: 1}
OPS = {"dots": 0, "axpys": 1, "scale": 2, "combine": 3}         # SLUAMD_KRYLOV_*

# the smallest orders at which each boundary of gm_blocks, k_gm_sum and the grid-stride loops exists
ORDERS = {False: (1, 2, 3, 127, 128, 129, 511, 512, 513, 1025, 131072, 131074, 524287, 524288, 524289, 524288 + 4097),
          True: (1, 63, 64, 65, 255, 256, 257, 65536, 65537, 262143, 262145, 262144 + 2049)}
SMALL_MAX = 1025
BIG_NV_ORDERS = (257, 513)                                      # both in both precisions
BIG_NV = (16, 17, 63, 64)


def small(n):
    return n <= SMALL_MAX


def orders(z, large=None):
    return tuple(n for n in ORDERS[z] if large is None or large != small(n))


def nvs(op, z, n):
    """the nv of an operation at an order that is in ORDERS[z] (BIG_NV comes on top at BIG_NV_ORDERS)"""
    lo = 0 if op == "dots" else 1
    base = tuple(range(lo, 10)) if small(n) else tuple(v for v in (0, 1, 8) if v >= lo)
    return base + (BIG_NV if n in BIG_NV_ORDERS else ())


def max_nv(n):
    return MAX_NV if n in BIG_NV_ORDERS else 9 if small(n) else 8


def ns_of(n, z):
    """doubles of one padded vector"""
    return 2 * n if z else n + (n & 1)


def nu_of(n, z):
    return ns_of(n, z) // 2


def strides(n, z):
    return (ns_of(n, z), ns_of(n, z) + 6)


def gm_blocks(nu):
    return min(GM_GRID, max(1, (nu + GM_BLOCK - 1) // GM_BLOCK))


def constants_in_source():
    """GM_BLOCK, GM_GRID, GM_CHUNK as the kernels' file defines them, GM_MAX_RESTART from their caller"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "superlu_dist_amd", "csrc")
    inc = open(os.path.join(csrc, "sluamd_gkernels.inc")).read()
    out = {k: int(re.search(r"^#define\s+%s\s+(\d+)" % k, inc, flags=re.M).group(1)) for k in ("GM_BLOCK", "GM_GRID", "GM_CHUNK")}
    out["GM_MAX_RESTART"] = int(re.search(r"GM_MAX_RESTART\s*=\s*(\d+)\s*;", open(os.path.join(csrc, "sluamd_gmres.cpp")).read()).group(1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------------------------------------------------------
def probe_classes(n, z):
    """{class: value index} for the classes that exist at this order.  The classes are positions of UNITS in the launch (thread t of workgroup b takes the
    units b GM_BLOCK + t, + SWEEP, ...); of a unit of two doubles the probe is the second value where the unit ends something and the first where it starts
    something, so that 127 | 128 and 511 | 512 are neighbours in memory"""
    per, nu = PER[z], nu_of(n, z)
    first_of = lambda unit: unit * per
    last_of = lambda unit: min(unit * per + per - 1, n - 1)       # (the second half of the last unit of an odd double vector is the pad)
    out = {"first": 0, "last": n - 1}
    if nu >= WAVE:
        out["wave0_last"] = last_of(WAVE - 1)
    if nu > WAVE:
        out["wave1_first"] = first_of(WAVE)
    if nu >= GM_BLOCK:
        out["wg0_last"] = last_of(GM_BLOCK - 1)
    if nu > GM_BLOCK:
        out["wg1_first"] = first_of(GM_BLOCK)
    if nu > GM_BLOCK * GM_BLOCK:                                # the partial of workgroup GM_BLOCK is the first that k_gm_sum's own loop wraps to
        out["sum_wrap_before"] = last_of(GM_BLOCK * GM_BLOCK - 1)
        out["sum_wrap_after"] = first_of(GM_BLOCK * GM_BLOCK)
    if nu >= SWEEP:
        out["grid_wrap_before"] = last_of(SWEEP - 1)
    if nu > SWEEP:
        out["grid_wrap_after"] = first_of(SWEEP)
    if not z and n & 1:
        out["next_to_pad"] = n - 1
    assert all(0 <= i < n for i in out.values()), (n, z, out)
    return out


def probes(n, z):
    return sorted(set(probe_classes(n, z).values()))


def coded(i, k, z):
    """v_k[i] of the index-coded basis, i and k arrays or integers: (re, im) for complex16"""
    re_ = (i + 3 * k) % 7 - 3
    return (re_, (2 * i + k) % 5 - 2) if z else re_


@functools.lru_cache(maxsize=2)
def coded_basis(n, z):
    """index-coded V with max_nv(n) vectors, int8"""
    i, k = np.arange(n, dtype=np.int64)[None, :], np.arange(max_nv(n), dtype=np.int64)[:, None]
    c = coded(i, k, z)
    return (np.stack(c, axis=-1) if z else c).astype(np.int8)


def unit_vector(n, z, i):
    w = np.zeros((n, 2) if z else (n,), dtype=np.int8)
    w[(i, 0) if z else i] = 1
    return w


def probe_expected(i, nv, z):
    """(coefficients [nv] or [nv, 2], ||w||^2) that w = e_i must return: conj(v_k[i])"""
    k = np.arange(nv, dtype=np.int64)
    c = coded(np.int64(i), k, z)
    return (np.stack([c[0], -c[1]], axis=-1) if z else c), 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# dense data
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def dense(n, z):
    """dict(V [max_nv(n), n(, 2)], w, u [n(, 2)], coef [MAX_NV(, 2)]), int8"""
    rng = np.random.default_rng(7919 * n + (1 if z else 0))
    tail = (2,) if z else ()
    nz = np.array([-3, -2, -1, 1, 2, 3], dtype=np.int8)
    return dict(V=rng.integers(-3, 4, size=(max_nv(n), n) + tail, dtype=np.int8), w=rng.integers(-3, 4, size=(n,) + tail, dtype=np.int8),
                u=rng.integers(-3, 4, size=(n,) + tail, dtype=np.int8), coef=nz[rng.integers(0, 6, size=(MAX_NV,) + tail)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# expected values: integer arithmetic in dt (numpy.int64, or object = Python integers)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _parts(a, z, dt):
    a = np.asarray(a).astype(dt)
    return (a[..., 0], a[..., 1]) if z else (a, None)


def _join(re_, im, z):
    return np.stack([re_, im], axis=-1) if z else re_


def _lincomb(V, c, z, dt):
    """sum_k v_k c_k as (re, im)"""
    vr, vi = _parts(V, z, dt)
    cr, ci = _parts(c, z, dt)
    n = vr.shape[1]
    if not z:
        return (vr * cr[:, None]).sum(axis=0) if len(cr) else np.zeros(n, dtype=dt), None
    if not len(cr):
        return np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
    return (vr * cr[:, None] - vi * ci[:, None]).sum(axis=0), (vr * ci[:, None] + vi * cr[:, None]).sum(axis=0)


def _norm2(re_, im):
    return (re_ * re_).sum() + (0 if im is None else (im * im).sum())


def expected_dots(V, w, z, dt=np.int64):
    """(v_k^H w for every k, ||w||^2)"""
    vr, vi = _parts(V, z, dt)
    wr, wi = _parts(w, z, dt)
    if not z:
        return (vr * wr[None, :]).sum(axis=1), _norm2(wr, None)
    return _join((vr * wr[None, :] + vi * wi[None, :]).sum(axis=1), (vr * wi[None, :] - vi * wr[None, :]).sum(axis=1), True), _norm2(wr, wi)


def expected_axpys(V, w, h, z, dt=np.int64):
    """(w - sum_k v_k h_k, the ||.||^2 of that)"""
    sr, si = _lincomb(V, h, z, dt)
    wr, wi = _parts(w, z, dt)
    nr, ni = wr - sr, (wi - si if z else None)
    return _join(nr, ni, z), _norm2(nr, ni)


def expected_combine(V, u, y, add, z, dt=np.int64):
    """(add ? u : 0) + sum_k v_k y_k"""
    sr, si = _lincomb(V, y, z, dt)
    ur, ui = _parts(u, z, dt)
    return _join(sr + ur, si + ui if z else None, z) if add else _join(sr, si, z)


def magnitude_bounds(V, w, u, c, z):
    """int64 bounds on every partial sum an order of summation can meet: (dots: sum |v||w| per k and sum |w|^2, both over re and im parts together;
    axpys / combine: max_i (|x_i| + sum_k |v_k,i| |c_k|), parts added; the norm of the updated w: n (that maximum)^2)"""
    def a(x):                                                   # |re| + |im|: |parts of v c| <= a(v) a(c)
        x = np.abs(np.asarray(x).astype(np.int64))
        return x.sum(axis=-1) if z else x
    aV, aw, au, ac = a(V), a(w), a(u), a(c)
    dots = int(max([int((aV * aw[None, :]).sum(axis=1).max()) if len(aV) else 0, int((aw * aw).sum())]))
    elem = int((np.maximum(aw, au) + (aV * ac[:len(aV), None]).sum(axis=0)).max())
    return dots, elem, len(aw) * elem * elem


def padded(x, n, z):
    """the values of a vector as the float64 words of its padded device layout: ns doubles, the pad of an odd double vector 0.0"""
    out = np.zeros(ns_of(n, z), dtype=np.float64)
    flat = np.asarray(x).reshape(-1)
    out[:flat.size] = flat
    return out
