"""What test_gpu_krylov_kernels.py relies on, by numpy and Python integers alone (tests/krylov_cases.py): the constants restated there are those of the
kernels' source; the orders sit on every boundary of gm_blocks, k_gm_sum and the grid-stride loops; the probe positions reach every class of position in the
launch that exists at an order; the nv cross the chunk boundaries and reach the last dot slot; every expected value is the same in int64 and in Python
integers, and every partial sum any order of summation can meet is an integer below 2^53 (the dots below 2^25), so fp64 is exact on these data."""
import numpy as np
import pytest
import krylov_cases as kc

ZN = [(z, n) for z in (False, True) for n in kc.ORDERS[z]] + [(z, n) for z in (False, True) for n in kc.BIG_NV_ORDERS if n not in kc.ORDERS[z]]
IDS = [("z" if z else "d") + str(n) for z, n in ZN]


def test_constants_are_those_of_the_source():
    src = kc.constants_in_source()
    assert src == dict(GM_BLOCK=kc.GM_BLOCK, GM_GRID=kc.GM_GRID, GM_CHUNK=kc.GM_CHUNK, GM_MAX_RESTART=kc.MAX_NV), src
    assert kc.GM_BLOCK == 4 * kc.WAVE and kc.SWEEP == kc.GM_GRID * kc.GM_BLOCK


@pytest.mark.parametrize("z", [False, True], ids=["d", "z"])
def test_orders_sit_on_the_boundaries(z):
    nus = {kc.nu_of(n, z) for n in kc.ORDERS[z]}
    blocks = {kc.gm_blocks(nu) for nu in nus}
    assert 1 in nus                                                                          # one unit, one thread
    assert {kc.WAVE, kc.WAVE + 1} <= nus and {kc.GM_BLOCK, kc.GM_BLOCK + 1} <= nus           # a full wave | a second wave; a full workgroup | a second one
    assert {1, 2, kc.GM_BLOCK, kc.GM_BLOCK + 1, kc.GM_GRID} <= blocks                        # k_gm_sum: one partial, two, a full pass of its loop, a wrapped one
    assert (kc.SWEEP in nus or kc.SWEEP - 1 in nus) and kc.SWEEP + 1 in nus                  # no unit wraps | the first wrapped unit
    assert any(nu > kc.SWEEP + kc.GM_BLOCK for nu in nus)                                    # more than one workgroup wraps
    if not z:                                                                                # half-filled last units beside every boundary
        odd = {n for n in kc.ORDERS[z] if n & 1}
        assert {1, 2 * kc.WAVE - 1, 2 * kc.WAVE + 1, 2 * kc.GM_BLOCK - 1, 2 * kc.GM_BLOCK + 1, 2 * kc.SWEEP - 1, 2 * kc.SWEEP + 1} <= odd
        assert max(kc.ORDERS[z]) & 1
    for n in kc.BIG_NV_ORDERS:
        assert kc.small(n) and kc.nu_of(n, z) > kc.WAVE                                      # the long bases run on more than one wave


def _where(i, z):
    """(sweep, workgroup, thread) of the unit that holds value i"""
    u = i // kc.PER[z]
    return u // kc.SWEEP, (u % kc.SWEEP) // kc.GM_BLOCK, u % kc.GM_BLOCK


@pytest.mark.parametrize("z,n", ZN, ids=IDS)
def test_probes_reach_every_class_of_position(z, n):
    nu, P = kc.nu_of(n, z), kc.probes(n, z)
    at = {_where(i, z) for i in P}
    assert all(0 <= i < n for i in P) and 0 in P and n - 1 in P
    want = set()
    if nu >= kc.WAVE:
        want.add((0, 0, kc.WAVE - 1))
    if nu > kc.WAVE:
        want.add((0, 0, kc.WAVE))
    if nu >= kc.GM_BLOCK:
        want.add((0, 0, kc.GM_BLOCK - 1))
    if nu > kc.GM_BLOCK:
        want.add((0, 1, 0))
    if kc.gm_blocks(nu) > kc.GM_BLOCK:                                                       # k_gm_sum's thread 0 takes the partials 0 and GM_BLOCK
        want |= {(0, kc.GM_BLOCK - 1, kc.GM_BLOCK - 1), (0, kc.GM_BLOCK, 0)}
    if nu >= kc.SWEEP:
        want.add((0, kc.GM_GRID - 1, kc.GM_BLOCK - 1))
    if nu > kc.SWEEP:
        want.add((1, 0, 0))
    assert want <= at, (want - at, P)
    if not z:                                                                                # neighbours in memory, not only in units
        for b in (kc.WAVE, kc.GM_BLOCK, kc.SWEEP):
            if n > 2 * b:
                assert 2 * b - 1 in P and 2 * b in P
        if n & 1:                                                                            # the value that shares its unit with the pad
            assert (n - 1) % 2 == 0 and (n - 1) // 2 == nu - 1 and n - 1 in P
    if z:                                                                                    # pairs with conj(v) w != v conj(w): a coefficient with an imaginary part
        assert any(kc.probe_expected(i, kc.max_nv(n), z)[0][:, 1].any() for i in P)


def test_nv_cross_the_chunks_and_reach_the_last_slot():
    for z in (False, True):
        for n in kc.ORDERS[z]:
            for op in ("dots", "axpys", "combine"):
                v = kc.nvs(op, z, n)
                assert min(v) == (0 if op == "dots" else 1) and max(v) <= kc.max_nv(n) <= kc.MAX_NV
                assert {1, kc.GM_CHUNK} <= set(v)
                if kc.small(n):
                    assert set(range(1, kc.GM_CHUNK + 2)) <= set(v)                          # every instantiation NV = 1 .. 8, and one vector into the second chunk
    assert {2 * kc.GM_CHUNK, 2 * kc.GM_CHUNK + 1, kc.MAX_NV - 1, kc.MAX_NV} <= set(kc.BIG_NV)   # whole chunks, a chunk of one, seven chunks + 7, eight whole chunks
    for z in (False, True):
        for n in kc.BIG_NV_ORDERS:
            if n in kc.ORDERS[z]:
                assert set(kc.BIG_NV) <= set(kc.nvs("dots", z, n)) and set(kc.BIG_NV) <= set(kc.nvs("combine", z, n))
    # complex16, nv = 64: the imaginary part of the last coefficient lies in the slot right below the one of ||w||^2 (GM_SLOT_NDOT = 2 GM_MAX_RESTART)
    assert 2 * (kc.MAX_NV - 1) + 1 == 2 * kc.MAX_NV - 1


def _same(a, b):
    """an int64 result and a result in Python integers (object array) hold the same numbers; the conversion raises where a Python integer does not fit"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.astype(np.int64), b.astype(np.int64))


@pytest.mark.parametrize("z,n", ZN, ids=IDS)
def test_expected_values_in_int64_and_in_python_integers(z, n):
    d = kc.dense(n, z)
    for a in (d["V"], d["w"], d["u"]):
        assert a.min() >= -3 and a.max() <= 3
    assert np.abs(d["coef"]).min() >= 1 and np.abs(d["coef"]).max() <= 3
    nvs = sorted(set(kc.nvs("dots", z, n)) | set(kc.BIG_NV if n in kc.BIG_NV_ORDERS else ()))
    top = max(nvs)
    dots_b, elem_b, norm_b = kc.magnitude_bounds(d["V"][:top], d["w"], d["u"], d["coef"], z)
    print(n, z, "bounds: dots", dots_b, "element", elem_b, "norm of the updated w", norm_b)
    assert dots_b < 2 ** 25 and elem_b < 2 ** 53 and norm_b < 2 ** 53
    for nv in (nvs if kc.small(n) else (0, top)):                                            # (large orders: nv = 1 is a prefix of nv = 8 in the dots)
        V, c = d["V"][:nv], d["coef"][:nv]
        got = {}
        for dt in (np.int64, object):
            got[dt] = (kc.expected_dots(V, d["w"], z, dt),) + ((kc.expected_axpys(V, d["w"], c, z, dt), kc.expected_combine(V, d["u"], c, 0, z, dt),
                                                                 kc.expected_combine(V, d["u"], c, 1, z, dt)) if nv else ())
        a, b = got[np.int64], got[object]
        assert _same(a[0][0], b[0][0]) and int(a[0][1]) == int(b[0][1])
        assert max([abs(int(a[0][1]))] + [abs(int(x)) for x in np.asarray(a[0][0]).reshape(-1)]) <= dots_b
        if nv:
            assert _same(a[1][0], b[1][0]) and int(a[1][1]) == int(b[1][1]) and _same(a[2], b[2]) and _same(a[3], b[3])
            assert int(np.abs(a[1][0]).max()) <= elem_b and int(np.abs(a[3]).max()) <= elem_b and 0 <= int(a[1][1]) <= norm_b
            assert not _same(a[2], a[3])                                                     # `add` makes a difference
        if z and nv == top:                                                                  # conj(v) w != v conj(w) for most of the vectors
            assert 2 * np.count_nonzero(np.asarray(a[0][0])[:, 1]) > nv


@pytest.mark.parametrize("z,n", ZN, ids=IDS)
def test_probe_expectations(z, n):
    """the coefficient a probe must return, three ways: the closed form, the int64 dot products with the index-coded basis, the formula in Python integers"""
    nv = kc.max_nv(n)
    V = kc.coded_basis(n, z)
    assert V.min() >= -3 and V.max() <= 3
    for i in kc.probes(n, z):
        coef, nrm = kc.probe_expected(i, nv, z)
        full, fnrm = kc.expected_dots(V, kc.unit_vector(n, z, i), z)
        assert np.array_equal(coef, full) and int(fnrm) == nrm == 1
        for k in range(nv):
            py = ((int(i) + 3 * k) % 7 - 3, -((2 * int(i) + k) % 5 - 2)) if z else (int(i) + 3 * k) % 7 - 3
            assert (tuple(int(x) for x in coef[k]) if z else int(coef[k])) == py
    # neighbours are told apart: the codes of i and i + 1 differ in every vector
    i = np.arange(n - 1, dtype=np.int64)
    a, b = kc.coded(i, np.int64(0), z), kc.coded(i + 1, np.int64(0), z)
    assert np.all((a[0] != b[0]) if z else (a != b))
