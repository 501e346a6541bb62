"""Properties of the LargeDiag_MC64 test cases and of the numpy restatement in rowperm_cases.py that test_gpu_rowperm.py relies on -- no GPU: the optimum
of the small cases by brute force, uniqueness, the counters the proposal rule fixes, augmenting paths of positive length, the exact certificate, and the
driver's host-side row permutation of a CSR."""
import functools
import numpy as np
import pytest
import rowperm_cases as rc
from superlu_dist_amd import driver


@functools.lru_cache(maxsize=None)
def _ref(name, host_only=False):
    n, rp, ci, v = rc.case(name)
    return n, rp, ci, v, rc.large_diag_ref(n, rp, ci, v, host_only=host_only)


@pytest.mark.parametrize("name", sorted(rc.EXACT))
def test_exact_certificate_of_the_restatement(name):
    n, rp, ci, v, d = _ref(name)
    assert d["info"] == 0 and sorted(d["perm_r"]) == list(range(n))
    assert np.all(np.isinf(d["cost"]) | (d["cost"] == np.floor(d["cost"])))                # integer costs
    for s in (d["r"], d["c"]):
        assert np.all(np.frexp(s)[0] == 0.5)                                                # powers of two
    assert rc.certificate(n, rp, ci, v, d["perm_r"], d["r"], d["c"]) == (0.0, 0.0)
    h = _ref(name, True)[4]
    assert (h["rounds"], h["matched_device"], h["augmentations"]) == (0, 0, n)
    assert rc.objective(n, rp, ci, d["cost"], h["perm_r"]) == rc.objective(n, rp, ci, d["cost"], d["perm_r"])
    assert rc.certificate(n, rp, ci, v, h["perm_r"], h["r"], h["c"]) == (0.0, 0.0)
    if name in rc.UNIQUE:
        assert np.array_equal(h["perm_r"], d["perm_r"])


@pytest.mark.parametrize("name", ["n1", "antidiag2", "rand8", "pospath3", "z_rand8"])
def test_small_optimum_is_unique_by_brute_force(name):
    A = rc.EXACT[name]()
    best, perms = rc.brute_force(A)
    assert len(perms) == 1 and name in rc.UNIQUE
    n, rp, ci, v, d = _ref(name)
    assert np.array_equal(d["perm_r"], perms[0])
    assert rc.objective(n, rp, ci, d["cost"], d["perm_r"]) == best


def test_block_cases_inherit_uniqueness():
    """blocks130 / pospath66 are block diagonal: a perfect matching matches inside the blocks, so the optimum is unique when the block's is"""
    for B in ([[2, 2], [2, 0]], rc.POSPATH3):
        assert len(rc.brute_force(np.array(B, dtype=float))[1]) == 1


@pytest.mark.parametrize("n", [64, 65, 257])
def test_cyclic_shift_dominates(n):
    """every shift entry is strictly the largest of its row and of its column: the shift is the only matching of cost 0, hence the unique optimum, and
    only the shift entries are tight, so the proposal rounds match every row"""
    A = np.abs(rc._cyclic(n))
    sh = A[np.arange(n), (np.arange(n) + 1) % n]
    B = A.copy(); B[np.arange(n), (np.arange(n) + 1) % n] = 0
    assert np.all(sh > B.max(axis=1)) and np.all(sh[(np.arange(n) - 1) % n] > B.max(axis=0))


@pytest.mark.parametrize("name", rc.ALL_ON_DEVICE)
def test_cyclic_is_matched_by_the_rounds(name):
    n, rp, ci, v, d = _ref(name)
    assert (d["matched_device"], d["augmentations"], d["rounds"]) == (n, 0, 1)
    assert np.array_equal(d["perm_r"], (np.arange(n) + 1) % n)


@pytest.mark.parametrize("name", ["blocks130", "z_blocks130"])
def test_blocks_counters(name):
    n, rp, ci, v, d = _ref(name)
    assert (d["matched_device"], d["augmentations"], d["rounds"]) == (65, 65, 2)
    assert np.array_equal(d["perm_r"], np.arange(n) ^ 1)            # row 0 -> column 1, row 1 -> column 0 of every block


@pytest.mark.parametrize("name", rc.POSITIVE_PATH)
def test_positive_path_length(name):
    n, rp, ci, v, d = _ref(name)
    assert d["augmentations"] > 0 and max(d["path_lengths"]) > 0
    u0 = rc.large_diag_ref(n, rp, ci, v, max_rounds=0)              # (the same initial duals)
    assert not np.array_equal(d["u"], np.minimum.reduceat(d["cost"], rp[:-1]))   # the duals moved on the host
    assert u0["info"] == 0


@pytest.mark.parametrize("name", rc.SINGULAR)
def test_singular(name):
    n, rp, ci, v, info = rc.singular(name)
    for host_only in (False, True):
        d = rc.large_diag_ref(n, rp, ci, v, host_only=host_only)
        assert d["info"] == info and d["perm_r"] is None


def test_general300():
    n, rp, ci, v = rc.general300()
    assert np.all(rc.dense_from_csr(n, rp, ci, v).diagonal() == 0) and len(ci) > 8 * n
    d = rc.large_diag_ref(n, rp, ci, v)
    h = rc.large_diag_ref(n, rp, ci, v, host_only=True)
    assert d["info"] == h["info"] == 0 and 0 < d["matched_device"] < n
    o1, o2 = rc.objective(n, rp, ci, d["cost"], d["perm_r"]), rc.objective(n, rp, ci, d["cost"], h["perm_r"])
    slack = rc.certificate(n, rp, ci, v, d["perm_r"], d["r"], d["c"])
    print("general300: objective", o1, o2, "matched by the rounds", d["matched_device"], "slack (all, matched)", slack)
    # two optimal matchings of one cost array: the sums of n costs differ by their rounding alone
    assert abs(o1 - o2) <= 2 * n * 2.0 ** -52 * max(o1, 1.0)
    assert max(slack) <= 1e-10


def test_permute_rows_csr():
    n, rp, ci, v = rc.general300()
    pr = np.random.default_rng(1).permutation(n).astype(np.int32)
    rp1, ci1, v1, pos = driver.permute_rows_csr(n, rp, ci, v, pr)
    A, A1 = rc.dense_from_csr(n, rp, ci, v), rc.dense_from_csr(n, rp1, ci1, v1)
    assert np.array_equal(A1[pr], A)                                 # row i of A is row perm_r[i] of Pr A
    assert np.array_equal(v1, v[pos]) and np.array_equal(ci1, ci[pos])


def test_shuffled_poisson_is_recovered_by_the_restatement():
    n, rp, ci, v, shuffle, (pn, prp, pci, pv) = rc.shuffled_poisson()
    d = rc.large_diag_ref(n, rp, ci, v)
    assert np.array_equal(d["perm_r"], shuffle) and (d["matched_device"], d["augmentations"]) == (n, 0)
    rp1, ci1, v1, _ = driver.permute_rows_csr(n, rp, ci, v, d["perm_r"])
    assert np.array_equal(rp1, prp) and np.array_equal(ci1, pci) and np.array_equal(v1, pv)
