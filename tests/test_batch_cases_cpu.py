"""Batches without a GPU: the replicated symbolic structure (sluamd_symb_replicate) is `count` shifted copies of the structure of one matrix; a handle created
from it with the block-diagonal CSR factors and solves on the CPU test build with the EXISTING kernels -- the planner accepts a forest of identical trees --
and returns the exact cases' integer solutions bit for bit; the case generators of batch_cases.py check themselves in numpy."""
import numpy as np
import pytest
import batch_cases as bc
from superlu_dist_amd import _lib, driver

BC_HEADER, LB_DESCRIPTOR, BR_HEADER, UB_DESCRIPTOR = 2, 2, 3, 2


def _shifted_copy(fs, k, m, ns):
    """the flat index arrays of copy k of a one-matrix store, shifted by hand from the formats (superlu_defs.h:156-198)"""
    li = fs.Lrowind.copy(); ui = fs.Ufstnz.copy()
    for s in range(ns):
        p = int(fs.Lrowind_off[s]); nblk = li[p]; q = p + BC_HEADER
        for _ in range(nblk):
            nbrow = li[q + 1]
            li[q] += k * ns
            li[q + LB_DESCRIPTOR:q + LB_DESCRIPTOR + nbrow] += k * m
            q += LB_DESCRIPTOR + nbrow
        assert q == fs.Lrowind_off[s + 1]
        p = int(fs.Ufstnz_off[s])
        if fs.Ufstnz_off[s + 1] > p:
            nub = ui[p]; q = p + BR_HEADER
            for _ in range(nub):
                jb = fs.Ufstnz[q]; nsj = fs.xsup[jb + 1] - fs.xsup[jb]
                ui[q] += k * ns
                ui[q + UB_DESCRIPTOR:q + UB_DESCRIPTOR + nsj] += k * m
                q += UB_DESCRIPTOR + nsj
            assert q == fs.Ufstnz_off[s + 1]
    return li, ui


@pytest.mark.parametrize("unsym", [False, True])
@pytest.mark.parametrize("name", ["m40x7", "m300x2", "m100x1"])
def test_replicated_structure_is_count_shifted_copies(name, unsym):
    c = bc.exact_case(name)
    s = driver.Symbolic(c.m, c.rp, c.ci, np.arange(c.m, dtype=np.int32), relax=8, maxsup=c.maxsup, unsym=unsym)
    r = s.replicate(c.count)
    a, b = s.flat_store(values=False), r.flat_store(values=False)
    ns, m = s.nsupers, c.m
    assert (r.n, r.nsupers, r.nnzL, r.nnzU) == (m * c.count, ns * c.count, s.nnzL * c.count, s.nnzU * c.count)
    assert r.flops == s.flops * c.count
    for k in range(c.count):
        li, ui = _shifted_copy(a, k, m, ns)
        assert np.array_equal(b.xsup[k * ns:(k + 1) * ns + 1], a.xsup + k * m)
        assert np.array_equal(b.Lrowind_off[k * ns:(k + 1) * ns + 1], a.Lrowind_off + k * len(a.Lrowind))
        assert np.array_equal(b.Ufstnz_off[k * ns:(k + 1) * ns + 1], a.Ufstnz_off + k * len(a.Ufstnz))
        assert np.array_equal(b.Lnzval_off[k * ns:(k + 1) * ns + 1], a.Lnzval_off + k * s.nnzL)
        assert np.array_equal(b.Unzval_off[k * ns:(k + 1) * ns + 1], a.Unzval_off + k * s.nnzU)
        assert np.array_equal(b.Lrowind[k * len(li):(k + 1) * len(li)], li)
        assert np.array_equal(b.Ufstnz[k * len(ui):(k + 1) * len(ui)], ui)
    assert np.array_equal(r.perm_c, np.concatenate([s.perm_c + k * m for k in range(c.count)]))
    # the partition of the forest of identical trees: every copy's supernodes belong to the copy's own trees
    assert len(r.partition(2)) == ns * c.count
    # host distribution through the replicated structure = the copies' own distributions side by side
    n, rp, ci, v = bc.block_diag_csr(c)
    r.distribute_host(v); big = r.flat_store()
    for k in range(c.count):
        s.distribute_host(c.values[k]); one = s.flat_store()
        assert np.array_equal(big.Lnzval[k * s.nnzL:(k + 1) * s.nnzL], one.Lnzval) and np.array_equal(big.Unzval[k * s.nnzU:(k + 1) * s.nnzU], one.Unzval)
    r.free(); s.free()


def test_replicate_refuses_bad_arguments():
    import ctypes as C
    c = bc.exact_case("m40x7")
    s = driver.Symbolic(c.m, c.rp, c.ci, np.arange(c.m, dtype=np.int32))
    L = _lib.load()
    out = C.c_void_p()
    assert L.sluamd_symb_replicate(s._h, 0, C.byref(out)) == -1 and not out.value
    assert L.sluamd_symb_replicate(s._h, -3, C.byref(out)) == -1
    assert L.sluamd_symb_replicate(None, 2, C.byref(out)) == -1
    assert L.sluamd_symb_replicate(s._h, 2 ** 31 // c.m + 1, C.byref(out)) == -1 and b"32-bit" in L.sluamd_last_error()


@pytest.mark.parametrize("name", ["m40x7", "m100x5", "m257x3", "m300x2", "m64x33", "m100x1"])
def test_block_diagonal_solve_on_emulation_is_exact(emul, name):
    """the planner takes the forest of identical trees; the existing kernels (CPU restatement) return every block's integer solution bit for bit"""
    c = bc.exact_case(name)
    s = driver.Symbolic(c.m, c.rp, c.ci, None, relax=8, maxsup=c.maxsup)
    r = s.replicate(c.count)
    n, rp, ci, v = bc.block_diag_csr(c)
    h = driver.LUHandle.from_symbolic(r, v)
    assert h.pdgstrf3d() == 0
    x, b, _ = c.rhs(3)
    xp = np.zeros((n, 3), order="F")
    xp[r.perm_c, :] = b.reshape(n, 3)
    y = h.pdgstrs3d(xp)
    assert np.array_equal(y[r.perm_c, :], x.reshape(n, 3))
    h.destroy(); r.free(); s.free()


@pytest.mark.parametrize("name", list(bc.SHAPES))
def test_exact_cases_are_exact(name):
    c = bc.exact_case(name)
    m = c.m
    i, j = np.indices((m, m))
    for k in range(c.count):
        L, U = c.L[k], c.U[k]
        S, T = L - np.eye(m), np.triu(U, 1)
        D = np.diag(U)
        assert np.all(np.tril(L, -1) == S) and np.all(np.diag(L) == 1) and np.all(np.tril(U, -1) == 0)
        assert set(np.unique(D)) <= {1.0, 2.0, 4.0}
        assert not np.any(S @ S) and not np.any(T @ np.diag(1 / D) @ T)          # inv(L) = I - S, inv(U) = D^-1 - D^-1 T D^-1
        assert np.array_equal((np.eye(m) - S) @ L, np.eye(m))
        Ui = np.diag(1 / D) - np.diag(1 / D) @ T @ np.diag(1 / D)
        assert np.array_equal(Ui @ U, np.eye(m))
        assert np.all(Ui * 16 == np.round(Ui * 16)) and np.abs(Ui).max() <= 2          # four fractional bits
        assert np.all(c.dense[k] == np.round(c.dense[k])) and np.abs(c.dense[k]).max() < 2 ** 20
    assert c.values.shape == (c.count, c.nnz)
    for nrhs in bc.NRHS:
        x, b, bt = c.rhs(nrhs)
        assert np.all(b == np.round(b)) and np.abs(b).max() < 2 ** 30 and np.abs(bt).max() < 2 ** 30
    if c.count > 1:
        assert not np.array_equal(c.values[0], c.values[1])


def test_wide_supernode_exists_in_the_300_case():
    c = bc.exact_case("m300x2")
    s = driver.Symbolic(c.m, c.rp, c.ci, None, relax=8, maxsup=c.maxsup)
    assert np.diff(s.xsup()).max() > 64
    s.free()


def test_singular_case_first_zero_pivot():
    name, k, c0 = "m100x5", 2, 37
    c = bc.exact_case(name, singular=(k, c0))
    reg = bc.exact_case(name)
    s = driver.Symbolic(c.m, c.rp, c.ci, None, relax=8, maxsup=c.maxsup)
    assert bc.first_zero_pivot(c.dense[k], s.perm_c) == s.perm_c[c0]
    for q in range(c.count):
        assert bc.first_zero_pivot(reg.dense[q], s.perm_c) == -1
        if q != k:
            assert np.array_equal(c.dense[q], reg.dense[q])
    s.free()


@pytest.mark.parametrize("name", list(bc.SHAPES))
def test_float_cases_are_well_conditioned(name):
    c = bc.float_case(name)
    for k in range(c.count):
        assert np.linalg.cond(c.dense[k]) <= 100.0
        d = np.abs(np.diag(c.dense[k]))
        assert np.all(d > np.abs(c.dense[k]).sum(axis=1) - d)
