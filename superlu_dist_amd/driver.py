"""Host-side mirror of the reference's expert-driver interface for the hot path.

Names follow the reference (SRC/double/pdgssvx3d.c:519 `pdgssvx3d`, SRC/double/pdgstrf3d.c:121 `pdgstrf3d`,
SRC/double/pdgstrs3d.c:6604 `pdgstrs3d`): Python here is only the test/bench harness above the C ABI
(include/superlu_dist_amd.h) -- all numerics run in libsluamd.so on the GPU; nothing here computes on the CPU
except permutation bookkeeping and the residual check.
"""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import LUView, ForestView, Options, Stats, P_int, P_dbl


def _pi(a):
    return a.ctypes.data_as(P_int)


def _pd(a):
    return a.ctypes.data_as(P_dbl)


class FlatStore:
    """One rank's L/U store as flat arrays + offsets over its LOCAL block columns / rows (what tests/golden holds),
    exposed to the C ABI through the reference's pointer-array view (Lrowind_bc_ptr[lk], Lnzval_bc_ptr[lk], ...)."""

    def __init__(self, n, xsup, Lrowind_off, Lrowind, Lnzval_off, Lnzval, Ufstnz_off, Ufstnz, Unzval_off, Unzval,
                 grid=(1, 1, 1), coords=(0, 0, 0)):
        self.n = int(n)
        self.xsup = np.ascontiguousarray(xsup, dtype=np.int32)
        self.nsupers = len(self.xsup) - 1
        self.Lrowind_off = np.asarray(Lrowind_off, dtype=np.int64)
        self.Lrowind = np.ascontiguousarray(Lrowind, dtype=np.int32)
        self.Lnzval_off = np.asarray(Lnzval_off, dtype=np.int64)
        self.z = bool(np.iscomplexobj(Lnzval) or np.iscomplexobj(Unzval))   # complex16 store (pzgstrf3d path)
        vt = np.complex128 if self.z else np.float64
        self.Lnzval = np.array(Lnzval, dtype=vt)
        self.Ufstnz_off = np.asarray(Ufstnz_off, dtype=np.int64)
        self.Ufstnz = np.ascontiguousarray(Ufstnz, dtype=np.int32)
        self.Unzval_off = np.asarray(Unzval_off, dtype=np.int64)
        self.Unzval = np.array(Unzval, dtype=vt)
        self.grid, self.coords = grid, coords
        self._build_view()

    @classmethod
    def from_golden(cls, g, rank=0, which="pre"):
        r = f"r{rank}__"
        grid = (int(g[r + "Pr"][0]), int(g[r + "Pc"][0]), int(g[r + "Pz"][0]))
        coords = (int(g[r + "myrow"][0]), int(g[r + "mycol"][0]), int(g[r + "myz"][0]))
        return cls(int(g[r + "n"][0]), g[r + "xsup"], g[r + "Lrowind_off"], g[r + "Lrowind"], g[r + "Lnzval_off"],
                   g[r + f"Lnzval_{which}"], g[r + "Ufstnz_off"], g[r + "Ufstnz"], g[r + "Unzval_off"],
                   g[r + f"Unzval_{which}"], grid, coords)

    def _build_view(self):
        ns = self.nsupers

        def ptrs(base, off, ctype, elem):
            nloc = len(off) - 1          # ceil(nsupers / npcol) block columns or ceil(nsupers / nprow) block rows
            arr = (C.POINTER(ctype) * max(nloc, 1))()
            addr = base.ctypes.data
            for k in range(nloc):
                if off[k + 1] > off[k]:
                    arr[k] = C.cast(addr + int(off[k]) * elem, C.POINTER(ctype))
            return arr
        self._lp = ptrs(self.Lrowind, self.Lrowind_off, C.c_int32, 4)
        self._lv = ptrs(self.Lnzval, self.Lnzval_off, C.c_double, self.Lnzval.itemsize)
        self._up = ptrs(self.Ufstnz, self.Ufstnz_off, C.c_int32, 4)
        self._uv = ptrs(self.Unzval, self.Unzval_off, C.c_double, self.Unzval.itemsize)
        v = LUView()
        v.n, v.nsupers, v.xsup = self.n, ns, _pi(self.xsup)
        v.nprow, v.npcol, v.npdep = self.grid
        v.myrow, v.mycol, v.myzlayer = self.coords
        v.Lrowind_bc_ptr = C.cast(self._lp, C.POINTER(P_int))
        v.Lnzval_bc_ptr = C.cast(self._lv, C.POINTER(P_dbl))
        v.Ufstnz_br_ptr = C.cast(self._up, C.POINTER(P_int))
        v.Unzval_br_ptr = C.cast(self._uv, C.POINTER(P_dbl))
        self.view = v


def order_nd(n, rowptr, colind, leaf=64):
    """perm_c[old] = new: nested dissection of the pattern of A + A^T without geometry (sluamd_order_nd)"""
    rp = np.ascontiguousarray(rowptr, dtype=np.int32); ci = np.ascontiguousarray(colind, dtype=np.int32)
    perm = np.zeros(n, dtype=np.int32)
    _lib.check(_lib.load().sluamd_order_nd(int(n), _pi(rp), _pi(ci), int(leaf), _pi(perm)), "sluamd_order_nd")
    return perm


def large_diag(n, rowptr, colind, nzval, scale=True, device=-1):
    """RowPerm = LargeDiag_MC64 (sluamd_[dz]LargeDiag; complex nzval takes the z form): the row permutation that maximises the product of the diagonal
    moduli.  Returns (perm_r, r, c, info): perm_r[i] = j -- row i of A is row j of Pr A, a(i, j) lands on the diagonal; r by original row and c by column
    with |r a c| <= 1 everywhere and = 1 on the matched entries (both None when scale=False); info = dict(info, rounds, matched_device, augmentations),
    info["info"] = k > 0: structurally singular, k rows unmatched, and perm_r, r, c are None."""
    rp = np.ascontiguousarray(rowptr, dtype=np.int32); ci = np.ascontiguousarray(colind, dtype=np.int32)
    z = np.iscomplexobj(nzval)
    v = np.ascontiguousarray(nzval, dtype=np.complex128 if z else np.float64)
    n = int(n)
    perm = np.full(n, -1, dtype=np.int32)
    r = np.zeros(n) if scale else None; c = np.zeros(n) if scale else None
    o = _lib.RowPerm()
    name = "sluamd_zLargeDiag" if z else "sluamd_dLargeDiag"
    _lib.check(_lib.entry(name)(int(device), n, _pi(rp), _pi(ci), v.ctypes.data_as(C.c_void_p), _pi(perm), None if r is None else _pd(r),
                                None if c is None else _pd(c), C.byref(o)), name)
    info = dict(info=int(o.info), rounds=int(o.rounds), matched_device=int(o.matched_device), augmentations=int(o.augmentations))
    if o.info > 0:
        return None, None, None, info
    return perm, r, c, info


def permute_rows_csr(n, rowptr, colind, nzval, perm_r):
    """CSR of Pr A for perm_r[i] = j (row i of A is row j of Pr A) and the position map of its values: returns (rowptr1, colind1, nzval1, pos) with
    nzval1 = nzval[pos] -- new values of the same pattern in A's order become those of Pr A by the same take."""
    rp = np.asarray(rowptr, dtype=np.int64); pr = np.asarray(perm_r, dtype=np.int64)
    n = int(n)
    inv = np.empty(n, dtype=np.int64); inv[pr] = np.arange(n)              # row k of Pr A is row inv[k] of A
    cnt = (rp[1:] - rp[:-1])[inv]
    rp1 = np.zeros(n + 1, dtype=np.int64); np.cumsum(cnt, out=rp1[1:])
    pos = np.repeat(rp[:-1][inv] - rp1[:-1], cnt) + np.arange(rp1[n])
    return rp1.astype(np.int32), np.ascontiguousarray(np.asarray(colind)[pos], dtype=np.int32), np.ascontiguousarray(np.asarray(nzval)[pos]), pos


class Symbolic:
    """sluamd_dsymbfact result (our symbfact_dist + pddistribute3d stand-in for a 1x1 layer)."""

    def __init__(self, n, rowptr, colind, perm_c=None, relax=32, maxsup=256, unsym=False):
        """unsym=True: sluamd_dsymbfact_unsym -- the exact unsymmetric structure with the reference's supernode rules (symbfact.c)"""
        L = _lib.load()
        self.n = int(n)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.colind = np.ascontiguousarray(colind, dtype=np.int32)
        self.perm_c = np.empty(self.n, dtype=np.int32)
        pin = None if perm_c is None else np.ascontiguousarray(perm_c, dtype=np.int32)
        self._h = C.c_void_p()
        fn = L.sluamd_dsymbfact_unsym if unsym else L.sluamd_dsymbfact
        _lib.check(fn(C.byref(self._h), self.n, _pi(self.rowptr), _pi(self.colind),
                      None if pin is None else _pi(pin), relax, maxsup, _pi(self.perm_c)), "sluamd_dsymbfact")
        ns = C.c_int32(); nl = C.c_int64(); nu = C.c_int64(); li = C.c_int64(); ui = C.c_int64(); fl = C.c_double()
        L.sluamd_symb_info(self._h, C.byref(ns), C.byref(nl), C.byref(nu), C.byref(li), C.byref(ui), C.byref(fl))
        self.nsupers, self.nnzL, self.nnzU, self.flops = ns.value, nl.value, nu.value, fl.value
        self.lidx_len, self.uidx_len = li.value, ui.value

    def replicate(self, count):
        """The Symbolic of diag(A, ..., A) with `count` copies of this pattern, matrix-major (sluamd_symb_replicate): no symbolic factorisation runs"""
        L = _lib.load()
        count = int(count)
        out = C.c_void_p()
        _lib.check(L.sluamd_symb_replicate(self._h, count, C.byref(out)), "sluamd_symb_replicate")
        r = Symbolic.__new__(Symbolic)
        nnz = len(self.colind)
        r.n = self.n * count
        r.rowptr = np.concatenate([self.rowptr[:-1] + k * nnz for k in range(count)] + [[count * nnz]]).astype(np.int32)
        r.colind = np.concatenate([self.colind + k * self.n for k in range(count)]).astype(np.int32)
        r.perm_c = np.concatenate([self.perm_c + k * self.n for k in range(count)]).astype(np.int32)
        r._h = out
        ns = C.c_int32(); nl = C.c_int64(); nu = C.c_int64(); li = C.c_int64(); ui = C.c_int64(); fl = C.c_double()
        L.sluamd_symb_info(r._h, C.byref(ns), C.byref(nl), C.byref(nu), C.byref(li), C.byref(ui), C.byref(fl))
        r.nsupers, r.nnzL, r.nnzU, r.flops = ns.value, nl.value, nu.value, fl.value
        r.lidx_len, r.uidx_len = li.value, ui.value
        return r

    def distribute_host(self, nzval):
        L = _lib.load()
        nz = np.ascontiguousarray(nzval, dtype=np.float64)
        _lib.check(L.sluamd_ddistribute_host(self._h, _pi(self.rowptr), _pi(self.colind), _pd(nz), _pi(self.perm_c)),
                   "sluamd_ddistribute_host")

    def xsup(self):
        xs = np.empty(self.nsupers + 1, dtype=np.int32)
        _lib.check(_lib.load().sluamd_symb_export(self._h, _pi(xs), None, None, None, None, None, None, None, None), "sluamd_symb_export")
        return xs

    def grid_footprint(self, Pr, Pc, Pz, sn_tree=None):
        """stored factor values / replicated values / index entries per world rank of a Pr x Pc x Pz grid (sluamd_symb_grid_footprint)"""
        P = Pr * Pc * Pz
        vals, rep, idx = (np.zeros(P, dtype=np.int64) for _ in range(3))
        t = None if sn_tree is None else np.ascontiguousarray(sn_tree, dtype=np.int32)
        p64 = C.POINTER(C.c_int64)
        _lib.check(_lib.load().sluamd_symb_grid_footprint(self._h, Pr, Pc, Pz, None if t is None else _pi(t), vals.ctypes.data_as(p64),
                                                          rep.ctypes.data_as(p64), idx.ctypes.data_as(p64)), "sluamd_symb_grid_footprint")
        return vals, rep, idx

    def partition(self, npdep):
        """Tree id (heap order) of every supernode for a 1 x 1 x npdep grid."""
        t = np.zeros(self.nsupers, dtype=np.int32)
        _lib.check(_lib.load().sluamd_symb_partition(self._h, npdep, _pi(t)), "sluamd_symb_partition")
        return t

    def flat_store(self, values=True):
        """Copy the host store out as a FlatStore (tests / CPU-baseline harness)."""
        L = _lib.load()
        ns = self.nsupers
        xsup = np.empty(ns + 1, dtype=np.int32)
        lo = np.empty(ns + 1, dtype=np.int64); lvo = np.empty(ns + 1, dtype=np.int64)
        uo = np.empty(ns + 1, dtype=np.int64); uvo = np.empty(ns + 1, dtype=np.int64)
        li = np.empty(self.lidx_len, dtype=np.int32); ui = np.empty(self.uidx_len, dtype=np.int32)
        lv = np.zeros(self.nnzL if values else 0); uv = np.zeros(self.nnzU if values else 0)
        P64 = C.POINTER(C.c_int64)
        p64 = lambda a: a.ctypes.data_as(P64)
        _lib.check(L.sluamd_symb_export(self._h, _pi(xsup), p64(lo), _pi(li), p64(lvo), _pd(lv) if values else None,
                                        p64(uo), _pi(ui), p64(uvo), _pd(uv) if values else None), "sluamd_symb_export")
        if not values:
            lv = np.zeros(self.nnzL); uv = np.zeros(self.nnzU)
        return FlatStore(self.n, xsup, lo, li, lvo, lv, uo, ui, uvo, uv)

    def free(self):
        if self._h:
            _lib.load().sluamd_symb_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


PLAN_COLS = 20


def plan_table(h):
    L = _lib.load()
    rows = C.c_int64(0)
    _lib.check(L.sluamd_plan_table(h, None, 0, C.byref(rows)), "sluamd_plan_table")
    out = np.zeros((max(rows.value, 1), PLAN_COLS))
    _lib.check(L.sluamd_plan_table(h, out.ctypes.data_as(C.POINTER(C.c_double)), rows.value, C.byref(rows)), "sluamd_plan_table")
    return out[:rows.value]


XLISTS = ("xs_red_send", "xs_red_recv", "xs_bc_send", "xs_bc_recv", "xt_red_send", "xt_red_recv", "xt_bc_send", "xt_bc_recv")


def plan_xlists(h, which):
    """this rank's x-segment exchange list `which` (a name of XLISTS: xs_* = the untransposed sweeps, xt_* = the transposed ones) as an int array of
    rows (Z level, DAG level, peer, first row, rows), one per run in list order (sluamd_plan_xlists)"""
    L = _lib.load()
    w = XLISTS.index(which)
    rows = C.c_int64(0)
    _lib.check(L.sluamd_plan_xlists(h, w, None, 0, C.byref(rows)), "sluamd_plan_xlists")
    out = np.zeros((max(rows.value, 1), 5), dtype=np.int32)
    _lib.check(L.sluamd_plan_xlists(h, w, _pi(out), rows.value, C.byref(rows)), "sluamd_plan_xlists")
    return out[:rows.value]


class LUHandle:
    """Device-resident L/U (sluamd_handle_t): dCreateLUgpuHandle / pdgstrf3d_LUv1 / dCopyLUGPU2Host /
    dDestroyLUgpuHandle replacement (SRC/CplusplusFactor/LUgpuCHandle_interface_impl.cu:11-73)."""

    def __init__(self, h, store=None):
        self._h = h
        self.store = store
        self.z = False
        self.n = None if store is None else store.n       # order of the matrix (from_symbolic sets it)
        self.nnz = None                                   # entries of the CSR the handle was created from (from_symbolic sets it)
        self.device = -1                                  # HIP device ordinal given at creation (-1: the device that was current)
        self.rowperm_pos = None                           # pdgssvx3d(rowperm=...): the handle was made from Pr A; values in A's order go through this map
        self.refine_rho = None                            # pdgsrfs3d(method="extra"): per column the largest ratio of successive corrections of the last call
        self.attached_nnz = None                          # entries of the matrix attach_matrix attached (adjoint_values returns that many); None: self.nnz

    @staticmethod
    def _opts(replace_tiny=False, deterministic=False, device=-1, info_rule=0):
        o = Options()
        _lib.load().sluamd_default_options(C.byref(o))
        o.device = device; o.replace_tiny_pivot = int(replace_tiny); o.deterministic = int(deterministic)
        o.info_rule = int(info_rule)        # 1 = SLUAMD_INFO_REFERENCE: the zero-pivot rule of the reference's code (what the binding selects)
        return o

    @classmethod
    def from_store(cls, store, forests=None, **kw):
        L = _lib.load()
        h = C.c_void_p()
        o = cls._opts(**kw)
        fv = None
        keep = None
        if forests is not None:
            fv, keep = _forest_view(forests)
        create = L.sluamd_zCreateLUHandle if store.z else L.sluamd_dCreateLUHandle
        _lib.check(create(C.byref(h), C.byref(store.view), None if fv is None else C.byref(fv), C.byref(o)),
                   "sluamd_zCreateLUHandle" if store.z else "sluamd_dCreateLUHandle")
        obj = cls(h, store)
        obj.z = store.z
        obj._keep = keep
        return obj

    @classmethod
    def from_symbolic(cls, symb, nzval, **kw):
        L = _lib.load()
        h = C.c_void_p()
        o = cls._opts(**kw)
        if np.iscomplexobj(nzval):
            nz = np.ascontiguousarray(nzval, dtype=np.complex128)
            _lib.check(L.sluamd_zCreateLUHandleFromSymb(C.byref(h), symb._h, _pi(symb.rowptr), _pi(symb.colind),
                                                        nz.ctypes.data_as(C.c_void_p), _pi(symb.perm_c), C.byref(o)),
                       "sluamd_zCreateLUHandleFromSymb")
            obj = cls(h, None); obj.z = True; obj.n = symb.n; obj.nnz = len(symb.colind); obj.device = int(o.device)
            return obj
        nz = np.ascontiguousarray(nzval, dtype=np.float64)
        _lib.check(L.sluamd_dCreateLUHandleFromSymb(C.byref(h), symb._h, _pi(symb.rowptr), _pi(symb.colind), _pd(nz),
                                                    _pi(symb.perm_c), C.byref(o)), "sluamd_dCreateLUHandleFromSymb")
        obj = cls(h, None); obj.n = symb.n; obj.nnz = len(symb.colind); obj.device = int(o.device)
        return obj

    def set_values(self, store):
        L = _lib.load()
        _lib.check((L.sluamd_zSetValues if self.z else L.sluamd_dSetValues)(self._h, C.byref(store.view)), "sluamd_[dz]SetValues")

    def pdgstrf3d(self, thresh=0.0):
        """pdgstrf3d, or pzgstrf3d on a complex16 handle."""
        L = _lib.load()
        info = C.c_int32(0)
        _lib.check((L.sluamd_pzgstrf3d if self.z else L.sluamd_pdgstrf3d)(self._h, float(thresh), C.byref(info)), "sluamd_p[dz]gstrf3d")
        return info.value

    pzgstrf3d = pdgstrf3d

    def copy_to_host(self, store=None):
        store = store or self.store
        _check_store_dtype(store, self.z)
        L = _lib.load()
        _lib.check((L.sluamd_zCopyLU2Host if self.z else L.sluamd_dCopyLU2Host)(self._h, C.byref(store.view)), "sluamd_[dz]CopyLU2Host")
        return store

    def pdgstrs3d(self, x, trans="N"):
        """pdgstrs3d, or pzgstrs3d on a complex16 handle.  trans = "T" / "C": the transposed / conjugate-transposed solve (L U)^T y = x,
        (L U)^H y = x with the same factors (sluamd_p[dz]gstrs3d_trans)."""
        t = _trans_code(trans)
        x = np.asfortranarray(np.array(x, dtype=np.complex128 if self.z else np.float64))
        if x.ndim == 1:
            x = np.asfortranarray(x[:, None])
        L = _lib.load()
        if t:
            name = "sluamd_pzgstrs3d_trans" if self.z else "sluamd_pdgstrs3d_trans"
            _lib.check(_lib.entry(name)(self._h, t, x.ctypes.data_as(C.c_void_p), x.shape[0], x.shape[1]), name)
        elif self.z:
            _lib.check(L.sluamd_pzgstrs3d(self._h, x.ctypes.data_as(C.c_void_p), x.shape[0], x.shape[1]), "sluamd_pzgstrs3d")
        else:
            _lib.check(L.sluamd_pdgstrs3d(self._h, _pd(x), x.shape[0], x.shape[1]), "sluamd_pdgstrs3d")
        return x

    pzgstrs3d = pdgstrs3d

    def pdgstrs3d_dist(self, B, perm=None, fst_row=0):
        """sluamd_pdgstrs3d_dist on a single-rank handle: B in the ORIGINAL row order (all n rows), perm[i] = row of the factored system."""
        B = np.asfortranarray(np.array(B, dtype=np.float64))
        if B.ndim == 1:
            B = np.asfortranarray(B[:, None])
        pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        _lib.check(_lib.load().sluamd_pdgstrs3d_dist(self._h, B.ctypes.data_as(C.c_void_p), max(B.shape[0], 1), B.shape[1], B.shape[0], int(fst_row),
                                                     None if pm is None else _pi(pm), None if pm is None else _pi(pm)), "sluamd_pdgstrs3d_dist")
        return B

    def pdgstrs3d_dev(self, ptr, ldx, nrhs, trans="N"):
        """the solve on a device pointer (ldx in values); complex16 handles and trans = "T" / "C" go through sluamd_p[dz]gstrs3d_trans_dev"""
        t = _trans_code(trans)
        if t or self.z:
            name = "sluamd_pzgstrs3d_trans_dev" if self.z else "sluamd_pdgstrs3d_trans_dev"
            _lib.check(_lib.entry(name)(self._h, t, C.c_void_p(ptr), ldx, nrhs), name)
        else:
            _lib.check(_lib.load().sluamd_pdgstrs3d_dev(self._h, C.c_void_p(ptr), ldx, nrhs), "sluamd_pdgstrs3d_dev")

    def reset_values(self):
        _lib.check(_lib.load().sluamd_dResetValues(self._h), "sluamd_dResetValues")

    def update_values(self, nzval, want_norm=False):
        """New values for the SAME CSR the handle was created from (from_symbolic), Fact = SamePattern_SameRowPerm: sluamd_[dz]UpdateValues for a numpy
        array (or a torch tensor on the CPU), sluamd_[dz]UpdateValues_dev with data_ptr() for a torch tensor on the handle's device -- values assembled
        on the GPU never visit the host; the tensor must stay alive and unchanged until the next synchronising call on the handle (a factorisation).
        The handle is then unfactored; an equilibrated handle scales the new values with its R and C; an attached matrix takes them too.
        Returns None, or dict(anorm, equed) when want_norm (needs an attached matrix).  ValueError, before any library call: wrong dtype, wrong
        length, non-contiguous data, a tensor on another device.
        A handle made by pdgssvx3d(rowperm=...) holds Pr A: nzval is in the order of A's CSR and is taken through the position map first (numpy take; torch
        index_select on the tensor's device, so device values still never visit the host)."""
        if self.rowperm_pos is not None:
            nzval = self._taken = _take_values(nzval, self.rowperm_pos, self.nnz)      # kept: the _dev form reads it until the next synchronising call
        return _update_values(self._h, self.z, self.nnz, self.device, nzval, want_norm)

    def attach_matrix(self, n, rowptr, colind, nzval, perm_c):
        """Device copy of the ORIGINAL matrix (CSR) + perm_c for pdgsrfs3d (sluamd_dAttachMatrix, or sluamd_zAttachMatrix on a complex16 handle)."""
        _attach_matrix(self._h, self.z, n, rowptr, colind, nzval, perm_c)
        self.attached_nnz = int(np.asarray(rowptr)[int(n)])

    def pdgsrfs3d(self, b, x, trans="N", method="plain", restart=None, inner_tol=None, max_solves=None, block=False):
        """Iterative refinement of x (original ordering) for the attached matrix; returns (x, berr[nrhs], steps).
        block=True: all right-hand sides go through the loop together, in panels of 16 columns with one solve per step for the columns that continue
        (sluamd_p[dz]gsrfs3d_block); returns (x, berr[nrhs], steps[nrhs]), every column's own count; b and x are checked as for trans = "T" / "C";
        not with method="gmres" (ValueError).
        method="gmres": the correction of every step is a cycle of GMRES preconditioned by the factors (sluamd_p[dz]gsrfs3d_gmres; restart, inner_tol,
        max_solves: sluamd_gmres_t, None = the library's default); returns (x, berr[nrhs], steps, solves[nrhs]), steps counting the outer steps.  b and x
        are checked as for trans = "T" / "C"; ValueError also for another method, or for restart / inner_tol / max_solves with method="plain".
        pzgsrfs3d on a complex16 handle (complex b and x).  trans = "T" / "C": the transposed / conjugate-transposed system A^T x = b, A^H x = b of
        the attached matrix (sluamd_p[dz]gsrfs3d_trans), x e.g. from pdgstrs3d(trans=...).  ValueError, before any library call:
        a trans other than "N", "T", "C"; b or x of another dtype than the handle's; shapes that differ or are not (n,) / (n, nrhs).
        method="extra": IterRefine = SLU_EXTRA (sluamd_p[dz]gsrfs3d_extra) -- the residual of every step accumulated in twice the working precision, the
        loop stopped by the corrections instead of berr; returns (x, berr[nrhs], steps[nrhs], dxrel[nrhs], state[nrhs]): state 0 / 1 / 2 = CONVERGED /
        NO_PROGRESS / LIMIT (_lib.XR_STATES), dxrel = max|dx| / max|x| of the last correction computed.  self.refine_rho[nrhs] then holds the largest ratio
        of successive corrections, and dxrel / (1 - rho) estimates -- it does not bound -- the relative forward error.  b and x are checked as for
        trans = "T" / "C"; not with block=True, restart, inner_tol or max_solves (ValueError)."""
        _check_block(block, method)
        opt = _gmres_opt(method, restart, inner_tol, max_solves)
        out = _refine(self._h, self.z, "block" if block else method, self.n, b, x, trans, opt)
        if method == "extra":
            *out, self.refine_rho = out
        return tuple(out)

    pzgsrfs3d = pdgsrfs3d

    def residual(self, b, x, trans="N", extra=False):
        """r = b - op(A) x of the attached matrix in the caller's ordering and its componentwise backward error: (r, berr[nrhs]) (sluamd_[dz]Residual).
        extra=False: the refinement's fp64 pass, bitwise; extra=True: the doubled accumulation of method="extra", every r_i one rounding of the exact
        residual up to second-order terms.  b and x are checked as for pdgsrfs3d(trans="T")."""
        return _residual(self._h, self.z, b, x, trans, extra, self.n)

    def residual_dev(self, d_b, ldb, d_x, ldx, nrhs, d_r, ldr, trans="N", extra=False):
        """sluamd_[dz]Residual_dev: b, x, r device pointers (column-major, ld in values); returns berr[nrhs]"""
        berr = np.zeros(max(int(nrhs), 1))
        name = "sluamd_zResidual_dev" if self.z else "sluamd_dResidual_dev"
        _lib.check(_lib.entry(name)(self._h, _trans_code(trans), 1 if extra else 0, C.c_void_p(d_b), int(ldb), C.c_void_p(d_x), int(ldx), int(nrhs), C.c_void_p(d_r),
                                    int(ldr), _pd(berr)), name)
        return berr[:int(nrhs)]

    def pdgsrfs3d_dev(self, d_b, ldb, d_x, ldx, nrhs, trans="N", method="plain", restart=None, inner_tol=None, max_solves=None, block=False):
        """sluamd_p[dz]gsrfs3d_dev: b, x device pointers (column-major, ld in values); x refined in place.  Returns (berr[nrhs], steps).
        block=True: sluamd_p[dz]gsrfs3d_block_dev, returns (berr[nrhs], steps[nrhs]); not with method="gmres" (ValueError).
        trans = "T" / "C": sluamd_p[dz]gsrfs3d_trans_dev.  method="gmres": sluamd_p[dz]gsrfs3d_gmres_dev, returns (berr[nrhs], steps, solves[nrhs]).
        method="extra": sluamd_p[dz]gsrfs3d_extra_dev, returns (berr[nrhs], steps[nrhs], dxrel[nrhs], state[nrhs]); self.refine_rho as pdgsrfs3d."""
        _check_block(block, method)
        opt = _gmres_opt(method, restart, inner_tol, max_solves)
        out = _refine_call(self._h, self.z, "block" if block else method, False, trans, d_b, ldb, d_x, ldx, nrhs, opt)
        if method == "extra":
            *out, self.refine_rho = out
        return tuple(out)

    pzgsrfs3d_dev = pdgsrfs3d_dev

    def equilibrate(self, n, rowptr, colind, nzval, perm_c):
        """Equil = YES on a handle made by from_symbolic (sluamd_[dz]Equilibrate): pass the arrays the handle was created from.  Returns
        dict(equed="N"|"R"|"C"|"B", info, rowcnd, colcnd, amax, anorm); the handle then holds the scaled matrix, unfactored."""
        return _equilibrate(self._h, self.z, n, rowptr, colind, nzval, perm_c)

    def equilibrate_with(self, n, rowptr, colind, nzval, perm_c, r=None, c=None):
        """sluamd_[dz]EquilibrateWith: equilibrate() with R and C given (either may be None), e.g. those of large_diag; same return value"""
        return _equilibrate(self._h, self.z, n, rowptr, colind, nzval, perm_c, with_rc=(r, c))

    def set_row_perm(self, perm_r):
        """sluamd_SetRowPerm: the handle was made from Pr A; gssvx_solve then takes b and returns x in A's ordering.  After equilibrate_with / attach_matrix."""
        pr = np.ascontiguousarray(perm_r, dtype=np.int32)
        if pr.shape != (self.n,):
            raise ValueError(f"set_row_perm: {self.n} entries expected, got shape {pr.shape}")
        _lib.check(_lib.entry("sluamd_SetRowPerm")(self._h, _pi(pr)), "sluamd_SetRowPerm")

    def scalings(self):
        """(R, C) of the equilibration; all ones where that side was not scaled (sluamd_GetScalings)"""
        return _scalings(self._h, self.n)

    def gssvx_solve(self, b, trans="N", refine=False):
        """The solve phase of the expert driver (sluamd_p[dz]gssvx3d_solve): b in the ORIGINAL ordering and scaling -> x likewise; needs
        equilibrate() or attach_matrix() (for perm_c).  refine=True returns (x, berr, steps)."""
        return _gssvx_solve(self._h, self.z, b, trans, refine)

    def gssvx_solve_dev(self, d_b, ldb, d_x, ldx, nrhs, trans="N", refine=False):
        """the same on device pointers (ld in values); d_b is not modified; returns (berr, steps) when refine"""
        return _gssvx_solve_dev(self._h, self.z, d_b, ldb, d_x, ldx, nrhs, trans, refine)

    def adjoint_values(self, lam, x, trans="N"):
        """The gradient of a loss through x = op(A)^-1 b with respect to the stored values of A (sluamd_[dz]AdjointValues): lam = the adjoint solution, x = the
        forward solution, both (n,) or (n, nrhs) in the caller's ordering and scaling; trans = the system that was solved.  Returns G[nnz] in the entry order
        of the CSR the handle was created from; the formulas per trans are at the declaration in include/superlu_dist_amd.h.  Needs an attached matrix
        (attach_matrix or equilibrate), no factors.  ValueError, before any library call: a trans other than "N", "T", "C"; lam or x of another dtype than the
        handle's; shapes that differ or are not (n,) / (n, nrhs)."""
        t = _trans_code(trans)
        dt = np.complex128 if self.z else np.float64
        lam, x = _adjoint_pair("adjoint_values", dt, lam, x, (self.n,))
        nrhs = 1 if lam.ndim == 1 else lam.shape[1]
        lam = np.asfortranarray(lam.reshape(self.n, nrhs)); x = np.asfortranarray(x.reshape(self.n, nrhs))
        g = np.zeros(self.nnz if self.attached_nnz is None else self.attached_nnz, dtype=dt)
        name = "sluamd_zAdjointValues" if self.z else "sluamd_dAdjointValues"
        ld = max(self.n, 1)
        _lib.check(_lib.entry(name)(self._h, t, lam.ctypes.data_as(C.c_void_p), ld, x.ctypes.data_as(C.c_void_p), ld, lam.shape[1], g.ctypes.data_as(C.c_void_p)), name)
        return g

    def adjoint_values_dev(self, d_lam, ldl, d_x, ldx, nrhs, d_g, trans="N"):
        """sluamd_[dz]AdjointValues_dev: lam, x (column-major, ld in values) and g[nnz] device pointers; what produced them must be complete"""
        name = "sluamd_zAdjointValues_dev" if self.z else "sluamd_dAdjointValues_dev"
        _lib.check(_lib.entry(name)(self._h, _trans_code(trans), C.c_void_p(d_lam), int(ldl), C.c_void_p(d_x), int(ldx), int(nrhs), C.c_void_p(d_g)), name)

    def set_profile(self, on=True):
        _lib.load().sluamd_set_profile(self._h, int(on))

    def stats(self):
        s = Stats()
        _lib.load().sluamd_get_stats(self._h, C.byref(s))
        return {f[0]: getattr(s, f[0]) for f in Stats._fields_}

    def plan_table(self):
        """this rank's plan, one row per (Z level, DAG level): columns as documented at sluamd_plan_table (include/superlu_dist_amd.h)"""
        return plan_table(self._h)

    def diag_inv(self, k, ns):
        """(Linv, Uinv) of the diagonal block of supernode k: ns x ns, column-major (sluamd_dGetDiagInv)"""
        li = np.zeros((ns, ns), order="F"); ui = np.zeros((ns, ns), order="F")
        _lib.check(_lib.load().sluamd_dGetDiagInv(self._h, int(k), _pd(li), _pd(ui)), "sluamd_dGetDiagInv")
        return li, ui

    def setup_times(self):
        """{phase: seconds} of this handle's creation (sluamd_setup_times)"""
        buf = C.create_string_buffer(4096)
        if _lib.load().sluamd_setup_times(self._h, buf, 4096):
            return {}
        out = {}
        for tok in buf.value.decode().split(";"):
            if "=" in tok:
                k, v = tok.split("=")
                out[k] = out.get(k, 0.0) + float(v)
        return out

    def destroy(self):
        if self._h:
            _lib.load().sluamd_dDestroyLUHandle(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _trans_code(trans):
    """"N" | "T" | "C" -> SLUAMD_NOTRANS / SLUAMD_TRANS / SLUAMD_CONJ"""
    try:
        return {"N": 0, "T": 1, "C": 2}[str(trans).upper()]
    except KeyError:
        raise ValueError(f"trans must be 'N', 'T' or 'C', not {trans!r}") from None


def _adjoint_pair(who, dt, lam, x, lead):
    """lam and x of adjoint_values as arrays; ValueError (before any library call) for another dtype, shapes that differ or are not lead + () / lead + (nrhs,)"""
    lam, x = np.asarray(lam), np.asarray(x)
    for what, a in (("lam", lam), ("x", x)):
        if a.dtype != np.dtype(dt):
            raise ValueError(f"{who}: the handle holds {np.dtype(dt).name} values, {what} is {a.dtype}")
        if not (a.flags.c_contiguous or a.flags.f_contiguous):
            raise ValueError(f"{who}: {what} is not contiguous")
    if lam.shape != x.shape or lam.ndim not in (len(lead), len(lead) + 1) or lam.shape[:len(lead)] != tuple(lead):
        raise ValueError(f"{who}: lam and x must both be {tuple(lead)} or {tuple(lead) + ('nrhs',)}, got {lam.shape} and {x.shape}")
    return lam, x


def _check_store_dtype(store, z):
    """The copy writes the handle's values into the store's arrays: a real store holds half the bytes of a complex16 handle's factors."""
    if bool(store.z) != bool(z):
        raise ValueError(f"copy_to_host: the store holds {'complex128' if store.z else 'float64'} values, the handle "
                         f"{'complex16' if z else 'double'} factors")


def _attach_matrix(h, z, n, rowptr, colind, nzval, perm_c):
    rp = np.ascontiguousarray(rowptr, dtype=np.int32); ci = np.ascontiguousarray(colind, dtype=np.int32)
    pc = np.ascontiguousarray(perm_c, dtype=np.int32)
    if z:
        v = np.ascontiguousarray(nzval, dtype=np.complex128)
        _lib.check(_lib.entry("sluamd_zAttachMatrix")(h, int(n), _pi(rp), _pi(ci), v.ctypes.data_as(C.c_void_p), _pi(pc)), "sluamd_zAttachMatrix")
    else:
        v = np.ascontiguousarray(nzval, dtype=np.float64)
        _lib.check(_lib.load().sluamd_dAttachMatrix(h, int(n), _pi(rp), _pi(ci), _pd(v), _pi(pc)), "sluamd_dAttachMatrix")


def _rhs_pair(who, z, b, x, n, strict=True):
    """b and x of a refinement or residual call as Fortran-ordered copies of the handle's dtype, promoted to 2-D: (b, x, one), one = they came as vectors.
    strict: ValueError (before any library call, the message starting with `who`) for another dtype, shapes that differ or are not (n,) / (n, nrhs);
    strict=False is the plain untransposed call, which converts instead."""
    dt = np.dtype(np.complex128 if z else np.float64)
    if strict:
        for what, a in (("b", b), ("x", x)):
            if np.asarray(a).dtype != dt:
                raise ValueError(f"{who}: the handle holds {dt.name} values, {what} is {np.asarray(a).dtype}")
        if np.shape(b) != np.shape(x) or np.ndim(b) not in (1, 2) or (n is not None and np.shape(b)[0] != n):
            raise ValueError(f"{who}: b and x must both be ({n},) or ({n}, nrhs), got {np.shape(b)} and {np.shape(x)}")
    b = np.asfortranarray(np.array(b, dtype=dt)); x = np.asfortranarray(np.array(x, dtype=dt))
    one = b.ndim == 1
    if one:
        b = np.asfortranarray(b[:, None]); x = np.asfortranarray(x[:, None])
    return b, x, one


def _check_block(block, method):
    if block and method in ("gmres", "extra"):
        noun = "GMRES" if method == "gmres" else "extra-precise"
        raise ValueError(f"block=True belongs to method='plain': the {noun} refinement takes one right-hand side at a time")


def _gmres_opt(method, restart, inner_tol, max_solves):
    """None for method="plain" and "extra"; else sluamd_gmres_t with the library's defaults where an argument is None.  ValueError: another method, options
    without method="gmres".  (The ranges are the library's to check: SLUAMD_EINVAL -> RuntimeError.)"""
    if method in ("plain", "extra"):
        if restart is not None or inner_tol is not None or max_solves is not None:
            raise ValueError("restart, inner_tol and max_solves belong to method='gmres'")
        return None
    if method != "gmres":
        raise ValueError(f"method must be 'plain', 'gmres' or 'extra', not {method!r}")
    from ._lib import Gmres
    o = Gmres()
    _lib.entry("sluamd_default_gmres")(C.byref(o))
    if restart is not None:
        o.restart = int(restart)
    if inner_tol is not None:
        o.inner_tol = float(inner_tol)
    if max_solves is not None:
        o.max_solves = int(max_solves)
    return o


def _xrefine_out(out, nrhs):
    """sluamd_xrefine_t[nrhs] -> steps, dxrel, state, rho as arrays"""
    o = out[:nrhs]
    return (np.array([v.steps for v in o], dtype=np.int32), np.array([v.dxrel for v in o], dtype=np.float64),
            np.array([v.state for v in o], dtype=np.int32), np.array([v.rho for v in o], dtype=np.float64))


def _refine_call(h, z, form, host, trans, b, ldb, x, ldx, nrhs, opt=None):
    """One call of sluamd_p[dz]gsrfs3d{,_trans,_block,_gmres,_extra}{,_dev}.  form: "plain" (with trans != "N": the _trans entry), "block", "gmres" (opt: its
    sluamd_gmres_t) or "extra"; b, x: Fortran-ordered arrays (host) or device pointers as integers.  Returns berr[nrhs] and the form's outputs --
    plain: steps; block: steps[nrhs]; gmres: steps, solves[nrhs]; extra: steps[nrhs], dxrel[nrhs], state[nrhs], rho[nrhs]"""
    t = _trans_code(trans)
    nrhs, m = int(nrhs), max(int(nrhs), 1)
    berr = np.zeros(m)
    if host:                                                # (sluamd_pdgsrfs3d alone is bound with double pointers)
        typed = form == "plain" and not t and not z
        pb, px = (_pd(b), _pd(x)) if typed else (b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p))
    else:
        pb, px = C.c_void_p(b), C.c_void_p(x)
    blocks = (pb, int(ldb), px, int(ldx), nrhs)
    steps = C.c_int32(0); per = np.zeros(m, dtype=np.int32)         # the call's step count / a count per column
    if form == "plain" and not t:
        suffix, args = "", (h,) + blocks + (_pd(berr), C.byref(steps))
    elif form == "plain":
        suffix, args = "_trans", (h, t) + blocks + (_pd(berr), C.byref(steps))
    elif form == "block":
        suffix, args = "_block", (h, t) + blocks + (_pd(berr), _pi(per))
    elif form == "gmres":
        suffix, args = "_gmres", (h, t) + blocks + (None if opt is None else C.byref(opt), _pd(berr), C.byref(steps), _pi(per))
    else:
        out = (_lib.XRefine * m)()
        suffix, args = "_extra", (h, t) + blocks + (_pd(berr), out)
    name = "sluamd_p%sgsrfs3d%s%s" % ("z" if z else "d", suffix, "" if host else "_dev")
    _lib.check(_lib.entry(name)(*args), name)
    berr = berr[:nrhs]
    if form == "plain":
        return berr, steps.value
    if form == "block":
        return berr, per[:nrhs]
    if form == "gmres":
        return berr, steps.value, per[:nrhs]
    return (berr,) + _xrefine_out(out, nrhs)


def _refine(h, z, form, n, b, x, trans="N", opt=None):
    """_refine_call on host arrays: (x,) + its outputs; b and x through _rhs_pair under the form's name -- the plain untransposed call converts them,
    every other form refuses what it would have to convert"""
    t = _trans_code(trans)
    who = {"plain": f"pdgsrfs3d(trans={trans!r})", "block": "pdgsrfs3d(block=True)", "gmres": "pdgsrfs3d(method='gmres')", "extra": "pdgsrfs3d(method='extra')"}[form]
    b, x, _ = _rhs_pair(who, z, b, x, n, strict=form != "plain" or bool(t))
    return (x,) + _refine_call(h, z, form, True, trans, b, max(b.shape[0], 1), x, max(x.shape[0], 1), b.shape[1], opt)


def _residual(h, z, b, x, trans, extra, n):
    """sluamd_[dz]Residual on host arrays: (r, berr[nrhs])"""
    t = _trans_code(trans)
    b, x, one = _rhs_pair("residual", z, b, x, n)
    nrhs = b.shape[1]
    r = np.zeros_like(b, order="F"); berr = np.zeros(max(nrhs, 1))
    name = "sluamd_zResidual" if z else "sluamd_dResidual"
    ld = max(b.shape[0], 1)
    _lib.check(_lib.entry(name)(h, t, 1 if extra else 0, b.ctypes.data_as(C.c_void_p), ld, x.ctypes.data_as(C.c_void_p), ld, nrhs, r.ctypes.data_as(C.c_void_p), ld,
                                _pd(berr)), name)
    return (r[:, 0] if one else r), berr[:nrhs]


EQUED = "NRCB"      # SLUAMD_EQUED_N / _R / _C / _B


def _update_values(h, z, nnz, device, nzval, want_norm):
    """argument checks (ValueError, before any library call) and the call of LUHandle.update_values / GridHandle.update_values"""
    want = "complex128" if z else "float64"
    ptr, dev = None, False
    if type(nzval).__module__.split(".")[0] == "torch" and hasattr(nzval, "data_ptr"):
        t = nzval
        if str(t.dtype) != "torch." + want:
            raise ValueError(f"update_values: the handle holds {want} values, the tensor is {t.dtype}")
        if t.dim() != 1 or (nnz is not None and t.numel() != nnz):
            raise ValueError(f"update_values: {nnz} values expected (the CSR the handle was created from), got a tensor of shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError("update_values: the tensor is not contiguous")
        if t.device.type == "cpu":
            nzval = t.numpy()
        else:
            if t.device.type != "cuda":
                raise ValueError(f"update_values: the tensor is on {t.device}, the handle on a HIP device")
            import torch
            mine = device if device >= 0 else torch.cuda.current_device()      # device = -1 at creation: the device that is current
            if t.device.index != mine:
                raise ValueError(f"update_values: the tensor is on {t.device}, the handle on device {mine}")
            ptr, dev, keep = t.data_ptr(), True, t
    if not dev:
        a = np.asarray(nzval)
        if a.dtype != np.dtype(want):
            raise ValueError(f"update_values: the handle holds {want} values, the array is {a.dtype}")
        if a.ndim != 1 or (nnz is not None and a.shape[0] != nnz):
            raise ValueError(f"update_values: {nnz} values expected (the CSR the handle was created from), got an array of shape {a.shape}")
        if not a.flags.c_contiguous:
            raise ValueError("update_values: the array is not contiguous")
        ptr, keep = a.ctypes.data, a
    name = ("sluamd_zUpdateValues" if z else "sluamd_dUpdateValues") + ("_dev" if dev else "")
    out = _lib.Update() if want_norm else None
    _lib.check(_lib.entry(name)(h, C.c_void_p(ptr), None if out is None else C.byref(out)), name)
    del keep
    return dict(anorm=float(out.anorm), equed=EQUED[out.equed]) if want_norm else None


def _take_values(nzval, pos, nnz):
    """nzval[pos] for the value arrays update_values accepts; anything else (or a wrong length) is passed on for _update_values to refuse"""
    if type(nzval).__module__.split(".")[0] == "torch" and hasattr(nzval, "data_ptr"):
        if nzval.dim() != 1 or nzval.numel() != nnz:
            return nzval
        import torch
        out = torch.index_select(nzval, 0, torch.as_tensor(pos, dtype=torch.int64, device=nzval.device))
        if out.device.type == "cuda":
            torch.cuda.current_stream(out.device).synchronize()      # the library reads it on the handle's stream
        return out
    a = np.asarray(nzval)
    return a.take(pos) if a.ndim == 1 and a.shape[0] == nnz else nzval


def _equilibrate(h, z, n, rowptr, colind, nzval, perm_c, with_rc=None):
    rp = np.ascontiguousarray(rowptr, dtype=np.int32); ci = np.ascontiguousarray(colind, dtype=np.int32)
    pc = np.ascontiguousarray(perm_c, dtype=np.int32)
    v = np.ascontiguousarray(nzval, dtype=np.complex128 if z else np.float64)
    e = _lib.Equil()
    given = ()
    if with_rc is not None:
        r, c = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in with_rc)
        for what, a in (("r", r), ("c", c)):
            if a is not None and a.shape != (int(n),):
                raise ValueError(f"equilibrate_with: {what} must have shape ({int(n)},), got {a.shape}")
        given = (None if r is None else _pd(r), None if c is None else _pd(c))
    name = ("sluamd_zEquilibrate" if z else "sluamd_dEquilibrate") + ("With" if given else "")
    _lib.check(_lib.entry(name)(h, int(n), _pi(rp), _pi(ci), v.ctypes.data_as(C.c_void_p), _pi(pc), *given, C.byref(e)), name)
    return dict(equed=EQUED[e.equed], info=int(e.info), rowcnd=float(e.rowcnd), colcnd=float(e.colcnd), amax=float(e.amax), anorm=float(e.anorm))


def _scalings(h, n):
    r = np.empty(n); c = np.empty(n)
    _lib.check(_lib.entry("sluamd_GetScalings")(h, _pd(r), _pd(c)), "sluamd_GetScalings")
    return r, c


def _gssvx_solve(h, z, b, trans, refine):
    t = _trans_code(trans)
    b = np.asfortranarray(np.array(b, dtype=np.complex128 if z else np.float64))
    if b.ndim == 1:
        b = np.asfortranarray(b[:, None])
    x = np.zeros_like(b, order="F")
    berr = np.zeros(max(b.shape[1], 1)); steps = C.c_int32(0)
    name = "sluamd_pzgssvx3d_solve" if z else "sluamd_pdgssvx3d_solve"
    _lib.check(_lib.entry(name)(h, t, b.ctypes.data_as(C.c_void_p), max(b.shape[0], 1), x.ctypes.data_as(C.c_void_p), max(x.shape[0], 1), b.shape[1],
                                int(bool(refine)), _pd(berr), C.byref(steps)), name)
    return (x, berr[:b.shape[1]], steps.value) if refine else x


def _gssvx_solve_dev(h, z, d_b, ldb, d_x, ldx, nrhs, trans, refine):
    berr = np.zeros(max(int(nrhs), 1)); steps = C.c_int32(0)
    name = "sluamd_pzgssvx3d_solve_dev" if z else "sluamd_pdgssvx3d_solve_dev"
    _lib.check(_lib.entry(name)(h, _trans_code(trans), C.c_void_p(d_b), int(ldb), C.c_void_p(d_x), int(ldx), int(nrhs), int(bool(refine)),
                                _pd(berr), C.byref(steps)), name)
    return (berr[:int(nrhs)], steps.value) if refine else None


def _forest_view(forests):
    """forests = dict(maxLvl, myTreeIdxs, myZeroTrIdxs, nodeLists=[array or None per forest])"""
    fv = ForestView()
    mt = np.ascontiguousarray(forests["myTreeIdxs"], dtype=np.int32)
    mz = np.ascontiguousarray(forests["myZeroTrIdxs"], dtype=np.int32)
    lists = [np.ascontiguousarray(a if a is not None else [], dtype=np.int32) for a in forests["nodeLists"]]
    nn = np.array([len(a) for a in lists], dtype=np.int32)
    arr = (P_int * len(lists))()
    for i, a in enumerate(lists):
        arr[i] = _pi(a) if len(a) else None
    fv.maxLvl = int(forests["maxLvl"]); fv.myTreeIdxs = _pi(mt); fv.myZeroTrIdxs = _pi(mz)
    fv.numForests = len(lists); fv.nNodes = _pi(nn); fv.nodeList = C.cast(arr, C.POINTER(P_int))
    return fv, (mt, mz, lists, nn, arr)


def pivot_thresh(n, rowptr, colind, nzval):
    """thresh = smach_dist("Epsilon") * anorm of pdgstrf3d (pdgstrf3d.c:132-133): single-precision epsilon in LAPACK's
    slamch('E') sense (FLT_EPSILON * 0.5 = 2^-24, smach_dist.c:64) times the 1-norm of A (max column sum,
    dcomputeA_Norm(notran), pdgssvx3d.c)."""
    if len(nzval) == 0:
        return 0.0
    colsum = np.bincount(np.asarray(colind), weights=np.abs(nzval), minlength=int(n))
    return 0.5 * float(np.finfo(np.float32).eps) * float(colsum.max())


def pdgssvx3d(n, rowptr, colind, nzval, b, perm_c=None, relax=32, maxsup=256, replace_tiny=False, anorm=None,
              keep=False, refine=False, trans="N", equil=False, rowperm=None, deterministic=False, grid=None):
    """Solve A x = b -- trans = "T": A^T x = b, "C": A^H x = b, with the same factorisation of A -- through the GPU hot path: symbolic (host) -> device-resident distribute -> pdgstrf3d ->
    pdgstrs3d, with Equil = NO, RowPerm = NOROWPERM, ColPerm = MY_PERMC/NATURAL, IterRefine = NOREFINE
    (the timing configuration of BASELINE.md section 4); refine=True adds IterRefine = SLU_DOUBLE (pdgsrfs3d on the device;
    pzgsrfs3d for complex nzval) and puts `berr` / `refine_steps` into the stats.  equil=True: Equil = YES -- the handle is equilibrated on
    the device (LUHandle.equilibrate), thresh comes from the 1-norm of the scaled matrix, and the solve (and the refinement) runs through
    LUHandle.gssvx_solve in the caller's ordering and scaling; `equed`, `rowcnd`, `colcnd`, `amax` and a positive `equil_info` go into the
    stats; `anorm` is not used then.
    rowperm="LargeDiag_MC64": RowPerm = LargeDiag_MC64 -- large_diag, the CSR of Pr A (permute_rows_csr), perm_c = order_nd of it when none is
    given, symbolic, handle, equilibrate_with(r, c) when equil (the matching's scalings ALONE; the reference composes them with pdgsequ's), else
    attach_matrix; set_row_perm; factorisation and gssvx_solve with b and x in A's ordering.  `rowperm` = the matching's counters goes into the
    stats; a structurally singular A raises RuntimeError.  With keep=True the handle's update_values takes values in A's order.
    deterministic=True: the handle option of that name (bitwise reproducible factors).
    grid=(Pr, Pc, Pz): the same on a process grid whose ranks are threads of this process over the in-process transport (grid3d.local_comms) -- every
    rank holds the complete matrix and b, the calls are collective (replicated forms), rank 0's x, info and stats are returned; trans, equil and refine
    as above; keep and rowperm are not part of this form (ValueError).
    refine="gmres": the refinement is the GMRES one (LUHandle.pdgsrfs3d(method="gmres")); `refine_solves` joins `berr` and `refine_steps` in the stats.
    With equil=True the solve runs with refine=0 and the SCALED system is refined: b' = R o b, x' = x / C, then x = C o x'.  Not with grid or rowperm
    (ValueError).
    refine="block": the refinement is the blocked one (LUHandle.pdgsrfs3d(block=True): all right-hand sides together, one solve per step); `refine_steps` in
    the stats is then an array, every column's own count.  With the forms that refine through gssvx_solve (equil, rowperm) the solve runs with refine=0 and
    the blocked refinement follows on the attached system (equil: the scaled one, as for "gmres"); not with rowperm (ValueError).
    refine="extra": IterRefine = SLU_EXTRA (LUHandle.pdgsrfs3d(method="extra")): `refine_steps` is an array, and `refine_dxrel`, `refine_state` and
    `refine_rho` (arrays per column) join `berr` in the stats.  With equil=True the scaled system is refined as for "gmres", and dxrel measures the scaled
    x'.  Not with grid or rowperm (ValueError).
    Returns (x, info, stats[, handle, symb])."""
    block = isinstance(refine, str) and refine == "block"
    if block and rowperm is not None:
        raise ValueError("refine='block' is not part of the rowperm form of this driver -- keep the handle and call LUHandle.pdgsrfs3d(block=True)")
    extra = isinstance(refine, str) and refine == "extra"
    if extra and ((grid is not None and tuple(grid) != (1, 1, 1)) or rowperm is not None):
        raise ValueError("refine='extra' is not part of the grid and rowperm forms of this driver -- keep the handle and call LUHandle.pdgsrfs3d(method='extra')")
    gmres = isinstance(refine, str) and not block and not extra
    if gmres and refine != "gmres":
        raise ValueError(f"refine must be False, True, 'gmres', 'block' or 'extra', not {refine!r}")
    if gmres and ((grid is not None and tuple(grid) != (1, 1, 1)) or rowperm is not None):
        raise ValueError("refine='gmres' is not part of the grid and rowperm forms of this driver -- keep the handle and call LUHandle.pdgsrfs3d(method='gmres')")
    if refine and _trans_code(trans):
        raise ValueError("refine=True with trans != 'N': not in this driver -- solve with refine=False and keep=True, then refine with "
                         "LUHandle.pdgsrfs3d(b, x, trans=...) on the attached matrix")
    if grid is not None and tuple(grid) != (1, 1, 1):
        if keep or rowperm is not None:
            raise ValueError("pdgssvx3d(grid=...): keep=True and rowperm are not part of the grid form -- use grid3d.GridHandle directly")
        return _gssvx3d_grid(n, rowptr, colind, nzval, b, perm_c, relax, maxsup, replace_tiny, anorm, refine, trans, equil, deterministic, tuple(grid))
    if rowperm is not None:
        if rowperm != "LargeDiag_MC64":
            raise ValueError(f"rowperm must be None or 'LargeDiag_MC64', not {rowperm!r}")
        return _gssvx3d_rowperm(n, rowptr, colind, nzval, b, perm_c, relax, maxsup, replace_tiny, keep, refine, trans, equil, deterministic)
    symb = Symbolic(n, rowptr, colind, perm_c, relax, maxsup)
    h = LUHandle.from_symbolic(symb, nzval, replace_tiny=replace_tiny, deterministic=deterministic)
    if equil:
        return _gssvx3d_equil(h, symb, n, rowptr, colind, nzval, b, keep, refine, trans)
    thresh = pivot_thresh(n, rowptr, colind, nzval) if anorm is None else 0.5 * float(np.finfo(np.float32).eps) * anorm
    info = h.pdgstrf3d(thresh)
    b = np.asfortranarray(np.array(b, dtype=np.complex128 if np.iscomplexobj(nzval) else np.float64))
    if b.ndim == 1:
        b = np.asfortranarray(b[:, None])
    xp = np.zeros_like(b, order="F")
    xp[symb.perm_c, :] = b                                     # Pc*b
    y = h.pdgstrs3d(xp, trans=trans)                           # the factors are of A1 = Pc A Pc^T: A^T x = b is A1^T (Pc x) = Pc b, the same permutation on both sides
    x = np.asfortranarray(y[symb.perm_c, :])                   # Pc^T y
    st = h.stats()
    if refine:
        h.attach_matrix(n, rowptr, colind, nzval, symb.perm_c)
        if gmres:
            x, st["berr"], st["refine_steps"], st["refine_solves"] = h.pdgsrfs3d(b, x, method="gmres")
        elif extra:
            x, st["berr"], st["refine_steps"], st["refine_dxrel"], st["refine_state"] = h.pdgsrfs3d(b, x, method="extra")
            st["refine_rho"] = h.refine_rho
        else:
            x, berr, steps = h.pdgsrfs3d(b, x, block=block)
            st["berr"] = berr; st["refine_steps"] = steps
    if keep:
        return x, info, st, h, symb
    h.destroy(); symb.free()
    return x, info, st


def _gssvx3d_grid(n, rowptr, colind, nzval, b, perm_c, relax, maxsup, replace_tiny, anorm, refine, trans, equil, deterministic, grid):
    """the grid=(Pr, Pc, Pz) path of pdgssvx3d: one thread per rank, replicated right-hand sides, every step collective"""
    from . import grid3d
    block = refine == "block"
    Pr, Pc, Pz = grid
    symb = Symbolic(n, rowptr, colind, perm_c, relax, maxsup)
    sn_tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)
    b = np.asfortranarray(np.array(b, dtype=np.complex128 if np.iscomplexobj(nzval) else np.float64))
    if b.ndim == 1:
        b = np.asfortranarray(b[:, None])

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, nzval, comms[rank], sn_tree, replace_tiny=replace_tiny, deterministic=deterministic)
        try:
            extra = {}
            if _trans_code(trans):
                h.plan_transposed()
            if equil:
                eq = h.equilibrate(n, rowptr, colind, nzval, symb.perm_c)
                info = h.pdgstrf3d(0.5 * float(np.finfo(np.float32).eps) * eq["anorm"])
                out = h.gssvx_solve(b, trans=trans, refine=refine and not block)
                extra.update(equed=eq["equed"], rowcnd=eq["rowcnd"], colcnd=eq["colcnd"], amax=eq["amax"])
                if eq["info"] > 0:
                    extra["equil_info"] = eq["info"]
                x = out
                if block:
                    x, extra["berr"], extra["refine_steps"] = _refine_scaled(h, b, x, block=True)
                elif refine:
                    x, extra["berr"], extra["refine_steps"] = out
            else:
                info = h.pdgstrf3d(pivot_thresh(n, rowptr, colind, nzval) if anorm is None else 0.5 * float(np.finfo(np.float32).eps) * anorm)
                xp = np.zeros_like(b, order="F")
                xp[symb.perm_c, :] = b
                x = np.asfortranarray(h.pdgstrs3d(xp, trans=trans)[symb.perm_c, :])
                if refine:
                    h.attach_matrix(n, rowptr, colind, nzval, symb.perm_c)
                    x, extra["berr"], extra["refine_steps"] = h.pdgsrfs3d(b, x, block=block)
            st = h.stats()
            st.update(extra)
            return x, info, st
        finally:
            h.destroy()

    try:
        out = grid3d.run_ranks(Pr * Pc * Pz, body)
    finally:
        symb.free()
    x, _, st = out[0]
    return x, max(o[1] for o in out), st


def _gssvx3d_rowperm(n, rowptr, colind, nzval, b, perm_c, relax, maxsup, replace_tiny, keep, refine, trans, equil, deterministic):
    """the RowPerm = LargeDiag_MC64 path of pdgssvx3d"""
    perm_r, r, c, rinfo = large_diag(n, rowptr, colind, nzval, scale=equil)
    if rinfo["info"] > 0:
        raise RuntimeError(f"pdgssvx3d(rowperm='LargeDiag_MC64'): the matrix is structurally singular, {rinfo['info']} rows cannot be matched")
    rp1, ci1, v1, pos = permute_rows_csr(n, rowptr, colind, nzval, perm_r)
    if perm_c is None:
        perm_c = order_nd(n, rp1, ci1)
    symb = Symbolic(n, rp1, ci1, perm_c, relax, maxsup)
    h = LUHandle.from_symbolic(symb, v1, replace_tiny=replace_tiny, deterministic=deterministic)
    h.rowperm_pos = pos
    eq = None
    if equil:
        r1 = np.empty(int(n)); r1[perm_r] = r                   # R by the rows of Pr A
        eq = h.equilibrate_with(n, rp1, ci1, v1, symb.perm_c, r1, c)
        thresh = 0.5 * float(np.finfo(np.float32).eps) * eq["anorm"]
    else:
        h.attach_matrix(n, rp1, ci1, v1, symb.perm_c)
        thresh = pivot_thresh(n, rp1, ci1, v1)
    h.set_row_perm(perm_r)
    info = h.pdgstrf3d(thresh)
    out = h.gssvx_solve(b, trans=trans, refine=refine)
    st = h.stats()
    st["rowperm"] = rinfo; st["perm_r"] = perm_r
    if eq is not None:
        st.update(equed=eq["equed"], rowcnd=eq["rowcnd"], colcnd=eq["colcnd"], amax=eq["amax"])
    x = out
    if refine:
        x, st["berr"], st["refine_steps"] = out
    if keep:
        return x, info, st, h, symb
    h.destroy(); symb.free()
    return x, info, st


def _gssvx3d_equil(h, symb, n, rowptr, colind, nzval, b, keep, refine, trans):
    """the Equil = YES path of pdgssvx3d: equilibrate on the device, thresh from the scaled matrix's 1-norm, factor, expert solve"""
    eq = h.equilibrate(n, rowptr, colind, nzval, symb.perm_c)
    info = h.pdgstrf3d(0.5 * float(np.finfo(np.float32).eps) * eq["anorm"])
    gmres, block, extra = refine == "gmres", refine == "block", refine == "extra"
    out = h.gssvx_solve(b, trans=trans, refine=refine and not gmres and not block and not extra)
    st = h.stats()
    st.update(equed=eq["equed"], rowcnd=eq["rowcnd"], colcnd=eq["colcnd"], amax=eq["amax"])
    if eq["info"] > 0:
        st["equil_info"] = eq["info"]
    x = out
    if gmres:                                                   # the attached matrix is the scaled one, R A C: refine (R A C) x' = R o b, x = C o x'
        r, c = h.scalings()
        bs = np.asfortranarray(np.array(b, dtype=x.dtype).reshape(x.shape) * r[:, None])
        xs, st["berr"], st["refine_steps"], st["refine_solves"] = h.pdgsrfs3d(bs, np.asfortranarray(x / c[:, None]), method="gmres")
        x = np.asfortranarray(xs * c[:, None])
    elif extra:                                                 # (as "gmres": the scaled system)
        r, c = h.scalings()
        bs = np.asfortranarray(np.array(b, dtype=x.dtype).reshape(x.shape) * r[:, None])
        xs, st["berr"], st["refine_steps"], st["refine_dxrel"], st["refine_state"] = h.pdgsrfs3d(bs, np.asfortranarray(x / c[:, None]), method="extra")
        st["refine_rho"] = h.refine_rho
        x = np.asfortranarray(xs * c[:, None])
    elif block:
        x, st["berr"], st["refine_steps"] = _refine_scaled(h, b, x, block=True)
    elif refine:
        x, st["berr"], st["refine_steps"] = out
    if keep:
        return x, info, st, h, symb
    h.destroy(); symb.free()
    return x, info, st


def _refine_scaled(h, b, x, **kw):
    """refinement of an equilibrated handle by hand (untransposed): the attached matrix is the scaled one, R A C -- refine (R A C) x' = R o b from x' = x / C,
    then x = C o x'.  Returns (x, berr, steps)"""
    r, c = h.scalings()
    bs = np.asfortranarray(np.array(b, dtype=x.dtype).reshape(x.shape) * r[:, None])
    xs, berr, steps = h.pdgsrfs3d(bs, np.asfortranarray(x / c[:, None]), **kw)
    return np.asfortranarray(xs * c[:, None]), berr, steps


pzgssvx3d = pdgssvx3d   # complex16 input (nzval complex) takes the pzgstrf3d / pzgstrs3d path of the same driver


class BatchHandle:
    """sluamd_batch_t: `count` matrices of one sparsity pattern on one handle (block-diagonal factorisation), with info, berr and refinement steps per
    matrix.  Values [count, nnz] in the order of the shared CSR; right-hand sides [count, n] or [count, n, nrhs].  float64 throughout; ZBatchHandle is the
    complex16 twin (sluamd_zBatch*)."""
    _p, _dt = "d", np.float64          # the precision letter of the entry points, the dtype of values, b and x

    @classmethod
    def _fn(cls, what):
        return f"sluamd_{cls._p}Batch{what}"

    def __init__(self, b, n, nnz, count):
        self._b = b
        self.n, self.nnz, self.count = int(n), int(nnz), int(count)

    @classmethod
    def create(cls, symb, nzvals, deterministic=False, device=-1, replace_tiny=False):
        """symb: the Symbolic of ONE matrix; nzvals: [count, >= nnz] (a row's first nnz values are the matrix)"""
        if cls._p == "d" and np.iscomplexobj(nzvals):
            raise ValueError("BatchHandle.create: complex16 values belong on a ZBatchHandle (BatchHandle holds double precision only)")
        nz = np.ascontiguousarray(nzvals, dtype=cls._dt)
        if nz.ndim != 2:
            raise ValueError("nzvals must be [count, nnz]")
        o = LUHandle._opts(replace_tiny=replace_tiny, deterministic=deterministic, device=device)
        b = C.c_void_p()
        _lib.check(_lib.entry(cls._fn("Create"))(C.byref(b), symb._h, nz.shape[0], _pi(symb.rowptr), _pi(symb.colind),
                                                 nz.ctypes.data_as(C.c_void_p if cls._p == "z" else _lib.P_dbl), nz.shape[1], _pi(symb.perm_c), C.byref(o)),
                   cls._fn("Create"))
        return cls(b, symb.n, len(symb.colind), nz.shape[0])

    def update_values(self, nzvals):
        """new values of the same pattern: a numpy array [count, >= nnz] (host form) or a torch device tensor of that shape (_dev form); the batch is
        unfactored afterwards"""
        if isinstance(nzvals, np.ndarray) or not hasattr(nzvals, "data_ptr"):
            nz = np.ascontiguousarray(nzvals, dtype=self._dt)
            if nz.ndim != 2 or nz.shape[0] != self.count:
                raise ValueError(f"nzvals must be [{self.count}, >= {self.nnz}]")
            _lib.check(_lib.entry(self._fn("UpdateValues"))(self._b, nz.ctypes.data_as(C.c_void_p), nz.shape[1]), self._fn("UpdateValues"))
            return
        import torch
        want = torch.complex128 if self._p == "z" else torch.float64
        if nzvals.dtype != want or nzvals.dim() != 2 or nzvals.shape[0] != self.count or not nzvals.is_contiguous() or not nzvals.is_cuda:
            raise ValueError(f"device values must be a contiguous {np.dtype(self._dt).name} device tensor [{self.count}, >= {self.nnz}]")
        torch.cuda.current_stream(nzvals.device).synchronize()      # what produced the tensor must be complete (contract of the _dev form)
        _lib.check(_lib.entry(self._fn("UpdateValues_dev"))(self._b, C.c_void_p(nzvals.data_ptr()), int(nzvals.shape[1])), self._fn("UpdateValues_dev"))

    def equilibrate(self):
        """pdgsequ + pdlaqgs per matrix (sluamd_[dz]BatchEquilibrate): a list of count dicts like LUHandle.equilibrate's (equed as "N" / "R" / "C" / "B")"""
        out = (_lib.Equil * self.count)()
        _lib.check(_lib.entry(self._fn("Equilibrate"))(self._b, out), self._fn("Equilibrate"))
        return [{"equed": EQUED[e.equed], "info": e.info, "rowcnd": e.rowcnd, "colcnd": e.colcnd, "amax": e.amax, "anorm": e.anorm} for e in out]

    def scalings(self):
        """(R, C), each [count, n]: ones where a matrix's side is not scaled"""
        r = np.ones((self.count, self.n)); c = np.ones((self.count, self.n))
        _lib.check(_lib.entry("sluamd_BatchGetScalings")(self._b, _pd(r), _pd(c)), "sluamd_BatchGetScalings")
        return r, c

    def factor(self):
        """info[count]: per matrix 0, or the 1-based column of its first exactly zero pivot"""
        info = np.zeros(self.count, dtype=np.int32)
        _lib.check(_lib.entry(self._fn("Factor"))(self._b, _pi(info)), self._fn("Factor"))
        return info

    def solve(self, b, trans="N", refine=False):
        """b: [count, n] or [count, n, nrhs] -> (x of the same shape, berr [count, nrhs] or None, steps [count]); trans = "T" / "C": A_k^T x = b / A_k^H x = b
        (the same system on a double batch), refined against the transposed system when refine is set"""
        b = np.asarray(b, dtype=self._dt)
        one = b.ndim == 2
        b3 = b[:, :, None] if one else b
        if b3.ndim != 3 or b3.shape[0] != self.count or b3.shape[1] != self.n:
            raise ValueError(f"b must be [{self.count}, {self.n}] or [{self.count}, {self.n}, nrhs]")
        nrhs = b3.shape[2]
        B = np.ascontiguousarray(b3.transpose(0, 2, 1))            # [count, nrhs, n]: every matrix's block column-major
        X = np.zeros_like(B)
        berr = np.zeros((self.count, max(nrhs, 1)))
        steps = np.zeros(self.count, dtype=np.int32)
        _lib.check(_lib.entry(self._fn("Solve"))(self._b, _trans_code(trans), B.ctypes.data_as(C.c_void_p), self.n, self.n * nrhs,
                                                 X.ctypes.data_as(C.c_void_p), self.n, self.n * nrhs, nrhs, int(bool(refine)), _pd(berr), _pi(steps)),
                   self._fn("Solve"))
        x = X.transpose(0, 2, 1)
        return (np.ascontiguousarray(x[:, :, 0]) if one else np.ascontiguousarray(x)), (berr[:, :nrhs] if refine else None), steps

    def solve_dev(self, d_b, ldb, stride_b, d_x, ldx, stride_x, nrhs, trans="N"):
        """sluamd_[dz]BatchSolve_dev without refinement: matrix k's column-major block at d_b + k stride_b / d_x + k stride_x (device pointers; ld and strides
        in values); d_b is not modified"""
        name = self._fn("Solve_dev")
        _lib.check(_lib.entry(name)(self._b, _trans_code(trans), C.c_void_p(d_b), int(ldb), int(stride_b), C.c_void_p(d_x), int(ldx), int(stride_x), int(nrhs), 0,
                                    None, None), name)

    def adjoint_values(self, lam, x, trans="N"):
        """LUHandle.adjoint_values for every matrix of the batch (sluamd_[dz]BatchAdjointValues): lam, x [count, n] or [count, n, nrhs] -> G [count, nnz]"""
        t = _trans_code(trans)
        lam, x = _adjoint_pair("adjoint_values", self._dt, lam, x, (self.count, self.n))
        nrhs = 1 if lam.ndim == 2 else lam.shape[2]
        Lm = np.ascontiguousarray(lam.reshape(self.count, self.n, nrhs).transpose(0, 2, 1))      # [count, nrhs, n]: every matrix's block column-major
        Xm = np.ascontiguousarray(x.reshape(self.count, self.n, nrhs).transpose(0, 2, 1))
        g = np.zeros((self.count, self.nnz), dtype=self._dt)
        name = self._fn("AdjointValues")
        ld = max(self.n, 1)
        _lib.check(_lib.entry(name)(self._b, t, Lm.ctypes.data_as(C.c_void_p), ld, ld * nrhs, Xm.ctypes.data_as(C.c_void_p), ld, ld * nrhs, nrhs,
                                    g.ctypes.data_as(C.c_void_p), self.nnz), name)
        return g

    def adjoint_values_dev(self, d_lam, ldl, stride_l, d_x, ldx, stride_x, nrhs, d_g, stride_g, trans="N"):
        """sluamd_[dz]BatchAdjointValues_dev on device pointers (ld and strides in values)"""
        name = self._fn("AdjointValues_dev")
        _lib.check(_lib.entry(name)(self._b, _trans_code(trans), C.c_void_p(d_lam), int(ldl), int(stride_l), C.c_void_p(d_x), int(ldx), int(stride_x), int(nrhs),
                                    C.c_void_p(d_g), int(stride_g)), name)

    def handle(self):
        """the batch's handle, borrowed (an LUHandle-shaped view for stats / setup_times / plan_table; it must not outlive the batch)"""
        fn = _lib.entry("sluamd_BatchHandle")
        return C.c_void_p(fn(self._b))

    def stats(self):
        s = Stats()
        _lib.load().sluamd_get_stats(self.handle(), C.byref(s))
        return {f[0]: getattr(s, f[0]) for f in Stats._fields_}

    def destroy(self):
        if self._b:
            _lib.entry("sluamd_BatchDestroy")(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class ZBatchHandle(BatchHandle):
    """the complex16 batch (sluamd_zBatch*): the interface of BatchHandle with complex128 values, b and x; device value updates take a contiguous complex128
    device tensor; trans = "T" and "C" differ; R, C and berr stay real"""
    _p, _dt = "z", np.complex128


def pdgssvx3d_batch(n, rowptr, colind, nzvals, b, perm_c=None, relax=32, maxsup=256, equil=False, refine=False, trans="N", deterministic=False,
                    keep=False):
    """The batched expert driver on one rank: `count` systems of one pattern, nzvals [count, nnz], b [count, n] or [count, n, nrhs].  One symbolic
    factorisation (and, when perm_c is None, one nested-dissection ordering) of ONE matrix serves the batch.  Returns (x, info[count], stats); stats carries
    the per-matrix berr [count, nrhs] and refine_steps [count] when refine is set, and the BatchHandle under "handle" with keep=True.
    equil: every matrix is equilibrated on its own; stats then holds equed [count] ("N" / "R" / "C" / "B"), rowcnd, colcnd, amax, anorm, equil_info [count].
    trans = "T" / "C": the transposed / conjugate-transposed systems, refined as such when refine is set.  pzgssvx3d_batch: the same for complex128 values."""
    return _gssvx3d_batch(BatchHandle, n, rowptr, colind, nzvals, b, perm_c, relax, maxsup, equil, refine, trans, deterministic, keep)


def pzgssvx3d_batch(n, rowptr, colind, nzvals, b, perm_c=None, relax=32, maxsup=256, equil=False, refine=False, trans="N", deterministic=False,
                    keep=False):
    """pdgssvx3d_batch on complex16 systems (ZBatchHandle): nzvals, b and x complex128, berr real"""
    return _gssvx3d_batch(ZBatchHandle, n, rowptr, colind, nzvals, b, perm_c, relax, maxsup, equil, refine, trans, deterministic, keep)


def _gssvx3d_batch(cls, n, rowptr, colind, nzvals, b, perm_c, relax, maxsup, equil, refine, trans, deterministic, keep):
    if perm_c is None:
        perm_c = order_nd(n, rowptr, colind)
    symb = Symbolic(n, rowptr, colind, perm_c, relax=relax, maxsup=min(int(maxsup), 256))
    bh = cls.create(symb, nzvals, deterministic=deterministic)
    symb.free()
    try:
        eq = bh.equilibrate() if equil else None
        info = bh.factor()
        x, berr, steps = bh.solve(b, trans=trans, refine=refine)
        st = bh.stats()
        st["count"] = bh.count
        if eq is not None:
            st["equed"] = [e["equed"] for e in eq]
            for key in ("rowcnd", "colcnd", "amax", "anorm"):
                st[key] = np.array([e[key] for e in eq])
            st["equil_info"] = np.array([e["info"] for e in eq], dtype=np.int32)
        if refine:
            st["berr"] = berr
            st["refine_steps"] = steps
    except Exception:
        bh.destroy()
        raise
    if keep:
        st["handle"] = bh
    else:
        bh.destroy()
    return x, info, st
