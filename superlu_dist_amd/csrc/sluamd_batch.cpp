// sluamd_batch.cpp -- fixed-size batches: `count` systems A_k X_k = B_k of order m that share one sparsity pattern and differ in values (the role of the
// reference's pdgssvx3d_csc_batch, reached there through pddrive3d -b and MAGMA).  Contract: include/superlu_dist_amd.h.
// The batch is the block-diagonal matrix diag(A_0 .. A_{count-1}) on ONE ordinary 1 x 1 x 1 handle, planned for the replicated symbolic structure
// (sluamd_symb_replicate): count copies of one elimination tree are count-wide DAG levels of the existing factor and sweep kernels.  What this file adds are
// the per-matrix semantics around that handle -- values gathered from the strided arrays through the entry map of ONE matrix, info per matrix, right-hand sides
// packed from / unpacked to the per-matrix blocks, a refinement loop with one backward error, one step count and one continue / stop decision per matrix --
// and their kernels (sluamd_bkernels.inc, compiled here).
// Written once for both precisions (the role of pzgssvx3d_csc_batch beside pdgssvx3d_csc_batch): sluamd_batch_s::z, vs = 1 | 2 doubles per value as in
// sluamd_refine.h; values, right-hand sides and solutions travel as double arrays of vs doubles per value, strides and leading dimensions count values.
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources against a CPU restatement of the older kernels only.
#include <algorithm>
#include <cstring>
#include "sluamd_refine.h"
#include "sluamd_bkernels.inc"

using namespace sluamd;

struct sluamd_batch_s {
    sluamd_handle_t h = nullptr;        // the handle on the replicated structure (owned)
    bool z = false;                     // complex16
    int m = 0, count = 0, ns = 0;       // order, matrices, supernodes of ONE matrix
    int64_t nnz = 0;                    // entries of ONE matrix
    DevBuf<int2> d_map;                 // [nnz] (slot, offset inside the slot) of every entry of one matrix
    DevBuf<int> d_pc;                   // [m] perm_c of one matrix
    DevBuf<int64_t> d_dpos;             // [count m] arena position (in values) of every column's U diagonal entry
    DevBuf<int> d_info;                 // [count]
    DevBuf<int> d_go;                   // [count] refinement: the matrix continues
    DevBuf<unsigned long long> d_s;     // [count] refinement: backward errors of a sweep
    // (vs doubles per value)
    DevBuf<double> d_stage;                             // host-pointer value updates
    DevBuf<double> d_xp;                                // packed right-hand sides, count m x nrhs
    DevBuf<double> d_bx;                                // host-pointer solves: [B | X]
    DevBuf<double> d_bs;                                // refinement of scaled systems: B' = s_in o B, count m x nrhs
    // sluamd_[dz]BatchEquilibrate: R and C by global row / column (ones where a matrix's equed leaves that side alone), the pdlaqgs decision of every matrix
    // (bit 0: rows, bit 1: columns) on both sides, the per-matrix reduction records {min, max, first zero} x count
    DevBuf<double> d_r, d_c; DevBuf<int> d_mode; DevBuf<unsigned long long> d_red;
    std::vector<int> mode;
    bool eq_done = false, scaled = false;               // scaled: some matrix has equed != N
    bool factored = false;
};

namespace sluamd {
void batch_shape(sluamd_batch_t b, int *m, int *count, int64_t *nnz, bool *z) { *m = b->m; *count = b->count; *nnz = b->nnz; *z = b->z; }
}

namespace {

void batch_free(sluamd_batch_t b)
{
    if (!b) return;
    if (b->h) { hipSetDevice(b->h->H.device); if (b->h->H.stream) hipStreamSynchronize(b->h->H.stream); }
    if (b->h) sluamd_dDestroyLUHandle(b->h);
    delete b;       // the buffers release themselves
}

// the borrowed handle must still be the batch's own: an equilibration or a row permutation made through it would be ignored by the batch's pack / unpack
int own_state(sluamd_batch_t b, const std::string &me)
{
    const Handle *H = &b->h->H;
    if (H->eq_done || H->d_rp_pr.p) { set_error(me + "the batch's handle was equilibrated or row-permuted through sluamd_BatchHandle: RowPerm and the single-matrix equilibration are not available on a batch (sluamd_[dz]BatchEquilibrate is)"); return SLUAMD_EINVAL; }
    return 0;
}

// a d call on a complex16 batch, a z call on a double batch: `other` names the call of the batch's precision
int precision(sluamd_batch_t b, bool z, const std::string &me, const char *other)
{
    if (b->z == z) return 0;
    set_error(me + (b->z ? "complex16 batch: call " : "double batch: call ") + other);
    return SLUAMD_EINVAL;
}

// the attached values (scaled in place when the batch is equilibrated) -> the zero-filled store, through the entry map of one matrix
int store_from_attached(sluamd_batch_t b)
{
    Handle *H = &b->h->H;
    if (int rc = reset_store(H, false)) return rc;
    beng::batch_values(H->stream, b->z, b->nnz, b->count, b->ns, b->nnz, H->d_rfs_av.p, b->d_map.p, H->T.sn_lval, H->T.sn_uval, nullptr, H->d_val.p);
    HIPCHK(hipGetLastError());
    b->factored = false;
    return 0;
}

// the distribution path of value updates: k_batch_values into the attached values and the store in one pass; an equilibrated batch takes the values into the
// attached copy first, re-applies the stored R / C with every matrix's own equed ((a r[i]) c[j], as sluamd_[dz]UpdateValues), and fills the store from there
int distribute(sluamd_batch_t b, const double *d_nz, int64_t stride)
{
    Handle *H = &b->h->H;
    if (!b->scaled) {
        if (int rc = reset_store(H, false)) return rc;
        beng::batch_values(H->stream, b->z, b->nnz, b->count, b->ns, stride, d_nz, b->d_map.p, H->T.sn_lval, H->T.sn_uval, H->d_rfs_av.p, H->d_val.p);
        HIPCHK(hipGetLastError());
        b->factored = false;
        return 0;
    }
    const int64_t n = (int64_t) b->m * b->count;
    beng::batch_values(H->stream, b->z, b->nnz, b->count, b->ns, stride, d_nz, b->d_map.p, H->T.sn_lval, H->T.sn_uval, H->d_rfs_av.p, nullptr);
    HIPCHK(hipMemsetAsync(H->d_rfs_work.p, 0, sizeof(double) * (size_t) n, H->stream));
    beng::batch_eq_scale(H->stream, b->z, n, b->m, H->d_rfs_rp.p, H->d_rfs_ci.p, H->d_rfs_av.p, b->d_r.p, b->d_c.p, b->d_mode.p, H->d_rfs_work.p);
    return store_from_attached(b);
}

int update_values(sluamd_batch_t b, bool z, const double *nzval, int64_t stride, bool host, const char *who, const char *other)
{
    const std::string me = std::string(who) + ": ";
    if (!b) { set_error(me + "null batch"); return SLUAMD_EINVAL; }
    if (int rc = precision(b, z, me, other)) return rc;
    const size_t vs = z ? 2 : 1;
    if (!nzval) { set_error(me + "null values"); return SLUAMD_EINVAL; }
    if (stride < b->nnz) { set_error(me + "stride is smaller than the number of entries of one matrix"); return SLUAMD_EINVAL; }
    Handle *H = &b->h->H;
    if (int rc = own_state(b, me)) return rc;
    if (!H->d_rfs_av.p || H->rfs_nnz != b->nnz * b->count) { set_error(me + "the matrix attached to the batch's handle is not the batch's own block-diagonal matrix"); return SLUAMD_EINVAL; }
    HIPCHK(hipSetDevice(H->device));
    const double *d_nz = nzval;
    if (host) {
        const int64_t len = stride * (b->count - 1) + b->nnz;
        if (int rc = b->d_stage.reserve((int64_t) vs * len, H->device, "the staged values")) return rc;
        HIPCHK(hipMemcpyAsync(b->d_stage.p, nzval, sizeof(double) * vs * (size_t) len, hipMemcpyHostToDevice, H->stream));
        d_nz = b->d_stage.p;
    }
    if (int rc = distribute(b, d_nz, stride)) return rc;
    if (host) HIPCHK(hipStreamSynchronize(H->stream));          // the caller may reuse nzval
    return 0;
}

int solve_dev(sluamd_batch_t b, int trans, const double *B, int64_t ldb, int64_t strideB, double *X, int64_t ldx, int64_t strideX, int32_t nrhs, int refine,
              double *berr, int32_t *steps)
{
    Handle *H = &b->h->H;
    hipStream_t s = H->stream;
    const bool z = b->z;
    const size_t vs = z ? 2 : 1;
    const int m = b->m, count = b->count;
    const int64_t n = (int64_t) m * count;
    if (int rc = b->d_xp.reserve((int64_t) vs * n * nrhs, H->device, "the packed right-hand sides")) return rc;
    // A' = R A C per matrix: op = N scales B by R and X by C, op = T / C the other way round (pdgssvx3d.c:1450-1465, :1806-1821)
    const double *s_in = !b->scaled ? nullptr : trans == SLUAMD_NOTRANS ? b->d_r.p : b->d_c.p, *s_out = !b->scaled ? nullptr : trans == SLUAMD_NOTRANS ? b->d_c.p : b->d_r.p;
    beng::batch_pack(s, z, m, count, nrhs, b->d_pc.p, s_in, B, ldb, strideB, b->d_xp.p, n);
    HIPCHK(hipGetLastError());
    if (int rc = z ? sluamd_pzgstrs3d_trans_dev(b->h, trans, reinterpret_cast<sluamd_doublecomplex *>(b->d_xp.p), n, nrhs) : sluamd_pdgstrs3d_trans_dev(b->h, trans, b->d_xp.p, n, nrhs)) return rc;
    beng::batch_unpack(s, z, m, count, nrhs, b->d_pc.p, refine ? nullptr : s_out, b->d_xp.p, n, X, ldx, strideX);
    HIPCHK(hipGetLastError());
    if (!refine) { HIPCHK(hipStreamSynchronize(s)); if (steps) std::fill(steps, steps + count, 0); return 0; }
    // the SCALED system is refined, as in the reference: X holds X' (unscaled above), B' = s_in o B goes to a block of its own (matrix k at k m, ld count m),
    // and X = s_out o X' at the end
    int64_t sB = strideB;
    if (b->scaled) {
        if (int rc = b->d_bs.reserve((int64_t) vs * n * nrhs, H->device, "the scaled right-hand sides")) return rc;
        beng::batch_pack(s, z, m, count, nrhs, nullptr, s_in, B, ldb, strideB, b->d_bs.p, n);
        B = b->d_bs.p; ldb = n; sB = m;
    }
    // The loop of sluamd_refine.h with lstres, the step count and the continue / stop decision per matrix.  SAFE1 / SAFE2 from m: the constants a matrix
    // would see alone.  One D2H copy of count doubles per sweep; a column ends when no matrix continues; a matrix that has stopped keeps the X and berr of
    // its stopping sweep (its residual is still formed, its correction computed with the others', neither is used).
    // trans != N: the loop of sluamd_trefine.cpp -- the residual over the transposed index of whatever matrix is attached (the batch's own block-diagonal one, or
    // a foreign block-diagonal one), the correction by the transposed sweeps on r_perm, the same permutation on both sides
    const bool tr = trans != SLUAMD_NOTRANS, conj = z && trans == SLUAMD_CONJ;
    if (tr) { if (int rc = ensure_tindex(H, z ? "sluamd_zBatchSolve" : "sluamd_dBatchSolve")) return rc; }
    const RfsGuards g = rfs_guards(m);
    const RfsMat A = rfs_mat(H, tr);
    double *r_perm = H->d_rfs_work.p;
    std::vector<double> sv(count), lstres(count);
    std::vector<int> cnt(count), go(count), live(count);
    for (int j = 0; j < nrhs; ++j) {
        const double *Bc = B + (size_t) j * ldb * vs;
        double *Xc = X + (size_t) j * ldx * vs;
        std::fill(lstres.begin(), lstres.end(), 3.0); std::fill(cnt.begin(), cnt.end(), 0); std::fill(live.begin(), live.end(), 1);
        for (;;) {
            HIPCHK(hipMemsetAsync(b->d_s.p, 0, sizeof(unsigned long long) * count, s));
            beng::batch_residual(s, z, conj, A, m, Xc, strideX, Bc, sB, r_perm, b->d_s.p, g.safe1, g.safe2);
            HIPCHK(hipMemcpyAsync(sv.data(), b->d_s.p, sizeof(double) * count, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            int any = 0;
            for (int k = 0; k < count; ++k) {
                go[k] = 0;
                if (!live[k]) continue;
                berr[(size_t) k * nrhs + j] = sv[k];
                go[k] = rfs_continue(sv[k], lstres[k], cnt[k]) ? 1 : 0;
                if (!go[k]) live[k] = 0;
                any |= go[k];
            }
            if (!any) break;
            HIPCHK(hipMemcpyAsync(b->d_go.p, go.data(), sizeof(int) * count, hipMemcpyHostToDevice, s));
            if (int rc = tr ? run_tsolve(H, conj, r_perm, n, 1) : run_solve_dev(H, r_perm, n, 1)) return rc;
            beng::batch_update(s, z, n, m, H->d_rfs_pc.p, b->d_go.p, r_perm, Xc, strideX);
            HIPCHK(hipStreamSynchronize(s));          // go[] is pageable host memory, rewritten by the next sweep
            for (int k = 0; k < count; ++k) if (go[k]) { lstres[k] = sv[k]; ++cnt[k]; }
        }
    }
    if (b->scaled) beng::batch_scale_x(s, z, m, count, nrhs, s_out, X, ldx, strideX);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (steps) std::copy(cnt.begin(), cnt.end(), steps);
    return 0;
}

int solve(sluamd_batch_t b, bool z, int trans, const double *B, int64_t ldb, int64_t strideB, double *X, int64_t ldx, int64_t strideX, int32_t nrhs, int refine,
          double *berr, int32_t *steps, bool host, const char *who, const char *other)
{
    const std::string me = std::string(who) + ": ";
    if (!b) { set_error(me + "null batch"); return SLUAMD_EINVAL; }
    if (int rc = precision(b, z, me, other)) return rc;
    const size_t vs = z ? 2 : 1;
    if (!B || !X || nrhs < 0) { set_error(me + "null right-hand sides or solutions, or nrhs < 0"); return SLUAMD_EINVAL; }
    if (trans != SLUAMD_NOTRANS && trans != SLUAMD_TRANS && trans != SLUAMD_CONJ) { set_error(me + "trans must be SLUAMD_NOTRANS, SLUAMD_TRANS or SLUAMD_CONJ"); return SLUAMD_EINVAL; }
    if (ldb < b->m || ldx < b->m) { set_error(me + "ldb or ldx is smaller than the order of one matrix"); return SLUAMD_EINVAL; }
    if (nrhs > 0 && b->count > 1 && (strideB < ldb * (nrhs - 1) + b->m || strideX < ldx * (nrhs - 1) + b->m)) { set_error(me + "strideB or strideX is smaller than one matrix's block"); return SLUAMD_EINVAL; }
    if (refine && !berr) { set_error(me + "refine needs berr[count * nrhs]"); return SLUAMD_EINVAL; }
    if (!b->factored) { set_error(me + "the batch holds no factors: call sluamd_" + (z ? "z" : "d") + "BatchFactor first (value updates leave the batch unfactored)"); return SLUAMD_EINVAL; }
    Handle *H = &b->h->H;
    if (int rc = own_state(b, me)) return rc;
    if (refine && (!H->d_rfs_rp.p || H->rfs_z != z || H->hs.n != (int64_t) b->m * b->count)) { set_error(me + "no " + (z ? "complex16" : "double") + " matrix is attached to the batch's handle"); return SLUAMD_EINVAL; }
    if (nrhs == 0) { if (steps) std::fill(steps, steps + b->count, 0); return 0; }
    HIPCHK(hipSetDevice(H->device));
    if (!host) return solve_dev(b, trans, B, ldb, strideB, X, ldx, strideX, nrhs, refine, berr, steps);
    // host pointers: the blocks are staged as they lie (strides kept), B behind X in one buffer
    const int64_t lenB = strideB * (b->count - 1) + ldb * (nrhs - 1) + b->m, lenX = strideX * (b->count - 1) + ldx * (nrhs - 1) + b->m;
    if (int rc = b->d_bx.reserve((int64_t) vs * (lenB + lenX), H->device, "the staged right-hand sides and solutions")) return rc;
    double *dB = b->d_bx.p, *dX = b->d_bx.p + vs * (size_t) lenB;
    HIPCHK(hipMemcpy(dB, B, sizeof(double) * vs * (size_t) lenB, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dX, X, sizeof(double) * vs * (size_t) lenX, hipMemcpyHostToDevice));      // (the gaps between the blocks of X go back unchanged)
    if (int rc = solve_dev(b, trans, dB, ldb, strideB, dX, ldx, strideX, nrhs, refine, berr, steps)) return rc;
    HIPCHK(hipMemcpy(X, dX, sizeof(double) * vs * (size_t) lenX, hipMemcpyDeviceToHost));
    return 0;
}

// nzval: vs doubles per value, matrix k at nzval + vs k stride
int create(sluamd_batch_t *out, bool z, sluamd_symb_t s, int32_t count, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const double *nzval, int64_t stride,
           const sluamd_int_t *perm_c_final, const sluamd_options_t *opt, const char *who)
{
    const std::string me = std::string(who) + ": ";
    const size_t vs = z ? 2 : 1;
    if (!out) { set_error(me + "null batch pointer"); return SLUAMD_EINVAL; }
    *out = nullptr;
    if (!s || !rowptr || !colind || !nzval || !perm_c_final) { set_error(me + "null argument"); return SLUAMD_EINVAL; }
    if (count <= 0) { set_error(me + "count must be positive"); return SLUAMD_EINVAL; }
    if (opt && opt->replace_tiny_pivot) { set_error(me + "replace_tiny_pivot is not available on a batch (it needs a threshold eps * anorm_k per matrix inside the diagonal LU kernels)"); return SLUAMD_EINVAL; }
    const Symb *sy = reinterpret_cast<const Symb *>(s);
    const int64_t m = sy->hs.n, nnz = rowptr[m];
    if (stride < nnz) { set_error(me + "stride is smaller than the number of entries of one matrix"); return SLUAMD_EINVAL; }
    if (m * count > 0x7fffffffLL || nnz * count > 0x7fffffffLL) { set_error(me + "count * n or count * nnz exceeds the 32-bit indices of the ABI"); return SLUAMD_EINVAL; }
    for (int k = 0; k < sy->hs.nsupers; ++k)
        if (sy->hs.xsup[k + 1] - sy->hs.xsup[k] > 256) { set_error(me + "a supernode is wider than 256 columns: build the symbolic structure with maxsup <= 256"); return SLUAMD_EINVAL; }
    // entry map of ONE matrix: (slot, offset inside the slot); the value offsets of a Symb ascend by supernode, L and U separately
    std::vector<int64_t> pos; std::vector<uint8_t> isu;
    compute_scatter_positions(*sy, sy->hs, m, rowptr, colind, perm_c_final, nullptr, pos, isu);
    std::vector<int2> map((size_t) nnz);
    for (int64_t i = 0; i < m; ++i)
        for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            if (pos[e] < 0) { set_error(me + "A entry outside the symbolic structure"); return SLUAMD_ESTRUCT; }
            const int pi = perm_c_final[i], pj = perm_c_final[colind[e]];
            const int slot = isu[e] ? sy->supno[pi] : sy->supno[pj];
            const int64_t off = pos[e] - (isu[e] ? sy->hs.uval_off[slot] : sy->hs.lval_off[slot]);
            map[e] = make_int2(isu[e] ? ~slot : slot, (int) off);
        }
    // the handle on the replicated structure; its arena is zero-filled and it keeps no entry map
    sluamd_symb_t big = nullptr;
    if (int rc = sluamd_symb_replicate(s, count, &big)) return rc;
    sluamd_batch_t b = new sluamd_batch_s();
    b->z = z; b->m = (int) m; b->count = count; b->ns = sy->hs.nsupers; b->nnz = nnz;
    int rc = create_symb_handle_empty(&b->h, big, opt, z);
    sluamd_symb_free(big);
    if (rc) { batch_free(b); return rc; }
    Handle *H = &b->h->H;
    H->batch_owned = true;
    auto fail = [&](int code, const char *what) { if (what) set_error(me + what); batch_free(b); return code; };
    if (H->split.active) return fail(SLUAMD_EINVAL, "the handle refined a wide supernode");
    {   // the block-diagonal CSR with its values, attached as sluamd_[dz]AttachMatrix would (the refinement and the equilibration read it): the one upload of the values
        const int64_t n = m * count;
        std::vector<int> rp((size_t) n + 1), ci((size_t) (nnz * count)), pc((size_t) n);
        std::vector<double> av(vs * (size_t) (nnz * count));
        for (int k = 0; k < count; ++k) {
            for (int64_t i = 0; i < m; ++i) { rp[(size_t) (k * m + i)] = rowptr[i] + (int) (k * nnz); pc[(size_t) (k * m + i)] = perm_c_final[i] + (int) (k * m); }
            for (int64_t e = 0; e < nnz; ++e) ci[(size_t) (k * nnz + e)] = colind[e] + (int) (k * m);
            std::memcpy(av.data() + vs * (size_t) (k * nnz), nzval + vs * (size_t) (k * stride), sizeof(double) * vs * (size_t) nnz);
        }
        rp[(size_t) n] = (int) (nnz * count);
        if ((rc = attach_rfs(b->h, (sluamd_int_t) n, rp.data(), ci.data(), av.data(), pc.data(), z, who))) return fail(rc, nullptr);
        // position of every column's diagonal entry: the diagonal block lies at the top of the column's own L slot (slot offsets and leading dimensions count
        // values in either precision: a complex16 store is an array of 16-byte values)
        std::vector<int64_t> dpos((size_t) n);
        for (int K = 0; K < H->hs.nsupers; ++K) {
            if (!(H->h_flags[K] & SNF_OWN_DIAG)) return fail(SLUAMD_ESTRUCT, "a diagonal block is not stored at the top of its own L slot");     // (always is on 1 x 1 x 1)
            for (int c = H->hs.xsup[K]; c < H->hs.xsup[K + 1]; ++c) dpos[c] = H->h_dptr[K] + (int64_t) (c - H->hs.xsup[K]) * (std::max(H->h_nsupr[K], 1) + 1);
        }
        const int dev = H->device;
        if ((rc = b->d_map.alloc(nnz, dev, "the batch's entry map")) || (rc = b->d_pc.alloc(m, dev, "the batch's perm_c")) ||
            (rc = b->d_dpos.alloc(n, dev, "the batch's diagonal positions")) || (rc = b->d_info.alloc(count, dev, "the batch's info words")) ||
            (rc = b->d_go.alloc(count, dev, "the batch's refinement flags")) || (rc = b->d_s.alloc(count, dev, "the batch's backward-error words")) ||
            (rc = b->d_mode.alloc(count, dev, "the batch's scaling modes")) || (rc = b->d_red.alloc(3 * (int64_t) count, dev, "the batch's reduction records")))
            return fail(rc, nullptr);
        if (hipMemcpy(b->d_map.p, map.data(), sizeof(int2) * nnz, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(b->d_pc.p, perm_c_final, sizeof(int) * m, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(b->d_dpos.p, dpos.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice) != hipSuccess) return fail(SLUAMD_EHIP, "hipMemcpy failed");
    }
    // the store takes the values from the attached copy, through the kernel and the entry map sluamd_[dz]BatchUpdateValues uses: they cross to the device once
    if ((rc = store_from_attached(b))) return fail(rc, nullptr);
    if (hipStreamSynchronize(H->stream) != hipSuccess) return fail(SLUAMD_EHIP, "the distribution kernel failed");
    H->setup.lap("batch.values");
    *out = b;
    return 0;
}

int factor(sluamd_batch_t b, bool z, int32_t *info, const char *who, const char *other)
{
    const std::string me = std::string(who) + ": ";
    if (!b || !info) { set_error(me + "null batch or null info"); return SLUAMD_EINVAL; }
    if (int rc = precision(b, z, me, other)) return rc;
    Handle *H = &b->h->H;
    if (int rc = own_state(b, me)) return rc;
    HIPCHK(hipSetDevice(H->device));
    int all = 0;
    if (int rc = z ? sluamd_pzgstrf3d(b->h, 0.0, &all) : sluamd_pdgstrf3d(b->h, 0.0, &all)) return rc;
    // per matrix: the smallest column whose U diagonal entry is exactly zero (complex16: 0 + 0i), over a preset of INT_MAX
    std::vector<int> h((size_t) b->count, 0x7fffffff);
    HIPCHK(hipMemcpyAsync(b->d_info.p, h.data(), sizeof(int) * b->count, hipMemcpyHostToDevice, H->stream));
    beng::batch_info(H->stream, z, (int64_t) b->m * b->count, b->m, b->d_dpos.p, H->d_val.p, b->d_info.p);
    HIPCHK(hipMemcpyAsync(h.data(), b->d_info.p, sizeof(int) * b->count, hipMemcpyDeviceToHost, H->stream));
    HIPCHK(hipStreamSynchronize(H->stream));
    HIPCHK(hipGetLastError());
    for (int k = 0; k < b->count; ++k) info[k] = h[k] == 0x7fffffff ? 0 : h[k];
    b->factored = true;
    return 0;
}

// pdgsequ + pdlaqgs (pzgsequ + pzlaqgs) per matrix.  The maxima per row and column come from the kernels of the single-matrix equilibration on the attached block-diagonal CSR
// (they are per row / column already); the reductions, the decision and the scaling are per matrix: count small records to the host per reduction
int equilibrate(sluamd_batch_t b, bool z, sluamd_equil_t *out, const char *who, const char *other)
{
    const std::string me = std::string(who) + ": ";
    if (!b || !out) { set_error(me + "null batch or null result array"); return SLUAMD_EINVAL; }
    if (int rc = precision(b, z, me, other)) return rc;
    Handle *H = &b->h->H;
    if (int rc = own_state(b, me)) return rc;
    if (b->eq_done) { set_error(me + "the batch has been equilibrated already"); return SLUAMD_EINVAL; }
    if (!H->d_rfs_av.p || H->rfs_nnz != b->nnz * b->count) { set_error(me + "the matrix attached to the batch's handle is not the batch's own block-diagonal matrix"); return SLUAMD_EINVAL; }
    HIPCHK(hipSetDevice(H->device));
    typedef unsigned long long u64;
    const int m = b->m, count = b->count;
    const int64_t n = (int64_t) m * count, nnz = H->rfs_nnz;
    hipStream_t s = H->stream;
    if (!b->d_r) {
        int rc;
        if ((rc = b->d_r.alloc(n, H->device, "the batch's row scalings R")) || (rc = b->d_c.alloc(n, H->device, "the batch's column scalings C"))) { b->d_r.reset(); return rc; }
    }
    std::vector<u64> red((size_t) 3 * count), init((size_t) 3 * count);
    for (int k = 0; k < count; ++k) { init[3 * k] = ~0ull; init[3 * k + 1] = 0; init[3 * k + 2] = ~0ull; }
    auto seg = [&](const double *v) -> int {     // red[3 k ..] = {min, max, first zero} of matrix k's part of v
        HIPCHK(hipMemcpyAsync(b->d_red.p, init.data(), sizeof(u64) * init.size(), hipMemcpyHostToDevice, s));
        beng::batch_seg_reduce(s, n, m, v, b->d_red.p);
        HIPCHK(hipMemcpyAsync(red.data(), b->d_red.p, sizeof(u64) * red.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    };
    auto dbl = [](u64 v) { double d; memcpy(&d, &v, sizeof d); return d; };
    const double smlnum = 0x1p-1022, bignum = 1.0 / smlnum;
    const double THRESH = 0.1, small = smlnum / 0x1p-52, large = 1.0 / small;
    for (int k = 0; k < count; ++k) out[k] = sluamd_equil_t{SLUAMD_EQUED_N, 0, 0.0, 0.0, 0.0, 0.0};
    // rows (pdgsequ.c:130-169); the global record of eq_rowmax lands in the first slot of d_red and is not read
    HIPCHK(hipMemcpyAsync(b->d_red.p, init.data(), sizeof(u64) * 3, hipMemcpyHostToDevice, s));
    eng::eq_rowmax(s, z, (int) n, nnz, H->d_rfs_rp.p, H->d_rfs_av.p, b->d_r.p, b->d_red.p);
    if (int rc = seg(b->d_r.p)) return rc;
    for (int k = 0; k < count; ++k) {
        const double rcmin = std::min(bignum, dbl(red[3 * k])), rcmax = dbl(red[3 * k + 1]);
        out[k].amax = rcmax;
        if (rcmin == 0.0) out[k].info = (int32_t) red[3 * k + 2] + 1;
        else out[k].rowcnd = std::max(rcmin, smlnum) / std::min(rcmax, bignum);
    }
    eng::eq_invert(s, (int) n, b->d_r.p, smlnum, bignum);
    // columns under the row scaling (:174-213); a matrix that stopped at a zero row is carried along and not read
    HIPCHK(hipMemsetAsync(b->d_c.p, 0, sizeof(double) * (size_t) n, s));
    eng::eq_colmax(s, z, (int) n, nnz, H->d_rfs_rp.p, H->d_rfs_ci.p, H->d_rfs_av.p, b->d_r.p, b->d_c.p);
    if (int rc = seg(b->d_c.p)) return rc;
    b->mode.assign(count, 0);
    b->scaled = false;
    for (int k = 0; k < count; ++k) {
        if (out[k].info) continue;
        const double rcmin = std::min(bignum, dbl(red[3 * k])), rcmax = dbl(red[3 * k + 1]);
        if (rcmin == 0.0) { out[k].info = m + (int32_t) red[3 * k + 2] + 1; continue; }
        out[k].colcnd = std::max(rcmin, smlnum) / std::min(rcmax, bignum);
        int md;                                                                            // pdlaqgs.c:107-146
        if (out[k].rowcnd >= THRESH && out[k].amax >= small && out[k].amax <= large) md = out[k].colcnd >= THRESH ? 0 : 2;
        else md = out[k].colcnd >= THRESH ? 1 : 3;
        b->mode[k] = md;
        out[k].equed = md == 0 ? SLUAMD_EQUED_N : md == 1 ? SLUAMD_EQUED_R : md == 2 ? SLUAMD_EQUED_C : SLUAMD_EQUED_B;
        if (md) b->scaled = true;
    }
    eng::eq_invert(s, (int) n, b->d_c.p, smlnum, bignum);
    HIPCHK(hipMemcpyAsync(b->d_mode.p, b->mode.data(), sizeof(int) * count, hipMemcpyHostToDevice, s));
    // every matrix's own scaling in place + the column sums of what is left; anorm per matrix = the largest of its column sums
    HIPCHK(hipMemsetAsync(H->d_rfs_work.p, 0, sizeof(double) * (size_t) n, s));
    beng::batch_eq_scale(s, z, n, m, H->d_rfs_rp.p, H->d_rfs_ci.p, H->d_rfs_av.p, b->d_r.p, b->d_c.p, b->d_mode.p, H->d_rfs_work.p);
    if (int rc = seg(H->d_rfs_work.p)) return rc;
    for (int k = 0; k < count; ++k) out[k].anorm = dbl(red[3 * k + 1]);
    beng::batch_eq_ones(s, n, m, b->d_mode.p, b->d_r.p, b->d_c.p);
    if (b->scaled) { if (int rc = store_from_attached(b)) return rc; }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    b->eq_done = true;
    return 0;
}

}  // namespace

extern "C" {

int sluamd_dBatchCreate(sluamd_batch_t *out, sluamd_symb_t s, int32_t count, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const double *nzval,
                        int64_t stride, const sluamd_int_t *perm_c_final, const sluamd_options_t *opt)
{
    return create(out, false, s, count, rowptr, colind, nzval, stride, perm_c_final, opt, "sluamd_dBatchCreate");
}

int sluamd_zBatchCreate(sluamd_batch_t *out, sluamd_symb_t s, int32_t count, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const sluamd_doublecomplex *nzval,
                        int64_t stride, const sluamd_int_t *perm_c_final, const sluamd_options_t *opt)
{
    return create(out, true, s, count, rowptr, colind, reinterpret_cast<const double *>(nzval), stride, perm_c_final, opt, "sluamd_zBatchCreate");
}

int sluamd_dBatchUpdateValues(sluamd_batch_t b, const double *nzval, int64_t stride) { return update_values(b, false, nzval, stride, true, "sluamd_dBatchUpdateValues", "sluamd_zBatchUpdateValues"); }
int sluamd_dBatchUpdateValues_dev(sluamd_batch_t b, const double *d_nzval, int64_t stride) { return update_values(b, false, d_nzval, stride, false, "sluamd_dBatchUpdateValues_dev", "sluamd_zBatchUpdateValues_dev"); }
int sluamd_zBatchUpdateValues(sluamd_batch_t b, const sluamd_doublecomplex *nzval, int64_t stride)
{
    return update_values(b, true, reinterpret_cast<const double *>(nzval), stride, true, "sluamd_zBatchUpdateValues", "sluamd_dBatchUpdateValues");
}
int sluamd_zBatchUpdateValues_dev(sluamd_batch_t b, const sluamd_doublecomplex *d_nzval, int64_t stride)
{
    return update_values(b, true, reinterpret_cast<const double *>(d_nzval), stride, false, "sluamd_zBatchUpdateValues_dev", "sluamd_dBatchUpdateValues_dev");
}

int sluamd_dBatchFactor(sluamd_batch_t b, int32_t *info) { return factor(b, false, info, "sluamd_dBatchFactor", "sluamd_zBatchFactor"); }
int sluamd_zBatchFactor(sluamd_batch_t b, int32_t *info) { return factor(b, true, info, "sluamd_zBatchFactor", "sluamd_dBatchFactor"); }

int sluamd_dBatchEquilibrate(sluamd_batch_t b, sluamd_equil_t *out) { return equilibrate(b, false, out, "sluamd_dBatchEquilibrate", "sluamd_zBatchEquilibrate"); }
int sluamd_zBatchEquilibrate(sluamd_batch_t b, sluamd_equil_t *out) { return equilibrate(b, true, out, "sluamd_zBatchEquilibrate", "sluamd_dBatchEquilibrate"); }

/* R[count m] and C[count m] to the host (either may be NULL), matrix-major; ones where a matrix's side is not scaled, also before any equilibration */
int sluamd_BatchGetScalings(sluamd_batch_t b, double *r, double *c)
{
    if (!b) { set_error("sluamd_BatchGetScalings: null batch"); return SLUAMD_EINVAL; }
    const size_t n = (size_t) b->m * b->count;
    if (!b->eq_done) { if (r) std::fill(r, r + n, 1.0); if (c) std::fill(c, c + n, 1.0); return 0; }
    HIPCHK(hipSetDevice(b->h->H.device));
    if (r) HIPCHK(hipMemcpy(r, b->d_r.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (c) HIPCHK(hipMemcpy(c, b->d_c.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

int sluamd_dBatchSolve(sluamd_batch_t b, int trans, const double *B, int64_t ldb, int64_t strideB, double *X, int64_t ldx, int64_t strideX, int32_t nrhs,
                       int refine, double *berr, int32_t *steps)
{
    return solve(b, false, trans, B, ldb, strideB, X, ldx, strideX, nrhs, refine, berr, steps, true, "sluamd_dBatchSolve", "sluamd_zBatchSolve");
}

int sluamd_dBatchSolve_dev(sluamd_batch_t b, int trans, const double *d_B, int64_t ldb, int64_t strideB, double *d_X, int64_t ldx, int64_t strideX, int32_t nrhs,
                           int refine, double *berr, int32_t *steps)
{
    return solve(b, false, trans, d_B, ldb, strideB, d_X, ldx, strideX, nrhs, refine, berr, steps, false, "sluamd_dBatchSolve_dev", "sluamd_zBatchSolve_dev");
}

int sluamd_zBatchSolve(sluamd_batch_t b, int trans, const sluamd_doublecomplex *B, int64_t ldb, int64_t strideB, sluamd_doublecomplex *X, int64_t ldx, int64_t strideX,
                       int32_t nrhs, int refine, double *berr, int32_t *steps)
{
    return solve(b, true, trans, reinterpret_cast<const double *>(B), ldb, strideB, reinterpret_cast<double *>(X), ldx, strideX, nrhs, refine, berr, steps, true,
                 "sluamd_zBatchSolve", "sluamd_dBatchSolve");
}

int sluamd_zBatchSolve_dev(sluamd_batch_t b, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, int64_t strideB, sluamd_doublecomplex *d_X, int64_t ldx,
                           int64_t strideX, int32_t nrhs, int refine, double *berr, int32_t *steps)
{
    return solve(b, true, trans, reinterpret_cast<const double *>(d_B), ldb, strideB, reinterpret_cast<double *>(d_X), ldx, strideX, nrhs, refine, berr, steps, false,
                 "sluamd_zBatchSolve_dev", "sluamd_dBatchSolve_dev");
}

sluamd_handle_t sluamd_BatchHandle(sluamd_batch_t b) { return b ? b->h : nullptr; }

void sluamd_BatchDestroy(sluamd_batch_t b) { batch_free(b); }

}  // extern "C"
