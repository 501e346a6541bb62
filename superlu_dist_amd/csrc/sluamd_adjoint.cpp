// sluamd_adjoint.cpp -- the adjoint value gradient: sluamd_[dz]AdjointValues[_dev] and sluamd_[dz]BatchAdjointValues[_dev] (contract and the formulas per trans:
// include/superlu_dist_amd.h; why one thread per entry, the entry -> row array: DESIGN.md section 4k).  The kernels read the PATTERN of the attached matrix and
// the two vectors the caller brings; no values of A, no factors.  Which vector is the kernel's P and which its Q (sluamd_akernels.inc, included here):
//   SLUAMD_NOTRANS   G[e] = - sum Lam[i, r] conj(X[j, r])      P = Lam, Q = X
//   SLUAMD_TRANS     G[e] = - sum conj(X[i, r]) Lam[j, r]      P = Lam, Q = X, SWAP          (real: P = X, Q = Lam, as SLUAMD_CONJ -- no conjugate, no swap)
//   SLUAMD_CONJ      G[e] = - sum X[i, r] conj(Lam[j, r])      P = X, Q = Lam
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources, none of which may reference a symbol of this file.
#include <algorithm>
#include "sluamd_refine.h"
#include "sluamd_akernels.inc"

using namespace sluamd;

namespace {

// the entry -> row array of the first `nnz` entries of the attached CSR (rows [0, n)), built on first use; a batch's handle asks for ONE matrix's entries, which
// are the first of its block-diagonal CSR
int ensure_rows(Handle *H, int n, int64_t nnz)
{
    if (H->d_adj_erow.p) return 0;
    if (int rc = H->d_adj_erow.alloc(nnz, H->device, "the entry -> row array of the adjoint value gradient")) return rc;
    aeng::rows(H->stream, n, (int) nnz, H->d_rfs_rp.p, H->d_adj_erow.p);
    HIPCHK(hipGetLastError());
    return 0;
}

// device pointers; `count` matrices of order n with nnz entries each over the pattern at the head of the attached CSR
int adjoint_dev(Handle *H, bool z, int trans, int n, int64_t nnz, int count, const double *Lam, int64_t ldl, int64_t strideL, const double *X, int64_t ldx,
                int64_t strideX, int32_t nrhs, double *G, int64_t strideG)
{
    hipStream_t s = H->stream;
    if (int rc = ensure_rows(H, n, nnz)) return rc;
    const bool lam_first = trans == SLUAMD_NOTRANS || (z && trans == SLUAMD_TRANS);
    const bool swap = z && trans == SLUAMD_TRANS;
    if (lam_first) aeng::values(s, z, swap, (int) nnz, H->d_adj_erow.p, H->d_rfs_ci.p, Lam, ldl, strideL, X, ldx, strideX, nrhs, G, strideG, count);
    else aeng::values(s, z, swap, (int) nnz, H->d_adj_erow.p, H->d_rfs_ci.p, X, ldx, strideX, Lam, ldl, strideL, nrhs, G, strideG, count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// host pointers: the blocks are staged as they lie (leading dimensions and strides kept) in the handle's staging block [Lam | X | G]
int adjoint_host(Handle *H, bool z, int trans, int n, int64_t nnz, int count, const double *Lam, int64_t ldl, int64_t strideL, const double *X, int64_t ldx,
                 int64_t strideX, int32_t nrhs, double *G, int64_t strideG)
{
    const size_t vs = z ? 2 : 1;
    const int64_t lenL = strideL * (count - 1) + ldl * (nrhs - 1) + n, lenX = strideX * (count - 1) + ldx * (nrhs - 1) + n, lenG = strideG * (count - 1) + nnz;
    if (int rc = H->d_adj_stage.reserve((int64_t) vs * (lenL + lenX + lenG), H->device, "the staged vectors and gradient of the adjoint value gradient")) return rc;
    double *dL = H->d_adj_stage.p, *dX = dL + vs * (size_t) lenL, *dG = dX + vs * (size_t) lenX;
    HIPCHK(hipMemcpy(dL, Lam, sizeof(double) * vs * (size_t) lenL, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dX, X, sizeof(double) * vs * (size_t) lenX, hipMemcpyHostToDevice));
    if (count > 1 && strideG > nnz) HIPCHK(hipMemcpy(dG, G, sizeof(double) * vs * (size_t) lenG, hipMemcpyHostToDevice));      // (the gaps between the blocks of G go back unchanged)
    if (int rc = adjoint_dev(H, z, trans, n, nnz, count, dL, ldl, strideL, dX, ldx, strideX, nrhs, dG, strideG)) return rc;
    HIPCHK(hipMemcpy(G, dG, sizeof(double) * vs * (size_t) lenG, hipMemcpyDeviceToHost));
    return 0;
}

// nrhs == 0: every block of G is zero
int zero_fill(Handle *H, bool z, int64_t nnz, int count, double *G, int64_t strideG, bool host)
{
    const size_t vs = z ? 2 : 1, bytes = sizeof(double) * vs * (size_t) nnz;
    for (int k = 0; k < count; ++k) {
        double *g = G + vs * (size_t) k * strideG;
        if (host) std::fill(g, g + vs * (size_t) nnz, 0.0);
        else if (bytes) HIPCHK(hipMemsetAsync(g, 0, bytes, H->stream));
    }
    if (!host) HIPCHK(hipStreamSynchronize(H->stream));
    return 0;
}

int bad_trans(int trans, const std::string &me)
{
    if (trans == SLUAMD_NOTRANS || trans == SLUAMD_TRANS || trans == SLUAMD_CONJ) return 0;
    set_error(me + "trans must be SLUAMD_NOTRANS, SLUAMD_TRANS or SLUAMD_CONJ");
    return SLUAMD_EINVAL;
}

int adjoint_entry(sluamd_handle_t h, int trans, const void *Lv, int64_t ldl, const void *Xv, int64_t ldx, int32_t nrhs, void *Gv, bool z, bool host, const char *name)
{
    const std::string me = std::string(name) + ": ";
    if (!h || !Lv || !Xv || !Gv || nrhs < 0 || ldl < h->H.hs.n || ldx < h->H.hs.n) { set_error(me + "bad adjoint arguments"); return SLUAMD_EINVAL; }
    if (int rc = bad_trans(trans, me)) return rc;
    Handle *H = &h->H;
    if (H->z != z) {
        std::string twin(name);
        twin[7] = z ? 'd' : 'z';
        set_error(me + (z ? "double" : "complex16") + " handle: call " + twin);
        return SLUAMD_EINVAL;
    }
    if (H->grid.size() > 1) { set_error(me + "the adjoint value gradient needs a 1 x 1 x 1 handle"); return SLUAMD_EINVAL; }
    if (H->batch_owned) { set_error(me + "the handle belongs to a batch (sluamd_BatchHandle): call sluamd_" + (z ? "z" : "d") + "BatchAdjointValues"); return SLUAMD_EINVAL; }
    if (int rc = rfs_checks(H)) return rc;
    if (H->d_rp_pr.p) { set_error(me + "the handle carries a row permutation (sluamd_SetRowPerm): its entries are those of Pr A, not of the caller's matrix"); return SLUAMD_EINVAL; }
    HIPCHK(hipSetDevice(H->device));
    const double *Lam = static_cast<const double *>(Lv), *X = static_cast<const double *>(Xv);
    double *G = static_cast<double *>(Gv);
    if (nrhs == 0) return zero_fill(H, z, H->rfs_nnz, 1, G, 0, host);
    return (host ? adjoint_host : adjoint_dev)(H, z, trans, (int) H->hs.n, H->rfs_nnz, 1, Lam, ldl, 0, X, ldx, 0, nrhs, G, 0);
}

int batch_entry(sluamd_batch_t b, int trans, const void *Lv, int64_t ldl, int64_t strideL, const void *Xv, int64_t ldx, int64_t strideX, int32_t nrhs, void *Gv,
                int64_t strideG, bool z, bool host, const char *name)
{
    const std::string me = std::string(name) + ": ";
    if (!b) { set_error(me + "null batch"); return SLUAMD_EINVAL; }
    int m = 0, count = 0; int64_t nnz = 0; bool bz = false;
    batch_shape(b, &m, &count, &nnz, &bz);
    if (bz != z) {
        std::string twin(name);
        twin[7] = z ? 'd' : 'z';
        set_error(me + (z ? "double" : "complex16") + " batch: call " + twin);
        return SLUAMD_EINVAL;
    }
    if (!Lv || !Xv || !Gv || nrhs < 0) { set_error(me + "null vectors or gradient, or nrhs < 0"); return SLUAMD_EINVAL; }
    if (int rc = bad_trans(trans, me)) return rc;
    if (ldl < m || ldx < m) { set_error(me + "ldl or ldx is smaller than the order of one matrix"); return SLUAMD_EINVAL; }
    if (count > 1 && (strideG < nnz || (nrhs > 0 && (strideL < ldl * (nrhs - 1) + m || strideX < ldx * (nrhs - 1) + m)))) {
        set_error(me + "strideL, strideX or strideG is smaller than one matrix's block");
        return SLUAMD_EINVAL;
    }
    Handle *H = &sluamd_BatchHandle(b)->H;
    if (!H->d_rfs_rp.p || H->rfs_nnz != nnz * count || H->hs.n != (int64_t) m * count) { set_error(me + "the matrix attached to the batch's handle is not the batch's own block-diagonal matrix"); return SLUAMD_EINVAL; }
    HIPCHK(hipSetDevice(H->device));
    const double *Lam = static_cast<const double *>(Lv), *X = static_cast<const double *>(Xv);
    double *G = static_cast<double *>(Gv);
    if (nrhs == 0) return zero_fill(H, z, nnz, count, G, strideG, host);
    return (host ? adjoint_host : adjoint_dev)(H, z, trans, m, nnz, count, Lam, ldl, strideL, X, ldx, strideX, nrhs, G, strideG);
}

}  // namespace

extern "C" {

int sluamd_dAdjointValues(sluamd_handle_t h, int trans, const double *Lam, int64_t ldl, const double *X, int64_t ldx, int32_t nrhs, double *G)
{
    return adjoint_entry(h, trans, Lam, ldl, X, ldx, nrhs, G, false, true, "sluamd_dAdjointValues");
}

int sluamd_dAdjointValues_dev(sluamd_handle_t h, int trans, const double *d_Lam, int64_t ldl, const double *d_X, int64_t ldx, int32_t nrhs, double *d_G)
{
    return adjoint_entry(h, trans, d_Lam, ldl, d_X, ldx, nrhs, d_G, false, false, "sluamd_dAdjointValues_dev");
}

int sluamd_zAdjointValues(sluamd_handle_t h, int trans, const sluamd_doublecomplex *Lam, int64_t ldl, const sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs,
                          sluamd_doublecomplex *G)
{
    return adjoint_entry(h, trans, Lam, ldl, X, ldx, nrhs, G, true, true, "sluamd_zAdjointValues");
}

int sluamd_zAdjointValues_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_Lam, int64_t ldl, const sluamd_doublecomplex *d_X, int64_t ldx, int32_t nrhs,
                              sluamd_doublecomplex *d_G)
{
    return adjoint_entry(h, trans, d_Lam, ldl, d_X, ldx, nrhs, d_G, true, false, "sluamd_zAdjointValues_dev");
}

int sluamd_dBatchAdjointValues(sluamd_batch_t b, int trans, const double *Lam, int64_t ldl, int64_t strideL, const double *X, int64_t ldx, int64_t strideX, int32_t nrhs,
                               double *G, int64_t strideG)
{
    return batch_entry(b, trans, Lam, ldl, strideL, X, ldx, strideX, nrhs, G, strideG, false, true, "sluamd_dBatchAdjointValues");
}

int sluamd_dBatchAdjointValues_dev(sluamd_batch_t b, int trans, const double *d_Lam, int64_t ldl, int64_t strideL, const double *d_X, int64_t ldx, int64_t strideX,
                                   int32_t nrhs, double *d_G, int64_t strideG)
{
    return batch_entry(b, trans, d_Lam, ldl, strideL, d_X, ldx, strideX, nrhs, d_G, strideG, false, false, "sluamd_dBatchAdjointValues_dev");
}

int sluamd_zBatchAdjointValues(sluamd_batch_t b, int trans, const sluamd_doublecomplex *Lam, int64_t ldl, int64_t strideL, const sluamd_doublecomplex *X, int64_t ldx,
                               int64_t strideX, int32_t nrhs, sluamd_doublecomplex *G, int64_t strideG)
{
    return batch_entry(b, trans, Lam, ldl, strideL, X, ldx, strideX, nrhs, G, strideG, true, true, "sluamd_zBatchAdjointValues");
}

int sluamd_zBatchAdjointValues_dev(sluamd_batch_t b, int trans, const sluamd_doublecomplex *d_Lam, int64_t ldl, int64_t strideL, const sluamd_doublecomplex *d_X,
                                   int64_t ldx, int64_t strideX, int32_t nrhs, sluamd_doublecomplex *d_G, int64_t strideG)
{
    return batch_entry(b, trans, d_Lam, ldl, strideL, d_X, ldx, strideX, nrhs, d_G, strideG, true, false, "sluamd_zBatchAdjointValues_dev");
}

}  // extern "C"
