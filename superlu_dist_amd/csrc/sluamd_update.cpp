// sluamd_update.cpp -- same-pattern value updates for handles created from the symbolic structure: options->Fact = SamePattern_SameRowPerm of the expert driver
// (superlu_defs.h:545-566; pdgssvx3d.c:672-697: DiagScale, R and C of the previous call are inputs and the new A is scaled with them).  Contract:
// include/superlu_dist_amd.h.
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources against a CPU restatement of the older kernels only, so no file
// of that list may reference the update kernels (eng::update_*).
//
// One call queues, on the handle's stream: [the staging copy of the host-pointer form] -> [first update of a scaled handle: the (row, column) table of the owned
// entries, from the attached CSR structure] -> the zero-fill of the arena (reset_store, shared with sluamd_dResetValues) -> k_update_values (d_aval and the
// arena in one pass over the owned entries) -> [a matrix is attached: k_update_attached over the caller's CSR, with the column sums when the norm is asked for]
// -> [eq_reduce + one synchronisation for the norm].  The (row, column) table is built here and not at creation: creation is what every user pays, and only an
// equilibrated handle that is updated ever reads it; it costs one bisection of rowptr per owned entry on the device and 8 bytes per owned entry.
#include <cstring>
#include "sluamd_refine.h"

using namespace sluamd;

namespace {

int update_values(sluamd_handle_t h, const void *nzval, sluamd_update_t *out, bool z, bool host, const char *who)
{
    const std::string me = std::string(who) + ": ";
    if (!h) { set_error(me + "null handle"); return SLUAMD_EINVAL; }
    if (!nzval) { set_error(me + "null values"); return SLUAMD_EINVAL; }
    Handle *H = &h->H;
    if (H->z != z) { set_error(me + (z ? "double handle: call sluamd_dUpdateValues" : "complex16 handle: call sluamd_zUpdateValues")); return SLUAMD_EINVAL; }
    if (!H->d_apos.p || !H->d_aent.p || H->a_csr_nnz < 0) {
        set_error(me + "the handle was not created from the symbolic structure (sluamd_[dz]CreateLUHandleFromSymb[Grid]): a view-created handle takes new values in store form through sluamd_dSetValues / sluamd_zSetValues");
        return SLUAMD_EINVAL;
    }
    const bool attached = H->d_rfs_rp.p != nullptr;
    const bool scaled = H->eq_row || H->eq_col;
    if (attached && (H->rfs_z != z || H->rfs_nnz != H->a_csr_nnz)) { set_error(me + "the attached matrix is not the one the handle was created from (precision or number of entries)"); return SLUAMD_EINVAL; }
    if (out && !attached) { set_error(me + "anorm needs an attached matrix (sluamd_[dz]AttachMatrix or sluamd_[dz]Equilibrate): the handle keeps the CSR structure only with one; pass out = NULL"); return SLUAMD_EINVAL; }
    if (scaled && !H->d_upd_ij.p && !attached) { set_error(me + "the equilibrated handle has lost its attached matrix: the rows and columns of its entries cannot be rebuilt"); return SLUAMD_EINVAL; }
    HIPCHK(hipSetDevice(H->device));
    hipStream_t s = H->stream;
    const int n = (int) H->hs.n;
    const size_t esz = z ? 16 : 8;
    // every allocation before anything is queued: a call that fails here has not touched the handle's values
    if (host) if (int rc = H->d_upd_stage.reserve(H->a_csr_nnz * (z ? 2 : 1), H->device, "the staged new values")) return rc;
    if (host && !H->ev_upd) HIPCHK(hipEventCreateWithFlags(&H->ev_upd, hipEventDisableTiming));
    const bool build_ij = scaled && !H->d_upd_ij.p && H->a_nnz > 0;
    DevBuf<int2> ij;                                                         // handed to the handle with the launch that fills it
    if (build_ij) if (int rc = ij.alloc(H->a_nnz, H->device, "the rows and columns of the owned entries")) return rc;
    DevBuf<unsigned long long> red;
    if (out) if (int rc = red.alloc(3, H->device, "the reduction words of the 1-norm")) return rc;

    const void *d_nz = nzval;
    if (host && H->a_csr_nnz > 0) {
        HIPCHK(hipMemcpyAsync(H->d_upd_stage.p, nzval, esz * (size_t) H->a_csr_nnz, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(H->ev_upd, s));
        d_nz = H->d_upd_stage.p;
    }
    if (build_ij) { H->d_upd_ij = std::move(ij); eng::update_rowcol(s, H->a_nnz, n, H->d_rfs_rp.p, H->d_rfs_ci.p, H->d_aent.p, H->d_upd_ij.p); }
    const double *R = H->eq_row ? H->d_eq_r.p : nullptr, *Cs = H->eq_col ? H->d_eq_c.p : nullptr;
    if (int rc = reset_store(H, false)) return rc;
    eng::update_values(s, z, H->a_nnz, H->d_aent.p, H->d_upd_ij.p, d_nz, R, Cs, H->d_aval.p, H->d_apos.p, H->d_val.p);
    if (attached) {
        double *colsum = out ? H->d_rfs_work.p : nullptr;         // the refinement's work vector, as sluamd_[dz]Equilibrate
        if (colsum) HIPCHK(hipMemsetAsync(colsum, 0, sizeof(double) * (size_t) n, s));
        eng::update_attached(s, z, n, H->rfs_nnz, H->d_rfs_rp.p, H->d_rfs_ci.p, d_nz, R, Cs, H->d_rfs_av.p, colsum);
    }
    HIPCHK(hipGetLastError());
    if (out) {
        unsigned long long bits[3] = {~0ull, 0ull, ~0ull};
        HIPCHK(hipMemcpyAsync(red.p, bits, sizeof bits, hipMemcpyHostToDevice, s));
        eng::eq_reduce(s, n, H->d_rfs_work.p, red.p);
        HIPCHK(hipMemcpyAsync(bits, red.p, sizeof bits, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        double anorm; memcpy(&anorm, &bits[1], sizeof anorm);
        out->anorm = anorm;
        out->equed = H->eq_row ? (H->eq_col ? SLUAMD_EQUED_B : SLUAMD_EQUED_R) : (H->eq_col ? SLUAMD_EQUED_C : SLUAMD_EQUED_N);
        out->reserved = 0;
    } else if (host && H->a_csr_nnz > 0) {
        HIPCHK(hipEventSynchronize(H->ev_upd));              // the caller may reuse nzval
    }
    return 0;
}

}  // namespace

extern "C" {

int sluamd_dUpdateValues(sluamd_handle_t h, const double *nzval, sluamd_update_t *out) { return update_values(h, nzval, out, false, true, "sluamd_dUpdateValues"); }
int sluamd_dUpdateValues_dev(sluamd_handle_t h, const double *d_nzval, sluamd_update_t *out) { return update_values(h, d_nzval, out, false, false, "sluamd_dUpdateValues_dev"); }
int sluamd_zUpdateValues(sluamd_handle_t h, const sluamd_doublecomplex *nzval, sluamd_update_t *out) { return update_values(h, nzval, out, true, true, "sluamd_zUpdateValues"); }
int sluamd_zUpdateValues_dev(sluamd_handle_t h, const sluamd_doublecomplex *d_nzval, sluamd_update_t *out)
{
    return update_values(h, d_nzval, out, true, false, "sluamd_zUpdateValues_dev");
}

}  // extern "C"
