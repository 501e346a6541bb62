// sluamd_xrefine.cpp -- extra-precise iterative refinement, IterRefine = SLU_EXTRA: sluamd_p[dz]gsrfs3d_extra[_dev], and the residual of the attached
// matrix on its own, sluamd_[dz]Residual[_dev] (contract: include/superlu_dist_amd.h; the loop and why berr cannot stop it: DESIGN.md "Extra-precise
// refinement").  The residual of a step is accumulated in twice the working precision (sluamd_xkernels.inc, included here), the correction and the update are
// the policies' K::solve and K::update (sluamd_refine.h), and the loop watches the corrections: it ends when one is below eps relative to x, when one fails
// to halve, or after ITMAX steps.  x stays fp64.
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources, none of which may reference a symbol of this file.
#include <algorithm>
#include <cmath>
#include <limits>
#include "sluamd_refine.h"
#include "sluamd_xkernels.inc"

using namespace sluamd;

namespace {

constexpr int XR_ITMAX = 20;                                    // pdgsrfs.c:371

// the pass of a step: r_out = b - op(A) x with the output index pc (null: the caller's ordering); returns the backward error in *sv
template <class K> int xr_pass(Handle *H, bool extra, const double *x, const double *b, const int *pc, double *r_out, const RfsGuards &g, double *sv)
{
    hipStream_t s = H->stream;
    HIPCHK(hipMemsetAsync(H->d_rfs_s.p, 0, sizeof(unsigned long long), s));
    xeng::residual(s, K::z, K::trans == 2, extra, rfs_mat(H, K::trans != 0), x, b, pc, r_out, H->d_rfs_s.p, g.safe1, g.safe2);
    HIPCHK(hipMemcpyAsync(sv, H->d_rfs_s.p, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// d_B, d_X: device-resident, original ordering, column-major (ld in values); X holds the initial solution and is refined in place
template <class K> int xrfs_dev(Handle *H, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, double *berr, sluamd_xrefine_t *out)
{
    const int vs = K::z ? 2 : 1;
    const int n = (int) H->hs.n;
    const RfsGuards g = rfs_guards(n);
    double *r_perm = H->d_rfs_work.p;
    hipStream_t s = H->stream;
    for (int j = 0; j < nrhs; ++j) {
        const double *Bc = d_B + (size_t) j * ldb * vs;
        double *Xc = d_X + (size_t) j * ldx * vs;
        double prev = std::numeric_limits<double>::infinity(), rho = 0.0, dxrel = 0.0;
        int count = 0, state = SLUAMD_XR_LIMIT;
        for (;;) {
            if (int rc = xr_pass<K>(H, true, Xc, Bc, H->d_rfs_pc.p, r_perm, g, berr + j)) return rc;
            if (count == XR_ITMAX) { state = SLUAMD_XR_LIMIT; break; }
            if (int rc = K::solve(H, r_perm, n)) return rc;
            double nrm[2] = {0.0, 0.0};                         // max abs1(dx), max abs1(x) of the x the correction belongs to
            HIPCHK(hipMemsetAsync(H->d_xr_s.p, 0, 2 * sizeof(unsigned long long), s));
            xeng::norms(s, K::z, n, r_perm, Xc, H->d_xr_s.p);
            HIPCHK(hipMemcpyAsync(nrm, H->d_xr_s.p, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            const double ndx = nrm[0], nx = nrm[1];
            dxrel = ndx == 0.0 ? 0.0 : ndx / nx;
            if (ndx == 0.0) { state = SLUAMD_XR_CONVERGED; break; }
            // a correction that did not halve, or one that is not finite (the norms count a NaN as +inf), is dropped: berr belongs to the x that stays
            if ((count > 0 && 2 * ndx > prev) || !std::isfinite(ndx)) { state = SLUAMD_XR_NO_PROGRESS; break; }
            K::update(s, H, r_perm, Xc);
            ++count;
            if (count > 1) rho = std::max(rho, ndx / prev);
            if (ndx <= RFS_EPS * nx) {
                if (int rc = xr_pass<K>(H, true, Xc, Bc, H->d_rfs_pc.p, r_perm, g, berr + j)) return rc;
                state = SLUAMD_XR_CONVERGED;
                break;
            }
            prev = ndx;
        }
        if (out) { out[j].dxrel = dxrel; out[j].rho = rho; out[j].steps = count; out[j].state = state; }
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return 0;
}

// B, X: host memory; one column at a time through the resident work vectors of the plain refinement (r_perm | b | x), as rfs_host
template <class K> int xrfs_host(Handle *H, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, double *berr, sluamd_xrefine_t *out)
{
    const int vs = K::z ? 2 : 1;
    const int64_t n = H->hs.n;
    const size_t col = sizeof(double) * (size_t) n * vs;
    double *d_b = H->d_rfs_work.p + (size_t) n * vs, *d_x = H->d_rfs_work.p + 2 * (size_t) n * vs;
    for (int j = 0; j < nrhs; ++j) {
        HIPCHK(hipMemcpy(d_b, B + (size_t) j * ldb * vs, col, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_x, X + (size_t) j * ldx * vs, col, hipMemcpyHostToDevice));
        if (int rc = xrfs_dev<K>(H, d_b, n, d_x, n, 1, berr + j, out ? out + j : nullptr)) return rc;
        HIPCHK(hipMemcpy(X + (size_t) j * ldx * vs, d_x, col, hipMemcpyDeviceToHost));
    }
    return 0;
}

int xrefine_entry(sluamd_handle_t h, int trans, const void *Bv, int64_t ldb, void *Xv, int64_t ldx, int32_t nrhs, double *berr, sluamd_xrefine_t *out, bool z, bool host,
                  const char *name)
{
    const int c = check_solve_args(h, trans, Bv, ldb, Xv, ldx, nrhs, berr, true, z, name, "refinement");
    if (c < 0) return c;
    const std::string me = std::string(name) + ": ";
    Handle *H = &h->H;
    if (H->grid.size() > 1) { set_error(me + "the extra-precise refinement needs a 1 x 1 x 1 handle (grid handles refine with sluamd_p[dz]gsrfs3d[_trans])"); return SLUAMD_EINVAL; }
    if (H->batch_owned) { set_error(me + "the handle belongs to a batch (sluamd_BatchHandle): the extra-precise refinement does not run on batches"); return SLUAMD_EINVAL; }
    if (int rc = z ? rfs_checks<Rfs<true, 0>>(H) : rfs_checks<Rfs<false, 0>>(H)) return rc;
    if (nrhs == 0) return 0;
    HIPCHK(hipSetDevice(H->device));
    if (trans != SLUAMD_NOTRANS) { if (int rc = ensure_tindex(H, name)) return rc; }
    if (!H->d_xr_s.p) { if (int rc = H->d_xr_s.alloc(2, H->device, "the norm words of the extra-precise refinement")) return rc; }
    const double *B = static_cast<const double *>(Bv);
    double *X = static_cast<double *>(Xv);
    return rfs_dispatch(z, trans, [&](auto K) { return host ? xrfs_host<decltype(K)>(H, B, ldb, X, ldx, nrhs, berr, out) : xrfs_dev<decltype(K)>(H, B, ldb, X, ldx, nrhs, berr, out); });
}

// R = B - op(A) X, column by column; host: through the resident work vectors (r | b | x)
template <class K> int residual_cols(Handle *H, bool extra, const double *B, int64_t ldb, const double *X, int64_t ldx, int32_t nrhs, double *R, int64_t ldr, double *berr,
                                     bool host)
{
    const int vs = K::z ? 2 : 1;
    const int64_t n = H->hs.n;
    const RfsGuards g = rfs_guards(n);
    const size_t col = sizeof(double) * (size_t) n * vs;
    double *d_r = H->d_rfs_work.p, *d_b = d_r + (size_t) n * vs, *d_x = d_r + 2 * (size_t) n * vs;
    for (int j = 0; j < nrhs; ++j) {
        const double *Bc = B + (size_t) j * ldb * vs, *Xc = X + (size_t) j * ldx * vs;
        double *Rc = R + (size_t) j * ldr * vs;
        double sv = 0.0;
        if (host) {
            HIPCHK(hipMemcpy(d_b, Bc, col, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_x, Xc, col, hipMemcpyHostToDevice));
        }
        if (int rc = xr_pass<K>(H, extra, host ? d_x : Xc, host ? d_b : Bc, nullptr, host ? d_r : Rc, g, &sv)) return rc;
        if (host) HIPCHK(hipMemcpy(Rc, d_r, col, hipMemcpyDeviceToHost));
        if (berr) berr[j] = sv;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int residual_entry(sluamd_handle_t h, int trans, int extra, const void *Bv, int64_t ldb, const void *Xv, int64_t ldx, int32_t nrhs, void *Rv, int64_t ldr, double *berr,
                   bool z, bool host, const char *name)
{
    const std::string me = std::string(name) + ": ";
    if (!h || !Bv || !Xv || !Rv || nrhs < 0 || ldb < h->H.hs.n || ldx < h->H.hs.n || ldr < h->H.hs.n) { set_error(me + "bad residual arguments"); return SLUAMD_EINVAL; }
    if (trans != SLUAMD_NOTRANS && trans != SLUAMD_TRANS && trans != SLUAMD_CONJ) { set_error(me + "trans must be SLUAMD_NOTRANS, SLUAMD_TRANS or SLUAMD_CONJ"); return SLUAMD_EINVAL; }
    Handle *H = &h->H;
    if (H->z != z) {
        std::string twin(name);
        twin[7] = z ? 'd' : 'z';
        set_error(me + (z ? "double" : "complex16") + " handle: call " + twin);
        return SLUAMD_EINVAL;
    }
    if (int rc = z ? rfs_checks<Rfs<true, 0>>(H) : rfs_checks<Rfs<false, 0>>(H)) return rc;
    if (nrhs == 0) return 0;
    HIPCHK(hipSetDevice(H->device));
    if (trans != SLUAMD_NOTRANS) { if (int rc = ensure_tindex(H, name)) return rc; }
    const double *B = static_cast<const double *>(Bv), *X = static_cast<const double *>(Xv);
    double *R = static_cast<double *>(Rv);
    return rfs_dispatch(z, trans, [&](auto K) { return residual_cols<decltype(K)>(H, extra != 0, B, ldb, X, ldx, nrhs, R, ldr, berr, host); });
}

}  // namespace

extern "C" {

int sluamd_pdgsrfs3d_extra(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, double *berr, sluamd_xrefine_t *out)
{
    return xrefine_entry(h, trans, B, ldb, X, ldx, nrhs, berr, out, false, true, "sluamd_pdgsrfs3d_extra");
}

int sluamd_pdgsrfs3d_extra_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, double *berr, sluamd_xrefine_t *out)
{
    return xrefine_entry(h, trans, d_B, ldb, d_X, ldx, nrhs, berr, out, false, false, "sluamd_pdgsrfs3d_extra_dev");
}

int sluamd_pzgsrfs3d_extra(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs, double *berr,
                           sluamd_xrefine_t *out)
{
    return xrefine_entry(h, trans, B, ldb, X, ldx, nrhs, berr, out, true, true, "sluamd_pzgsrfs3d_extra");
}

int sluamd_pzgsrfs3d_extra_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X, int64_t ldx, int32_t nrhs,
                               double *berr, sluamd_xrefine_t *out)
{
    return xrefine_entry(h, trans, d_B, ldb, d_X, ldx, nrhs, berr, out, true, false, "sluamd_pzgsrfs3d_extra_dev");
}

int sluamd_dResidual(sluamd_handle_t h, int trans, int extra, const double *B, int64_t ldb, const double *X, int64_t ldx, int32_t nrhs, double *R, int64_t ldr, double *berr)
{
    return residual_entry(h, trans, extra, B, ldb, X, ldx, nrhs, R, ldr, berr, false, true, "sluamd_dResidual");
}

int sluamd_dResidual_dev(sluamd_handle_t h, int trans, int extra, const double *d_B, int64_t ldb, const double *d_X, int64_t ldx, int32_t nrhs, double *d_R, int64_t ldr,
                         double *berr)
{
    return residual_entry(h, trans, extra, d_B, ldb, d_X, ldx, nrhs, d_R, ldr, berr, false, false, "sluamd_dResidual_dev");
}

int sluamd_zResidual(sluamd_handle_t h, int trans, int extra, const sluamd_doublecomplex *B, int64_t ldb, const sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs,
                     sluamd_doublecomplex *R, int64_t ldr, double *berr)
{
    return residual_entry(h, trans, extra, B, ldb, X, ldx, nrhs, R, ldr, berr, true, true, "sluamd_zResidual");
}

int sluamd_zResidual_dev(sluamd_handle_t h, int trans, int extra, const sluamd_doublecomplex *d_B, int64_t ldb, const sluamd_doublecomplex *d_X, int64_t ldx, int32_t nrhs,
                         sluamd_doublecomplex *d_R, int64_t ldr, double *berr)
{
    return residual_entry(h, trans, extra, d_B, ldb, d_X, ldx, nrhs, d_R, ldr, berr, true, false, "sluamd_zResidual_dev");
}

}  // extern "C"
