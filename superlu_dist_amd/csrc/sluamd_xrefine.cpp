// sluamd_xrefine.cpp -- extra-precise iterative refinement, IterRefine = SLU_EXTRA: sluamd_p[dz]gsrfs3d_extra[_dev], and the residual of the attached
// matrix on its own, sluamd_[dz]Residual[_dev] (contract: include/superlu_dist_amd.h; the loop and why berr cannot stop it: DESIGN.md "Extra-precise
// refinement").  The residual of a step is accumulated in twice the working precision (sluamd_xkernels.inc, included here), the correction and the update are
// the policies' K::solve and K::update (sluamd_refine.h), and the loop watches the corrections: it ends when one is below eps relative to x, when one fails
// to halve, or after ITMAX steps.  x stays fp64.  That stop rule keeps the loop (xrfs_dev) apart from rfs_dev; the entries, the pass (rfs_berr_pass around this
// file's residual launch) and the host staging are sluamd_refine.h's.
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
    return rfs_berr_pass(H, sv, [&](hipStream_t s) { xeng::residual(s, K::z, K::trans == 2, extra, rfs_mat(H, K::trans != 0), x, b, pc, r_out, H->d_rfs_s.p, g.safe1, g.safe2); });
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

int xrefine_entry(sluamd_handle_t h, int trans, const void *Bv, int64_t ldb, void *Xv, int64_t ldx, int32_t nrhs, double *berr, sluamd_xrefine_t *out, bool z, bool host,
                  const char *name)
{
    const RfsCall a = {h, trans, Bv, ldb, Xv, ldx, nrhs, berr, z, host, name};
    if (const int c = rfs_args(a); c < 0) return c;
    const RfsMethod m = {"extra-precise", false, false, false, nullptr};   // neither on grids nor on batches; nrhs == 0 writes nothing
    return rfs_frame_by_column<RfsAnyForm>(m, a,
        [](Handle *H) { return H->d_xr_s.p ? 0 : H->d_xr_s.alloc(2, H->device, "the norm words of the extra-precise refinement"); },
        [&](auto K, Handle *H, const double *d_B, int64_t ldb_, double *d_X, int64_t ldx_, int32_t nr, int j0) {
            return xrfs_dev<decltype(K)>(H, d_B, ldb_, d_X, ldx_, nr, berr + j0, out ? out + j0 : nullptr);
        });
}

// R = B - op(A) X, column by column; host: through the resident work vectors (r | b | x), r copied back
template <class K> int residual_cols(Handle *H, bool extra, const double *B, int64_t ldb, const double *X, int64_t ldx, int32_t nrhs, double *R, int64_t ldr, double *berr,
                                     bool host)
{
    const int vs = K::z ? 2 : 1;
    const RfsGuards g = rfs_guards(H->hs.n);
    auto column = [&](int j, const double *b, const double *x, double *r) {
        double sv = 0.0;
        if (int rc = xr_pass<K>(H, extra, x, b, nullptr, r, g, &sv)) return rc;
        if (berr) berr[j] = sv;
        return 0;
    };
    if (host) {
        if (int rc = rfs_staged(H, B, ldb, X, ldx, nrhs, R, ldr, 0, [&](int j, const double *d_b, const double *d_x) { return column(j, d_b, d_x, H->d_rfs_work.p); })) return rc;
    } else {
        for (int j = 0; j < nrhs; ++j)
            if (int rc = column(j, B + (size_t) j * ldb * vs, X + (size_t) j * ldx * vs, R + (size_t) j * ldr * vs)) return rc;
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
    // its own argument checks above (a third block R, berr optional); from here the frame.  X is only read
    const RfsCall a = {h, trans, Bv, ldb, const_cast<void *>(Xv), ldx, nrhs, berr, z, host, name};
    const RfsMethod m = {nullptr, true, true, false, nullptr};
    double *R = static_cast<double *>(Rv);
    auto cols = [&](auto K, Handle *H_) { return residual_cols<decltype(K)>(H_, extra != 0, a.b(), ldb, a.x(), ldx, nrhs, R, ldr, berr, host); };
    return rfs_frame<RfsAnyForm>(m, a, [](Handle *) { return 0; }, cols, cols);
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
