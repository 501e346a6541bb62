// sluamd_refine.h -- internal: the iterative refinement driver of pdgsrfs3d (SRC/double/pdgsrfs.c:345-510) and pzgsrfs3d
// (SRC/complex16/pzgsrfs.c:365-514), written once for both precisions.  The stopping rule, the per-column work through the
// resident work vectors and the collective continue / stop decision on grids live here; a precision supplies its two kernels as
// a policy K:
//   K::z                 complex16 (values, x, b, r_perm of two doubles)
//   K::attach            name for the error messages: this precision's attach call
//   K::residual(s, H, x, b, r_perm, safe1, safe2)   r_perm = Pc (b - A x), *H->d_rfs_s.p = max(*H->d_rfs_s.p, berr bits)
//   K::update(s, H, dx_perm, x)                     x += Pc^T dx_perm
//   K::solve(H, r_perm, n)                          the correction, in place in r_perm: run_solve_dev for A x = b; the transposed policies run the
//                                                   transposed sweeps (A^T d = r is A1^T (Pc d) = Pc r for the factors of A1 = Pc A Pc^T: the same
//                                                   permutation on both sides, so r_perm and K::update are used exactly alike)
// The policies are declared below and DEFINED beside their entry points: DRfs in sluamd_api.cpp (eng::rfs_*), ZRfs in sluamd_zrefine.cpp (eng::zrfs_*),
// TRfs<Z, CONJ> in sluamd_trefine.cpp for the transposed and conjugate-transposed systems of both (eng::rfs_residual_t / eng::zrfs_residual_t).  Keep the
// complex and transposed definitions out of sluamd_api.cpp: the CPU test build links the host sources without the complex and the transposed kernels.
// The GMRES refinement (sluamd_gmres.cpp) runs the same three calls of the same policies around its Krylov kernels.
#pragma once
#include "sluamd_comm.h"
#include "sluamd_plan.h"

namespace sluamd {

void free_rfs(Handle *H);   // sluamd_api.cpp
// device copy of the ORIGINAL matrix (CSR, z: doublecomplex values) + perm_c; `who` names the entry point in messages
int attach_rfs(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const void *nzval,
               const sluamd_int_t *perm_c, bool z, const char *who);
// the transposed index of the attached matrix (Handle::d_rfs_tcp / d_rfs_tri / d_rfs_tpos), built on first use: sluamd_trefine.cpp, which describes it
int ensure_tindex(Handle *H, const char *who);

struct DRfs {   // double, A x = b: sluamd_api.cpp
    static constexpr bool z = false;
    static constexpr const char *attach = "sluamd_dAttachMatrix";
    static void residual(hipStream_t s, const Handle *H, const double *x, const double *b, double *r_perm, double safe1, double safe2);
    static void update(hipStream_t s, const Handle *H, const double *dx_perm, double *x);
    static int solve(Handle *H, double *r_perm, int n);
};
struct ZRfs {   // complex16, A x = b: sluamd_zrefine.cpp
    static constexpr bool z = true;
    static constexpr const char *attach = "sluamd_zAttachMatrix";
    static void residual(hipStream_t s, const Handle *H, const double *x, const double *b, double *r_perm, double safe1, double safe2);
    static void update(hipStream_t s, const Handle *H, const double *dx_perm, double *x);
    static int solve(Handle *H, double *r_perm, int n);
};
template <bool Z, bool CONJ> struct TRfs {   // A^T x = b / A^H x = b of either precision: sluamd_trefine.cpp, which instantiates <false, false>, <true, false>, <true, true>
    static constexpr bool z = Z;
    static constexpr const char *attach = Z ? "sluamd_zAttachMatrix" : "sluamd_dAttachMatrix";
    static void residual(hipStream_t s, const Handle *H, const double *x, const double *b, double *r_perm, double safe1, double safe2);
    static void update(hipStream_t s, const Handle *H, const double *dx_perm, double *x);
    static int solve(Handle *H, double *r_perm, int n);
};
extern template struct TRfs<false, false>;
extern template struct TRfs<true, false>;
extern template struct TRfs<true, true>;

// what the driver needs beyond the arguments its entry points check (check_solve_args, sluamd_plan.h: handle, blocks, nrhs, leading dimensions, berr, trans,
// precision, planned transposed sweeps): a matrix attached to the handle -- always of the handle's precision, attach_rfs refuses any other
template <class K> int rfs_checks(const Handle *H)
{
    if (!H->d_rfs_rp.p) { set_error(std::string("no matrix attached: call ") + K::attach + " first"); return SLUAMD_EINVAL; }
    return 0;
}

// d_B, d_X: device-resident, original ordering, column-major (ld in values); X holds the initial solution and is refined in place.
// On a grid handle (replicated form, like sluamd_pdgstrs3d) every rank passes the complete B and X and the call is collective.
template <class K> int rfs_dev(sluamd_handle_t h, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps)
{
    Handle *H = &h->H;
    if (int rc = rfs_checks<K>(H)) return rc;
    const bool grid = H->grid.size() > 1;
    if (grid && !H->comm) { set_error("handle of a multi-rank grid has no communicator"); return SLUAMD_EINVAL; }
    HIPCHK(hipSetDevice(H->device));
    const int vs = K::z ? 2 : 1;
    const int n = (int) H->hs.n;
    const int ITMAX = 20;                                   // pdgsrfs.c:371
    const double eps = 0x1p-53, safmin = 2.2250738585072014e-308;
    const double safe1 = (double) (n + 1) * safmin, safe2 = safe1 / eps;
    double *r_perm = H->d_rfs_work.p;
    hipStream_t s = H->stream;
    int count = 0;
    for (int j = 0; j < nrhs; ++j) {
        const double *Bc = d_B + (size_t) j * ldb * vs;
        double *Xc = d_X + (size_t) j * ldx * vs;
        double lstres = 3.0;
        count = 0;
        for (;;) {
            HIPCHK(hipMemsetAsync(H->d_rfs_s.p, 0, sizeof(unsigned long long), s));
            K::residual(s, H, Xc, Bc, r_perm, safe1, safe2);
            double sv = 0.0;
            HIPCHK(hipMemcpyAsync(&sv, H->d_rfs_s.p, sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            berr[j] = sv;
            int go = (sv > eps && sv * 2 <= lstres && count < ITMAX) ? 1 : 0;
            // every rank computed sv from the same all-gathered x, but the step's solve is collective: decide it together, so that the
            // ranks can never split into unmatched solves
            if (grid) { if (int rc = H->comm->allreduce_min(&go, 1, s)) return rc; }
            if (!go) break;
            if (int rc = K::solve(H, r_perm, n)) return rc;
            K::update(s, H, r_perm, Xc);
            lstres = sv;
            ++count;
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (steps) *steps = count;
    return 0;
}

// B, X: host memory, column-major; one column at a time through the two resident work vectors (r_perm | b | x)
template <class K> int rfs_host(sluamd_handle_t h, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps)
{
    if (nrhs == 0) { if (steps) *steps = 0; return 0; }
    Handle *H = &h->H;
    if (int rc = rfs_checks<K>(H)) return rc;
    HIPCHK(hipSetDevice(H->device));
    const int vs = K::z ? 2 : 1;
    const int64_t n = H->hs.n;
    const size_t col = sizeof(double) * (size_t) n * vs;
    double *d_b = H->d_rfs_work.p + (size_t) n * vs, *d_x = H->d_rfs_work.p + 2 * (size_t) n * vs;
    int last = 0;
    for (int j = 0; j < nrhs; ++j) {
        HIPCHK(hipMemcpy(d_b, B + (size_t) j * ldb * vs, col, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_x, X + (size_t) j * ldx * vs, col, hipMemcpyHostToDevice));
        if (int rc = rfs_dev<K>(h, d_b, n, d_x, n, 1, berr + j, &last)) return rc;
        HIPCHK(hipMemcpy(X + (size_t) j * ldx * vs, d_x, col, hipMemcpyDeviceToHost));
    }
    if (steps) *steps = last;
    return 0;
}

// An untransposed refinement entry point of the precision of K: the shared argument checks, then the driver on host or device blocks
template <class K> int rfs_entry(sluamd_handle_t h, const void *B, int64_t ldb, void *X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps, bool host, const char *name)
{
    const int c = check_solve_args(h, SLUAMD_NOTRANS, B, ldb, X, ldx, nrhs, berr, true, K::z, name, "refinement");
    if (c < 0) return c;
    const double *b = static_cast<const double *>(B);
    double *x = static_cast<double *>(X);
    return host ? rfs_host<K>(h, b, ldb, x, ldx, nrhs, berr, steps) : rfs_dev<K>(h, b, ldb, x, ldx, nrhs, berr, steps);
}

}  // namespace sluamd
