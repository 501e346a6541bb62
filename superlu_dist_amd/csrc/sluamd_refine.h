// sluamd_refine.h -- internal: the iterative refinement driver of pdgsrfs3d (SRC/double/pdgsrfs.c:345-510) and pzgsrfs3d
// (SRC/complex16/pzgsrfs.c:365-514), written once for both precisions and for A x = b, A^T x = b and A^H x = b.  The stopping rule and its constants
// (rfs_guards, rfs_continue), the per-column work through the resident work vectors and the collective continue / stop decision on grids live here.
// A form is the policy K = Rfs<Z, TRANS> below:
//   K::z                 complex16 (values, x, b, r_perm of two doubles);  K::trans   0 / 1 / 2 as below
//   K::attach            name for the error messages: this precision's attach call
//   K::residual(s, H, x, b, r_perm, safe1, safe2)   r_perm = Pc (b - op(A) x), *H->d_rfs_s.p = max(*H->d_rfs_s.p, berr bits)
//   K::update(s, H, dx_perm, x)                     x += Pc^T dx_perm
//   K::solve(H, r_perm, n[, nrhs])                  the correction, in place in r_perm: run_solve_dev for A x = b, the transposed sweeps otherwise
//                                                   (A^T d = r is A1^T (Pc d) = Pc r for the factors of A1 = Pc A Pc^T: the same permutation on both
//                                                   sides, so r_perm and K::update are used exactly alike)
// A template, so a file instantiates the forms it names and no others: sluamd_api.cpp names Rfs<false, 0> only, and the CPU test build, which links the host
// sources without sluamd_tsolve.cpp, never sees run_tsolve.  That build's engine (oracle/emul/engine_cpu.cpp) restates the double A x = b kernels under their
// flat signature and nothing else, so Rfs<false, 0> calls that pair; every other form calls the general entries.  The batch loop (sluamd_batch.cpp) and the GMRES refinement (sluamd_gmres.cpp) share the
// stopping rule, and the latter runs the same three calls of the same policies around its Krylov kernels.
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

template <bool Z, int TRANS> struct Rfs {   // TRANS: 0 = A x = b, 1 = A^T x = b, 2 = A^H x = b (complex16; needs ensure_tindex first, like 1)
    static constexpr bool z = Z;
    static constexpr int trans = TRANS;
    static constexpr const char *attach = Z ? "sluamd_zAttachMatrix" : "sluamd_dAttachMatrix";
    static void residual(hipStream_t s, const Handle *H, const double *x, const double *b, double *r_perm, double safe1, double safe2)
    {
        const RfsMat A = rfs_mat(H, TRANS != 0);
        if constexpr (!Z && TRANS == 0) eng::rfs_residual(s, (int) A.n, A.ptr, A.idx, A.av, x, b, A.pc, r_perm, H->d_rfs_s.p, safe1, safe2);   // the form the CPU test build restates
        else eng::rfs_residual(s, Z, TRANS == 2, A, x, b, r_perm, H->d_rfs_s.p, safe1, safe2);
    }
    static void update(hipStream_t s, const Handle *H, const double *dx_perm, double *x)
    {
        if constexpr (!Z && TRANS == 0) eng::rfs_update(s, (int) H->hs.n, H->d_rfs_pc.p, dx_perm, x);
        else eng::rfs_update(s, Z, (int) H->hs.n, H->d_rfs_pc.p, dx_perm, x);
    }
    static int solve(Handle *H, double *r_perm, int n, int nrhs = 1)      // nrhs > 1: the block form (sluamd_brefine.cpp), columns n values apart
    {
        if constexpr (TRANS != 0) return run_tsolve(H, Z && TRANS == 2, r_perm, n, nrhs);
        else return run_solve_dev(H, r_perm, n, nrhs);
    }
};
// the policy of a (precision, trans) pair known at run time: f(Rfs<..>()) of the form that SLUAMD_NOTRANS / SLUAMD_TRANS / SLUAMD_CONJ names (the conjugate
// of a real matrix is itself)
template <class F> auto rfs_dispatch(bool z, int trans, F f)
{
    if (trans == SLUAMD_NOTRANS) return z ? f(Rfs<true, 0>()) : f(Rfs<false, 0>());
    return !z ? f(Rfs<false, 1>()) : trans == SLUAMD_CONJ ? f(Rfs<true, 2>()) : f(Rfs<true, 1>());
}

// The stopping rule (pdgsrfs.c:371, :463-469, :477): the guards of a matrix of order n, and whether a step follows a backward error sv
constexpr double RFS_EPS = 0x1p-53, RFS_SAFMIN = 2.2250738585072014e-308;      // dmach_dist("Epsilon"), ("Safe minimum")
struct RfsGuards { double eps, safe1, safe2; };
inline RfsGuards rfs_guards(int64_t n)
{
    const double safe1 = (double) (n + 1) * RFS_SAFMIN;
    return {RFS_EPS, safe1, safe1 / RFS_EPS};
}
inline bool rfs_continue(double sv, double lstres, int count)
{
    constexpr int ITMAX = 20;                                   // pdgsrfs.c:371
    return sv > RFS_EPS && sv * 2 <= lstres && count < ITMAX;
}

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
    const RfsGuards g = rfs_guards(n);
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
            K::residual(s, H, Xc, Bc, r_perm, g.safe1, g.safe2);
            double sv = 0.0;
            HIPCHK(hipMemcpyAsync(&sv, H->d_rfs_s.p, sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            berr[j] = sv;
            int go = rfs_continue(sv, lstres, count) ? 1 : 0;
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
