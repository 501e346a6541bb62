// sluamd_equil.cpp -- Equil = YES for handles created from the symbolic structure: pdgsequ + pdlaqgs on the device (SRC/double/pdgsequ.c:126-215,
// SRC/double/pdlaqgs.c:89-146; complex16: pzgsequ.c / pzlaqgs.c) and the solve phase of the expert driver in the caller's ordering and scaling
// (pdgssvx3d.c:1450-1465 B scaled before the solve, :1806-1821 X after it).  Contract: include/superlu_dist_amd.h.
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources against a CPU restatement of the older kernels only, so
// no file of that list may reference the equilibration kernels (eng::eq_*).
//
// The device computes what is large (maxima per row and column, scaling, column sums, gather into the store order); the decisions of pdgsequ / pdlaqgs
// are a handful of scalar comparisons on the host between the launches.  The solve wraps the existing drivers: sluamd_p[dz]gstrs3d_trans_dev between two
// fused permute-and-scale launches, sluamd_p[dz]gsrfs3d_dev for the refinement (three more passes over the block there, see solve_dev) -- the multi-right-hand-side block forms, the grids' replicated form and
// their error codes come with them.
// RowPerm = LargeDiag_MC64 meets the handle here: sluamd_[dz]EquilibrateWith is the same equilibration with R and C given (those of sluamd_[dz]LargeDiag),
// sluamd_SetRowPerm makes the solve take B and X in the ordering of A for a handle created from Pr A (the matching itself: sluamd_rowperm.cpp).
#include <cstring>
#include "sluamd_refine.h"

using namespace sluamd;

namespace {

typedef unsigned long long u64;
double as_double(u64 b) { double d; memcpy(&d, &b, sizeof d); return d; }

// with: sluamd_[dz]EquilibrateWith -- R = r_in and C = c_in (host, either may be null) are inputs, equed follows from which of them is given
int equilibrate(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const void *nzval, const sluamd_int_t *perm_c,
                sluamd_equil_t *out, bool z, const char *who, bool with = false, const double *r_in = nullptr, const double *c_in = nullptr)
{
    const std::string me = std::string(who) + ": ";
    if (!h || !rowptr || !colind || !nzval || !perm_c || !out) { set_error(me + "null argument"); return SLUAMD_EINVAL; }
    Handle *H = &h->H;
    if (H->z != z) { set_error(me + (z ? "double handle: call sluamd_dEquilibrate" : "complex16 handle: call sluamd_zEquilibrate")); return SLUAMD_EINVAL; }
    if (!H->d_aent.p || H->a_csr_nnz < 0) { set_error(me + "the handle was not created from the symbolic structure (sluamd_[dz]CreateLUHandleFromSymb[Grid]): the caller of a view-created handle scales its own values"); return SLUAMD_EINVAL; }
    if (n != H->hs.n || rowptr[n] != H->a_csr_nnz) { set_error(me + "n or the number of entries differs from the matrix the handle was created from"); return SLUAMD_EINVAL; }
    if (H->eq_done) { set_error(me + "the handle has been equilibrated already"); return SLUAMD_EINVAL; }
    const double smlnum = 0x1p-1022, bignum = 1.0 / smlnum;          // dmach_dist("S")
    double cnd[2] = {1.0, 1.0};                                      // rowcnd, colcnd of given scalings: smallest over largest, as pdgsequ.c:169, :213
    if (with) {
        const double *vec[2] = {r_in, c_in};
        for (int k = 0; k < 2; ++k) {
            if (!vec[k] || n == 0) continue;
            double lo = HUGE_VAL, hi = 0.0;
            for (sluamd_int_t i = 0; i < n; ++i) {
                const double t = vec[k][i];
                if (!(t > 0.0) || !(t < HUGE_VAL)) { set_error(me + (k ? "c" : "r") + " holds a value that is not positive and finite"); return SLUAMD_EINVAL; }
                lo = std::min(lo, t); hi = std::max(hi, t);
            }
            cnd[k] = std::max(lo, smlnum) / std::min(hi, bignum);
        }
    }
    if (int rc = attach_rfs(h, n, rowptr, colind, nzval, perm_c, z, who)) return rc;
    *out = sluamd_equil_t{SLUAMD_EQUED_N, 0, 0.0, 0.0, 0.0, 0.0};
    if (n == 0) { out->rowcnd = out->colcnd = 1.0; H->eq_done = true; return 0; }      // pdgsequ.c:114-119
    // eq_done is set on success only: a failed call leaves the handle open for another one, which attaches the caller's (unscaled) values afresh
    hipStream_t s = H->stream;
    const int64_t nnz = H->rfs_nnz;
    DevBuf<u64> red_buf;
    if (int rc = H->d_eq_r.alloc(n, H->device, "the row scalings R")) return rc;
    if (int rc = H->d_eq_c.alloc(n, H->device, "the column scalings C")) return rc;
    if (int rc = red_buf.alloc(3, H->device, "the reduction words of the equilibration")) return rc;
    u64 *const d_red = red_buf.p;
    // the three global values of one reduction launch: {min, max, first index of an exact zero}
    u64 red[3];
    auto reset = [&]() { const u64 init[3] = {~0ull, 0ull, ~0ull}; return hipMemcpyAsync(d_red, init, sizeof init, hipMemcpyHostToDevice, s) == hipSuccess ? hipStreamSynchronize(s) : hipErrorUnknown; };
    auto fetch = [&]() { return hipMemcpyAsync(red, d_red, sizeof red, hipMemcpyDeviceToHost, s) == hipSuccess ? hipStreamSynchronize(s) : hipErrorUnknown; };
    int mode = 0;                                                   // bit 0: rows, bit 1: columns
    if (with) {   // amax of the unscaled matrix (the row maxima land in the work vector the column sums zero-fill below); R and C as given
        HIPCHK(reset());
        eng::eq_rowmax(s, z, n, nnz, H->d_rfs_rp.p, H->d_rfs_av.p, H->d_rfs_work.p, d_red);
        HIPCHK(fetch());
        out->amax = as_double(red[1]);
        out->rowcnd = cnd[0]; out->colcnd = cnd[1];
        if (r_in) HIPCHK(hipMemcpyAsync(H->d_eq_r.p, r_in, sizeof(double) * n, hipMemcpyHostToDevice, s));
        if (c_in) HIPCHK(hipMemcpyAsync(H->d_eq_c.p, c_in, sizeof(double) * n, hipMemcpyHostToDevice, s));
        mode = (r_in ? 1 : 0) | (c_in ? 2 : 0);
    } else do {
        HIPCHK(reset());
        eng::eq_rowmax(s, z, n, nnz, H->d_rfs_rp.p, H->d_rfs_av.p, H->d_eq_r.p, d_red);
        HIPCHK(fetch());
        double rcmin = std::min(bignum, as_double(red[0])), rcmax = as_double(red[1]);
        out->amax = rcmax;
        if (rcmin == 0.0) { out->info = (int32_t) red[2] + 1; break; }                     // pdgsequ.c:158-164
        eng::eq_invert(s, n, H->d_eq_r.p, smlnum, bignum);
        out->rowcnd = std::max(rcmin, smlnum) / std::min(rcmax, bignum);
        HIPCHK(hipMemsetAsync(H->d_eq_c.p, 0, sizeof(double) * n, s));
        eng::eq_colmax(s, z, n, nnz, H->d_rfs_rp.p, H->d_rfs_ci.p, H->d_rfs_av.p, H->d_eq_r.p, H->d_eq_c.p);
        HIPCHK(reset());
        eng::eq_reduce(s, n, H->d_eq_c.p, d_red);
        HIPCHK(fetch());
        rcmin = std::min(bignum, as_double(red[0])); rcmax = as_double(red[1]);
        if (rcmin == 0.0) { out->info = n + (int32_t) red[2] + 1; break; }                 // pdgsequ.c:202-208
        eng::eq_invert(s, n, H->d_eq_c.p, smlnum, bignum);
        out->colcnd = std::max(rcmin, smlnum) / std::min(rcmax, bignum);
        // pdlaqgs.c:107-146
        const double THRESH = 0.1, small = smlnum / 0x1p-52, large = 1.0 / small;          // dmach("Safe minimum") / dmach("Precision")
        if (out->rowcnd >= THRESH && out->amax >= small && out->amax <= large) mode = out->colcnd >= THRESH ? 0 : 2;
        else mode = out->colcnd >= THRESH ? 1 : 3;
    } while (0);
    // scaling in place + the 1-norm of what is left (mode 0: the norm alone); the column sums go through the refinement's work vector
    double *colsum = H->d_rfs_work.p;
    HIPCHK(hipMemsetAsync(colsum, 0, sizeof(double) * n, s));
    eng::eq_scale_norm(s, z, n, nnz, H->d_rfs_rp.p, H->d_rfs_ci.p, H->d_rfs_av.p, H->d_eq_r.p, H->d_eq_c.p, mode, colsum);
    HIPCHK(reset());
    eng::eq_reduce(s, n, colsum, d_red);
    HIPCHK(fetch());
    out->anorm = as_double(red[1]);
    out->equed = mode == 0 ? SLUAMD_EQUED_N : mode == 1 ? SLUAMD_EQUED_R : mode == 2 ? SLUAMD_EQUED_C : SLUAMD_EQUED_B;
    if (mode) {   // the store takes the scaled values (equed == N: it holds them already)
        eng::eq_gather(s, z, H->a_nnz, H->d_aent.p, H->d_rfs_av.p, H->d_aval.p);
        if (int rc = sluamd_dResetValues(h)) return rc;
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    H->eq_row = (mode & 1) != 0; H->eq_col = (mode & 2) != 0;
    H->eq_done = true;
    return 0;
}

// the shared checks of the solves (check_solve_args), then what this call adds; 1: nothing to do (nrhs == 0)
int check_solve(sluamd_handle_t h, int trans, const void *B, int64_t ldb, const void *X, int64_t ldx, int32_t nrhs, int refine, const double *berr,
                int32_t *steps, bool z, const char *name)
{
    const int c = check_solve_args(h, trans, B, ldb, X, ldx, nrhs, berr, refine != 0, z, name);
    if (c < 0) return c;
    const std::string me = std::string(name) + ": ";
    if (!h->H.d_rfs_pc.p) { set_error(me + "no matrix attached (perm_c): call sluamd_[dz]Equilibrate or sluamd_[dz]AttachMatrix first"); return SLUAMD_EINVAL; }
    if (refine && trans != SLUAMD_NOTRANS) { set_error(me + "refine with a transposed system is not part of this call: solve with refine = 0, then refine the attached (scaled) system with sluamd_p[dz]gsrfs3d_trans"); return SLUAMD_EINVAL; }
    if (steps) *steps = 0;
    return c;
}

// d_B, d_X: device, original ordering and scaling; xp: n x nrhs values of work space (ld n)
int solve_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, int refine, double *berr, int32_t *steps,
              double *xp)
{
    Handle *H = &h->H;
    HIPCHK(hipSetDevice(H->device));
    const bool z = H->z;
    const int n = (int) H->hs.n;
    hipStream_t s = H->stream;
    const double *R = H->eq_row ? H->d_eq_r.p : nullptr, *Cs = H->eq_col ? H->d_eq_c.p : nullptr;
    const double *s_in = trans == SLUAMD_NOTRANS ? R : Cs, *s_out = trans == SLUAMD_NOTRANS ? Cs : R;      // pdgssvx3d.c:1450-1465, :1806-1821
    // sluamd_SetRowPerm: the handle holds Pr A, B and X are in A's ordering.  Row i of A is row perm_r[i] of the attached system, so whatever is indexed by
    // the ROWS -- B and R of op = N, X and R of op = T / C -- goes through perm_r; the column side is untouched
    const int *p_in = H->d_rfs_pc.p, *p_out = H->d_rfs_pc.p, *p_rows = nullptr;
    if (H->d_rp_pr.p) {
        p_rows = H->d_rp_pr.p;
        if (trans == SLUAMD_NOTRANS) { p_in = H->d_rp_pcpr.p; if (R) s_in = H->d_rp_rs.p; }
        else { p_out = H->d_rp_pcpr.p; if (R) s_out = H->d_rp_rs.p; }
    }
    eng::eq_permscale(s, z, false, n, nrhs, p_in, s_in, d_B, ldb, xp, n);
    HIPCHK(hipGetLastError());
    int rc = z ? sluamd_pzgstrs3d_trans_dev(h, trans, reinterpret_cast<sluamd_doublecomplex *>(xp), n, nrhs) : sluamd_pdgstrs3d_trans_dev(h, trans, xp, n, nrhs);
    if (rc) return rc;
    if (!refine) {
        eng::eq_permscale(s, z, true, n, nrhs, p_out, s_out, xp, n, d_X, ldx);
    } else {   // the scaled system is refined, then X = s_out o X' (pdgssvx3d.c:1700-1821); op = N here (check_solve), so p_out is perm_c
        eng::eq_permscale(s, z, true, n, nrhs, p_out, nullptr, xp, n, d_X, ldx);
        eng::eq_permscale(s, z, false, n, nrhs, p_rows, s_in, d_B, ldb, xp, n);      // B' in the attached system's row order
        HIPCHK(hipGetLastError());
        rc = z ? sluamd_pzgsrfs3d_dev(h, reinterpret_cast<const sluamd_doublecomplex *>(xp), n, reinterpret_cast<sluamd_doublecomplex *>(d_X), ldx, nrhs, berr, steps)
               : sluamd_pdgsrfs3d_dev(h, xp, n, d_X, ldx, nrhs, berr, steps);
        if (rc) return rc;
        if (s_out) eng::eq_permscale(s, z, true, n, nrhs, nullptr, s_out, d_X, ldx, d_X, ldx);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int solve_entry(sluamd_handle_t h, int trans, const void *B, int64_t ldb, void *X, int64_t ldx, int32_t nrhs, int refine, double *berr, int32_t *steps, bool z,
                bool host, const char *name)
{
    const int c = check_solve(h, trans, B, ldb, X, ldx, nrhs, refine, berr, steps, z, name);
    if (c) return c < 0 ? c : 0;
    Handle *H = &h->H;
    HIPCHK(hipSetDevice(H->device));
    const int vs = z ? 2 : 1;
    const int64_t n = H->hs.n, blk = n * nrhs * vs;              // doubles of one n x nrhs block
    if (int rc = H->d_eq_work.reserve(host ? 3 * blk : blk, H->device, "the work block of the expert solve")) return rc;
    if (!host) return solve_dev(h, trans, (const double *) B, ldb, (double *) X, ldx, nrhs, refine, berr, steps, H->d_eq_work.p);
    double *d_b = H->d_eq_work.p + blk, *d_x = H->d_eq_work.p + 2 * blk;
    const size_t row = sizeof(double) * (size_t) n * vs;
    HIPCHK(hipMemcpy2D(d_b, row, B, sizeof(double) * (size_t) ldb * vs, row, (size_t) nrhs, hipMemcpyHostToDevice));
    if (int rc = solve_dev(h, trans, d_b, n, d_x, n, nrhs, refine, berr, steps, H->d_eq_work.p)) return rc;
    HIPCHK(hipMemcpy2D(X, sizeof(double) * (size_t) ldx * vs, d_x, row, row, (size_t) nrhs, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" {

int sluamd_dEquilibrate(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const double *nzval,
                        const sluamd_int_t *perm_c, sluamd_equil_t *out)
{
    return equilibrate(h, n, rowptr, colind, nzval, perm_c, out, false, "sluamd_dEquilibrate");
}

int sluamd_zEquilibrate(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const sluamd_doublecomplex *nzval,
                        const sluamd_int_t *perm_c, sluamd_equil_t *out)
{
    return equilibrate(h, n, rowptr, colind, nzval, perm_c, out, true, "sluamd_zEquilibrate");
}

int sluamd_dEquilibrateWith(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const double *nzval,
                            const sluamd_int_t *perm_c, const double *r, const double *c, sluamd_equil_t *out)
{
    return equilibrate(h, n, rowptr, colind, nzval, perm_c, out, false, "sluamd_dEquilibrateWith", true, r, c);
}

int sluamd_zEquilibrateWith(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const sluamd_doublecomplex *nzval,
                            const sluamd_int_t *perm_c, const double *r, const double *c, sluamd_equil_t *out)
{
    return equilibrate(h, n, rowptr, colind, nzval, perm_c, out, true, "sluamd_zEquilibrateWith", true, r, c);
}

int sluamd_SetRowPerm(sluamd_handle_t h, const sluamd_int_t *perm_r)
{
    const std::string me = "sluamd_SetRowPerm: ";
    if (!h || !perm_r) { set_error(me + "null argument"); return SLUAMD_EINVAL; }
    Handle *H = &h->H;
    if (!H->d_rfs_pc.p) { set_error(me + "no matrix attached (perm_c): call sluamd_[dz]EquilibrateWith, sluamd_[dz]Equilibrate or sluamd_[dz]AttachMatrix first"); return SLUAMD_EINVAL; }
    if (H->factored) { set_error(me + "the handle holds factors: set the row permutation before the factorisation"); return SLUAMD_EINVAL; }
    const int64_t n = H->hs.n;
    std::vector<uint8_t> seen((size_t) n, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t j = perm_r[i];
        if (j < 0 || j >= n || seen[j]) { set_error(me + "perm_r is not a permutation of 0 .. n-1"); return SLUAMD_EINVAL; }
        seen[j] = 1;
    }
    HIPCHK(hipSetDevice(H->device));
    auto drop = [&]() { H->d_rp_pr.reset(); H->d_rp_pcpr.reset(); H->d_rp_rs.reset(); };
    drop();
    if (n == 0) return 0;
    int rc;
    if ((rc = H->d_rp_pr.alloc(n, H->device, "the row permutation perm_r")) || (rc = H->d_rp_pcpr.alloc(n, H->device, "the composed permutation perm_c o perm_r")) ||
        (H->eq_row && (rc = H->d_rp_rs.alloc(n, H->device, "the permuted row scalings")))) { drop(); return rc; }
    hipError_t e = hipMemcpyAsync(H->d_rp_pr.p, perm_r, sizeof(int) * (size_t) n, hipMemcpyHostToDevice, H->stream);
    if (e == hipSuccess) {
        eng::rp_compose(H->stream, (int) n, H->d_rp_pr.p, H->d_rfs_pc.p, H->eq_row ? H->d_eq_r.p : nullptr, H->d_rp_pcpr.p, H->d_rp_rs.p);
        e = hipStreamSynchronize(H->stream);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { drop(); set_error(me + hipGetErrorString(e)); return SLUAMD_EHIP; }
    return 0;
}

int sluamd_GetScalings(sluamd_handle_t h, double *r, double *c)
{
    if (!h) { set_error("sluamd_GetScalings: null handle"); return SLUAMD_EINVAL; }
    Handle *H = &h->H;
    HIPCHK(hipSetDevice(H->device));
    const size_t n = (size_t) H->hs.n;
    if (r) { if (H->eq_row) HIPCHK(hipMemcpy(r, H->d_eq_r.p, sizeof(double) * n, hipMemcpyDeviceToHost)); else std::fill(r, r + n, 1.0); }
    if (c) { if (H->eq_col) HIPCHK(hipMemcpy(c, H->d_eq_c.p, sizeof(double) * n, hipMemcpyDeviceToHost)); else std::fill(c, c + n, 1.0); }
    return 0;
}

int sluamd_pdgssvx3d_solve(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, int refine, double *berr,
                           int32_t *steps)
{
    return solve_entry(h, trans, B, ldb, X, ldx, nrhs, refine, berr, steps, false, true, "sluamd_pdgssvx3d_solve");
}

int sluamd_pdgssvx3d_solve_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, int refine, double *berr,
                               int32_t *steps)
{
    return solve_entry(h, trans, d_B, ldb, d_X, ldx, nrhs, refine, berr, steps, false, false, "sluamd_pdgssvx3d_solve_dev");
}

int sluamd_pzgssvx3d_solve(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs,
                           int refine, double *berr, int32_t *steps)
{
    return solve_entry(h, trans, B, ldb, X, ldx, nrhs, refine, berr, steps, true, true, "sluamd_pzgssvx3d_solve");
}

int sluamd_pzgssvx3d_solve_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X, int64_t ldx,
                               int32_t nrhs, int refine, double *berr, int32_t *steps)
{
    return solve_entry(h, trans, d_B, ldb, d_X, ldx, nrhs, refine, berr, steps, true, false, "sluamd_pzgssvx3d_solve_dev");
}

}  // extern "C"
