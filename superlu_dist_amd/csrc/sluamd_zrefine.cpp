// sluamd_zrefine.cpp -- complex16 iterative refinement: pzgsrfs3d (SRC/complex16/pzgsrfs.c:365-514) on the device, the twin of
// sluamd_pdgsrfs3d.  The driver is sluamd_refine.h's, with the complex kernels eng::zrfs_residual / eng::zrfs_update.
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources against a CPU restatement of
// the double kernels only, so no file of that list may reference the complex refinement kernels.
#include "sluamd_refine.h"

using namespace sluamd;

void ZRfs::residual(hipStream_t s, const Handle *H, const double *x, const double *b, double *r_perm, double safe1, double safe2)
{
    eng::zrfs_residual(s, (int) H->hs.n, H->d_rfs_rp.p, H->d_rfs_ci.p, H->d_rfs_av.p, x, b, H->d_rfs_pc.p, r_perm, H->d_rfs_s.p, safe1, safe2);
}
void ZRfs::update(hipStream_t s, const Handle *H, const double *dx_perm, double *x) { eng::zrfs_update(s, (int) H->hs.n, H->d_rfs_pc.p, dx_perm, x); }
int ZRfs::solve(Handle *H, double *r_perm, int n) { return run_solve_dev(H, r_perm, n, 1); }

extern "C" {

int sluamd_zAttachMatrix(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const sluamd_doublecomplex *nzval,
                         const sluamd_int_t *perm_c)
{
    return attach_rfs(h, n, rowptr, colind, nzval, perm_c, true, "sluamd_zAttachMatrix");
}

int sluamd_pzgsrfs3d_dev(sluamd_handle_t h, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X, int64_t ldx, int32_t nrhs, double *berr,
                         int32_t *steps)
{
    return rfs_entry<ZRfs>(h, d_B, ldb, d_X, ldx, nrhs, berr, steps, false, "sluamd_pzgsrfs3d_dev");
}

int sluamd_pzgsrfs3d(sluamd_handle_t h, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs, double *berr,
                     int32_t *steps)
{
    return rfs_entry<ZRfs>(h, B, ldb, X, ldx, nrhs, berr, steps, true, "sluamd_pzgsrfs3d");
}

}  // extern "C"
