// sluamd_zrefine.cpp -- complex16 iterative refinement: pzgsrfs3d (SRC/complex16/pzgsrfs.c:365-514) on the device, the twin of
// sluamd_pdgsrfs3d.  The frame, the loop and the policy Rfs<true, 0> are sluamd_refine.h's; this file names that one form.
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources, whose complex16 solves it cannot run.
#include "sluamd_refine.h"

using namespace sluamd;

extern "C" {

int sluamd_zAttachMatrix(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const sluamd_doublecomplex *nzval,
                         const sluamd_int_t *perm_c)
{
    return attach_rfs(h, n, rowptr, colind, nzval, perm_c, true, "sluamd_zAttachMatrix");
}

int sluamd_pzgsrfs3d_dev(sluamd_handle_t h, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X, int64_t ldx, int32_t nrhs, double *berr,
                         int32_t *steps)
{
    return rfs_plain<Rfs<true, 0>>({h, SLUAMD_NOTRANS, d_B, ldb, d_X, ldx, nrhs, berr, true, false, "sluamd_pzgsrfs3d_dev"}, steps);
}

int sluamd_pzgsrfs3d(sluamd_handle_t h, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs, double *berr,
                     int32_t *steps)
{
    return rfs_plain<Rfs<true, 0>>({h, SLUAMD_NOTRANS, B, ldb, X, ldx, nrhs, berr, true, true, "sluamd_pzgsrfs3d"}, steps);
}

}  // extern "C"
