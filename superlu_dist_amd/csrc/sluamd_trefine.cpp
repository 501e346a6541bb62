// sluamd_trefine.cpp -- iterative refinement of the TRANSPOSED and CONJUGATE-TRANSPOSED systems A^T x = b / A^H x = b of the attached matrix
// (xGERFS with trans; the reference's pdgsrfs3d / pzgsrfs3d know A x = b only): sluamd_p[dz]gsrfs3d_trans[_dev].  The frame, the loop and the policies
// Rfs<Z, 1> / Rfs<true, 2> are sluamd_refine.h's:
//   residual   eng::rfs_residual over the transposed index of the attached CSR matrix (below),
//   solve      the transposed sweeps of sluamd_tsolve.cpp on r_perm: with the factors of A1 = Pc A Pc^T, A^T d = r is A1^T (Pc d) = Pc r -- the same
//              permutation on both sides, so r_perm and the update kernel are used exactly as in the untransposed loop,
//   update     eng::rfs_update, unchanged.
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources without the transposed sweeps, so no file of that list
// may instantiate a transposed policy -- this one instantiates them all (RfsAnyForm) and defines ensure_tindex, which only that instantiation references.
//
// The transposed index (Handle::d_rfs_tcp / d_rfs_tri / d_rfs_tpos).  Column pointers, and per entry in column order its row and its POSITION in the CSR
// value array -- no second copy of the values: sluamd_[dz]UpdateValues and sluamd_[dz]Equilibrate rewrite / scale d_rfs_av in place and nothing can go
// stale.  Built on the first transposed refinement of a handle (a handle that never asks pays nothing) and on the HOST: the pattern is copied back and
// sorted by column with one stable counting sort, O(nnz), rows ascending inside a column, so every sum has a fixed order.  A device build would need a
// stable segmented sort to save tens of milliseconds once per attached matrix.  free_rfs drops it with the pattern it indexes (re-attaching, equilibrating).
#include <vector>
#include "sluamd_refine.h"

using namespace sluamd;

int sluamd::ensure_tindex(Handle *H, const char *who)
{
    if (H->d_rfs_tcp.p) return 0;
    HIPCHK(hipSetDevice(H->device));
    H->setup.start();
    const int64_t n = H->hs.n, nnz = H->rfs_nnz;
    std::vector<int> rp((size_t) n + 1), ci((size_t) std::max<int64_t>(nnz, 1));
    HIPCHK(hipMemcpy(rp.data(), H->d_rfs_rp.p, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
    if (nnz) HIPCHK(hipMemcpy(ci.data(), H->d_rfs_ci.p, sizeof(int) * nnz, hipMemcpyDeviceToHost));
    // stable counting sort by column: the rows are visited in ascending order, so they ascend inside every column
    std::vector<int> tcp((size_t) n + 1, 0), tri((size_t) std::max<int64_t>(nnz, 1)), tpos((size_t) std::max<int64_t>(nnz, 1));
    for (int64_t e = 0; e < nnz; ++e) {
        if (ci[e] < 0 || ci[e] >= n) { set_error(std::string(who) + ": the attached matrix has a column index outside [0, n)"); return SLUAMD_EINVAL; }
        ++tcp[ci[e] + 1];
    }
    for (int64_t j = 0; j < n; ++j) tcp[j + 1] += tcp[j];
    {
        std::vector<int> next(tcp.begin(), tcp.end() - 1);
        for (int64_t i = 0; i < n; ++i) {
            if (rp[i] < 0 || rp[i + 1] < rp[i] || rp[i + 1] > nnz) { set_error(std::string(who) + ": the attached matrix has row pointers that do not ascend to nnz"); return SLUAMD_EINVAL; }
            for (int e = rp[i]; e < rp[i + 1]; ++e) { const int p = next[ci[e]]++; tri[p] = (int) i; tpos[p] = e; }
        }
    }
    DevBuf<int> d[3];           // handed to the handle once all three are up
    const std::vector<int> *src[3] = {&tcp, &tri, &tpos};
    for (int k = 0; k < 3; ++k) {
        if (int rc = d[k].alloc((int64_t) src[k]->size(), H->device, "the transposed index of the attached matrix")) return rc;
        if (hipMemcpy(d[k].p, src[k]->data(), sizeof(int) * src[k]->size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void) hipGetLastError();
            set_error(std::string(who) + ": the transposed index of the attached matrix could not be uploaded");
            return SLUAMD_EHIP;
        }
    }
    H->d_rfs_tcp = std::move(d[0]); H->d_rfs_tri = std::move(d[1]); H->d_rfs_tpos = std::move(d[2]);
    H->setup.lap("refine.transposed_index");
    return 0;
}

// The plain method of sluamd_refine.h with trans at run time (rfs_plain<RfsAnyForm>); SLUAMD_NOTRANS is the untransposed call of the precision
extern "C" {

int sluamd_pdgsrfs3d_trans(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps)
{
    return rfs_plain<RfsAnyForm>({h, trans, B, ldb, X, ldx, nrhs, berr, false, true, "sluamd_pdgsrfs3d_trans"}, steps);
}

int sluamd_pdgsrfs3d_trans_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps)
{
    return rfs_plain<RfsAnyForm>({h, trans, d_B, ldb, d_X, ldx, nrhs, berr, false, false, "sluamd_pdgsrfs3d_trans_dev"}, steps);
}

int sluamd_pzgsrfs3d_trans(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs, double *berr,
                           int32_t *steps)
{
    return rfs_plain<RfsAnyForm>({h, trans, B, ldb, X, ldx, nrhs, berr, true, true, "sluamd_pzgsrfs3d_trans"}, steps);
}

int sluamd_pzgsrfs3d_trans_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X, int64_t ldx, int32_t nrhs,
                               double *berr, int32_t *steps)
{
    return rfs_plain<RfsAnyForm>({h, trans, d_B, ldb, d_X, ldx, nrhs, berr, true, false, "sluamd_pzgsrfs3d_trans_dev"}, steps);
}

}  // extern "C"
