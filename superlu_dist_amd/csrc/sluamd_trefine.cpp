// sluamd_trefine.cpp -- iterative refinement of the TRANSPOSED and CONJUGATE-TRANSPOSED systems A^T x = b / A^H x = b of the attached matrix
// (xGERFS with trans; the reference's pdgsrfs3d / pzgsrfs3d know A x = b only): sluamd_p[dz]gsrfs3d_trans[_dev].  The driver and the policies
// Rfs<Z, 1> / Rfs<true, 2> are sluamd_refine.h's:
//   residual   eng::rfs_residual over the transposed index of the attached CSR matrix (below),
//   solve      the transposed sweeps of sluamd_tsolve.cpp on r_perm: with the factors of A1 = Pc A Pc^T, A^T d = r is A1^T (Pc d) = Pc r -- the same
//              permutation on both sides, so r_perm and the update kernel are used exactly as in the untransposed loop,
//   update     eng::rfs_update, unchanged.
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources without the transposed sweeps, so no file of that list
// may instantiate a transposed policy.
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

namespace {

// One entry for the four calls below.  trans == SLUAMD_NOTRANS: the untransposed call of the precision.  Else the checks in the order of the transposed
// solves, then the index, then the shared driver.  B, X: n x nrhs values of precision z, on the host or on the device
int refine_entry(sluamd_handle_t h, int trans, const void *Bv, int64_t ldb, void *Xv, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps, bool z, bool host, const char *name)
{
    const int c = check_solve_args(h, trans, Bv, ldb, Xv, ldx, nrhs, berr, true, z, name, "refinement");
    if (c < 0) return c;
    const double *B = static_cast<const double *>(Bv);
    double *X = static_cast<double *>(Xv);
    if (trans == SLUAMD_NOTRANS) {
        auto zB = static_cast<const sluamd_doublecomplex *>(Bv); auto zX = static_cast<sluamd_doublecomplex *>(Xv);
        if (z) return host ? sluamd_pzgsrfs3d(h, zB, ldb, zX, ldx, nrhs, berr, steps) : sluamd_pzgsrfs3d_dev(h, zB, ldb, zX, ldx, nrhs, berr, steps);
        return host ? sluamd_pdgsrfs3d(h, B, ldb, X, ldx, nrhs, berr, steps) : sluamd_pdgsrfs3d_dev(h, B, ldb, X, ldx, nrhs, berr, steps);
    }
    Handle *H = &h->H;
    if (int rc = z ? rfs_checks<Rfs<true, 1>>(H) : rfs_checks<Rfs<false, 1>>(H)) return rc;
    if (nrhs == 0) { if (steps) *steps = 0; return 0; }
    if (int rc = ensure_tindex(H, name)) return rc;
    return rfs_dispatch(z, trans, [&](auto K) { return host ? rfs_host<decltype(K)>(h, B, ldb, X, ldx, nrhs, berr, steps) : rfs_dev<decltype(K)>(h, B, ldb, X, ldx, nrhs, berr, steps); });
}

}  // namespace

extern "C" {

int sluamd_pdgsrfs3d_trans(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps)
{
    return refine_entry(h, trans, B, ldb, X, ldx, nrhs, berr, steps, false, true, "sluamd_pdgsrfs3d_trans");
}

int sluamd_pdgsrfs3d_trans_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps)
{
    return refine_entry(h, trans, d_B, ldb, d_X, ldx, nrhs, berr, steps, false, false, "sluamd_pdgsrfs3d_trans_dev");
}

int sluamd_pzgsrfs3d_trans(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs, double *berr,
                           int32_t *steps)
{
    return refine_entry(h, trans, B, ldb, X, ldx, nrhs, berr, steps, true, true, "sluamd_pzgsrfs3d_trans");
}

int sluamd_pzgsrfs3d_trans_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X, int64_t ldx, int32_t nrhs,
                               double *berr, int32_t *steps)
{
    return refine_entry(h, trans, d_B, ldb, d_X, ldx, nrhs, berr, steps, true, false, "sluamd_pzgsrfs3d_trans_dev");
}

}  // extern "C"
