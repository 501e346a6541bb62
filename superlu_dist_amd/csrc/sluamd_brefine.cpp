// sluamd_brefine.cpp -- blocked iterative refinement: sluamd_p[dz]gsrfs3d_block[_dev] (contract: include/superlu_dist_amd.h; the loop, the column list and
// the storage: DESIGN.md "Blocked refinement").  rfs_dev (sluamd_refine.h) takes the right-hand sides one at a time: one residual pass, one sweep over the
// factors with nrhs = 1 and one update per column and step.  One pass of the sweeps serves 16 right-hand sides, so here a panel of RFS_PANEL = 16 columns goes
// through the loop together: per step ONE residual pass over the active columns, one K::solve with nrhs = the columns that continue, one update of exactly
// those.  Per column everything is rfs_dev's: the residual and berr (the block kernel runs the column kernel's text), the decision rfs_continue with the
// column's own lstres and count, the update; a column that has stopped is never read or written again.  Written once over the policies K of rfs_dispatch;
// the entry is rfs_frame's with this method's facts.  The panel loop (per-column lstres and count, the active list) and the host staging (16-column panels
// through a buffer of their own, hipMemcpy2D) stay here: folding either into the column forms' would take a mode flag.
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources, none of which may reference a symbol of this file.
#include <vector>
#include "sluamd_refine.h"
#include "sluamd_mkernels.inc"

using namespace sluamd;

namespace {

// r_perm of a panel and its berr words, on the first block call of a handle (DevBuf::alloc gives the pool's chunks back and tries once more)
int ensure_panel(Handle *H, int vs)
{
    const int64_t n = H->hs.n;
    if (!H->d_rfs_bwork.p) { if (int rc = H->d_rfs_bwork.alloc((int64_t) vs * n * RFS_PANEL, H->device, "the residual panel of the blocked refinement")) return rc; }
    if (!H->d_rfs_bs.p) { if (int rc = H->d_rfs_bs.alloc(RFS_PANEL, H->device, "the backward-error words of the blocked refinement")) return rc; }
    return 0;
}

// One panel: pw <= RFS_PANEL columns at d_B / d_X (device, ld in values), berr[pw], steps[pw] (may be null)
template <class K> int brfs_panel(Handle *H, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int pw, double *berr, int32_t *steps)
{
    const bool grid = H->grid.size() > 1;
    const int vs = K::z ? 2 : 1;
    const int n = (int) H->hs.n;
    const RfsGuards g = rfs_guards(n);
    const size_t col = sizeof(double) * (size_t) n * vs;
    double *r_perm = H->d_rfs_bwork.p;
    hipStream_t s = H->stream;
    double lstres[RFS_PANEL], sv[RFS_PANEL];
    int count[RFS_PANEL], go[RFS_PANEL];
    RfsCols act;
    act.count = pw;
    for (int c = 0; c < RFS_PANEL; ++c) { act.col[c] = c < pw ? c : 0; lstres[c] = 3.0; count[c] = 0; }
    const RfsMat A = rfs_mat(H, K::trans != 0);
    while (act.count > 0) {
        const int na = act.count;
        HIPCHK(hipMemsetAsync(H->d_rfs_bs.p, 0, sizeof(unsigned long long) * RFS_PANEL, s));
        meng::residual_block(s, K::z, K::trans == 2, A, d_X, ldx, d_B, ldb, r_perm, H->d_rfs_bs.p, g.safe1, g.safe2, act);
        HIPCHK(hipMemcpyAsync(sv, H->d_rfs_bs.p, sizeof(double) * (size_t) na, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int c = 0; c < na; ++c) {
            const int j = act.col[c];
            berr[j] = sv[c];
            go[c] = rfs_continue(sv[c], lstres[j], count[j]) ? 1 : 0;
        }
        // every rank computed the same sv from the same all-gathered X, but the step's solve is collective: decide every column together, so that the
        // ranks can never split into solves of different widths
        if (grid) { if (int rc = H->comm->allreduce_min(go, na, s)) return rc; }
        // the residuals of the columns that continue, made contiguous: an ordered subset, so every move goes to a lower slot and the moves, queued in
        // ascending order on one stream, never overwrite a column that is still to move
        RfsCols next;
        next.count = 0;
        for (int c = 0; c < RFS_PANEL; ++c) next.col[c] = 0;
        for (int c = 0; c < na; ++c) {
            if (!go[c]) continue;
            const int m = next.count++;
            next.col[m] = act.col[c];
            if (m != c) HIPCHK(hipMemcpyAsync(r_perm + (size_t) m * n * vs, r_perm + (size_t) c * n * vs, col, hipMemcpyDeviceToDevice, s));
        }
        if (next.count == 0) break;
        if (int rc = K::solve(H, r_perm, n, next.count)) return rc;
        meng::update_block(s, K::z, n, A.pc, r_perm, d_X, ldx, next);
        for (int c = 0, m = 0; c < na; ++c) {
            if (!go[c]) continue;
            const int j = next.col[m++];
            lstres[j] = sv[c];
            ++count[j];
        }
        act = next;
    }
    if (steps) for (int j = 0; j < pw; ++j) steps[j] = count[j];
    return 0;
}

// d_B, d_X: device-resident, original ordering, column-major (ld in values); X holds the initial solution and is refined in place.  On a grid handle
// (replicated form) every rank passes the complete B and X and the call is collective
template <class K> int brfs_dev(Handle *H, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps)
{
    const int vs = K::z ? 2 : 1;
    for (int p0 = 0; p0 < nrhs; p0 += RFS_PANEL) {
        const int pw = std::min<int>(RFS_PANEL, nrhs - p0);
        if (int rc = brfs_panel<K>(H, d_B + (size_t) p0 * ldb * vs, ldb, d_X + (size_t) p0 * ldx * vs, ldx, pw, berr + p0, steps ? steps + p0 : nullptr)) return rc;
    }
    HIPCHK(hipStreamSynchronize(H->stream));
    HIPCHK(hipGetLastError());
    return 0;
}

// B, X: host memory, column-major; a panel at a time through [B panel | X panel] on the device (ld = n)
template <class K> int brfs_host(Handle *H, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps)
{
    const int vs = K::z ? 2 : 1;
    const int64_t n = H->hs.n;
    if (!H->d_rfs_bstage.p) { if (int rc = H->d_rfs_bstage.alloc(2 * (int64_t) vs * n * RFS_PANEL, H->device, "the staged panels of the blocked refinement")) return rc; }
    const size_t col = sizeof(double) * (size_t) n * vs;
    double *d_b = H->d_rfs_bstage.p, *d_x = d_b + (size_t) vs * n * RFS_PANEL;
    for (int p0 = 0; p0 < nrhs; p0 += RFS_PANEL) {
        const int pw = std::min<int>(RFS_PANEL, nrhs - p0);
        const double *Bp = B + (size_t) p0 * ldb * vs;
        double *Xp = X + (size_t) p0 * ldx * vs;
        HIPCHK(hipMemcpy2D(d_b, col, Bp, sizeof(double) * (size_t) ldb * vs, col, (size_t) pw, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy2D(d_x, col, Xp, sizeof(double) * (size_t) ldx * vs, col, (size_t) pw, hipMemcpyHostToDevice));
        if (int rc = brfs_dev<K>(H, d_b, n, d_x, n, pw, berr + p0, steps ? steps + p0 : nullptr)) return rc;
        HIPCHK(hipMemcpy2D(Xp, sizeof(double) * (size_t) ldx * vs, d_x, col, col, (size_t) pw, hipMemcpyDeviceToHost));
    }
    return 0;
}

int brefine_entry(sluamd_handle_t h, int trans, const void *Bv, int64_t ldb, void *Xv, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps, bool z, bool host, const char *name)
{
    const RfsCall a = {h, trans, Bv, ldb, Xv, ldx, nrhs, berr, z, host, name};
    if (const int c = rfs_args(a); c < 0) return c;
    const RfsMethod m = {"blocked", true, false, false, nullptr};      // runs on grids, not on batches; nrhs == 0 writes nothing
    return rfs_frame<RfsAnyForm>(m, a,
        [&](Handle *H) {
            // (no creation call leaves such a handle: both refuse a multi-rank grid without a communicator)
            if (H->grid.size() > 1 && !H->comm) { set_error(std::string(name) + ": handle of a multi-rank grid has no communicator"); return (int) SLUAMD_EINVAL; }
            return ensure_panel(H, z ? 2 : 1);
        },
        [&](auto K, Handle *H) { return brfs_host<decltype(K)>(H, a.b(), ldb, a.x(), ldx, nrhs, berr, steps); },
        [&](auto K, Handle *H) { return brfs_dev<decltype(K)>(H, a.b(), ldb, a.x(), ldx, nrhs, berr, steps); });
}

}  // namespace

extern "C" {

int sluamd_pdgsrfs3d_block(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps)
{
    return brefine_entry(h, trans, B, ldb, X, ldx, nrhs, berr, steps, false, true, "sluamd_pdgsrfs3d_block");
}

int sluamd_pdgsrfs3d_block_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, double *berr, int32_t *steps)
{
    return brefine_entry(h, trans, d_B, ldb, d_X, ldx, nrhs, berr, steps, false, false, "sluamd_pdgsrfs3d_block_dev");
}

int sluamd_pzgsrfs3d_block(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs, double *berr,
                           int32_t *steps)
{
    return brefine_entry(h, trans, B, ldb, X, ldx, nrhs, berr, steps, true, true, "sluamd_pzgsrfs3d_block");
}

int sluamd_pzgsrfs3d_block_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X, int64_t ldx, int32_t nrhs,
                               double *berr, int32_t *steps)
{
    return brefine_entry(h, trans, d_B, ldb, d_X, ldx, nrhs, berr, steps, true, false, "sluamd_pzgsrfs3d_block_dev");
}

}  // extern "C"
