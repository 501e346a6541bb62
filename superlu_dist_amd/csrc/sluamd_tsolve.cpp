// sluamd_tsolve.cpp -- transposed and conjugate-transposed solves with the resident factors: (L U)^T y = b / (L U)^H y = b, on one rank and on process grids
// (replicated form, collective, like sluamd_pdgstrs3d; sluamd_p[dz]gstrs3d_dist -- B distributed by rows -- stays untransposed).
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources against a CPU restatement of the untransposed
// kernels only, so no file of that list may reference the transposed sweeps (eng::*_t).
//
// Schedule.  The DAG levels of a handle are longest paths over the L AND the U blocks of every supernode, so every target of supernode k in either
// triangle lies in a later level; the same LevelSched therefore orders the transposed dependencies (U^T forward: block row k updates the columns of
// U(k, :); L^T backward: supernode k reads the rows of L(:, k)), also for unsymmetric patterns.  Per chunk of max_rhs_chunk right-hand sides, in place in x:
//   forward  (levels ascending):   y_k = Uinv_k^T x_k (complex16: substitution on U_kk^T / its conjugate), then x[gc] -= U_k[:, c]^T y_k per non-empty column
//   backward (levels descending):  x_k -= L_k[below, c]^T x[lrow], then x_k = Linv_k^T x_k (complex16: unit substitution on L_kk^T)
// = one diagonal and one update launch per level and sweep: stats.solve_launches = 4 x levels per chunk.  The joined, fused and grouped schedules of the
// untransposed sweeps are not used (handles created under those switches keep the plain per-level prefix tables this path reads).
//
// Grids (tsweep under run_grid_solve; the level loop itself: sweep_forest, sluamd_sweep.h).  Block (i, j) of either factor lives on rank (i % Pr, j % Pc), so against the untransposed sweeps
// of sluamd_factor.cpp the two directions of a layer swap; the same kernels and prefix tables run (they count locally stored chunks / strips only):
//   forward:  U(k, :) lives on process row k % Pr -> y_k is BROADCAST ALONG THAT ROW; its chunks subtract into x_j on the ranks of process column j % Pc, whose
//             partial sums are REDUCED ALONG THAT COLUMN to j's diagonal owner in front of j's level
//   backward: the strips of L(:, k) on process column k % Pc read the solved x_i of process row i % Pr (broadcast along the row at i's level) and their partial
//             sums are reduced along the column to the owner, which then applies Linv_k^T
// = per level [reduce xt_red] -> diagonal -> [broadcast xt_bc] -> update ascending, update -> [reduce] -> diagonal -> [broadcast] descending (LevelSched::xt_*).
// Non-owners use their rows of x as zero accumulators, exactly as in the untransposed sweeps: the reduce packs and clears, the broadcast overwrites.  A rank
// (r, c) accumulates into row block j only when j % Pc == c and receives broadcast copies only when j % Pr == r -- both only at j's owner -- so an accumulator
// is never a broadcast copy; the accumulators of the backward sweep are the ones the forward reduce cleared (or rows of forests this layer never sweeps).
// Along Z the partial sums of the ancestors (rows of my process COLUMN, forest_runs role 1) go to the partner layer after a forest's forward sweep and the
// solved ancestors (rows of my process ROW, role 0) come down before its backward sweep: the roles of run_solve_dev exchanged.
// A handle of more than one rank takes these solves once sluamd_PlanTransposedSweeps has planned the xt_* lists (every rank calls it; until then the handle
// refuses them as it always did).  Every rank takes the same decisions before the first exchange: the argument checks see state that is the same on all
// ranks (precision, trans, planned, factored, communicator).
// stats.solve_launches: the sweep launches this rank queued (two per level and sweep of the forests it sweeps, per chunk).
#include <algorithm>
#include "sluamd_sweep.h"

using namespace sluamd;

namespace {

// the level kernels of the transposed sweeps (sluamd_sweep.h); ctx: conj
void d_level_diag(hipStream_t s, bool fwd, const DevTables &T, const int *nodes, int nn, double *x, int64_t ldx, int nr, int mx, void *) { eng::solve_diag_t(s, fwd, T, nodes, nn, x, ldx, nr, mx); }
void d_level_update(hipStream_t s, bool fwd, const DevTables &T, const int *nodes, const int *prefix, int nn, int nwork, double *x, int64_t ldx, int nr, int mx, void *)
{
    if (fwd) eng::fwd_update_t(s, T, nodes, prefix, nn, nwork, x, ldx, nr, mx);
    else eng::bwd_update_t(s, T, nodes, prefix, nn, nwork, x, ldx, nr);
}
void z_level_diag(hipStream_t s, bool fwd, const DevTables &T, const int *nodes, int nn, double *x, int64_t ldx, int nr, int mx, void *ctx) { eng::zsolve_diag_t(s, fwd, *static_cast<const bool *>(ctx), T, nodes, nn, x, ldx, nr, mx); }
void z_level_update(hipStream_t s, bool fwd, const DevTables &T, const int *nodes, const int *prefix, int nn, int nwork, double *x, int64_t ldx, int nr, int mx, void *ctx)
{
    const bool conj = *static_cast<const bool *>(ctx);
    if (fwd) eng::zfwd_update_t(s, conj, T, nodes, prefix, nn, nwork, x, ldx, nr, mx);
    else eng::zbwd_update_t(s, conj, T, nodes, prefix, nn, nwork, x, ldx, nr);
}
// U^T forward: the chunks of bwd_prefix; L^T backward: the strips of fwd_prefix / zfwd_prefix
const LevelKernels trans_d = {d_level_diag, d_level_update, UNITS_BWD, UNITS_FWD, true}, trans_z = {z_level_diag, z_level_update, UNITS_BWD, UNITS_ZFWD, true};

// one forest, forward / backward; x: the chunk's vector (ldx in values)
int tsweep(Handle *H, int z, bool fwd, double *x, int64_t ldx, int nr, void *ctx)
{
    const int n = sweep_forest(H, H->sched[z], fwd, x, ldx, nr, H->z ? trans_z : trans_d, ctx);
    if (n < 0) return n;
    H->st.solve_launches += n;
    return 0;
}

}  // namespace

// (also the correction step of the transposed refinement: sluamd_trefine.cpp)
int sluamd::run_tsolve(Handle *H, bool conj, double *d_x, int64_t ldx, int nrhs)
{
    int rc = eng::tsolve_setup();
    if (!rc && H->grid.size() > 1) {
        const GridSweepOps ops = {tsweep, &conj, 1, 0};
        return run_grid_solve(H, d_x, ldx, nrhs, ops);
    }
    if (!rc && !H->z) rc = ensure_inv(H);
    if (rc) return rc;
    H->st.solve_launches = 0;
    const int ch = max_rhs_chunk(H);
    const int vs = H->z ? 2 : 1;
    const int nz = (int) H->sched.size();
    for (int j0 = 0; j0 < nrhs; j0 += ch) {
        const int nr = std::min(ch, nrhs - j0);
        double *x = d_x + (size_t) j0 * ldx * vs;
        for (int z = 0; z < nz; ++z) if ((rc = tsweep(H, z, true, x, ldx, nr, &conj))) return rc;
        for (int z = nz - 1; z >= 0; --z) if ((rc = tsweep(H, z, false, x, ldx, nr, &conj))) return rc;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

namespace {

// x: n x nrhs values of precision z, on the host (staged through the handle's own device vector) or on the device.  SLUAMD_NOTRANS runs the driver of the
// untransposed entry points (sluamd_api.cpp) in the same frame
int solve_entry(sluamd_handle_t h, int trans, void *x, int64_t ldx, int32_t nrhs, bool z, bool host, const char *name)
{
    const int c = check_solve_args(h, trans, x, ldx, x, ldx, nrhs, nullptr, false, z, name);
    if (c) return c < 0 ? c : 0;
    Handle *H = &h->H;
    return framed_solve(H, static_cast<double *>(x), ldx, nrhs, host, [&](double *d_x) {
        return trans == SLUAMD_NOTRANS ? run_solve_dev(H, d_x, ldx, nrhs) : run_tsolve(H, trans == SLUAMD_CONJ, d_x, ldx, nrhs);
    });
}

}  // namespace

extern "C" {

int sluamd_pdgstrs3d_trans(sluamd_handle_t h, int trans, double *x, int64_t ldx, int32_t nrhs) { return solve_entry(h, trans, x, ldx, nrhs, false, true, "sluamd_pdgstrs3d_trans"); }

int sluamd_pdgstrs3d_trans_dev(sluamd_handle_t h, int trans, double *d_x, int64_t ldx, int32_t nrhs) { return solve_entry(h, trans, d_x, ldx, nrhs, false, false, "sluamd_pdgstrs3d_trans_dev"); }

int sluamd_pzgstrs3d_trans(sluamd_handle_t h, int trans, sluamd_doublecomplex *x, int64_t ldx, int32_t nrhs) { return solve_entry(h, trans, x, ldx, nrhs, true, true, "sluamd_pzgstrs3d_trans"); }

// (SLUAMD_NOTRANS: the device-pointer form of sluamd_pzgstrs3d -- the same driver on the caller's vector, grids included)
int sluamd_pzgstrs3d_trans_dev(sluamd_handle_t h, int trans, sluamd_doublecomplex *d_x, int64_t ldx, int32_t nrhs) { return solve_entry(h, trans, d_x, ldx, nrhs, true, false, "sluamd_pzgstrs3d_trans_dev"); }

}  // extern "C"
