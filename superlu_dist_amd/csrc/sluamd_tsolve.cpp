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
// Grids (tsweep_fwd_z / tsweep_bwd_z under run_grid_solve).  Block (i, j) of either factor lives on rank (i % Pr, j % Pc), so against the untransposed sweeps
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
#include "sluamd_plan.h"

using namespace sluamd;

namespace {

// one forest of a grid handle, forward / backward; x: the chunk's vector (ldx in values); the exchanges see it as doubles
int tsweep_fwd_z(Handle *H, int z, double *x, int64_t ldx, int nr, void *ctx)
{
    const bool conj = *static_cast<const bool *>(ctx);
    const DevTables &T = H->T;
    hipStream_t s = H->stream;
    LevelSched &S = H->sched[z];
    const bool xy = H->grid.Pr * H->grid.Pc > 1;
    const int64_t ldxd = ldx * (H->z ? 2 : 1);
    for (int l = 0; l < S.nlevels; ++l) {
        const int n0 = S.lvl_off[l], nn = S.lvl_off[l + 1] - n0, po = S.lvl_poff[l];
        int rc;
        if (xy && (rc = xseg_exchange(H, x, ldxd, nr, S.xt_red_send[l], 3, S.xt_red_recv[l], 2, s))) return rc;
        if (H->z) eng::zsolve_diag_t(s, true, conj, T, S.d_nodes + n0, nn, x, ldx, nr, S.max_nsupc[l]);
        else eng::solve_diag_t(s, true, T, S.d_nodes + n0, nn, x, ldx, nr, S.max_nsupc[l]);
        if (xy && (rc = xseg_exchange(H, x, ldxd, nr, S.xt_bc_send[l], 0, S.xt_bc_recv[l], 1, s))) return rc;
        if (H->z) eng::zfwd_update_t(s, conj, T, S.d_nodes + n0, S.d_bwd_prefix + po, nn, S.bwd_prefix[po + nn], x, ldx, nr, S.max_nsupc[l]);
        else eng::fwd_update_t(s, T, S.d_nodes + n0, S.d_bwd_prefix + po, nn, S.bwd_prefix[po + nn], x, ldx, nr, S.max_nsupc[l]);
        H->st.solve_launches += 2;
    }
    return 0;
}

int tsweep_bwd_z(Handle *H, int z, double *x, int64_t ldx, int nr, void *ctx)
{
    const bool conj = *static_cast<const bool *>(ctx);
    const DevTables &T = H->T;
    hipStream_t s = H->stream;
    LevelSched &S = H->sched[z];
    const bool xy = H->grid.Pr * H->grid.Pc > 1;
    const int64_t ldxd = ldx * (H->z ? 2 : 1);
    for (int l = S.nlevels - 1; l >= 0; --l) {
        const int n0 = S.lvl_off[l], nn = S.lvl_off[l + 1] - n0, po = S.lvl_poff[l];
        int rc;
        if (H->z) eng::zbwd_update_t(s, conj, T, S.d_nodes + n0, S.d_zfwd_prefix + po, nn, S.zfwd_prefix[po + nn], x, ldx, nr);
        else eng::bwd_update_t(s, T, S.d_nodes + n0, S.d_fwd_prefix + po, nn, S.fwd_prefix[po + nn], x, ldx, nr);
        if (xy && (rc = xseg_exchange(H, x, ldxd, nr, S.xt_red_send[l], 3, S.xt_red_recv[l], 2, s))) return rc;
        if (H->z) eng::zsolve_diag_t(s, false, conj, T, S.d_nodes + n0, nn, x, ldx, nr, S.max_nsupc[l]);
        else eng::solve_diag_t(s, false, T, S.d_nodes + n0, nn, x, ldx, nr, S.max_nsupc[l]);
        if (xy && (rc = xseg_exchange(H, x, ldxd, nr, S.xt_bc_send[l], 0, S.xt_bc_recv[l], 1, s))) return rc;
        H->st.solve_launches += 2;
    }
    return 0;
}

}  // namespace

// (also the correction step of the transposed refinement: sluamd_trefine.cpp)
int sluamd::run_tsolve(Handle *H, bool conj, double *d_x, int64_t ldx, int nrhs)
{
    int rc = eng::tsolve_setup();
    if (!rc && H->grid.size() > 1) {
        const GridSweepOps ops = {tsweep_fwd_z, tsweep_bwd_z, &conj, 1, 0};
        return run_grid_solve(H, d_x, ldx, nrhs, ops);
    }
    if (!rc && !H->z) rc = ensure_inv(H);
    if (rc) return rc;
    H->st.solve_launches = 0;
    const DevTables &T = H->T;
    hipStream_t s = H->stream;
    const int ch = max_rhs_chunk(H);
    const int vs = H->z ? 2 : 1;
    for (int j0 = 0; j0 < nrhs; j0 += ch) {
        const int nr = std::min(ch, nrhs - j0);
        double *x = d_x + (size_t) j0 * ldx * vs;
        for (auto &S : H->sched)
            for (int l = 0; l < S.nlevels; ++l) {
                const int n0 = S.lvl_off[l], nn = S.lvl_off[l + 1] - n0, po = S.lvl_poff[l];
                if (H->z) {
                    eng::zsolve_diag_t(s, true, conj, T, S.d_nodes + n0, nn, x, ldx, nr, S.max_nsupc[l]);
                    eng::zfwd_update_t(s, conj, T, S.d_nodes + n0, S.d_bwd_prefix + po, nn, S.bwd_prefix[po + nn], x, ldx, nr, S.max_nsupc[l]);
                } else {
                    eng::solve_diag_t(s, true, T, S.d_nodes + n0, nn, x, ldx, nr, S.max_nsupc[l]);
                    eng::fwd_update_t(s, T, S.d_nodes + n0, S.d_bwd_prefix + po, nn, S.bwd_prefix[po + nn], x, ldx, nr, S.max_nsupc[l]);
                }
                H->st.solve_launches += 2;
            }
        for (int z = (int) H->sched.size() - 1; z >= 0; --z) {
            LevelSched &S = H->sched[z];
            for (int l = S.nlevels - 1; l >= 0; --l) {
                const int n0 = S.lvl_off[l], nn = S.lvl_off[l + 1] - n0, po = S.lvl_poff[l];
                if (H->z) {
                    eng::zbwd_update_t(s, conj, T, S.d_nodes + n0, S.d_zfwd_prefix + po, nn, S.zfwd_prefix[po + nn], x, ldx, nr);
                    eng::zsolve_diag_t(s, false, conj, T, S.d_nodes + n0, nn, x, ldx, nr, S.max_nsupc[l]);
                } else {
                    eng::bwd_update_t(s, T, S.d_nodes + n0, S.d_fwd_prefix + po, nn, S.fwd_prefix[po + nn], x, ldx, nr);
                    eng::solve_diag_t(s, false, T, S.d_nodes + n0, nn, x, ldx, nr, S.max_nsupc[l]);
                }
                H->st.solve_launches += 2;
            }
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

namespace {

// the checks every entry point shares; 1: nothing to do (nrhs == 0)
int check_args(sluamd_handle_t h, int trans, const void *x, int64_t ldx, int32_t nrhs, bool z, const char *name)
{
    if (!h || !x || nrhs < 0 || ldx < h->H.hs.n) { set_error(std::string(name) + ": bad solve arguments"); return SLUAMD_EINVAL; }
    if (trans != SLUAMD_NOTRANS && trans != SLUAMD_TRANS && trans != SLUAMD_CONJ) { set_error(std::string(name) + ": trans must be SLUAMD_NOTRANS, SLUAMD_TRANS or SLUAMD_CONJ"); return SLUAMD_EINVAL; }
    if (h->H.z != z) { set_error(std::string(name) + (z ? ": double handle: call sluamd_pdgstrs3d_trans" : ": complex16 handle: call sluamd_pzgstrs3d_trans")); return SLUAMD_EINVAL; }
    if (trans != SLUAMD_NOTRANS && h->H.grid.size() > 1 && !h->H.xt_ready) { set_error(std::string(name) + ": transposed solves need a 1 x 1 x 1 handle, or a grid handle after sluamd_PlanTransposedSweeps (the transposed sweeps of a grid need exchange plans of their own)"); return SLUAMD_EINVAL; }
    return nrhs == 0 ? 1 : 0;
}

// d_x: device, n x nrhs values of the handle's precision
int tsolve_dev(sluamd_handle_t h, int trans, double *d_x, int64_t ldx, int32_t nrhs)
{
    Handle *H = &h->H;
    HIPCHK(hipSetDevice(H->device));
    HIPCHK(hipEventRecord(H->ev0, H->stream));
    int rc = trans == SLUAMD_NOTRANS ? run_solve_dev(H, d_x, ldx, nrhs) : run_tsolve(H, trans == SLUAMD_CONJ, d_x, ldx, nrhs);
    if (rc) return rc;
    HIPCHK(hipEventRecord(H->ev1, H->stream));
    HIPCHK(hipStreamSynchronize(H->stream));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, H->ev0, H->ev1));
    H->st.t_solve_ms = ms;
    return 0;
}

// x: host; staged through the handle's own device vector like sluamd_pdgstrs3d
int tsolve_host(sluamd_handle_t h, int trans, double *x, int64_t ldx, int32_t nrhs)
{
    Handle *H = &h->H;
    HIPCHK(hipSetDevice(H->device));
    const int64_t need = ldx * nrhs * (H->z ? 2 : 1);   // in doubles
    if (int rc = H->d_x.reserve(need, H->device, "the right-hand sides")) return rc;
    HIPCHK(hipMemcpy(H->d_x.p, x, sizeof(double) * need, hipMemcpyHostToDevice));
    int rc = tsolve_dev(h, trans, H->d_x.p, ldx, nrhs);
    if (rc) return rc;
    HIPCHK(hipMemcpy(x, H->d_x.p, sizeof(double) * need, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" {

int sluamd_pdgstrs3d_trans(sluamd_handle_t h, int trans, double *x, int64_t ldx, int32_t nrhs)
{
    const int c = check_args(h, trans, x, ldx, nrhs, false, "sluamd_pdgstrs3d_trans");
    if (c) return c < 0 ? c : 0;
    if (trans == SLUAMD_NOTRANS) return sluamd_pdgstrs3d(h, x, ldx, nrhs);
    return tsolve_host(h, trans, x, ldx, nrhs);
}

int sluamd_pdgstrs3d_trans_dev(sluamd_handle_t h, int trans, double *d_x, int64_t ldx, int32_t nrhs)
{
    const int c = check_args(h, trans, d_x, ldx, nrhs, false, "sluamd_pdgstrs3d_trans_dev");
    if (c) return c < 0 ? c : 0;
    if (trans == SLUAMD_NOTRANS) return sluamd_pdgstrs3d_dev(h, d_x, ldx, nrhs);
    return tsolve_dev(h, trans, d_x, ldx, nrhs);
}

int sluamd_pzgstrs3d_trans(sluamd_handle_t h, int trans, sluamd_doublecomplex *x, int64_t ldx, int32_t nrhs)
{
    const int c = check_args(h, trans, x, ldx, nrhs, true, "sluamd_pzgstrs3d_trans");
    if (c) return c < 0 ? c : 0;
    if (trans == SLUAMD_NOTRANS) return sluamd_pzgstrs3d(h, x, ldx, nrhs);
    return tsolve_host(h, trans, reinterpret_cast<double *>(x), ldx, nrhs);
}

// (SLUAMD_NOTRANS: the device-pointer form of sluamd_pzgstrs3d -- the same driver on the caller's vector, grids included)
int sluamd_pzgstrs3d_trans_dev(sluamd_handle_t h, int trans, sluamd_doublecomplex *d_x, int64_t ldx, int32_t nrhs)
{
    const int c = check_args(h, trans, d_x, ldx, nrhs, true, "sluamd_pzgstrs3d_trans_dev");
    if (c) return c < 0 ? c : 0;
    return tsolve_dev(h, trans, reinterpret_cast<double *>(d_x), ldx, nrhs);
}

}  // extern "C"
