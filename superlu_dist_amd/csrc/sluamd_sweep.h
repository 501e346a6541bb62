// sluamd_sweep.h -- internal: the in-place level sweep of one forest, written once for both precisions, both transpositions, one rank and XY layers.
//   ascending  (fwd):  per level  [reduce] -> diagonal -> [broadcast] -> update
//   descending (!fwd): per level  update -> [reduce] -> diagonal -> [broadcast]
// in place in the chunk's vector x.  The exchanges in brackets run on XY layers only: the partial sums of the level's x_k are reduced to the diagonal owners
// (pack and clear / accumulate), the solved x_k are broadcast to the ranks whose updates read them (pack / overwrite).  What differs between the callers is a
// LevelKernels table: the plain sweeps of sluamd_factor.cpp (double, complex16) and the transposed ones of sluamd_tsolve.cpp (double, complex16; conj in ctx).
// The tables are thin functions over the eng:: twins and live with their callers: this header references no kernel, so the CPU test build (oracle/Makefile)
// links the files that include it whatever kernels its engine restates.  The joined, serial, grouped and fused schedules of sluamd_factor.cpp are not sweeps
// of this shape (a second vector, one launch per level) and keep their own drivers.
#pragma once
#include "sluamd_plan.h"

namespace sluamd {

// the table an update launch counts its work units in: one of LevelSched's per-level prefix tables (lvl_poff layout)
typedef PlanTable<int> LevelSched::*UnitTable;
constexpr UnitTable UNITS_FWD = &LevelSched::fwd_prefix;     // 64-row L strips
constexpr UnitTable UNITS_BWD = &LevelSched::bwd_prefix;     // 64-column U chunks
constexpr UnitTable UNITS_ZFWD = &LevelSched::zfwd_prefix;   // complex16: 256-row L strips

struct LevelKernels {
    // the two launches of a level: x = the chunk's vector, ldx in values of the handle's precision; fwd = the ascending sweep
    void (*diag)(hipStream_t s, bool fwd, const DevTables &T, const int *nodes, int nn, double *x, int64_t ldx, int nr, int max_nsupc, void *ctx);
    void (*update)(hipStream_t s, bool fwd, const DevTables &T, const int *nodes, const int *prefix, int nn, int nwork, double *x, int64_t ldx, int nr, int max_nsupc,
                   void *ctx);
    UnitTable fwd_units, bwd_units;   // the units of the ascending / descending update
    bool trans;                       // XY layers exchange along LevelSched::xt_* (transposed sweeps) instead of xs_*
};

// one level; returns the launches queued (2) or an error code (< 0)
static inline int sweep_level(Handle *H, LevelSched &S, int l, bool fwd, double *x, int64_t ldx, int nr, const LevelKernels &K, void *ctx = nullptr)
{
    hipStream_t s = H->stream;
    const bool xy = H->grid.Pr * H->grid.Pc > 1;
    const int64_t ldxd = ldx * (H->z ? 2 : 1);      // the exchanges see doubles (run lists in doubles), the kernels values
    const auto &red_send = K.trans ? S.xt_red_send : S.xs_red_send, &red_recv = K.trans ? S.xt_red_recv : S.xs_red_recv;
    const auto &bc_send = K.trans ? S.xt_bc_send : S.xs_bc_send, &bc_recv = K.trans ? S.xt_bc_recv : S.xs_bc_recv;
    const PlanTable<int> &U = S.*(fwd ? K.fwd_units : K.bwd_units);
    const int n0 = S.lvl_off[l], nn = S.lvl_off[l + 1] - n0, po = S.lvl_poff[l];
    int rc;
    if (!fwd) K.update(s, fwd, H->T, S.nodes.d + n0, U.d + po, nn, U.h[po + nn], x, ldx, nr, S.max_nsupc[l], ctx);
    if (xy && (rc = xseg_exchange(H, x, ldxd, nr, red_send[l], 3, red_recv[l], 2, s))) return rc;
    K.diag(s, fwd, H->T, S.nodes.d + n0, nn, x, ldx, nr, S.max_nsupc[l], ctx);
    if (xy && (rc = xseg_exchange(H, x, ldxd, nr, bc_send[l], 0, bc_recv[l], 1, s))) return rc;
    if (fwd) K.update(s, fwd, H->T, S.nodes.d + n0, U.d + po, nn, U.h[po + nn], x, ldx, nr, S.max_nsupc[l], ctx);
    return 2;
}

// every level of the forest, ascending (fwd) or descending; returns the launches queued or an error code (< 0).  Whether they count in stats.solve_launches
// is the caller's decision (the rule: Handle::st)
static inline int sweep_forest(Handle *H, LevelSched &S, bool fwd, double *x, int64_t ldx, int nr, const LevelKernels &K, void *ctx = nullptr)
{
    int launches = 0;
    for (int i = 0; i < S.nlevels; ++i) {
        const int n = sweep_level(H, S, fwd ? i : S.nlevels - 1 - i, fwd, x, ldx, nr, K, ctx);
        if (n < 0) return n;
        launches += n;
    }
    return launches;
}

}  // namespace sluamd
