// sluamd_refine.h -- internal: the iterative refinement driver of pdgsrfs3d (SRC/double/pdgsrfs.c:345-510) and pzgsrfs3d
// (SRC/complex16/pzgsrfs.c:365-514), written once for both precisions and for A x = b, A^T x = b and A^H x = b.  Here live
//   the policies       K = Rfs<Z, TRANS> and rfs_dispatch, below;
//   the stopping rule  and its constants (rfs_guards, rfs_continue), shared with the batch loop (sluamd_batch.cpp) and the blocked form (sluamd_brefine.cpp);
//   the pass           rfs_pass: clear the berr word, residual, copy the word back, synchronise;
//   the outer loop     rfs_dev: columns and steps, the collective continue / stop decision on grids, the step a callable -- rfs_plain_step (K::solve +
//                      K::update) for the plain forms, a GMRES cycle for sluamd_gmres.cpp;
//   the host staging   rfs_staged: one column of B and X at a time through the resident work vectors (r_perm | b | x);
//   the entry frame    rfs_frame, and the RfsMethod of facts in which the plain / transposed, blocked, GMRES and extra-precise refinement and the residual
//                      entry points differ: refusals, the attached matrix, nrhs == 0, device, transposed index, scratch, dispatch (behind rfs_args).
// A form is the policy K = Rfs<Z, TRANS> below:
//   K::z                 complex16 (values, x, b, r_perm of two doubles);  K::trans   0 / 1 / 2 as below
//   K::residual(s, H, x, b, r_perm, safe1, safe2)   r_perm = Pc (b - op(A) x), *H->d_rfs_s.p = max(*H->d_rfs_s.p, berr bits)
//   K::update(s, H, dx_perm, x)                     x += Pc^T dx_perm
//   K::solve(H, r_perm, n[, nrhs])                  the correction, in place in r_perm: run_solve_dev for A x = b, the transposed sweeps otherwise
//                                                   (A^T d = r is A1^T (Pc d) = Pc r for the factors of A1 = Pc A Pc^T: the same permutation on both
//                                                   sides, so r_perm and K::update are used exactly alike)
// Everything is a template, so a file instantiates the forms it names and no others: sluamd_api.cpp and sluamd_zrefine.cpp name one form each
// (rfs_frame<Rfs<false, 0>>, <Rfs<true, 0>>), every other entry point names them all (rfs_frame<RfsAnyForm>: ensure_tindex and rfs_dispatch).  The CPU test
// build (oracle/Makefile) links sluamd_api.cpp without sluamd_tsolve.cpp, sluamd_*refine.cpp and sluamd_gmres.cpp, so it never sees run_tsolve, ensure_tindex
// or a kernel of the method files.  That build's engine (oracle/emul/engine_cpu.cpp) restates the double A x = b kernels under their flat signature and
// nothing else, so Rfs<false, 0> calls that pair; every other form calls the general entries.
#pragma once
#include <string>
#include <type_traits>
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

// what the refinements need beyond the arguments their entry points check (check_solve_args, sluamd_plan.h: handle, blocks, nrhs, leading dimensions, berr,
// trans, precision, planned transposed sweeps): a matrix attached to the handle -- always of the handle's precision, attach_rfs refuses any other
inline int rfs_checks(const Handle *H)
{
    if (!H->d_rfs_rp.p) { set_error(std::string("no matrix attached: call ") + (H->z ? "sluamd_zAttachMatrix" : "sluamd_dAttachMatrix") + " first"); return SLUAMD_EINVAL; }
    return 0;
}

// The pass of a step: the handle's berr word cleared, residual(s) queued on the handle's stream, the word copied back into *sv, the stream synchronised.
// rfs_pass is the pass of the policies; the extra-precise residual (sluamd_xrefine.cpp), another kernel set, goes through rfs_berr_pass with its own launch
template <class F> int rfs_berr_pass(Handle *H, double *sv, F &&residual)
{
    hipStream_t s = H->stream;
    HIPCHK(hipMemsetAsync(H->d_rfs_s.p, 0, sizeof(unsigned long long), s));
    residual(s);
    HIPCHK(hipMemcpyAsync(sv, H->d_rfs_s.p, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}
template <class K> int rfs_pass(Handle *H, const double *x, const double *b, double *r_perm, const RfsGuards &g, double *sv)
{
    return rfs_berr_pass(H, sv, [&](hipStream_t s) { K::residual(s, H, x, b, r_perm, g.safe1, g.safe2); });
}

// What the step of the loop below returns; an error code (< 0) ends the call
constexpr int RFS_STEPPED = 0, RFS_STOP = 1;
// the plain step: the correction through the sweeps, in place in r_perm, and the update
template <class K> int rfs_plain_step(Handle *H, double *Xc, double *r_perm)
{
    if (int rc = K::solve(H, r_perm, (int) H->hs.n)) return rc;
    K::update(H->stream, H, r_perm, Xc);
    return RFS_STEPPED;
}

// The outer loop, columns and steps.  d_B, d_X: device-resident, original ordering, column-major (ld in values); X holds the initial solution and is refined
// in place; r_perm: the residual vector of the method (n values).  On a grid handle (replicated form, like sluamd_pdgstrs3d) every rank passes the complete
// B and X and the call is collective.  step(j, Xc, r_perm, sv) corrects column j after a pass that left its residual in r_perm and its backward error in sv:
// RFS_STEPPED, RFS_STOP (this column ends with the berr it has, X as the step left it) or an error code.  *steps: the steps of the last column
template <class K, class Step> int rfs_dev(Handle *H, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, double *r_perm, double *berr, int32_t *steps,
                                           Step &&step)
{
    const bool grid = H->grid.size() > 1;
    if (grid && !H->comm) { set_error("handle of a multi-rank grid has no communicator"); return SLUAMD_EINVAL; }
    const int vs = K::z ? 2 : 1;
    const RfsGuards g = rfs_guards(H->hs.n);
    hipStream_t s = H->stream;
    int count = 0;
    for (int j = 0; j < nrhs; ++j) {
        const double *Bc = d_B + (size_t) j * ldb * vs;
        double *Xc = d_X + (size_t) j * ldx * vs;
        double lstres = 3.0;
        count = 0;
        for (;;) {
            double sv = 0.0;
            if (int rc = rfs_pass<K>(H, Xc, Bc, r_perm, g, &sv)) return rc;
            berr[j] = sv;
            int go = rfs_continue(sv, lstres, count) ? 1 : 0;
            // every rank computed sv from the same all-gathered x, but the step's solve is collective: decide it together, so that the
            // ranks can never split into unmatched solves
            if (grid) { if (int rc = H->comm->allreduce_min(&go, 1, s)) return rc; }
            if (!go) break;
            const int rc = step(j, Xc, r_perm, sv);
            if (rc < 0) return rc;
            if (rc == RFS_STOP) break;
            lstres = sv;
            ++count;
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (steps) *steps = count;
    return 0;
}

// Host blocks, one column at a time through the resident work vectors (r_perm | b | x): column j of B and of X goes up into the b and the x slot,
// run(j, d_b, d_x) works on the copies, and work vector `slot` (0: r, 2: x) comes back as column j of `out` (host, ld in values)
template <class F> int rfs_staged(Handle *H, const double *B, int64_t ldb, const double *X, int64_t ldx, int32_t nrhs, double *out, int64_t ldo, int slot, F &&run)
{
    const int vs = H->z ? 2 : 1;
    const size_t nv = (size_t) H->hs.n * vs, col = sizeof(double) * nv;
    double *w = H->d_rfs_work.p, *d_b = w + nv, *d_x = w + 2 * nv;
    for (int j = 0; j < nrhs; ++j) {
        HIPCHK(hipMemcpy(d_b, B + (size_t) j * ldb * vs, col, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_x, X + (size_t) j * ldx * vs, col, hipMemcpyHostToDevice));
        if (int rc = run(j, d_b, d_x)) return rc;
        HIPCHK(hipMemcpy(out + (size_t) j * ldo * vs, w + slot * nv, col, hipMemcpyDeviceToHost));
    }
    return 0;
}

// ---- the entry frame ----
// The arguments every entry point of the refinements shares.  B, X: n x nrhs values of precision z, on the host or on the device
struct RfsCall {
    sluamd_handle_t h; int trans; const void *B; int64_t ldb; void *X; int64_t ldx; int32_t nrhs; double *berr; bool z, host; const char *name;
    const double *b() const { return static_cast<const double *>(B); }
    double *x() const { return static_cast<double *>(X); }
};
// the argument checks of a refinement call (check_solve_args, sluamd_plan.h), the first line of every entry point but the residual's, which has its own;
// < 0: refused
inline int rfs_args(const RfsCall &a) { return check_solve_args(a.h, a.trans, a.B, a.ldb, a.X, a.ldx, a.nrhs, a.berr, true, a.z, a.name, "refinement"); }
// The facts in which the methods differ; tests/test_gpu_refine_refusals.py is their witness.
//                      noun             grids  batches  zero_unchecked           zero_steps
//   plain, transposed  --               yes    yes      host form, NOTRANS only  steps
//   blocked            "blocked"        yes    no       no                       --
//   GMRES              "GMRES"          no     no       no                       steps       (its option refusals: between rfs_args and the frame)
//   extra-precise      "extra-precise"  no     no       no                       --
//   residual           --               yes    yes      no                       --          (argument checks of its own: a third block R, berr optional)
struct RfsMethod {
    const char *noun;           // the method in the two refusals below ("the <noun> refinement ...")
    bool grids, batches;        // false: a handle of a multi-rank grid / of a batch is refused, in this order, before the attached matrix is asked for
    bool zero_unchecked;        // nrhs == 0 returns before the attached matrix is asked for (else right after)
    int32_t *zero_steps;        // nrhs == 0 writes *zero_steps = 0 (null: writes nothing)
};
struct RfsAnyForm {};           // Form of an entry point that takes trans at run time (else: the one policy its file names)

// One frame for every entry point, behind its argument checks: the method's refusals, the attached matrix, nrhs == 0, the device, the transposed index, the
// method's scratch (prepare(H)), then the method's body on host or device blocks, on_host(K, H) / on_dev(K, H), for the policy K of (z, trans).  A refused
// call touches nothing; after an error further on (a HIP call, an allocation, a sweep) X, berr and the per-column outputs are unspecified
template <class Form, class Prepare, class OnHost, class OnDev>
int rfs_frame(const RfsMethod &m, const RfsCall &a, Prepare &&prepare, OnHost &&on_host, OnDev &&on_dev)
{
    Handle *H = &a.h->H;
    if (!m.grids && H->grid.size() > 1) { set_error(std::string(a.name) + ": the " + m.noun + " refinement needs a 1 x 1 x 1 handle (grid handles refine with sluamd_p[dz]gsrfs3d[_trans])"); return SLUAMD_EINVAL; }
    if (!m.batches && H->batch_owned) { set_error(std::string(a.name) + ": the handle belongs to a batch (sluamd_BatchHandle): the " + m.noun + " refinement does not run on batches"); return SLUAMD_EINVAL; }
    const auto nothing_to_do = [&] { if (m.zero_steps) *m.zero_steps = 0; return 0; };
    if (a.nrhs == 0 && m.zero_unchecked) return nothing_to_do();
    if (int rc = rfs_checks(H)) return rc;
    if (a.nrhs == 0) return nothing_to_do();
    HIPCHK(hipSetDevice(H->device));
    auto run = [&](auto K) { return a.host ? on_host(K, H) : on_dev(K, H); };
    if constexpr (std::is_same<Form, RfsAnyForm>::value) {
        if (a.trans != SLUAMD_NOTRANS) { if (int rc = ensure_tindex(H, a.name)) return rc; }
        if (int rc = prepare(H)) return rc;
        return rfs_dispatch(a.z, a.trans, run);
    } else {
        if (int rc = prepare(H)) return rc;
        return run(Form());
    }
}

// The frame of a method that takes the columns one after the other: dev(K, H, d_B, ldb, d_X, ldx, nrhs, j0) is its device form, its per-column outputs
// from index j0 on; its host form is that device form on one staged column at a time, X copied back
template <class Form, class Prepare, class Dev> int rfs_frame_by_column(const RfsMethod &m, const RfsCall &a, Prepare &&prepare, Dev &&dev)
{
    return rfs_frame<Form>(m, a, prepare,
        [&](auto K, Handle *H) {
            const int64_t n = H->hs.n;
            return rfs_staged(H, a.b(), a.ldb, a.x(), a.ldx, a.nrhs, a.x(), a.ldx, 2, [&](int j, const double *d_b, double *d_x) { return dev(K, H, d_b, n, d_x, n, 1, j); });
        },
        [&](auto K, Handle *H) { return dev(K, H, a.b(), a.ldb, a.x(), a.ldx, a.nrhs, 0); });
}

// The plain refinement, sluamd_p[dz]gsrfs3d[_trans][_dev]: the loop with the plain step, the residual in the first resident work vector
template <class Form> int rfs_plain(const RfsCall &a, int32_t *steps)
{
    if (const int c = rfs_args(a); c < 0) return c;
    const RfsMethod m = {nullptr, true, true, a.host && a.trans == SLUAMD_NOTRANS, steps};
    return rfs_frame_by_column<Form>(m, a, [](Handle *) { return 0; },
        [&](auto K, Handle *H, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, int j0) {
            typedef decltype(K) P;
            return rfs_dev<P>(H, d_B, ldb, d_X, ldx, nrhs, H->d_rfs_work.p, a.berr + j0, steps, [&](int, double *Xc, double *r_perm, double) { return rfs_plain_step<P>(H, Xc, r_perm); });
        });
}

}  // namespace sluamd
