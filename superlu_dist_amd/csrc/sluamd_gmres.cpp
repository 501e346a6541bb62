// sluamd_gmres.cpp -- GMRES refinement preconditioned by the resident factors: sluamd_p[dz]gsrfs3d_gmres[_dev] (contract: include/superlu_dist_amd.h;
// the algorithm, CGS2, the reduction order and the storage: DESIGN.md "GMRES refinement").  The entry frame, the host staging and the outer loop are
// sluamd_refine.h's (rfs_frame_by_column, rfs_dev) with the same policies K -- the true residual and berr by K::residual, the same stop rule, K::update --
// and, as the step of that loop, the correction K::solve(r) replaced by one cycle of right-preconditioned
// GMRES on A1 d = r in the permuted space, A1 = Pc op(A) Pc^T, M = L U, d_0 = 0.  K::solve is the only way into the sweeps.
//   A1 z from the policy kernels: x0 = 0; K::update(x0 += Pc^T z); K::residual(x0, b = 0) = Pc (0 - op(A) x0) = -A1 z.  The sign is not undone by a pass of
//   its own: CGS2 runs on w' = -w (every coefficient comes out negated, the norm does not), the host negates the Hessenberg column and v_{j+1} = w' / (-h).
//   K::residual also leaves a backward error of that product in the handle's berr word; the outer loop clears the word before every true residual and reads
//   it right after, so nothing of it reaches the caller.
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources, none of which may reference a symbol of this file.
#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>
#include "sluamd_refine.h"
#include "sluamd_gkernels.inc"

using namespace sluamd;

namespace {

typedef std::complex<double> cplx;
const int GM_MAX_RESTART = 64;
// slots of the partials slab: the dots of up to GM_MAX_RESTART basis vectors (two doubles each for complex16), ||w||^2 from k_gm_dots, ||w||^2 from k_gm_axpys
const int GM_SLOT_NDOT = 2 * GM_MAX_RESTART, GM_SLOT_NAXPY = GM_SLOT_NDOT + 1, GM_SLOTS = GM_SLOT_NAXPY + 1;
const int GM_RES = 2 * 2 * GM_MAX_RESTART + 2;      // results behind the slab: [h of pass 1 | h of pass 2 | ||w||^2], doubles

struct Work {                                       // the Krylov workspace of one call
    int64_t ns = 0, nu = 0;                         // doubles / 16-byte units per vector
    int64_t vstride = 0;                            // doubles from one basis vector to the next: ns in a handle's workspace, the caller's choice in the self-test
    double *V = nullptr, *z = nullptr, *w = nullptr, *x0 = nullptr, *zero = nullptr, *slab = nullptr, *res = nullptr;
};

// [v_0 .. v_restart | z | w | x0 | 0]: allocated on the first call, regrown when restart grows; zero-filled, and the pad of a double vector of odd order is
// cleared again on every call (a NaN met once must not stay in it)
int ensure_work(Handle *H, int restart, bool z, Work &W)
{
    const int64_t n = H->hs.n;
    W.ns = z ? 2 * n : ((n + 1) & ~(int64_t) 1);
    W.nu = W.ns / 2;
    W.vstride = W.ns;
    const int64_t nvec = (int64_t) restart + 5;
    if (!H->d_gm_work.p || H->gm_restart < restart) {
        if (int rc = H->d_gm_work.alloc(nvec * W.ns, H->device, "the Krylov basis of the GMRES refinement")) { H->gm_restart = 0; return rc; }
        H->gm_restart = restart;
        HIPCHK(hipMemsetAsync(H->d_gm_work.p, 0, sizeof(double) * (size_t) (nvec * W.ns), H->stream));
    }
    if (!H->d_gm_part.p) {
        if (int rc = H->d_gm_part.alloc((int64_t) GM_SLOTS * GM_GRID + GM_RES, H->device, "the partial sums of the GMRES refinement")) return rc;
    }
    const int64_t have = (int64_t) H->gm_restart + 5;
    if (!z && W.ns != n) HIPCHK(hipMemset2DAsync(H->d_gm_work.p + n, sizeof(double) * (size_t) W.ns, 0, sizeof(double), (size_t) have, H->stream));
    double *p = H->d_gm_work.p;
    W.V = p; W.z = p + (have - 4) * W.ns; W.w = p + (have - 3) * W.ns; W.x0 = p + (have - 2) * W.ns; W.zero = p + (have - 1) * W.ns;
    W.slab = H->d_gm_part.p; W.res = H->d_gm_part.p + (int64_t) GM_SLOTS * GM_GRID;
    return 0;
}

// The three loops over more basis vectors than one launch takes, written once: the cycle and sluamd_krylov_selftest run the Krylov kernels through them alone.
// h[0 .. nb vs) = V[0 .. nb)^H w (device memory, vs doubles per coefficient): the dots GM_CHUNK vectors at a time, vector c0 + k into the slots
// (c0 + k) vs .., then ONE k_gm_sum over all of them.  norm_slot >= 0: ||w||^2 as well, its partials from the first launch (the only one when nb == 0),
// its sum into *nrm
void basis_dots(hipStream_t s, bool z, const Work &W, int nb, int norm_slot, double *h, double *nrm)
{
    const int vs = z ? 2 : 1;
    for (int c0 = 0; c0 < std::max(nb, norm_slot >= 0 ? 1 : 0); c0 += GM_CHUNK)
        geng::dots(s, z, W.nu, W.V + (int64_t) c0 * W.vstride, W.vstride, std::min(GM_CHUNK, nb - c0), W.w, W.slab, c0 * vs, c0 == 0 ? norm_slot : -1);
    geng::sum(s, W.nu, W.slab, 0, nb * vs, h);
    if (norm_slot >= 0) geng::sum(s, W.nu, W.slab, norm_slot, 1, nrm);
}

// w -= V[0 .. nb) h, h in device memory as basis_dots left it; every launch stores the partials of ||w||^2 of ITS new w into GM_SLOT_NAXPY: the last one's stay
void basis_axpys(hipStream_t s, bool z, const Work &W, int nb, const double *h)
{
    const int vs = z ? 2 : 1;
    for (int c0 = 0; c0 < nb; c0 += GM_CHUNK)
        geng::axpys(s, z, W.nu, W.V + (int64_t) c0 * W.vstride, W.vstride, std::min(GM_CHUNK, nb - c0), W.w, h + (int64_t) c0 * vs, W.slab, GM_SLOT_NAXPY);
}

// u = (add ? u : 0) + V[0 .. nb) y, y on the host: `add` decides for the first launch alone, every later one adds to what the launches before it left
void basis_combine(hipStream_t s, bool z, const Work &W, int nb, double *u, const cplx *y, bool add)
{
    for (int c0 = 0; c0 < nb; c0 += GM_CHUNK) {
        double yc[2 * GM_CHUNK];
        const int nv = std::min(GM_CHUNK, nb - c0);
        for (int k = 0; k < nv; ++k) { yc[2 * k] = y[c0 + k].real(); yc[2 * k + 1] = y[c0 + k].imag(); }
        geng::combine(s, z, W.nu, W.V + (int64_t) c0 * W.vstride, W.vstride, nv, u, yc, add || c0 > 0);
    }
}

// One cycle on the residual in W.w (overwritten): the correction u = M^-1 V y ends up in W.z and is added to x.  `solves`: applications of the factors so far
// for this right-hand side, at least two short of the budget on entry.  Returns 1, with the residual untouched, when its 2-norm is not a positive finite
// double: the caller then takes the plain step.  Returns 2, with X untouched and one application spent, when the first Krylov vector maps to zero: the
// caller ends the refinement of this right-hand side with the berr it has
template <class K> int gmres_cycle(Handle *H, const Work &W, const sluamd_gmres_t &o, double *Xc, double safe1, double safe2, int &solves)
{
    const bool z = K::z;
    const int vs = z ? 2 : 1, n = (int) H->hs.n, m = o.restart;
    hipStream_t s = H->stream;
    const size_t vbytes = sizeof(double) * (size_t) W.ns;
    double hres[GM_RES];
    // beta = ||r||_2, v_0 = r / beta
    basis_dots(s, z, W, 0, GM_SLOT_NDOT, W.res, W.res);
    HIPCHK(hipMemcpyAsync(hres, W.res, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double beta = std::sqrt(hres[0]);
    if (!(beta > 0.0) || !std::isfinite(beta)) return 1;       // ||r||^2 under- or overflowed: no Krylov space to build, W.w still holds r
    geng::scale(s, W.nu, W.V, W.w, beta);
    std::vector<cplx> R((size_t) m * m, cplx(0.0)), g((size_t) m + 1, cplx(0.0)), sn((size_t) m, cplx(0.0)), col((size_t) m + 1);
    std::vector<double> cs((size_t) m, 0.0);
    g[0] = beta;
    int kdim = 0;
    for (int j = 0; j < m; ++j) {
        const int nb = j + 1;                                   // basis vectors so far
        // z = M^-1 v_j;  w' = -A1 z
        HIPCHK(hipMemcpyAsync(W.z, W.V + (int64_t) j * W.ns, vbytes, hipMemcpyDeviceToDevice, s));
        if (int rc = K::solve(H, W.z, n)) return rc;
        ++solves;
        HIPCHK(hipMemsetAsync(W.x0, 0, vbytes, s));
        K::update(s, H, W.z, W.x0);
        K::residual(s, H, W.x0, W.zero, W.w, safe1, safe2);
        // CGS2: h = V^H w', w' -= V h, twice, the coefficients staying on the device between the two launches of a pass
        for (int pass = 0; pass < 2; ++pass) {
            double *h = W.res + (int64_t) pass * nb * vs;
            basis_dots(s, z, W, nb, -1, h, nullptr);                // (the norm CGS2 uses is k_gm_axpys')
            basis_axpys(s, z, W, nb, h);
        }
        geng::sum(s, W.nu, W.slab, GM_SLOT_NAXPY, 1, W.res + 2 * (int64_t) nb * vs);
        HIPCHK(hipMemcpyAsync(hres, W.res, sizeof(double) * (size_t) (2 * nb * vs + 1), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const double hn = std::sqrt(hres[2 * nb * vs]);
        for (int i = 0; i < nb; ++i) {
            const double *a = hres + i * vs, *b = hres + (nb + i) * vs;
            col[i] = -(cplx(a[0], z ? a[1] : 0.0) + cplx(b[0], z ? b[1] : 0.0));
        }
        // the rotations so far, then the one that removes h_{j+1,j}
        for (int i = 0; i < j; ++i) {
            const cplx t = cs[i] * col[i] + sn[i] * col[i + 1];
            col[i + 1] = -std::conj(sn[i]) * col[i] + cs[i] * col[i + 1];
            col[i] = t;
        }
        const double aa = std::abs(col[j]), den = std::hypot(aa, hn);
        if (!(den > 0.0) || !std::isfinite(den)) break;         // a column of zeros (or worse): the cycle ends with the columns before it
        const cplx ph = aa > 0.0 ? col[j] / aa : cplx(1.0);
        cs[j] = aa / den; sn[j] = ph * (hn / den);
        col[j] = ph * den;
        for (int i = 0; i <= j; ++i) R[(size_t) i * m + j] = col[i];
        g[j + 1] = -std::conj(sn[j]) * g[j];
        g[j] = cs[j] * g[j];
        kdim = j + 1;
        // before v_{j+1} is formed: a happy breakdown never divides
        if (std::abs(g[j + 1]) <= o.inner_tol * beta || hn == 0.0 || j + 1 == m || solves + 2 > o.max_solves) break;
        geng::scale(s, W.nu, W.V + (int64_t) (j + 1) * W.ns, W.w, -hn);
    }
    if (kdim == 0) return 2;                                    // op(A) M^-1 r = 0 (or not finite): no correction to propose, X untouched
    // R y = g on the host, u = V y, d = M^-1 u, x += Pc^T d
    std::vector<cplx> y((size_t) kdim);
    for (int i = kdim - 1; i >= 0; --i) {
        cplx t = g[i];
        for (int k = i + 1; k < kdim; ++k) t -= R[(size_t) i * m + k] * y[k];
        y[i] = t / R[(size_t) i * m + i];
    }
    basis_combine(s, z, W, kdim, W.z, y.data(), false);
    if (int rc = K::solve(H, W.z, n)) return rc;
    ++solves;
    K::update(s, H, W.z, Xc);
    return 0;
}

// d_B, d_X: device-resident, original ordering, column-major (ld in values): rfs_dev with the residual in W.w and the step below.  solves_out[nrhs], may be
// null: the applications of the factors per column, at most o.max_solves
template <class K> int gmres_dev(Handle *H, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, const sluamd_gmres_t &o, double *berr, int32_t *steps,
                                 int32_t *solves_out)
{
    Work W;
    if (int rc = ensure_work(H, o.restart, K::z, W)) return rc;
    const RfsGuards g = rfs_guards(H->hs.n);
    std::vector<int32_t> own(solves_out ? 0 : (size_t) nrhs);
    int32_t *solves = solves_out ? solves_out : own.data();
    std::fill(solves, solves + nrhs, 0);
    return rfs_dev<K>(H, d_B, ldb, d_X, ldx, nrhs, W.w, berr, steps, [&](int j, double *Xc, double *r, double) -> int {
        if (solves[j] >= o.max_solves) return RFS_STOP;             // the budget ends the column like the stop rule does
        // one application left: a cycle needs two (an iteration and the end of the cycle), so the step is the plain one
        const int rc = o.max_solves - solves[j] < 2 ? 1 : gmres_cycle<K>(H, W, o, Xc, g.safe1, g.safe2, solves[j]);
        if (rc < 0) return rc;
        if (rc == 2) return RFS_STOP;
        if (rc == 1) {
            if (int rs = rfs_plain_step<K>(H, Xc, r)) return rs;
            ++solves[j];
        }
        return RFS_STEPPED;
    });
}

int gmres_entry(sluamd_handle_t h, int trans, const void *Bv, int64_t ldb, void *Xv, int64_t ldx, int32_t nrhs, const sluamd_gmres_t *opt, double *berr, int32_t *steps,
                int32_t *solves, bool z, bool host, const char *name)
{
    const RfsCall a = {h, trans, Bv, ldb, Xv, ldx, nrhs, berr, z, host, name};
    if (const int c = rfs_args(a); c < 0) return c;
    const std::string me = std::string(name) + ": ";
    sluamd_gmres_t o;
    sluamd_default_gmres(&o);
    if (opt) o = *opt;
    if (o.restart < 1 || o.restart > GM_MAX_RESTART) { set_error(me + "restart must lie in [1, 64]"); return SLUAMD_EINVAL; }
    if (o.max_solves < 1) { set_error(me + "max_solves must be at least 1"); return SLUAMD_EINVAL; }
    if (!(o.inner_tol > 0.0 && o.inner_tol < 1.0)) { set_error(me + "inner_tol must lie in (0, 1)"); return SLUAMD_EINVAL; }
    const RfsMethod m = {"GMRES", false, false, false, steps};                // (the options above: before these) neither on grids nor on batches; nrhs == 0 writes *steps = 0
    return rfs_frame_by_column<RfsAnyForm>(m, a, [](Handle *) { return 0; },   // (the Krylov workspace: ensure_work, per call of gmres_dev -- it clears the pad every time)
        [&](auto K, Handle *H, const double *d_B, int64_t ldb_, double *d_X, int64_t ldx_, int32_t nr, int j0) {
            return gmres_dev<decltype(K)>(H, d_B, ldb_, d_X, ldx_, nr, o, berr + j0, steps, solves ? solves + j0 : nullptr);
        });
}

}  // namespace

extern "C" {

void sluamd_default_gmres(sluamd_gmres_t *o)
{
    if (!o) return;
    o->restart = 20; o->max_solves = 100; o->inner_tol = 0x1p-30;
}

int sluamd_pdgsrfs3d_gmres(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, const sluamd_gmres_t *opt, double *berr,
                           int32_t *steps, int32_t *solves)
{
    return gmres_entry(h, trans, B, ldb, X, ldx, nrhs, opt, berr, steps, solves, false, true, "sluamd_pdgsrfs3d_gmres");
}

int sluamd_pdgsrfs3d_gmres_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs, const sluamd_gmres_t *opt, double *berr,
                               int32_t *steps, int32_t *solves)
{
    return gmres_entry(h, trans, d_B, ldb, d_X, ldx, nrhs, opt, berr, steps, solves, false, false, "sluamd_pdgsrfs3d_gmres_dev");
}

int sluamd_pzgsrfs3d_gmres(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs,
                           const sluamd_gmres_t *opt, double *berr, int32_t *steps, int32_t *solves)
{
    return gmres_entry(h, trans, B, ldb, X, ldx, nrhs, opt, berr, steps, solves, true, true, "sluamd_pzgsrfs3d_gmres");
}

int sluamd_pzgsrfs3d_gmres_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X, int64_t ldx, int32_t nrhs,
                               const sluamd_gmres_t *opt, double *berr, int32_t *steps, int32_t *solves)
{
    return gmres_entry(h, trans, d_B, ldb, d_X, ldx, nrhs, opt, berr, steps, solves, true, false, "sluamd_pzgsrfs3d_gmres_dev");
}

// test hook (contract: include/superlu_dist_amd.h): one operation of the Krylov kernels through the loops gmres_cycle runs them through, on a workspace of its
// own laid out as ensure_work's -- [v_0 .. v_nv | x | dst], zero-filled vectors -- with NaN wherever the cycle's layout has no memory of a vector (the gap
// behind a basis vector when vstride > ns) and wherever a result is expected (dst, the partials slab, the result words): all bits set is a NaN
int sluamd_krylov_selftest(int op, int zi, int64_t n, int32_t nv, int64_t vstride, const double *V, const double *x, const double *coef, double h, int add,
                           double *xout, double *res)
{
    const std::string me = "sluamd_krylov_selftest: ";
    const bool z = zi != 0, basis = op != SLUAMD_KRYLOV_SCALE;
    const int vs = z ? 2 : 1, lo = op == SLUAMD_KRYLOV_AXPYS || op == SLUAMD_KRYLOV_COMBINE ? 1 : 0;
    if (op < SLUAMD_KRYLOV_DOTS || op > SLUAMD_KRYLOV_COMBINE) { set_error(me + "unknown operation"); return SLUAMD_EINVAL; }
    if (n < 1 || n > INT32_MAX) { set_error(me + "n must lie in [1, 2^31)"); return SLUAMD_EINVAL; }
    Work W;
    W.ns = z ? 2 * n : ((n + 1) & ~(int64_t) 1);
    W.nu = W.ns / 2;
    if (!basis) { nv = 0; vstride = W.ns; }
    if (nv < lo || nv > GM_MAX_RESTART) { set_error(me + "nv must lie in [" + std::to_string(lo) + ", 64] for this operation"); return SLUAMD_EINVAL; }
    if ((vstride & 1) || vstride < W.ns) { set_error(me + "vstride must be even and at least the padded length of a vector"); return SLUAMD_EINVAL; }
    const bool wants_coef = op == SLUAMD_KRYLOV_AXPYS || op == SLUAMD_KRYLOV_COMBINE, wants_res = op == SLUAMD_KRYLOV_DOTS || op == SLUAMD_KRYLOV_AXPYS;
    if (!x || !xout || (nv > 0 && !V) || (wants_coef && !coef) || (wants_res && !res)) { set_error(me + "null pointer"); return SLUAMD_EINVAL; }
    if (int rc = check_device(-1)) return rc;
    W.vstride = vstride;
    DevBuf<double> work, part;
    const int64_t nwork = nv * vstride + 2 * W.ns, npart = (int64_t) GM_SLOTS * GM_GRID + GM_RES;
    if (int rc = work.alloc(nwork, -1, "the vectors of the Krylov self-test")) return rc;
    if (int rc = part.alloc(npart, -1, "the partial sums of the Krylov self-test")) return rc;
    W.V = work.p; W.w = work.p + nv * vstride;
    double *dst = W.w + W.ns;
    W.slab = part.p; W.res = part.p + (int64_t) GM_SLOTS * GM_GRID;
    hipStream_t s = 0;
    const size_t vbytes = sizeof(double) * (size_t) W.ns, nbytes = sizeof(double) * (size_t) (n * vs);
    HIPCHK(hipMemsetAsync(part.p, 0xFF, sizeof(double) * (size_t) npart, s));
    HIPCHK(hipMemsetAsync(work.p, 0xFF, sizeof(double) * (size_t) nwork, s));
    for (int k = 0; k <= nv; ++k) {                             // the basis vectors, then x
        double *d = k < nv ? W.V + (int64_t) k * vstride : W.w;
        HIPCHK(hipMemsetAsync(d, 0, vbytes, s));
        HIPCHK(hipMemcpy(d, k < nv ? V + (int64_t) k * n * vs : x, nbytes, hipMemcpyHostToDevice));
    }
    if (op == SLUAMD_KRYLOV_DOTS) {
        basis_dots(s, z, W, nv, GM_SLOT_NDOT, W.res, W.res + nv * vs);
        HIPCHK(hipMemcpy(res, W.res, sizeof(double) * (size_t) (nv * vs + 1), hipMemcpyDeviceToHost));
    } else if (op == SLUAMD_KRYLOV_AXPYS) {                     // the coefficients where a pass of CGS2 has them, the norm where the cycle sums it
        HIPCHK(hipMemcpy(W.res, coef, sizeof(double) * (size_t) (nv * vs), hipMemcpyHostToDevice));
        basis_axpys(s, z, W, nv, W.res);
        geng::sum(s, W.nu, W.slab, GM_SLOT_NAXPY, 1, W.res + 2 * (int64_t) nv * vs);
        HIPCHK(hipMemcpy(res, W.res + 2 * (int64_t) nv * vs, sizeof(double), hipMemcpyDeviceToHost));
    } else if (op == SLUAMD_KRYLOV_SCALE) {
        geng::scale(s, W.nu, dst, W.w, h);
    } else {
        std::vector<cplx> y((size_t) nv);
        for (int k = 0; k < nv; ++k) y[k] = cplx(coef[k * vs], z ? coef[k * vs + 1] : 0.0);
        basis_combine(s, z, W, nv, W.w, y.data(), add != 0);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(xout, basis ? W.w : dst, vbytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
