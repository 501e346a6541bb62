// sluamd_bkernels.inc -- kernels of the batch object (sluamd_batch.cpp, which includes this file: the batch kernels are compiled with their only caller and
// are no part of sluamd_kernels.hip; the CPU test build of the host sources has no restatement of them).  A batch is `count` matrices of order m with ONE
// sparsity pattern, factored as the block-diagonal matrix diag(A_0 .. A_{count-1}) on one ordinary handle: global row / column k m + i belongs to matrix k,
// supernode k ns + s is copy k of supernode s.  Every kernel here addresses matrix k through tables of ONE matrix plus the per-copy offset.
// gfx950, wave64; all of them are HBM streams of a few bytes per entry, one thread per entry, consecutive lanes on consecutive entries.
// Both precisions: V = double, or bzc (complex16) whose values move as ONE 16-byte access, so consecutive lanes still cover consecutive memory.  Offsets,
// strides and leading dimensions count VALUES in either precision (the complex store counts its slots and diagonal positions in values too).  The scalings
// R and C and the backward errors are real.  The complex moduli are those of the single-matrix kernels: abs1(z) = |re| + |im| wherever the reference uses
// slud_z_abs1 (refinement; the equilibration's maxima come from eng::eq_rowmax / eq_colmax themselves), hypot for the 1-norm (k_eq_scale_norm).

#include "sluamd_rkernels.inc"   // rfs_row, rfs_add: the refinement arithmetic of the single-matrix kernels

typedef double2 bzc;
template <bool Z> struct BVal { typedef double T; };
template <> struct BVal<true> { typedef bzc T; };
__device__ __forceinline__ double bk_mul(double a, double s) { return a * s; }
__device__ __forceinline__ bzc bk_mul(bzc a, double s) { return make_double2(a.x * s, a.y * s); }        // eq_mul
__device__ __forceinline__ double bk_mod(double a) { return fabs(a); }
__device__ __forceinline__ double bk_mod(bzc a) { return hypot(a.x, a.y); }                             // eq_mod: the modulus pzlangs sums
__device__ __forceinline__ bool bk_zero(double a) { return a == 0.0; }
__device__ __forceinline__ bool bk_zero(bzc a) { return a.x == 0.0 && a.y == 0.0; }

// The distribution kernel (creation and value updates alike): entry e of the shared CSR pattern, matrix k (blockIdx.y, strided)
//   av[k nnz + e] = val[slot(k, e) + map[e].y] = nz[k stride + e]                     (av or val may be null: that side is not written)
// map[e] = (slot id, offset inside the slot) of entry e in ONE matrix: slot id s >= 0: the L slot of supernode s, ~s (negative): the U slot of block row s.  The
// slots of copy k start at sn_lval / sn_uval[k ns + s] (the handle's own tables); inside a slot every copy has the layout of the first.
template <class V>
__global__ __launch_bounds__(256) void k_batch_values(int64_t nnz, int count, int ns, int64_t stride, const V *nz, const int2 *__restrict__ map,
                                                      const int64_t *__restrict__ sn_lval, const int64_t *__restrict__ sn_uval, V *av, V *__restrict__ val)
{
    for (int k = blockIdx.y; k < count; k += gridDim.y) {
        const int64_t ks = (int64_t) k * ns;
        for (int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x; e < nnz; e += (int64_t) gridDim.x * 256) {
            const int2 q = map[e];
            const V v = nz[(int64_t) k * stride + e];
            if (av) av[(int64_t) k * nnz + e] = v;
            if (val) {
                const int64_t base = q.x >= 0 ? sn_lval[ks + q.x] : sn_uval[ks + ~q.x];
                val[base + q.y] = v;
            }
        }
    }
}

// The batched twins of k_eq_permscale.  One thread per global row g = k m + i (flat: full waves whatever m is), right-hand sides in a loop; pc = perm_c of ONE
// matrix (null: identity), s_in / s_out (real; may be null) indexed by g.
//   pack:   xp[k m + pc[i], j] = s_in[k m + i] B_k[i, j]          unpack:  X_k[i, j] = s_out[k m + i] xp[k m + pc[i], j]
template <class V, bool UNPACK>
__global__ __launch_bounds__(256) void k_batch_permscale(int m, int64_t n, int nrhs, const int *__restrict__ pc, const double *__restrict__ sc, V *xp,
                                                         int64_t ldxp, V *bx, int64_t ld, int64_t strideb)
{
    const int64_t g = (int64_t) blockIdx.x * 256 + threadIdx.x;            // flat over (k, i): full waves whatever m is
    if (g >= n) return;
    const int k = (int) (g / m), i = (int) (g - (int64_t) k * m);
    const int p = pc ? pc[i] : i;
    const double si = sc ? sc[g] : 1.0;
    for (int j = 0; j < nrhs; ++j) {
        V *a = xp + (g - i) + p + (int64_t) j * ldxp;
        V *b = bx + (int64_t) k * strideb + i + (int64_t) j * ld;
        if (UNPACK) *b = sc ? bk_mul(*a, si) : *a; else *a = sc ? bk_mul(*b, si) : *b;
    }
}

// X_k[i, j] *= s[k m + i] in place (the unscaling after a refinement of the scaled system)
template <class V>
__global__ __launch_bounds__(256) void k_batch_scale_x(int m, int64_t n, int nrhs, const double *__restrict__ sc, V *__restrict__ x, int64_t ld, int64_t stride)
{
    const int64_t g = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int k = (int) (g / m), i = (int) (g - (int64_t) k * m);
    for (int j = 0; j < nrhs; ++j) {
        V *p = x + (int64_t) k * stride + i + (int64_t) j * ld;
        *p = bk_mul(*p, sc[g]);
    }
}

// ---- segmented equilibration.  Row and column maxima are per row / column already (eng::eq_rowmax / eq_colmax on the attached block-diagonal CSR); these
// kernels add what a batch needs per MATRIX.
// red[3 k + 0 .. 2] = {min bits, max bits, first LOCAL index whose value is exactly 0} of v[k m .. (k + 1) m), preset to {~0, 0, ~0}: the twin of k_eq_reduce.
// Non-negative doubles order like their bit patterns; integer atomics: order-independent, bit-exact.  A wave inside one matrix reduces first.
__global__ __launch_bounds__(256) void k_batch_seg_reduce(int64_t n, int m, const double *__restrict__ v, unsigned long long *__restrict__ red)
{
    typedef unsigned long long u64;
    const int64_t g = (int64_t) blockIdx.x * 256 + threadIdx.x;
    const bool in = g < n;
    const int k = in ? (int) (g / m) : -1;
    const double x = in ? v[g] : 0.0;
    u64 vmin = in ? (u64) __double_as_longlong(x) : ~0ull, vmax = in ? (u64) __double_as_longlong(x) : 0ull;
    u64 idx = in && x == 0.0 ? (u64) (g - (int64_t) k * m) : ~0ull;
    const int k0 = __shfl(k, 0), k1 = __shfl(k, 63);
    if (k0 == k1) {
        if (k0 < 0) return;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 a = __shfl_xor(vmin, o), b = __shfl_xor(vmax, o), c = __shfl_xor(idx, o);
            vmin = a < vmin ? a : vmin; vmax = b > vmax ? b : vmax; idx = c < idx ? c : idx;
        }
        if ((threadIdx.x & 63) != 0) return;
    } else if (!in) return;
    u64 *r = red + 3 * (int64_t) k;
    atomicMin(r + 0, vmin);
    if (vmax != 0) atomicMax(r + 1, vmax);
    if (idx != ~0ull) atomicMin(r + 2, idx);
}

// pdlaqgs / pzlaqgs on the attached values with matrix k's OWN decision: mode[k] bit 0: a *= r[i], bit 1: a *= c[j], both: (a r[i]) c[j] in exactly that
// order (as k_eq_scale_norm; complex16: both parts by the real factor); colsum (zero-filled) += the moduli of what is left (complex16: hypot), by column: fp64
// atomic adds, the summation caveat of sluamd_equil_t::anorm.  One thread per row: the rows of a batch's matrices are short
template <class V>
__global__ __launch_bounds__(256) void k_batch_eq_scale(int64_t n, int m, const int *__restrict__ rp, const int *__restrict__ ci, V *__restrict__ av,
                                                        const double *__restrict__ r, const double *__restrict__ c, const int *__restrict__ mode,
                                                        double *__restrict__ colsum)
{
    const int64_t g = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int md = mode[g / m];
    const double ri = (md & 1) ? r[g] : 1.0;
    for (int e = rp[g], e1 = rp[g + 1]; e < e1; ++e) {
        const int j = ci[e];
        V a = av[e];
        if (md & 1) a = bk_mul(a, ri);
        if (md & 2) a = bk_mul(a, c[j]);
        if (md) av[e] = a;
        const double t = bk_mod(a);
        if (t != 0.0) unsafeAtomicAdd(colsum + j, t);
    }
}

// R and C as the solves use them: ones where matrix k's mode leaves that side unscaled (a product with 1.0 is exact)
__global__ __launch_bounds__(256) void k_batch_eq_ones(int64_t n, int m, const int *__restrict__ mode, double *__restrict__ r, double *__restrict__ c)
{
    const int64_t g = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int md = mode[g / m];
    if (!(md & 1)) r[g] = 1.0;
    if (!(md & 2)) c[g] = 1.0;
}

// info[k] = min(info[k], c + 1) over the columns c of matrix k whose U diagonal entry is exactly zero (complex16: 0 + 0i); info preset to INT_MAX by the
// caller.  dpos[g]: arena position (in values) of the diagonal entry of global column g (inside the diagonal block at the top of the column's L slot), built
// once at creation
template <class V>
__global__ __launch_bounds__(256) void k_batch_info(int64_t ncol, int m, const int64_t *__restrict__ dpos, const V *__restrict__ val, int *__restrict__ info)
{
    const int64_t g = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (g >= ncol) return;
    if (bk_zero(val[dpos[g]])) atomicMin(info + g / m, (int) (g % m) + 1);
}

// the backward error q of one row / column (q = 0 outside the matrix, k = -1 there) maximised into s_out[k] (integer atomicMax on the bit pattern of a
// non-negative double).  A wave whose rows all belong to one matrix reduces first; a wave that straddles a matrix boundary lets every lane do its own atomic.
// All 64 lanes of the wave call it.
__device__ __forceinline__ void bk_berr_max(int k, double q, unsigned long long *__restrict__ s_out)
{
    const int k0 = __shfl(k, 0), k1 = __shfl(k, 63);
    if (k0 == k1) {                                   // (k1 == -1 != k0 on the wave that holds the last row: per-lane atomics there too)
        if (k0 < 0) return;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q = fmax(q, __shfl_xor(q, o));
        if ((threadIdx.x & 63) == 0 && q > 0.0) atomicMax(s_out + k0, (unsigned long long) __double_as_longlong(q));      // (q > 0 is false for NaN: both branches drop it alike)
    } else if (k >= 0 && q > 0.0) {
        atomicMax(s_out + k, (unsigned long long) __double_as_longlong(q));
    }
}

// k_rfs_residual<V, TRANS, CONJ> on the attached block-diagonal matrix: one thread per global row g = k m + i of op(A), (ptr, idx, pos) its CSR or (TRANS) its
// transposed index over GLOBAL rows and columns, x and b read from matrix k's own block (x = X_k[:, j] at xs + k stridex, b likewise),
// r_perm[pc[g]] = b_i - sum_e op(a_e) x_k[idx[e] - k m], the backward error of the row maximised into s_out[k].  The row is rfs_row (sluamd_rkernels.inc), the
// text the single-matrix kernels run: a batch is bitwise one matrix alone.
template <bool Z, bool TRANS, bool CONJ>
__global__ __launch_bounds__(256) void k_batch_residual(int64_t n, int m, const int *__restrict__ ptr, const int *__restrict__ idx, const int *__restrict__ pos,
                                                        const typename BVal<Z>::T *__restrict__ av, const typename BVal<Z>::T *__restrict__ xs, int64_t stridex,
                                                        const typename BVal<Z>::T *__restrict__ bs, int64_t strideb, const int *__restrict__ pc,
                                                        typename BVal<Z>::T *__restrict__ r_perm, unsigned long long *__restrict__ s_out, double safe1, double safe2)
{
    typedef typename BVal<Z>::T V;
    const int64_t g = (int64_t) blockIdx.x * 256 + threadIdx.x;
    double q = 0.0;
    int k = -1;
    if (g < n) {
        k = (int) (g / m);
        const int i = (int) (g - (int64_t) k * m);
        const V *x = xs + (int64_t) k * stridex - (int64_t) k * m;     // indexed by the global column (TRANS: row)
        V r;
        q = rfs_row<V, CONJ, TRANS>(ptr[g], ptr[g + 1], idx, pos, av, x, bs[(int64_t) k * strideb + i], safe1, safe2, r);
        r_perm[pc[g]] = r;
    }
    bk_berr_max(k, q, s_out);
}

// masked k_rfs_update: X_k[i] += dx_perm[pc[k m + i]] for the matrices that continue (go[k] != 0)
template <bool Z>
__global__ __launch_bounds__(256) void k_batch_update(int64_t n, int m, const int *__restrict__ pc, const int *__restrict__ go,
                                                      const typename BVal<Z>::T *__restrict__ dx_perm, typename BVal<Z>::T *__restrict__ xs, int64_t stridex)
{
    const int64_t g = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int k = (int) (g / m);
    if (!go[k]) return;
    auto *p = xs + (int64_t) k * stridex + (g - (int64_t) k * m);
    auto v = *p;
    rfs_add(v, dx_perm[pc[g]]);
    *p = v;
}

namespace sluamd { namespace beng {

// z: complex16 -- the value pointers (void) are bzc arrays then, double arrays otherwise; strides and leading dimensions in values
static inline unsigned batch_yblocks(int count) { return (unsigned) std::min(count, 65535); }
static inline dim3 batch_rows(int64_t n) { return dim3((unsigned) ((n + 255) / 256)); }
#define BZ(p) reinterpret_cast<bzc *>(p)
#define BZC(p) reinterpret_cast<const bzc *>(p)
#define BD(p) reinterpret_cast<double *>(p)
#define BDC(p) reinterpret_cast<const double *>(p)

void batch_values(hipStream_t s, bool z, int64_t nnz, int count, int ns, int64_t stride, const void *nz, const int2 *map, const int64_t *sn_lval,
                  const int64_t *sn_uval, void *av, void *val)
{
    if (nnz <= 0 || count <= 0) return;
    const dim3 g((unsigned) std::min<int64_t>((nnz + 255) / 256, 4096), batch_yblocks(count));
    if (z) hipLaunchKernelGGL(k_batch_values<bzc>, g, dim3(256), 0, s, nnz, count, ns, stride, BZC(nz), map, sn_lval, sn_uval, BZ(av), BZ(val));
    else hipLaunchKernelGGL(k_batch_values<double>, g, dim3(256), 0, s, nnz, count, ns, stride, BDC(nz), map, sn_lval, sn_uval, BD(av), BD(val));
}

void batch_pack(hipStream_t s, bool z, int m, int count, int nrhs, const int *pc, const double *s_in, const void *B, int64_t ldb, int64_t strideb, void *xp, int64_t ldxp)
{
    if (m <= 0 || count <= 0 || nrhs <= 0) return;
    const int64_t n = (int64_t) m * count;
    if (z) hipLaunchKernelGGL((k_batch_permscale<bzc, false>), batch_rows(n), dim3(256), 0, s, m, n, nrhs, pc, s_in, BZ(xp), ldxp, const_cast<bzc *>(BZC(B)), ldb, strideb);
    else hipLaunchKernelGGL((k_batch_permscale<double, false>), batch_rows(n), dim3(256), 0, s, m, n, nrhs, pc, s_in, BD(xp), ldxp, const_cast<double *>(BDC(B)), ldb, strideb);
}

void batch_unpack(hipStream_t s, bool z, int m, int count, int nrhs, const int *pc, const double *s_out, void *xp, int64_t ldxp, void *X, int64_t ldx, int64_t stridex)
{
    if (m <= 0 || count <= 0 || nrhs <= 0) return;
    const int64_t n = (int64_t) m * count;
    if (z) hipLaunchKernelGGL((k_batch_permscale<bzc, true>), batch_rows(n), dim3(256), 0, s, m, n, nrhs, pc, s_out, BZ(xp), ldxp, BZ(X), ldx, stridex);
    else hipLaunchKernelGGL((k_batch_permscale<double, true>), batch_rows(n), dim3(256), 0, s, m, n, nrhs, pc, s_out, BD(xp), ldxp, BD(X), ldx, stridex);
}

void batch_scale_x(hipStream_t s, bool z, int m, int count, int nrhs, const double *sc, void *X, int64_t ldx, int64_t stridex)
{
    const int64_t n = (int64_t) m * count;
    if (n <= 0 || nrhs <= 0) return;
    if (z) hipLaunchKernelGGL(k_batch_scale_x<bzc>, batch_rows(n), dim3(256), 0, s, m, n, nrhs, sc, BZ(X), ldx, stridex);
    else hipLaunchKernelGGL(k_batch_scale_x<double>, batch_rows(n), dim3(256), 0, s, m, n, nrhs, sc, BD(X), ldx, stridex);
}

void batch_seg_reduce(hipStream_t s, int64_t n, int m, const double *v, unsigned long long *red)
{
    if (n > 0) hipLaunchKernelGGL(k_batch_seg_reduce, batch_rows(n), dim3(256), 0, s, n, m, v, red);
}

void batch_eq_scale(hipStream_t s, bool z, int64_t n, int m, const int *rp, const int *ci, void *av, const double *r, const double *c, const int *mode, double *colsum)
{
    if (n <= 0) return;
    if (z) hipLaunchKernelGGL(k_batch_eq_scale<bzc>, batch_rows(n), dim3(256), 0, s, n, m, rp, ci, BZ(av), r, c, mode, colsum);
    else hipLaunchKernelGGL(k_batch_eq_scale<double>, batch_rows(n), dim3(256), 0, s, n, m, rp, ci, BD(av), r, c, mode, colsum);
}

void batch_eq_ones(hipStream_t s, int64_t n, int m, const int *mode, double *r, double *c)
{
    if (n > 0) hipLaunchKernelGGL(k_batch_eq_ones, batch_rows(n), dim3(256), 0, s, n, m, mode, r, c);
}

void batch_info(hipStream_t s, bool z, int64_t ncol, int m, const int64_t *dpos, const void *val, int *info)
{
    if (ncol <= 0) return;
    if (z) hipLaunchKernelGGL(k_batch_info<bzc>, batch_rows(ncol), dim3(256), 0, s, ncol, m, dpos, BZC(val), info);
    else hipLaunchKernelGGL(k_batch_info<double>, batch_rows(ncol), dim3(256), 0, s, ncol, m, dpos, BDC(val), info);
}

// A: rfs_mat() of the batch's handle (A.pos: the transposed index); conj is read on that complex16 form only: the conjugate of a real matrix is itself
void batch_residual(hipStream_t s, bool z, bool conj, const RfsMat &A, int m, const void *xs, int64_t stridex, const void *bs, int64_t strideb, void *r_perm,
                    unsigned long long *s_out, double safe1, double safe2)
{
    if (A.n <= 0) return;
#define BATCH_RESIDUAL(Z, TRANS, CONJ)                                                                                                                  \
    hipLaunchKernelGGL((k_batch_residual<Z, TRANS, CONJ>), batch_rows(A.n), dim3(256), 0, s, A.n, m, A.ptr, A.idx, A.pos,                               \
                       reinterpret_cast<const typename BVal<Z>::T *>(A.av), reinterpret_cast<const typename BVal<Z>::T *>(xs), stridex,                 \
                       reinterpret_cast<const typename BVal<Z>::T *>(bs), strideb, A.pc, reinterpret_cast<typename BVal<Z>::T *>(r_perm), s_out, safe1, safe2)
    if (!z) { if (A.pos) BATCH_RESIDUAL(false, true, false); else BATCH_RESIDUAL(false, false, false); }
    else if (!A.pos) BATCH_RESIDUAL(true, false, false);
    else if (conj) BATCH_RESIDUAL(true, true, true);
    else BATCH_RESIDUAL(true, true, false);
#undef BATCH_RESIDUAL
}

void batch_update(hipStream_t s, bool z, int64_t n, int m, const int *pc, const int *go, const void *dx_perm, void *xs, int64_t stridex)
{
    if (n <= 0) return;
    if (z) hipLaunchKernelGGL(k_batch_update<true>, batch_rows(n), dim3(256), 0, s, n, m, pc, go, BZC(dx_perm), BZ(xs), stridex);
    else hipLaunchKernelGGL(k_batch_update<false>, batch_rows(n), dim3(256), 0, s, n, m, pc, go, BDC(dx_perm), BD(xs), stridex);
}
#undef BZ
#undef BZC
#undef BD
#undef BDC

} }  // namespace sluamd::beng
