// sluamd_ekernels.inc -- row / column equilibration on the device (pdgsequ + pdlaqgs, SRC/double/pdgsequ.c:126-215, SRC/double/pdlaqgs.c:89-146; complex16:
// pzgsequ.c / pzlaqgs.c with abs1(z) = |re| + |im|), the 1-norm of the scaled matrix and the fused permute-and-scale of right-hand sides and solutions.
// Included by sluamd_kernels.hip; the launchers (eng::eq_*) are referenced only by sluamd_equil.cpp (the CPU test build of the host sources has no restatement
// of them).
//
// Every matrix kernel walks the attached CSR copy of A by rows: LPR = 1, 8 or 64 lanes share a row (the host picks LPR from the mean row length), 256 / LPR
// rows per workgroup, one row group per thread group and no grid-stride loop (n < 2^31 rows in at least 4-row workgroups fit gridDim.x).  The 8- and 64-lane
// groups are aligned sub-ranges of one wave, so their reductions are __shfl_xor butterflies below the group size.
// Global minima / maxima / first zero index: non-negative doubles order like their bit patterns, so they are 64-bit integer atomicMin / atomicMax on the bits,
// one per workgroup after a wave butterfly and a 4-entry LDS step -- order-independent, bit-exact results.  red[] = {min bits, max bits, first index with an
// exactly zero maximum}, initialised by the host to {~0, 0, ~0}.

template <bool Z> struct EqVal { typedef double T; };
template <> struct EqVal<true> { typedef zc T; };
__device__ __forceinline__ double eq_abs1(double a) { return fabs(a); }
__device__ __forceinline__ double eq_abs1(zc a) { return fabs(a.x) + fabs(a.y); }       // slud_z_abs1 (pzgsequ.c:136, :182)
__device__ __forceinline__ double eq_mod(double a) { return fabs(a); }
__device__ __forceinline__ double eq_mod(zc a) { return hypot(a.x, a.y); }              // slud_z_abs: the modulus pzlangs sums
__device__ __forceinline__ double eq_mul(double a, double s) { return a * s; }
__device__ __forceinline__ zc eq_mul(zc a, double s) { return make_double2(a.x * s, a.y * s); }

typedef unsigned long long eq_u64;
constexpr eq_u64 EQ_NONE = ~0ull;

// min / max / first-zero of one candidate per thread (idle threads pass v = +inf bits EQ_NONE for the minimum, 0 for the maximum, idx = EQ_NONE), combined
// into red[0..2].  All 256 threads of the workgroup call it.
__device__ __forceinline__ void eq_block_reduce(eq_u64 vmin, eq_u64 vmax, eq_u64 idx, eq_u64 *__restrict__ red)
{
    __shared__ eq_u64 sh[3][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const eq_u64 a = __shfl_xor(vmin, o), b = __shfl_xor(vmax, o), c = __shfl_xor(idx, o);
        vmin = a < vmin ? a : vmin; vmax = b > vmax ? b : vmax; idx = c < idx ? c : idx;
    }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = vmin; sh[1][threadIdx.x >> 6] = vmax; sh[2][threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            vmin = sh[0][w] < vmin ? sh[0][w] : vmin; vmax = sh[1][w] > vmax ? sh[1][w] : vmax; idx = sh[2][w] < idx ? sh[2][w] : idx;
        }
        if (vmin != EQ_NONE) atomicMin(red + 0, vmin);
        if (vmax != 0) atomicMax(red + 1, vmax);
        if (idx != EQ_NONE) atomicMin(red + 2, idx);
    }
}

// r[i] = max_j abs1(a_ij) (pdgsequ.c:130-138) + the global min / max of r and the first exactly zero row (:141-164) in the same launch
template <int LPR, bool Z>
__global__ __launch_bounds__(256) void k_eq_rowmax(int n, const int *__restrict__ rp, const typename EqVal<Z>::T *__restrict__ av, double *__restrict__ r,
                                                   eq_u64 *__restrict__ red)
{
    const int64_t i = (int64_t) blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int lane = threadIdx.x % LPR;
    double m = 0.0;
    if (i < n)
        for (int e = rp[i] + lane, e1 = rp[i + 1]; e < e1; e += LPR) m = fmax(m, eq_abs1(av[e]));
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    const bool lead = i < n && lane == 0;
    if (lead) r[i] = m;
    const eq_u64 bits = (eq_u64) __double_as_longlong(m);
    eq_block_reduce(lead ? bits : EQ_NONE, lead ? bits : 0, lead && m == 0.0 ? (eq_u64) i : EQ_NONE, red);
}

// the same three global values of a vector (the column maxima, pdgsequ.c:195-208; the column sums of the 1-norm: only red[1] is read)
__global__ __launch_bounds__(256) void k_eq_reduce(int n, const double *__restrict__ v, eq_u64 *__restrict__ red)
{
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const double m = in ? v[i] : 0.0;
    const eq_u64 bits = (eq_u64) __double_as_longlong(m);
    eq_block_reduce(in ? bits : EQ_NONE, in ? bits : 0, in && m == 0.0 ? (eq_u64) i : EQ_NONE, red);
}

// v[i] = 1 / min(max(v[i], smlnum), bignum)  (pdgsequ.c:167-168, :211-212)
__global__ __launch_bounds__(256) void k_eq_invert(int n, double *__restrict__ v, double smlnum, double bignum)
{
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = 1.0 / fmin(fmax(v[i], smlnum), bignum);
}

// c[j] = max_i abs1(a_ij) * r[i] under the row scaling (pdgsequ.c:174-185): one integer atomicMax on the bit pattern per non-zero product (c starts as 0)
template <int LPR, bool Z>
__global__ __launch_bounds__(256) void k_eq_colmax(int n, const int *__restrict__ rp, const int *__restrict__ ci, const typename EqVal<Z>::T *__restrict__ av,
                                                   const double *__restrict__ r, eq_u64 *__restrict__ cbits)
{
    const int64_t i = (int64_t) blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int lane = threadIdx.x % LPR;
    if (i >= n) return;
    const double ri = r[i];
    for (int e = rp[i] + lane, e1 = rp[i + 1]; e < e1; e += LPR) {
        const double t = eq_abs1(av[e]) * ri;
        if (t > 0.0) atomicMax(cbits + ci[e], (eq_u64) __double_as_longlong(t));
    }
}

// pdlaqgs.c:111-146 on the attached values, in place -- mode bit 0: a *= r[i], bit 1: a *= c[j]; both: (a * r[i]) * c[j] in exactly that order -- and the
// column sums of the moduli of the values it leaves (the 1-norm of the matrix the handle will factor).  The sums are fp64 atomic adds: their low bits depend
// on the arrival order, relative error <= k 2^-52 for a column of k entries.
template <int LPR, bool Z>
__global__ __launch_bounds__(256) void k_eq_scale_norm(int n, const int *__restrict__ rp, const int *__restrict__ ci, typename EqVal<Z>::T *__restrict__ av,
                                                       const double *__restrict__ r, const double *__restrict__ c, int mode, double *__restrict__ colsum)
{
    const int64_t i = (int64_t) blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int lane = threadIdx.x % LPR;
    if (i >= n) return;
    const double ri = (mode & 1) ? r[i] : 1.0;
    for (int e = rp[i] + lane, e1 = rp[i + 1]; e < e1; e += LPR) {
        const int j = ci[e];
        typename EqVal<Z>::T a = av[e];
        if (mode & 1) a = eq_mul(a, ri);
        if (mode & 2) a = eq_mul(a, c[j]);
        if (mode) av[e] = a;
        const double t = eq_mod(a);
        if (t != 0.0) unsafeAtomicAdd(colsum + j, t);
    }
}

// d_aval[q] = attached_values[ent[q]]: the retained entries of this rank in the order of their arena positions (Handle::d_apos)
template <bool Z>
__global__ __launch_bounds__(256) void k_eq_gather(int64_t cnt, const int *__restrict__ ent, const typename EqVal<Z>::T *__restrict__ av,
                                                   typename EqVal<Z>::T *__restrict__ out)
{
    const int64_t q = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (q < cnt) out[q] = av[ent[q]];
}

// Fused permute-and-scale of n x nrhs column-major blocks, rows over blockIdx.x, columns over blockIdx.y (strided: gridDim.y <= 65535).
//   scatter: dst[perm[i], j] = s[i] * src[i, j]      (right-hand sides into the ordering and scaling of the factored matrix)
//   gather:  dst[i, j] = s[i] * src[perm[i], j]      (solutions back)
// s == nullptr: no scaling; perm == nullptr: identity.  dst may be src only when perm == nullptr.
template <bool Z, bool GATHER>
__global__ __launch_bounds__(256) void k_eq_permscale(int n, int nrhs, const int *__restrict__ perm, const double *__restrict__ s,
                                                      const typename EqVal<Z>::T *src, int64_t lds, typename EqVal<Z>::T *dst, int64_t ldd)
{
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = perm ? perm[i] : i;
    const double si = s ? s[i] : 1.0;
    for (int j = blockIdx.y; j < nrhs; j += gridDim.y) {
        const typename EqVal<Z>::T v = src[(GATHER ? p : i) + (int64_t) j * lds];
        dst[(GATHER ? i : p) + (int64_t) j * ldd] = s ? eq_mul(v, si) : v;
    }
}

namespace eng {

// lanes per row from the mean row length
static inline int eq_lpr(int n, int64_t nnz) { const int64_t mean = n > 0 ? nnz / n : 0; return mean < 4 ? 1 : mean < 32 ? 8 : 64; }
#define EQ_ROWS_LAUNCH(KERNEL, ...)                                                                                                             \
    do {                                                                                                                                        \
        const int lpr = eq_lpr(n, nnz);                                                                                                         \
        const unsigned nb = (unsigned) (((int64_t) n + 256 / lpr - 1) / (256 / lpr));                                                           \
        if (lpr == 1) hipLaunchKernelGGL((KERNEL<1, false>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                          \
        else if (lpr == 8) hipLaunchKernelGGL((KERNEL<8, false>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                     \
        else hipLaunchKernelGGL((KERNEL<64, false>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                                  \
    } while (0)
#define EQ_ROWS_LAUNCH_Z(KERNEL, ...)                                                                                                           \
    do {                                                                                                                                        \
        const int lpr = eq_lpr(n, nnz);                                                                                                         \
        const unsigned nb = (unsigned) (((int64_t) n + 256 / lpr - 1) / (256 / lpr));                                                           \
        if (lpr == 1) hipLaunchKernelGGL((KERNEL<1, true>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                           \
        else if (lpr == 8) hipLaunchKernelGGL((KERNEL<8, true>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                      \
        else hipLaunchKernelGGL((KERNEL<64, true>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                                   \
    } while (0)

void eq_rowmax(hipStream_t s, bool z, int n, int64_t nnz, const int *rp, const void *av, double *r, unsigned long long *red)
{
    if (n <= 0) return;
    if (z) EQ_ROWS_LAUNCH_Z(k_eq_rowmax, n, rp, reinterpret_cast<const zc *>(av), r, red);
    else EQ_ROWS_LAUNCH(k_eq_rowmax, n, rp, reinterpret_cast<const double *>(av), r, red);
}

void eq_reduce(hipStream_t s, int n, const double *v, unsigned long long *red)
{
    if (n > 0) hipLaunchKernelGGL(k_eq_reduce, dim3((n + 255) / 256), dim3(256), 0, s, n, v, red);
}

void eq_invert(hipStream_t s, int n, double *v, double smlnum, double bignum)
{
    if (n > 0) hipLaunchKernelGGL(k_eq_invert, dim3((n + 255) / 256), dim3(256), 0, s, n, v, smlnum, bignum);
}

void eq_colmax(hipStream_t s, bool z, int n, int64_t nnz, const int *rp, const int *ci, const void *av, const double *r, double *c)
{
    if (n <= 0) return;
    eq_u64 *cb = reinterpret_cast<eq_u64 *>(c);
    if (z) EQ_ROWS_LAUNCH_Z(k_eq_colmax, n, rp, ci, reinterpret_cast<const zc *>(av), r, cb);
    else EQ_ROWS_LAUNCH(k_eq_colmax, n, rp, ci, reinterpret_cast<const double *>(av), r, cb);
}

void eq_scale_norm(hipStream_t s, bool z, int n, int64_t nnz, const int *rp, const int *ci, void *av, const double *r, const double *c, int mode, double *colsum)
{
    if (n <= 0) return;
    if (z) EQ_ROWS_LAUNCH_Z(k_eq_scale_norm, n, rp, ci, reinterpret_cast<zc *>(av), r, c, mode, colsum);
    else EQ_ROWS_LAUNCH(k_eq_scale_norm, n, rp, ci, reinterpret_cast<double *>(av), r, c, mode, colsum);
}
#undef EQ_ROWS_LAUNCH
#undef EQ_ROWS_LAUNCH_Z

void eq_gather(hipStream_t s, bool z, int64_t cnt, const int *ent, const void *av, void *out)
{
    if (cnt <= 0) return;
    const dim3 g((unsigned) ((cnt + 255) / 256));
    if (z) hipLaunchKernelGGL(k_eq_gather<true>, g, dim3(256), 0, s, cnt, ent, reinterpret_cast<const zc *>(av), reinterpret_cast<zc *>(out));
    else hipLaunchKernelGGL(k_eq_gather<false>, g, dim3(256), 0, s, cnt, ent, reinterpret_cast<const double *>(av), reinterpret_cast<double *>(out));
}

void eq_permscale(hipStream_t s, bool z, bool gather, int n, int nrhs, const int *perm, const double *scale, const void *src, int64_t lds, void *dst, int64_t ldd)
{
    if (n <= 0 || nrhs <= 0) return;
    const dim3 g((unsigned) ((n + 255) / 256), (unsigned) std::min(nrhs, 65535));
    if (z) {
        const zc *a = reinterpret_cast<const zc *>(src); zc *d = reinterpret_cast<zc *>(dst);
        if (gather) hipLaunchKernelGGL((k_eq_permscale<true, true>), g, dim3(256), 0, s, n, nrhs, perm, scale, a, lds, d, ldd);
        else hipLaunchKernelGGL((k_eq_permscale<true, false>), g, dim3(256), 0, s, n, nrhs, perm, scale, a, lds, d, ldd);
    } else {
        const double *a = reinterpret_cast<const double *>(src); double *d = reinterpret_cast<double *>(dst);
        if (gather) hipLaunchKernelGGL((k_eq_permscale<false, true>), g, dim3(256), 0, s, n, nrhs, perm, scale, a, lds, d, ldd);
        else hipLaunchKernelGGL((k_eq_permscale<false, false>), g, dim3(256), 0, s, n, nrhs, perm, scale, a, lds, d, ldd);
    }
}

}  // namespace eng
