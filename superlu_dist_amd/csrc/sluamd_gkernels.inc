// sluamd_gkernels.inc -- the Krylov kernels of the GMRES refinement (sluamd_gmres.cpp, which includes this file: they are compiled with their only caller
// and are no part of sluamd_kernels.hip; the CPU test build of the host sources has no restatement of them).  gfx950, wave64.
// All of them stream vectors of n values once: HBM-bound, no reuse, so nothing is staged through LDS -- a thread keeps one 16-byte fragment of w and up to
// GM_CHUNK accumulators (or coefficients) in registers and every access is one 16-byte load or store, consecutive lanes on consecutive memory.
// Both precisions in ONE unit: a vector is `nu` double2.  complex16: one unit = one value, nu = n.  double: one unit = two values, nu = (n + 1) / 2 -- every
// vector these kernels touch lives in the handle's Krylov workspace, starts 16-byte aligned and is padded to an even count with a zero that stays zero
// (0 * v adds nothing to a dot product, 0 - 0 h = 0, 0 / h = 0).
// Reductions.  A FIXED launch shape -- gm_blocks(nu) workgroups of GM_BLOCK threads, grid-stride -- so which elements a thread sums, and in which order,
// depends on n alone; inside the wave by __shfl_xor (a fixed butterfly), across the four waves through LDS in wave order; every workgroup stores ONE partial
// per quantity into the slab (slab[slot * nblk + workgroup], plain stores), and k_gm_sum, a launch of its own, adds the partials of a slot in a fixed order.
// No floating-point atomics: the results repeat bit for bit.
// GM_GRID x GM_BLOCK units are one full sweep of the grid: 262144 units = 524288 doubles or 262144 complex16 values; beyond that the grid-stride loops wrap
// (tests/gmres_cases.py: LARGE_N = 524288 + 4097 is the first size class that does).
// Tested one operation at a time, exactly, through sluamd_krylov_selftest (sluamd_gmres.cpp): tests/test_gpu_krylov_kernels.py; the constants below are
// restated in tests/krylov_cases.py.

#define GM_BLOCK 256
#define GM_GRID 1024
#define GM_CHUNK 8        // basis vectors per pass over w

template <bool Z> __device__ __forceinline__ void gm_dot(double2 &a, const double2 v, const double2 w)      // a += conj(v) w  (double: the two lanes of the unit into a.x)
{
    a.x = fma(v.x, w.x, a.x); a.x = fma(v.y, w.y, a.x);
    if (Z) { a.y = fma(v.x, w.y, a.y); a.y = fma(-v.y, w.x, a.y); }
}
template <bool Z> __device__ __forceinline__ void gm_axpy(double2 &w, const double2 v, const double2 h)     // w -= v h
{
    if (Z) { w.x = fma(-v.x, h.x, w.x); w.x = fma(v.y, h.y, w.x); w.y = fma(-v.x, h.y, w.y); w.y = fma(-v.y, h.x, w.y); }
    else { w.x = fma(-v.x, h.x, w.x); w.y = fma(-v.y, h.x, w.y); }
}
template <bool Z> __device__ __forceinline__ void gm_madd(double2 &u, const double2 v, const double2 y)     // u += v y
{
    if (Z) { u.x = fma(v.x, y.x, u.x); u.x = fma(-v.y, y.y, u.x); u.y = fma(v.x, y.y, u.y); u.y = fma(v.y, y.x, u.y); }
    else { u.x = fma(v.x, y.x, u.x); u.y = fma(v.y, y.x, u.y); }
}

// the sum of `a` over the workgroup, valid in thread 0: butterfly inside the wave, then the four waves in order.  red: GM_BLOCK / 64 doubles of LDS
__device__ __forceinline__ double gm_block_sum(double a, double *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    __syncthreads();                                   // the previous quantity's readers are done with red
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// slab[(slot0 + vs k + c) nblk + b] = partial of (v_k^H w) (c = 0: real part, 1: imaginary part, complex16 only), k < NV;
// slab[norm_slot nblk + b] = partial of ||w||^2 (norm_slot < 0: not wanted).  One read of w
template <bool Z, int NV>
__global__ __launch_bounds__(GM_BLOCK) void k_gm_dots(int64_t nu, const double2 *__restrict__ V, int64_t vstride, const double2 *__restrict__ w, double *__restrict__ slab,
                                                      int slot0, int norm_slot)
{
    __shared__ double red[GM_BLOCK / 64];
    double2 acc[NV > 0 ? NV : 1];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = make_double2(0.0, 0.0);
    double nrm = 0.0;
    for (int64_t i = (int64_t) blockIdx.x * GM_BLOCK + threadIdx.x; i < nu; i += (int64_t) gridDim.x * GM_BLOCK) {
        const double2 wv = w[i];
        double2 vv[NV > 0 ? NV : 1];
#pragma unroll
        for (int k = 0; k < NV; ++k) vv[k] = V[(int64_t) k * vstride + i];         // all loads in flight before the first use
        nrm = fma(wv.x, wv.x, nrm); nrm = fma(wv.y, wv.y, nrm);
#pragma unroll
        for (int k = 0; k < NV; ++k) gm_dot<Z>(acc[k], vv[k], wv);
    }
    const int vs = Z ? 2 : 1;
    const int64_t nblk = gridDim.x;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double re = gm_block_sum(acc[k].x, red);
        if (threadIdx.x == 0) slab[(int64_t) (slot0 + vs * k) * nblk + blockIdx.x] = re;
        if (Z) {
            const double im = gm_block_sum(acc[k].y, red);
            if (threadIdx.x == 0) slab[(int64_t) (slot0 + vs * k + 1) * nblk + blockIdx.x] = im;
        }
    }
    if (norm_slot >= 0) {                                  // (the same in every thread)
        const double t = gm_block_sum(nrm, red);
        if (threadIdx.x == 0) slab[(int64_t) norm_slot * nblk + blockIdx.x] = t;
    }
}

// dst[q] = the partials of slot first + q (q = blockIdx.x) added in a fixed order: thread t takes the partials t, t + GM_BLOCK, ... in turn, then the workgroup sum
__global__ __launch_bounds__(GM_BLOCK) void k_gm_sum(const double *__restrict__ slab, int nblk, int first, double *__restrict__ dst)
{
    __shared__ double red[GM_BLOCK / 64];
    const double *p = slab + (int64_t) (first + blockIdx.x) * nblk;
    double a = 0.0;
    for (int b = threadIdx.x; b < nblk; b += GM_BLOCK) a += p[b];
    const double t = gm_block_sum(a, red);
    if (threadIdx.x == 0) dst[blockIdx.x] = t;
}

// w -= sum_k v_k h_k, k < NV, the coefficients read from device memory (vs doubles each: what k_gm_sum left of the dots); slab[norm_slot nblk + b] =
// partial of ||w||^2 of the NEW w: the norm needs no pass of its own after the last chunk
template <bool Z, int NV>
__global__ __launch_bounds__(GM_BLOCK) void k_gm_axpys(int64_t nu, const double2 *__restrict__ V, int64_t vstride, double2 *__restrict__ w, const double *__restrict__ coef,
                                                       double *__restrict__ slab, int norm_slot)
{
    __shared__ double red[GM_BLOCK / 64];
    double2 h[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) h[k] = Z ? make_double2(coef[2 * k], coef[2 * k + 1]) : make_double2(coef[k], 0.0);
    double nrm = 0.0;
    for (int64_t i = (int64_t) blockIdx.x * GM_BLOCK + threadIdx.x; i < nu; i += (int64_t) gridDim.x * GM_BLOCK) {
        double2 wv = w[i];
        double2 vv[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) vv[k] = V[(int64_t) k * vstride + i];
#pragma unroll
        for (int k = 0; k < NV; ++k) gm_axpy<Z>(wv, vv[k], h[k]);
        w[i] = wv;
        nrm = fma(wv.x, wv.x, nrm); nrm = fma(wv.y, wv.y, nrm);
    }
    const double t = gm_block_sum(nrm, red);
    if (threadIdx.x == 0) slab[(int64_t) norm_slot * gridDim.x + blockIdx.x] = t;
}

// dst = src / h, h real: v_0 = r / beta, v_{j+1} = w / h_{j+1,j}
__global__ __launch_bounds__(GM_BLOCK) void k_gm_scale(int64_t nu, double2 *__restrict__ dst, const double2 *__restrict__ src, double h)
{
    for (int64_t i = (int64_t) blockIdx.x * GM_BLOCK + threadIdx.x; i < nu; i += (int64_t) gridDim.x * GM_BLOCK) {
        const double2 a = src[i];
        dst[i] = make_double2(a.x / h, a.y / h);
    }
}

// u = (add ? u : 0) + sum_k v_k y_k, k < NV; the coefficients travel in the kernel arguments (the host back-substituted them)
struct GmCoef { double2 y[GM_CHUNK]; };
template <bool Z, int NV>
__global__ __launch_bounds__(GM_BLOCK) void k_gm_combine(int64_t nu, const double2 *__restrict__ V, int64_t vstride, double2 *__restrict__ u, GmCoef c, int add)
{
    for (int64_t i = (int64_t) blockIdx.x * GM_BLOCK + threadIdx.x; i < nu; i += (int64_t) gridDim.x * GM_BLOCK) {
        double2 uv = add ? u[i] : make_double2(0.0, 0.0);
        double2 vv[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) vv[k] = V[(int64_t) k * vstride + i];
#pragma unroll
        for (int k = 0; k < NV; ++k) gm_madd<Z>(uv, vv[k], c.y[k]);
        u[i] = uv;
    }
}

namespace sluamd { namespace geng {

static inline unsigned gm_blocks(int64_t nu) { return (unsigned) std::min<int64_t>(GM_GRID, std::max<int64_t>(1, (nu + GM_BLOCK - 1) / GM_BLOCK)); }

#define GM_NV_SWITCH(nv, CALL) \
    switch (nv) { case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; \
                  case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break; }

// In the wrappers below vectors are double arrays and `vstride`, the distance between two basis vectors, counts DOUBLES (even: the vectors are padded); the
// kernels take it in 16-byte units.
// nv in [0, GM_CHUNK]: the dots of w with V[0 .. nv) into the slots slot0 .., ||w||^2 into norm_slot
static void dots(hipStream_t s, bool z, int64_t nu, const double *V, int64_t vstride, int nv, const double *w, double *slab, int slot0, int norm_slot)
{
    vstride /= 2;
    const dim3 g(gm_blocks(nu)), b(GM_BLOCK);
    auto Vp = reinterpret_cast<const double2 *>(V); auto wp = reinterpret_cast<const double2 *>(w);
    if (nv <= 0) {
        if (z) hipLaunchKernelGGL((k_gm_dots<true, 0>), g, b, 0, s, nu, Vp, vstride, wp, slab, slot0, norm_slot);
        else hipLaunchKernelGGL((k_gm_dots<false, 0>), g, b, 0, s, nu, Vp, vstride, wp, slab, slot0, norm_slot);
        return;
    }
#define GM_CALL(N) do { if (z) hipLaunchKernelGGL((k_gm_dots<true, N>), g, b, 0, s, nu, Vp, vstride, wp, slab, slot0, norm_slot); \
                        else hipLaunchKernelGGL((k_gm_dots<false, N>), g, b, 0, s, nu, Vp, vstride, wp, slab, slot0, norm_slot); } while (0)
    GM_NV_SWITCH(nv, GM_CALL)
#undef GM_CALL
}

// dst[0 .. count) = the sums of the slots first .. first + count - 1 of a slab written by launches over nu units
static void sum(hipStream_t s, int64_t nu, const double *slab, int first, int count, double *dst)
{
    if (count > 0) hipLaunchKernelGGL(k_gm_sum, dim3((unsigned) count), dim3(GM_BLOCK), 0, s, slab, (int) gm_blocks(nu), first, dst);
}

// nv in [1, GM_CHUNK]
static void axpys(hipStream_t s, bool z, int64_t nu, const double *V, int64_t vstride, int nv, double *w, const double *coef, double *slab, int norm_slot)
{
    vstride /= 2;
    const dim3 g(gm_blocks(nu)), b(GM_BLOCK);
    auto Vp = reinterpret_cast<const double2 *>(V); auto wp = reinterpret_cast<double2 *>(w);
#define GM_CALL(N) do { if (z) hipLaunchKernelGGL((k_gm_axpys<true, N>), g, b, 0, s, nu, Vp, vstride, wp, coef, slab, norm_slot); \
                        else hipLaunchKernelGGL((k_gm_axpys<false, N>), g, b, 0, s, nu, Vp, vstride, wp, coef, slab, norm_slot); } while (0)
    GM_NV_SWITCH(nv, GM_CALL)
#undef GM_CALL
}

static void scale(hipStream_t s, int64_t nu, double *dst, const double *src, double h)
{
    hipLaunchKernelGGL(k_gm_scale, dim3(gm_blocks(nu)), dim3(GM_BLOCK), 0, s, nu, reinterpret_cast<double2 *>(dst), reinterpret_cast<const double2 *>(src), h);
}

// nv in [1, GM_CHUNK]; y: nv coefficients (re, im)
static void combine(hipStream_t s, bool z, int64_t nu, const double *V, int64_t vstride, int nv, double *u, const double *y, bool add)
{
    vstride /= 2;
    const dim3 g(gm_blocks(nu)), b(GM_BLOCK);
    auto Vp = reinterpret_cast<const double2 *>(V); auto up = reinterpret_cast<double2 *>(u);
    GmCoef c;
    for (int k = 0; k < GM_CHUNK; ++k) c.y[k] = k < nv ? make_double2(y[2 * k], y[2 * k + 1]) : make_double2(0.0, 0.0);
    const int a = add ? 1 : 0;
#define GM_CALL(N) do { if (z) hipLaunchKernelGGL((k_gm_combine<true, N>), g, b, 0, s, nu, Vp, vstride, up, c, a); \
                        else hipLaunchKernelGGL((k_gm_combine<false, N>), g, b, 0, s, nu, Vp, vstride, up, c, a); } while (0)
    GM_NV_SWITCH(nv, GM_CALL)
#undef GM_CALL
}

#undef GM_NV_SWITCH

} }  // namespace sluamd::geng
