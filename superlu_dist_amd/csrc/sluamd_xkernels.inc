// sluamd_xkernels.inc -- the kernels of the extra-precise refinement (IterRefine = SLU_EXTRA: "accumulate residual in extra precision"), compiled with their
// only caller, sluamd_xrefine.cpp, which includes this file: no part of sluamd_kernels.hip, nothing behind eng::, no restatement in the CPU test build.
// gfx950, wave64.
// k_xrfs_residual is k_rfs_residual (sluamd_rkernels.inc, included below) with the row's sum carried as a head and a compensation.  Per part of the
// residual (one for double; real and imaginary for complex16, each with its own pair) and per entry in the row's stored order:
//     p = a * x (rounded)      pe = fma(a, x, -p): the product's error, exact      (s, se) = TwoSum(s, -p): the sum's error, exact      c += se - pe
// from s = b_i, c = 0, and r_i = s + c at the end: the error of r_i is one rounding of the exact residual plus the roundings of c alone, which are of
// second order -- twice the working precision, in fp64 registers.  The weight t, the quotient and the maximum are the plain form's, text and order
// (rfs_abs1 products summed in fp64, |b_i| last: rfs_ratio, rfs_block_max), so t is bitwise the plain pass's.
// The error-free transforms must not be contracted: the compiler's default for HIP fuses s + (-(a * x)) into one multiply-add, which rounds once, leaves a
// "sum error" of another value and an unrounded p -- the pair is then no longer exact.  They stand in functions under `#pragma clang fp contract(off)`.
// Shape: one thread per row, 256 per workgroup, as the plain pass.  A 7-point row is a chain of seven dependent TwoSums (six additions each) behind the same
// gathers as the plain pass; no floating-point atomics anywhere.
#include "sluamd_rkernels.inc"

// s + e = a + b exactly (Knuth: six operations, no branch)
__device__ __forceinline__ void xr_two_sum(double a, double b, double &s, double &e)
{
#pragma clang fp contract(off)
    s = a + b;
    const double bb = s - a;
    const double aa = s - bb;
    e = (a - aa) + (b - bb);
}

// (s, c) -= a * x: head and compensation of one part
__device__ __forceinline__ void xr_sub_prod(double &s, double &c, double a, double xv)
{
#pragma clang fp contract(off)
    const double p = a * xv;
    const double pe = __builtin_fma(a, xv, -p);
    double se;
    xr_two_sum(s, -p, s, se);
    c = c + (se - pe);
}

struct XrAcc1 { double s, c; };
struct XrAcc2 { XrAcc1 re, im; };
__device__ __forceinline__ XrAcc1 xr_start(double b) { return {b, 0.0}; }
__device__ __forceinline__ XrAcc2 xr_start(double2 b) { return {{b.x, 0.0}, {b.y, 0.0}}; }
__device__ __forceinline__ void xr_entry(XrAcc1 &r, double a, double xv) { xr_sub_prod(r.s, r.c, a, xv); }
// op(a) x: the real part takes + a.x x.x then - a.y x.y, the imaginary part + a.x x.y then + a.y x.x
__device__ __forceinline__ void xr_entry(XrAcc2 &r, double2 a, double2 xv)
{
    xr_sub_prod(r.re.s, r.re.c, a.x, xv.x);
    xr_sub_prod(r.re.s, r.re.c, -a.y, xv.y);
    xr_sub_prod(r.im.s, r.im.c, a.x, xv.y);
    xr_sub_prod(r.im.s, r.im.c, a.y, xv.x);
}
__device__ __forceinline__ double xr_round(const XrAcc1 &r) { return r.s + r.c; }
__device__ __forceinline__ double2 xr_round(const XrAcc2 &r) { return make_double2(r.re.s + r.re.c, r.im.s + r.im.c); }

// one thread per row i of op(A); TRANS: (ptr, idx, pos) = the transposed index, else the CSR (pos unused).  r_out[pc[i]] = r_i, or r_out[i] when pc is null
template <class V, bool TRANS, bool CONJ>
__global__ __launch_bounds__(256) void k_xrfs_residual(int n, const int *__restrict__ ptr, const int *__restrict__ idx, const int *__restrict__ pos,
                                                       const V *__restrict__ av, const V *__restrict__ x, const V *__restrict__ b,
                                                       const int *__restrict__ pc, V *__restrict__ r_out, unsigned long long *__restrict__ s_out,
                                                       double safe1, double safe2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    double q = 0.0;
    if (i < n) {
        const V bval = b[i];
        auto acc = xr_start(bval);
        double t = 0.0;
        const int e1 = ptr[i + 1];
        for (int e = ptr[i]; e < e1; ++e) {
            const V a = rfs_op<CONJ>(av[TRANS ? pos[e] : e]), xv = x[idx[e]];
            xr_entry(acc, a, xv);
            t += rfs_abs1(a) * rfs_abs1(xv);
        }
        const V r = xr_round(acc);
        q = rfs_ratio(r, t, bval, safe1, safe2);
        r_out[pc ? pc[i] : i] = r;
    }
    rfs_block_max(q, s_out);
}

// the plain pass of sluamd_[dz]Residual: the row text of k_rfs_residual (rfs_row), so the same bits, with the output index of the kernel above
template <class V, bool TRANS, bool CONJ>
__global__ __launch_bounds__(256) void k_xrfs_residual_plain(int n, const int *__restrict__ ptr, const int *__restrict__ idx, const int *__restrict__ pos,
                                                             const V *__restrict__ av, const V *__restrict__ x, const V *__restrict__ b,
                                                             const int *__restrict__ pc, V *__restrict__ r_out, unsigned long long *__restrict__ s_out,
                                                             double safe1, double safe2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    double q = 0.0;
    if (i < n) {
        V r;
        q = rfs_row<V, CONJ, TRANS>(ptr[i], ptr[i + 1], idx, pos, av, x, b[i], safe1, safe2, r);
        r_out[pc ? pc[i] : i] = r;
    }
    rfs_block_max(q, s_out);
}

// s_out[0] = max(s_out[0], max_i abs1(dx_i)), s_out[1] = the same of x: one value of each per thread (the maxima do not care that dx is permuted), the two
// maxima by rfs_block_max into integer atomicMax on the bit patterns.  A NaN counts as +inf: fmax would drop it, and the loop must see a correction that is
// not finite
template <class V>
__global__ __launch_bounds__(256) void k_xrfs_norms(int n, const V *__restrict__ dx_perm, const V *__restrict__ x, unsigned long long *__restrict__ s_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    double d = 0.0, v = 0.0;
    if (i < n) {
        d = rfs_abs1(dx_perm[i]);
        v = rfs_abs1(x[i]);
        if (d != d) d = __builtin_inf();
        if (v != v) v = __builtin_inf();
    }
    rfs_block_max(d, s_out);
    __syncthreads();                                                           // the reader of the first maximum is done with the LDS words of rfs_block_max
    rfs_block_max(v, s_out + 1);
}

namespace sluamd { namespace xeng {

// z: interleaved doublecomplex; A: rfs_mat() of the handle (A.pos: the transposed index); pc: the output permutation or null; extra: the doubled accumulation
static void residual(hipStream_t s, bool z, bool conj, bool extra, const RfsMat &A, const double *x, const double *b, const int *pc, double *r_out,
                     unsigned long long *s_out, double safe1, double safe2)
{
    if (A.n <= 0) return;
    const int n = (int) A.n;
    const dim3 g((unsigned) ((n + 255) / 256)), blk(256);
#define XRFS_CALL(K, V, T, CJ) hipLaunchKernelGGL((K<V, T, CJ>), g, blk, 0, s, n, A.ptr, A.idx, A.pos, reinterpret_cast<const V *>(A.av), \
                                                  reinterpret_cast<const V *>(x), reinterpret_cast<const V *>(b), pc, reinterpret_cast<V *>(r_out), s_out, safe1, safe2)
#define XRFS_FORMS(K) do { if (!z) { if (t) XRFS_CALL(K, double, true, false); else XRFS_CALL(K, double, false, false); } \
                           else if (!t) XRFS_CALL(K, double2, false, false); \
                           else if (conj) XRFS_CALL(K, double2, true, true); \
                           else XRFS_CALL(K, double2, true, false); } while (0)
    const bool t = A.pos != nullptr;
    if (extra) XRFS_FORMS(k_xrfs_residual); else XRFS_FORMS(k_xrfs_residual_plain);
#undef XRFS_FORMS
#undef XRFS_CALL
}

static void norms(hipStream_t s, bool z, int n, const double *dx_perm, const double *x, unsigned long long *s_out)
{
    if (n <= 0) return;
    const dim3 g((unsigned) ((n + 255) / 256)), blk(256);
    if (z) hipLaunchKernelGGL((k_xrfs_norms<double2>), g, blk, 0, s, n, reinterpret_cast<const double2 *>(dx_perm), reinterpret_cast<const double2 *>(x), s_out);
    else hipLaunchKernelGGL((k_xrfs_norms<double>), g, blk, 0, s, n, dx_perm, x, s_out);
}

} }  // namespace sluamd::xeng
