// sluamd_mkernels.inc -- the kernels of the blocked refinement (sluamd_brefine.cpp, which includes this file: they are compiled with their only caller and are
// no part of sluamd_kernels.hip; the CPU test build of the host sources has no restatement of them).  gfx950, wave64.
// A panel of up to RFS_PANEL columns of X goes through one pass over the attached matrix: per column the operations and their order are those of the column
// form -- rfs_term per entry, rfs_quot at the end of the row, rfs_block_max into the column's own word (sluamd_rkernels.inc, included below) -- so a column of
// the block form is bitwise that column alone.
// The columns of a pass are the ACTIVE ones of the panel: the list (a count and at most 16 column numbers, ascending) travels by value in the kernel
// arguments, 68 bytes of the kernarg segment, read with scalar loads: no table is uploaded per pass.  Slot c = the c-th listed column.
// Registers: the columns are handled in groups of RFS_GROUP = 4.  A group keeps ax, t and the gathered x of its columns: 4 x (2 + 1 + 2) doubles for
// complex16 = 40 VGPRs of accumulators alone; compiled for gfx950 the kernels take 50 VGPRs (double) and 84 - 90 (complex16), no scratch, no spills -- under
// the 128 a workgroup of 256 may use per thread.  Sixteen complex accumulators (160 VGPRs with their x) would spill.  An entry's value and index are read once
// per group (the second to fourth group of a row find them in L2: the row was just read), the four x loads of an entry hit four columns at the same row
// index, each coalesced across the wave's rows as well as the column form's one is.
#include "sluamd_rkernels.inc"

#define RFS_PANEL 16      // columns per panel: the block one MFMA sweep serves
#define RFS_GROUP 4       // columns per register group

struct RfsCols { int count; int col[RFS_PANEL]; };

// the columns L.col[s0 .. s0 + G) of row i (live: i < n; every thread of the workgroup comes here, for the reductions)
template <class V, bool TRANS, bool CONJ, int G>
__device__ __forceinline__ void rfs_group(bool live, int i, int n, const int *__restrict__ ptr, const int *__restrict__ idx, const int *__restrict__ pos,
                                          const V *__restrict__ av, const V *__restrict__ x, int64_t ldx, const V *__restrict__ b, int64_t ldb,
                                          const int *__restrict__ pc, V *__restrict__ r_perm, unsigned long long *__restrict__ s_out, double safe1, double safe2,
                                          const RfsCols &L, int s0)
{
    double q[G];
#pragma unroll
    for (int k = 0; k < G; ++k) q[k] = 0.0;
    if (live) {
        const V *xc[G];
        V ax[G];
        double t[G];
#pragma unroll
        for (int k = 0; k < G; ++k) { xc[k] = x + (int64_t) L.col[s0 + k] * ldx; ax[k] = V(); t[k] = 0.0; }
        const int e1 = ptr[i + 1];
        for (int e = ptr[i]; e < e1; ++e) {
            const V a = rfs_op<CONJ>(av[TRANS ? pos[e] : e]);
            const int j = idx[e];
            V xv[G];
#pragma unroll
            for (int k = 0; k < G; ++k) xv[k] = xc[k][j];                      // all loads in flight before the first use
#pragma unroll
            for (int k = 0; k < G; ++k) rfs_term(ax[k], t[k], a, xv[k]);
        }
        const int p = pc[i];
#pragma unroll
        for (int k = 0; k < G; ++k) {
            V r;
            q[k] = rfs_quot(ax[k], t[k], b[i + (int64_t) L.col[s0 + k] * ldb], safe1, safe2, r);
            r_perm[(int64_t) (s0 + k) * n + p] = r;
        }
    }
#pragma unroll
    for (int k = 0; k < G; ++k) {
        if (s0 + k > 0) __syncthreads();                                       // the previous column's reader is done with the LDS words of rfs_block_max
        rfs_block_max(q[k], s_out + s0 + k);
    }
}

// one thread per row i of op(A); TRANS: (ptr, idx, pos) = the transposed index, else the CSR (pos unused).  x, b: the panel (column c at c * ld), r_perm:
// slot c at c * n, s_out: one word per slot
template <class V, bool TRANS, bool CONJ>
__global__ __launch_bounds__(256) void k_rfs_residual_block(int n, const int *__restrict__ ptr, const int *__restrict__ idx, const int *__restrict__ pos,
                                                            const V *__restrict__ av, const V *__restrict__ x, int64_t ldx, const V *__restrict__ b, int64_t ldb,
                                                            const int *__restrict__ pc, V *__restrict__ r_perm, unsigned long long *__restrict__ s_out,
                                                            double safe1, double safe2, const RfsCols L)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    int s0 = 0;
    for (; s0 + RFS_GROUP <= L.count; s0 += RFS_GROUP)
        rfs_group<V, TRANS, CONJ, RFS_GROUP>(live, i, n, ptr, idx, pos, av, x, ldx, b, ldb, pc, r_perm, s_out, safe1, safe2, L, s0);
    switch (L.count - s0) {                                                    // (the same in every thread)
    case 1: rfs_group<V, TRANS, CONJ, 1>(live, i, n, ptr, idx, pos, av, x, ldx, b, ldb, pc, r_perm, s_out, safe1, safe2, L, s0); break;
    case 2: rfs_group<V, TRANS, CONJ, 2>(live, i, n, ptr, idx, pos, av, x, ldx, b, ldb, pc, r_perm, s_out, safe1, safe2, L, s0); break;
    case 3: rfs_group<V, TRANS, CONJ, 3>(live, i, n, ptr, idx, pos, av, x, ldx, b, ldb, pc, r_perm, s_out, safe1, safe2, L, s0); break;
    default: break;
    }
}

// x[i + L.col[c] ldx] += dx_perm[c n + perm_c[i]]: the listed columns only, blockIdx.y = slot c
template <class V>
__global__ __launch_bounds__(256) void k_rfs_update_block(int n, const int *__restrict__ pc, const V *__restrict__ dx_perm, V *__restrict__ x, int64_t ldx, const RfsCols L)
{
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (i < n && c < L.count) {
        V *xc = x + (int64_t) L.col[c] * ldx;
        V v = xc[i];
        rfs_add(v, dx_perm[(int64_t) c * n + pc[i]]);
        xc[i] = v;
    }
}

namespace sluamd { namespace meng {

// z: interleaved doublecomplex (the double pointers and leading dimensions count VALUES: two doubles each then); A: rfs_mat() of the handle; L.count in
// [1, RFS_PANEL], every listed column inside the panel
static void residual_block(hipStream_t s, bool z, bool conj, const RfsMat &A, const double *x, int64_t ldx, const double *b, int64_t ldb, double *r_perm,
                           unsigned long long *s_out, double safe1, double safe2, const RfsCols &L)
{
    const int n = (int) A.n;
    const dim3 g((unsigned) ((n + 255) / 256)), blk(256);
#define RFS_BCALL(V, T, CJ) hipLaunchKernelGGL((k_rfs_residual_block<V, T, CJ>), g, blk, 0, s, n, A.ptr, A.idx, A.pos, reinterpret_cast<const V *>(A.av), \
                                               reinterpret_cast<const V *>(x), ldx, reinterpret_cast<const V *>(b), ldb, A.pc, reinterpret_cast<V *>(r_perm), s_out, safe1, safe2, L)
    const bool t = A.pos != nullptr;
    if (!z) { if (t) RFS_BCALL(double, true, false); else RFS_BCALL(double, false, false); }
    else if (!t) RFS_BCALL(double2, false, false);
    else if (conj) RFS_BCALL(double2, true, true);
    else RFS_BCALL(double2, true, false);
#undef RFS_BCALL
}

static void update_block(hipStream_t s, bool z, int n, const int *pc, const double *dx_perm, double *x, int64_t ldx, const RfsCols &L)
{
    const dim3 g((unsigned) ((n + 255) / 256), (unsigned) L.count), blk(256);
    if (z) hipLaunchKernelGGL((k_rfs_update_block<double2>), g, blk, 0, s, n, pc, reinterpret_cast<const double2 *>(dx_perm), reinterpret_cast<double2 *>(x), ldx, L);
    else hipLaunchKernelGGL((k_rfs_update_block<double>), g, blk, 0, s, n, pc, dx_perm, x, ldx, L);
}

} }  // namespace sluamd::meng
