// sluamd_akernels.inc -- the kernels of the adjoint value gradient (sluamd_adjoint.cpp, which includes this file: they are compiled with their only caller and
// are no part of sluamd_kernels.hip; the CPU test build of the host sources has no restatement of them).  gfx950, wave64.
// For x = op(A)^-1 b and a scalar loss the gradient with respect to the stored values of A is a sampled outer product on A's pattern: per stored entry e of
// row i and column j
//     G[e] = - sum over r < nrhs of P[a, r] op(Q[b, r]),    (a, b) = (i, j), or (j, i) with SWAP;  op = the conjugate with CONJQ (complex16)
// (which of Lam and X is P and which is Q, per trans: sluamd_adjoint.cpp).  One thread per stored entry, 256 per workgroup: colind[e], the entry's row and
// G[e] are coalesced, the gathers of P and Q hit rows that neighbouring entries share (a row's entries read the same P[i, :], consecutive columns read
// consecutive Q[j, :]).  Exactly one thread writes each G[e] and no atomic is used: two calls on the same input return the same bits.  A duplicated (i, j)
// receives the full value in each of its entries, the derivative of a matrix whose duplicates sum.
// The entry's row comes from an entry -> row array built once per attached matrix by k_adjoint_rows.
// Registers: the right-hand sides are taken in groups of ADJ_GROUP = 4 as sluamd_mkernels.inc takes its columns -- the eight loads of a group are in flight
// before the first multiply-add -- with a remainder loop; the sum over r is ascending, one chain of fused multiply-adds per part (real; re and im).
// blockIdx.y = k: matrix k of a batch, P, Q and G at k times their strides; the pattern (row, colind) is that of ONE matrix and is read for every k.
#define ADJ_GROUP 4       // right-hand sides per register group
#define ADJ_PANEL 32      // right-hand sides per launch: a larger nrhs takes several launches, every one after the first accumulating into G

// acc += p op(q)
template <bool CONJQ> __device__ __forceinline__ void adj_fma(double &acc, double p, double q) { acc = fma(p, q, acc); }
template <bool CONJQ> __device__ __forceinline__ void adj_fma(double2 &acc, double2 p, double2 q)
{
    const double qi = CONJQ ? -q.y : q.y;
    acc.x = fma(p.x, q.x, acc.x); acc.x = fma(-p.y, qi, acc.x);
    acc.y = fma(p.y, q.x, acc.y); acc.y = fma(p.x, qi, acc.y);
}
__device__ __forceinline__ double adj_zero(double) { return 0.0; }
__device__ __forceinline__ double2 adj_zero(double2) { return make_double2(0.0, 0.0); }
// g - acc: 0 - 0 is +0, what a zero-filled G holds
__device__ __forceinline__ double adj_sub(double g, double acc) { return g - acc; }
__device__ __forceinline__ double2 adj_sub(double2 g, double2 acc) { return make_double2(g.x - acc.x, g.y - acc.y); }

// erow[e] = the row of CSR entry e: the last i with rp[i] <= e (empty rows share their successor's pointer and are passed over); one thread per entry
__global__ __launch_bounds__(256) void k_adjoint_rows(int n, int nnz, const int *__restrict__ rp, int *__restrict__ erow)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    int lo = 0, hi = n - 1;                       // rp[lo] <= e always; rp[n] = nnz > e
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (rp[mid] <= e) lo = mid; else hi = mid - 1;
    }
    erow[e] = lo;
}

// ld and strides in values; accum: G[e] -= the sum instead of G[e] = 0 - the sum (the later panels of a call with nrhs > ADJ_PANEL)
template <class V, bool SWAP, bool CONJQ>
__global__ __launch_bounds__(256) void k_adjoint_values(int nnz, const int *__restrict__ erow, const int *__restrict__ ci, const V *__restrict__ P, int64_t ldp,
                                                        int64_t strideP, const V *__restrict__ Q, int64_t ldq, int64_t strideQ, int nrhs, V *__restrict__ G,
                                                        int64_t strideG, int accum)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int64_t k = blockIdx.y;
    const int i = erow[e], j = ci[e];
    const V *p = P + k * strideP + (SWAP ? j : i);
    const V *q = Q + k * strideQ + (SWAP ? i : j);
    V acc = adj_zero(V());
    int r = 0;
    for (; r + ADJ_GROUP <= nrhs; r += ADJ_GROUP) {
        V pv[ADJ_GROUP], qv[ADJ_GROUP];
#pragma unroll
        for (int t = 0; t < ADJ_GROUP; ++t) { pv[t] = p[(int64_t) (r + t) * ldp]; qv[t] = q[(int64_t) (r + t) * ldq]; }      // all loads in flight before the first use
#pragma unroll
        for (int t = 0; t < ADJ_GROUP; ++t) adj_fma<CONJQ>(acc, pv[t], qv[t]);
    }
    for (; r < nrhs; ++r) adj_fma<CONJQ>(acc, p[(int64_t) r * ldp], q[(int64_t) r * ldq]);
    V *g = G + k * strideG + e;
    *g = adj_sub(accum ? *g : adj_zero(V()), acc);
}

namespace sluamd { namespace aeng {

static void rows(hipStream_t s, int n, int nnz, const int *rp, int *erow)
{
    if (nnz > 0) hipLaunchKernelGGL(k_adjoint_rows, dim3((unsigned) ((nnz + 255) / 256)), dim3(256), 0, s, n, nnz, rp, erow);
}

// z: interleaved doublecomplex (the double pointers, leading dimensions and strides count VALUES: two doubles each then); swap / conjq: the kernel's SWAP and
// CONJQ -- real handles use neither, complex16 ones always conjugate Q; count matrices (strides unused when count == 1), nrhs >= 1
static void values(hipStream_t s, bool z, bool swap, int nnz, const int *erow, const int *ci, const double *P, int64_t ldp, int64_t strideP, const double *Q, int64_t ldq,
                   int64_t strideQ, int nrhs, double *G, int64_t strideG, int count)
{
    if (nnz <= 0 || count <= 0) return;
    const int vs = z ? 2 : 1;
    for (int k0 = 0; k0 < count; k0 += 65535) {                                 // (gridDim.y)
        const dim3 g((unsigned) ((nnz + 255) / 256), (unsigned) std::min(count - k0, 65535)), blk(256);
        for (int r0 = 0; r0 < nrhs; r0 += ADJ_PANEL) {
            const int nr = std::min(nrhs - r0, ADJ_PANEL), accum = r0 > 0;
            const double *Pp = P + ((size_t) k0 * strideP + (size_t) r0 * ldp) * vs, *Qp = Q + ((size_t) k0 * strideQ + (size_t) r0 * ldq) * vs;
            double *Gp = G + (size_t) k0 * strideG * vs;
#define ADJ_CALL(V, SW, CJ) hipLaunchKernelGGL((k_adjoint_values<V, SW, CJ>), g, blk, 0, s, nnz, erow, ci, reinterpret_cast<const V *>(Pp), ldp, strideP, \
                                               reinterpret_cast<const V *>(Qp), ldq, strideQ, nr, reinterpret_cast<V *>(Gp), strideG, accum)
            if (!z) ADJ_CALL(double, false, false);
            else if (swap) ADJ_CALL(double2, true, true);
            else ADJ_CALL(double2, false, true);
#undef ADJ_CALL
        }
    }
}

} }  // namespace sluamd::aeng
