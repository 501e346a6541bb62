// sluamd_pkernels.inc -- the data-parallel part of RowPerm = LargeDiag_MC64 (sluamd_[dz]LargeDiag, sluamd_rowperm.cpp): logarithmic costs, the initial duals
// and the proposal rounds of the maximum-product matching (Duff & Koster, "On algorithms for permuting large entries to the diagonal of a sparse matrix",
// SIAM J. Matrix Anal. Appl. 22 (2001): the initialisation and the cheap-assignment heuristic; the shortest augmenting paths that finish the matching run on
// the host, sluamd_match.cpp).  Included by sluamd_kernels.hip after sluamd_ekernels.inc (EqVal, eq_mod, eq_u64); the launchers (eng::rp_*) are referenced
// only by sluamd_rowperm.cpp and sluamd_equil.cpp (the CPU test build of the host sources has no restatement of them).
//
// Layout as the equilibration kernels: CSR by rows, LPR = 1, 8 or 64 lanes share a row, 256 / LPR rows per workgroup, no grid-stride loop.
// Everything a kernel writes through an atomic is an integer minimum / maximum / sum, and a kernel only READS what an earlier launch wrote: the outcome is
// independent of the order in which lanes, waves and workgroups run -- bitwise equal results from call to call.
//   cost(i, j) = lg(cmax_j) - lg|a_ij| >= 0,  lg(x) = e + log2(m) with x = m 2^e, 1/2 <= m < 1 (frexp); m == 1/2 gives the integer e - 1 exactly
//   u_i = min_j cost(i, j);  v_j = min_i (cost(i, j) - u_i)         stored zeros are no edges: cost = +inf
//   an entry is TIGHT when (cost - u_i) == v_j, evaluated in exactly this form everywhere (host included)

constexpr int RP_NONE = 0x7fffffff;

__device__ __forceinline__ double rp_lg(double x)
{
    int e;
    const double m = frexp(x, &e);
    return m == 0.5 ? (double) (e - 1) : (double) e + log2(m);
}

// cmax_j = max_i |a_ij| as the integer maximum of the bit patterns (cbits zero-filled)
template <int LPR, bool Z>
__global__ __launch_bounds__(256) void k_rp_colmax(int n, const int *__restrict__ rp, const int *__restrict__ ci, const typename EqVal<Z>::T *__restrict__ av,
                                                   eq_u64 *__restrict__ cbits)
{
    const int64_t i = (int64_t) blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int lane = threadIdx.x % LPR;
    if (i >= n) return;
    for (int e = rp[i] + lane, e1 = rp[i + 1]; e < e1; e += LPR) {
        const double t = eq_mod(av[e]);
        if (t > 0.0) atomicMax(cbits + ci[e], (eq_u64) __double_as_longlong(t));
    }
}

// cost[e] for every stored entry and u_i = the row's smallest cost (+inf for a row without an edge)
template <int LPR, bool Z>
__global__ __launch_bounds__(256) void k_rp_cost_u(int n, const int *__restrict__ rp, const int *__restrict__ ci, const typename EqVal<Z>::T *__restrict__ av,
                                                   const double *__restrict__ cmax, double *__restrict__ cost, double *__restrict__ u)
{
    const int64_t i = (int64_t) blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int lane = threadIdx.x % LPR;
    double m = HUGE_VAL;
    if (i < n)
        for (int e = rp[i] + lane, e1 = rp[i + 1]; e < e1; e += LPR) {
            const double t = eq_mod(av[e]);
            const double c = t > 0.0 ? fmax(rp_lg(cmax[ci[e]]) - rp_lg(t), 0.0) : HUGE_VAL;
            cost[e] = c;
            m = fmin(m, c);
        }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) m = fmin(m, __shfl_xor(m, o));
    if (i < n && lane == 0) u[i] = m;
}

// v_j = min_i (cost - u_i): integer minimum of the bit patterns of non-negative doubles (vbits filled with the bits of +inf)
template <int LPR>
__global__ __launch_bounds__(256) void k_rp_v(int n, const int *__restrict__ rp, const int *__restrict__ ci, const double *__restrict__ cost,
                                              const double *__restrict__ u, eq_u64 *__restrict__ vbits)
{
    const int64_t i = (int64_t) blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int lane = threadIdx.x % LPR;
    if (i >= n) return;
    const double ui = u[i];
    for (int e = rp[i] + lane, e1 = rp[i + 1]; e < e1; e += LPR) {
        const double c = cost[e];
        if (c < HUGE_VAL) atomicMin(vbits + ci[e], (eq_u64) __double_as_longlong(c - ui));
    }
}

// one proposal round, first half: every unmatched row proposes to its free tight column of lowest index; prop[j] = the lowest proposing row (RP_NONE: none).
// rowmatch / colmatch are only read here (the second half writes them), so a round sees the matching of the round before, whatever the schedule
template <int LPR>
__global__ __launch_bounds__(256) void k_rp_propose(int n, const int *__restrict__ rp, const int *__restrict__ ci, const double *__restrict__ cost,
                                                    const double *__restrict__ u, const double *__restrict__ v, const int *__restrict__ rowmatch,
                                                    const int *__restrict__ colmatch, int *__restrict__ prop)
{
    const int64_t i = (int64_t) blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int lane = threadIdx.x % LPR;
    int best = RP_NONE;
    if (i < n && rowmatch[i] < 0) {
        const double ui = u[i];
        for (int e = rp[i] + lane, e1 = rp[i + 1]; e < e1; e += LPR) {
            const double c = cost[e];
            const int j = ci[e];
            if (c < HUGE_VAL && j < best && colmatch[j] < 0 && (c - ui) == v[j]) best = j;
        }
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    if (lane == 0 && best != RP_NONE) atomicMin(prop + best, (int) i);
}

// second half: column j accepts prop[j]; count += the matches of the round.  A row proposes to one column, so no two columns write the same rowmatch entry
__global__ __launch_bounds__(256) void k_rp_accept(int n, int *__restrict__ prop, int *__restrict__ rowmatch, int *__restrict__ colmatch, int *__restrict__ count)
{
    __shared__ int sh[4];
    const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
    int got = 0;
    if (j < n) {
        const int i = prop[j];
        if (i != RP_NONE) { colmatch[j] = i; rowmatch[i] = (int) j; prop[j] = RP_NONE; got = 1; }
    }
    const eq_u64 b = __ballot(got);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) { const int t = sh[0] + sh[1] + sh[2] + sh[3]; if (t) atomicAdd(count, t); }
}

__global__ __launch_bounds__(256) void k_rp_fill(int64_t cnt, int *__restrict__ p, int value)
{
    const int64_t q = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (q < cnt) p[q] = value;
}

__global__ __launch_bounds__(256) void k_rp_fill64(int64_t cnt, eq_u64 *__restrict__ p, eq_u64 value)
{
    const int64_t q = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (q < cnt) p[q] = value;
}

// sluamd_SetRowPerm: pcpr[i] = perm_c[perm_r[i]] and (r != null) rs[i] = r[perm_r[i]] -- B and X in the ordering of A for a handle made from Pr A
__global__ __launch_bounds__(256) void k_rp_compose(int n, const int *__restrict__ pr, const int *__restrict__ pc, const double *__restrict__ r,
                                                    int *__restrict__ pcpr, double *__restrict__ rs)
{
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = pr[i];
    pcpr[i] = pc[p];
    if (r) rs[i] = r[p];
}

namespace eng {

#define RP_ROWS_LAUNCH(KERNEL, ...)                                                                                                             \
    do {                                                                                                                                        \
        const int lpr = eq_lpr(n, nnz);                                                                                                         \
        const unsigned nb = (unsigned) (((int64_t) n + 256 / lpr - 1) / (256 / lpr));                                                           \
        if (lpr == 1) hipLaunchKernelGGL((KERNEL<1>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                                 \
        else if (lpr == 8) hipLaunchKernelGGL((KERNEL<8>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                            \
        else hipLaunchKernelGGL((KERNEL<64>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                                         \
    } while (0)
#define RP_ROWS_LAUNCH_V(KERNEL, ZV, ...)                                                                                                       \
    do {                                                                                                                                        \
        const int lpr = eq_lpr(n, nnz);                                                                                                         \
        const unsigned nb = (unsigned) (((int64_t) n + 256 / lpr - 1) / (256 / lpr));                                                           \
        if (lpr == 1) hipLaunchKernelGGL((KERNEL<1, ZV>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                             \
        else if (lpr == 8) hipLaunchKernelGGL((KERNEL<8, ZV>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                        \
        else hipLaunchKernelGGL((KERNEL<64, ZV>), dim3(nb), dim3(256), 0, s, __VA_ARGS__);                                                     \
    } while (0)

void rp_colmax(hipStream_t s, bool z, int n, int64_t nnz, const int *rp, const int *ci, const void *av, double *cmax)
{
    if (n <= 0) return;
    eq_u64 *cb = reinterpret_cast<eq_u64 *>(cmax);
    if (z) RP_ROWS_LAUNCH_V(k_rp_colmax, true, n, rp, ci, reinterpret_cast<const zc *>(av), cb);
    else RP_ROWS_LAUNCH_V(k_rp_colmax, false, n, rp, ci, reinterpret_cast<const double *>(av), cb);
}

void rp_cost_u(hipStream_t s, bool z, int n, int64_t nnz, const int *rp, const int *ci, const void *av, const double *cmax, double *cost, double *u)
{
    if (n <= 0) return;
    if (z) RP_ROWS_LAUNCH_V(k_rp_cost_u, true, n, rp, ci, reinterpret_cast<const zc *>(av), cmax, cost, u);
    else RP_ROWS_LAUNCH_V(k_rp_cost_u, false, n, rp, ci, reinterpret_cast<const double *>(av), cmax, cost, u);
}

void rp_v(hipStream_t s, int n, int64_t nnz, const int *rp, const int *ci, const double *cost, const double *u, double *v)
{
    if (n <= 0) return;
    RP_ROWS_LAUNCH(k_rp_v, n, rp, ci, cost, u, reinterpret_cast<eq_u64 *>(v));
}

void rp_propose(hipStream_t s, int n, int64_t nnz, const int *rp, const int *ci, const double *cost, const double *u, const double *v, const int *rowmatch,
                const int *colmatch, int *prop)
{
    if (n <= 0) return;
    RP_ROWS_LAUNCH(k_rp_propose, n, rp, ci, cost, u, v, rowmatch, colmatch, prop);
}
#undef RP_ROWS_LAUNCH
#undef RP_ROWS_LAUNCH_V

void rp_accept(hipStream_t s, int n, int *prop, int *rowmatch, int *colmatch, int *count)
{
    if (n > 0) hipLaunchKernelGGL(k_rp_accept, dim3((n + 255) / 256), dim3(256), 0, s, n, prop, rowmatch, colmatch, count);
}

void rp_fill(hipStream_t s, int64_t cnt, int *p, int value)
{
    if (cnt > 0) hipLaunchKernelGGL(k_rp_fill, dim3((unsigned) ((cnt + 255) / 256)), dim3(256), 0, s, cnt, p, value);
}

void rp_fill_inf(hipStream_t s, int64_t cnt, double *p)
{
    if (cnt > 0) hipLaunchKernelGGL(k_rp_fill64, dim3((unsigned) ((cnt + 255) / 256)), dim3(256), 0, s, cnt, reinterpret_cast<eq_u64 *>(p), 0x7ff0000000000000ull);
}

void rp_compose(hipStream_t s, int n, const int *pr, const int *pc, const double *r, int *pcpr, double *rs)
{
    if (n > 0) hipLaunchKernelGGL(k_rp_compose, dim3((n + 255) / 256), dim3(256), 0, s, n, pr, pc, r, pcpr, rs);
}

}  // namespace eng
