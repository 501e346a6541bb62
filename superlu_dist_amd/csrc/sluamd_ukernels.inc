// sluamd_ukernels.inc -- same-pattern value updates (sluamd_[dz]UpdateValues: options->Fact = SamePattern_SameRowPerm for handles created from the symbolic
// structure; with Equil the reference scales the new A by the R, C and DiagScale of the previous call, pdgssvx3d.c:672-697).  Included by sluamd_kernels.hip after
// sluamd_ekernels.inc (EqVal, eq_mul, eq_mod); the launchers (eng::update_*) are referenced only by sluamd_update.cpp (the CPU test build of the host sources
// has no restatement of them).
//
// k_update_values is the distribution kernel: one thread per owned entry e in arena order, grid-stride, consecutive lanes on consecutive e -- the loads of
// ent / ij / pos and the store of aval are coalesced 4- / 8- / 16-byte streams; nz[ent[e]] is a gather (ent ascends inside a supernode's column run, so most
// lanes of a wave share cache lines), val[pos[e]] the same scatter as k_scatter_values: one writer per arena position, no atomics.

// ij[e] = (row, column) in the caller's CSR of owned entry e: the row by bisection of rowptr (the last i with rp[i] <= ent[e]; empty rows are skipped by it)
__global__ __launch_bounds__(256) void k_update_rowcol(int64_t cnt, int n, const int *__restrict__ rp, const int *__restrict__ ci, const int *__restrict__ ent,
                                                       int2 *__restrict__ ij)
{
    for (int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x; e < cnt; e += (int64_t) gridDim.x * 256) {
        const int q = ent[e];
        int lo = 0, hi = n;              // invariant: rp[lo] <= q < rp[hi]
        while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if (rp[mid] <= q) lo = mid; else hi = mid; }
        ij[e] = make_int2(lo, ci[q]);
    }
}

// aval[e] = val[pos[e]] = (nz[ent[e]] r[i]) c[j] -- in exactly that order, as k_eq_scale_norm; r / c null: that side is not scaled (ij is read only when one is given)
template <typename V>
__global__ __launch_bounds__(256) void k_update_values(int64_t cnt, const int *__restrict__ ent, const int2 *__restrict__ ij, const V *__restrict__ nz,
                                                       const double *__restrict__ r, const double *__restrict__ c, V *__restrict__ aval,
                                                       const int64_t *__restrict__ pos, V *__restrict__ val)
{
    for (int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x; e < cnt; e += (int64_t) gridDim.x * 256) {
        V v = nz[ent[e]];
        if (r || c) {
            const int2 q = ij[e];
            if (r) v = eq_mul(v, r[q.x]);
            if (c) v = eq_mul(v, c[q.y]);
        }
        aval[e] = v;
        val[pos[e]] = v;
    }
}

// The attached CSR copy takes the new values in the caller's order: av[e] = (nz[e] r[i]) c[j] by rows, LPR lanes per row as the equilibration kernels; colsum
// (zero-filled; null: no norm asked for) += the moduli by column with fp64 atomic adds -- the summation caveat of k_eq_scale_norm
template <int LPR, bool Z>
__global__ __launch_bounds__(256) void k_update_attached(int n, const int *__restrict__ rp, const int *__restrict__ ci, const typename EqVal<Z>::T *__restrict__ nz,
                                                         const double *__restrict__ r, const double *__restrict__ c, typename EqVal<Z>::T *__restrict__ av,
                                                         double *__restrict__ colsum)
{
    const int64_t i = (int64_t) blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int lane = threadIdx.x % LPR;
    if (i >= n) return;
    const double ri = r ? r[i] : 1.0;
    for (int e = rp[i] + lane, e1 = rp[i + 1]; e < e1; e += LPR) {
        const int j = ci[e];
        typename EqVal<Z>::T a = nz[e];
        if (r) a = eq_mul(a, ri);
        if (c) a = eq_mul(a, c[j]);
        av[e] = a;
        if (colsum) {
            const double t = eq_mod(a);
            if (t != 0.0) unsafeAtomicAdd(colsum + j, t);
        }
    }
}

namespace eng {

// grid-stride launches: enough workgroups to fill the device several times over, never more than the work has
static inline unsigned update_blocks(int64_t cnt) { return (unsigned) std::min<int64_t>((cnt + 255) / 256, 8192); }

void update_rowcol(hipStream_t s, int64_t cnt, int n, const int *rp, const int *ci, const int *ent, int2 *ij)
{
    if (cnt > 0 && n > 0) hipLaunchKernelGGL(k_update_rowcol, dim3(update_blocks(cnt)), dim3(256), 0, s, cnt, n, rp, ci, ent, ij);
}

void update_values(hipStream_t s, bool z, int64_t cnt, const int *ent, const int2 *ij, const void *nz, const double *r, const double *c, void *aval,
                   const int64_t *pos, void *val)
{
    if (cnt <= 0) return;
    const dim3 g(update_blocks(cnt));
    if (z) hipLaunchKernelGGL(k_update_values<zc>, g, dim3(256), 0, s, cnt, ent, ij, reinterpret_cast<const zc *>(nz), r, c, reinterpret_cast<zc *>(aval), pos, reinterpret_cast<zc *>(val));
    else hipLaunchKernelGGL(k_update_values<double>, g, dim3(256), 0, s, cnt, ent, ij, reinterpret_cast<const double *>(nz), r, c, reinterpret_cast<double *>(aval), pos, reinterpret_cast<double *>(val));
}

template <bool Z>
static void update_attached_t(hipStream_t s, int n, int64_t nnz, const int *rp, const int *ci, const typename EqVal<Z>::T *nz, const double *r, const double *c,
                              typename EqVal<Z>::T *av, double *colsum)
{
    const int lpr = eq_lpr(n, nnz);
    const dim3 g((unsigned) (((int64_t) n + 256 / lpr - 1) / (256 / lpr)));
    if (lpr == 1) hipLaunchKernelGGL((k_update_attached<1, Z>), g, dim3(256), 0, s, n, rp, ci, nz, r, c, av, colsum);
    else if (lpr == 8) hipLaunchKernelGGL((k_update_attached<8, Z>), g, dim3(256), 0, s, n, rp, ci, nz, r, c, av, colsum);
    else hipLaunchKernelGGL((k_update_attached<64, Z>), g, dim3(256), 0, s, n, rp, ci, nz, r, c, av, colsum);
}

void update_attached(hipStream_t s, bool z, int n, int64_t nnz, const int *rp, const int *ci, const void *nz, const double *r, const double *c, void *av,
                     double *colsum)
{
    if (n <= 0) return;
    if (z) update_attached_t<true>(s, n, nnz, rp, ci, reinterpret_cast<const zc *>(nz), r, c, reinterpret_cast<zc *>(av), colsum);
    else update_attached_t<false>(s, n, nnz, rp, ci, reinterpret_cast<const double *>(nz), r, c, reinterpret_cast<double *>(av), colsum);
}

}  // namespace eng
