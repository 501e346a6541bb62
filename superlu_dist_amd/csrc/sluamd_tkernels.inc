// sluamd_tkernels.inc -- the sweeps of the TRANSPOSED and CONJUGATE-TRANSPOSED solves, (L U)^T y = b / (L U)^H y = b, on a 1 x 1 x 1 handle
// (sluamd_tsolve.cpp).  Included inside namespace sluamd by sluamd_kernels.hip, after the complex16 kernels (zc and its arithmetic).
//
// The factors stay as the factorisation left them; what changes is the axis of the reduction.  In the untransposed sweeps a unit's lanes own OUTPUT rows
// and every lane walks along a row of the panel / skyline (stride lda, coalesced across the lanes); here the output of a unit is indexed by the panel's
// COLUMNS, a column is contiguous, so the lanes run ALONG the column (8- or 16-byte coalesced loads) and the sum is taken ACROSS the lanes:
//   forward,  U^T, levels ascending:  y_k = Uinv_k^T x_k                       k_solve_diag_t<false>   (complex16: substitution on U_kk^T, kz_solve_diag_t<true>)
//                                     x[gc] -= sum_r U_k[r, c] y_k[r]          k_fwd_update_t          unit = (supernode, chunk of 64 non-empty columns): bwd_prefix
//   backward, L^T, levels descending: x_k -= sum_r L_k[r, c] x[lrow r]         k_bwd_update_t          unit = (supernode, strip of 64 (complex16: 256) panel rows): fwd_prefix / zfwd_prefix
//                                     x_k = Linv_k^T x_k                       k_solve_diag_t<true>    (complex16: unit substitution on L_kk^T, kz_solve_diag_t<false>)
// Everything is in place in ONE vector: a diagonal solve is one workgroup per supernode (x_k staged in LDS before the first store), and within a level the
// updates read rows of the level's own supernodes (or of later levels, backward) and write rows of other levels only.
// Atomics: the U^T units always (several block rows feed one column of x); the L^T units when the supernode has more than one strip.
//
// Cross-lane sums: a wave holds N partial sums per lane (N columns) and needs N totals.  wave_colsum folds the columns while it folds the lanes -- the step
// with lane distance 32 sends one half of the columns to the partner and keeps the other, distance 16 a quarter, ... -- N - 1 exchanges for the columns plus
// log2(64 / N) for the lanes left, instead of 6 N.  Afterwards column lane / (64 / N) of the batch is complete on its lanes.
// RK: right-hand sides per pass over a unit's factor entries (1, or 4 when nrhs >= 2), as in the untransposed scalar units.

typedef double dv2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double t_ntload(const double *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ zc t_ntload(const zc *p) { const dv2 v = __builtin_nontemporal_load(reinterpret_cast<const dv2 *>(p)); return make_double2(v.x, v.y); }
template <bool CONJ> __device__ __forceinline__ double t_op(double v) { return v; }
template <bool CONJ> __device__ __forceinline__ zc t_op(zc v) { return CONJ ? make_double2(v.x, -v.y) : v; }
__device__ __forceinline__ void t_mad(double &acc, double a, double b) { acc += a * b; }
__device__ __forceinline__ void t_mad(zc &acc, zc a, zc b) { acc.x += a.x * b.x - a.y * b.y; acc.y += a.y * b.x + a.x * b.y; }
__device__ __forceinline__ void t_zero(double &v) { v = 0.0; }
__device__ __forceinline__ void t_zero(zc &v) { v = make_double2(0.0, 0.0); }
__device__ __forceinline__ void t_atomic_sub(double *p, double v) { if (v != 0.0) atomic_sub_f64(p, v); }
__device__ __forceinline__ void t_atomic_sub(zc *p, zc v) { if (v.x != 0.0) unsafeAtomicAdd(&p->x, -v.x); if (v.y != 0.0) unsafeAtomicAdd(&p->y, -v.y); }
__device__ __forceinline__ void t_plain_sub(double *p, double v) { *p -= v; }
__device__ __forceinline__ void t_plain_sub(zc *p, zc v) { zc o = *p; o.x -= v.x; o.y -= v.y; *p = o; }

template <int N>
__device__ __forceinline__ void wave_colsum(double (&v)[N], int lane)
{
    static_assert(N >= 1 && N <= 64 && (N & (N - 1)) == 0, "a power of two of columns");
    int mask = 32;
#pragma unroll
    for (int h = N / 2; h >= 1; h >>= 1) {
        const bool up = (lane & mask) != 0;
#pragma unroll
        for (int i = 0; i < h; ++i) {
            const double a = v[i], b = v[i + h];
            v[i] = (up ? b : a) + __shfl_xor(up ? a : b, mask);
        }
        mask >>= 1;
    }
#pragma unroll
    for (; mask >= 1; mask >>= 1) v[0] += __shfl_xor(v[0], mask);
}
template <int N> __device__ __forceinline__ double wave_colsum_v(double (&a)[N], int lane) { wave_colsum<N>(a, lane); return a[0]; }
template <int N> __device__ __forceinline__ zc wave_colsum_v(zc (&a)[N], int lane)
{
    double re[N], im[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { re[i] = a[i].x; im[i] = a[i].y; }
    wave_colsum<N>(re, lane);
    wave_colsum<N>(im, lane);
    return make_double2(re[0], im[0]);
}

// ---- U^T chunks: x[gc] -= sum_r op(U_k[r, c]) y_k[r] for the chunk's <= 64 non-empty skyline columns ---------------------------------------------------------
// y_k (ns x nrhs, solved in place by the diagonal launch before) is staged in LDS once; wave w takes the columns w NC .. w NC + NC - 1 (mod 4 NC) of the chunk,
// its lanes the rows lane + 64 q of the segments (RB row blocks: 1 on levels of at most 64 columns, else 4): NC x RB independent loads per lane in flight, every
// factor entry read ONCE for all right-hand sides of the chunk.  One atomic per (column, right-hand side).
template <class V, bool CONJ, int RB, int NC, int RK>
__global__ __launch_bounds__(256) void k_fwd_update_t(DevTables T, const int *__restrict__ nodes, const int *__restrict__ prefix, int nn, V *__restrict__ x,
                                                      int64_t ldx, int nrhs)
{
    extern __shared__ double t_lds[];
    V *yk = reinterpret_cast<V *>(t_lds);          // [right-hand side][ns]
    __shared__ int s_cp[64], s_ld[64], s_gc[64];
    const int ni = find_node_wave(prefix, nn, blockIdx.x);
    const int k = nodes[ni], chunk = blockIdx.x - prefix[ni];
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;
    const int ncol = min(64, T.sn_ncolu[k] - chunk * 64);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < 64) {
        int cp = 0, ld = ns, gc = 0;
        if (tid < ncol) {
            const int64_t ci = T.sn_ucol[k] + chunk * 64 + tid;
            ld = T.ucol_ld[ci]; cp = T.ucol_cp[ci]; gc = T.ucol_gc[ci];
        }
        s_cp[tid] = cp; s_ld[tid] = ld; s_gc[tid] = gc;
    }
    for (int idx = tid; idx < ns * nrhs; idx += 256) yk[idx] = x[fst + (idx % ns) + (int64_t) (idx / ns) * ldx];
    __syncthreads();
    const V *Uv = reinterpret_cast<const V *>(T.val) + T.sn_uval[k];
    constexpr int LPC = 64 / NC;                   // lanes that end up with the same column's total
    for (int c0 = wave * NC; c0 < ncol; c0 += 4 * NC) {
        V uv[NC][RB];
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int c = min(c0 + cc, 63);
            const int ld = s_ld[c];                // ns past the chunk's last column: nothing is loaded
            const V *col = Uv + s_cp[c] - ld;
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                const int i = lane + 64 * q;
                if (c0 + cc < ncol && i >= ld && i < ns) uv[cc][q] = t_op<CONJ>(t_ntload(col + i)); else t_zero(uv[cc][q]);
            }
        }
        const int cmine = c0 + lane / LPC;
        const bool owner = (lane % LPC) == 0 && cmine < ncol;
        const int gc = s_gc[min(cmine, 63)];
        for (int q0 = 0; q0 < nrhs; q0 += RK) {
            V acc[RK][NC];
#pragma unroll
            for (int j = 0; j < RK; ++j)
#pragma unroll
                for (int cc = 0; cc < NC; ++cc) t_zero(acc[j][cc]);
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                const int i = min(lane + 64 * q, ns - 1);      // (rows past ns: the factor value is zero)
#pragma unroll
                for (int j = 0; j < RK; ++j) {
                    const V yv = yk[min(q0 + j, nrhs - 1) * ns + i];
#pragma unroll
                    for (int cc = 0; cc < NC; ++cc) t_mad(acc[j][cc], uv[cc][q], yv);
                }
            }
#pragma unroll
            for (int j = 0; j < RK; ++j) {
                const V sv = wave_colsum_v<NC>(acc[j], lane);
                if (owner && q0 + j < nrhs) t_atomic_sub(x + gc + (int64_t) (q0 + j) * ldx, sv);
            }
        }
    }
}

// ---- L^T strips: x_k[c] -= sum_r op(L_k[r, c]) x[lrow r] over the strip's rows below the diagonal block ------------------------------------------------------
// Strip = 64 RB panel rows (RB = 1: double, fwd_prefix; RB = 4: complex16, zfwd_prefix).  Per block of RK right-hand sides the gathered x rows of the strip are
// staged once in LDS (the row map is read once, before); lane l keeps its rows l + 64 q in registers.  Wave w takes the columns w NC .. w NC + NC - 1 (mod 4 NC):
// NC x RB loads per lane in flight.  A supernode with one strip stores plainly (its workgroup is the only writer of x_k in the launch), else fp64 atomics.
template <class V, bool CONJ, int RB, int NC, int RK>
__global__ __launch_bounds__(256) void k_bwd_update_t(DevTables T, const int *__restrict__ nodes, const int *__restrict__ prefix, int nn, V *__restrict__ x,
                                                      int64_t ldx, int nrhs)
{
    constexpr int SR = 64 * RB;
    __shared__ int s_row[SR];
    __shared__ V s_x[RK][SR];
    const int ni = find_node_wave(prefix, nn, blockIdx.x);
    const int k = nodes[ni], strip = blockIdx.x - prefix[ni];
    const bool single = prefix[ni + 1] - prefix[ni] == 1;
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;
    const int lda = T.sn_nsupr[k], row0 = T.sn_ldiag[k] + strip * SR;
    const int nrow = min(SR, lda - row0);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const V *L = reinterpret_cast<const V *>(T.val) + T.sn_lval[k] + row0;
    if (tid < SR) s_row[tid] = tid < nrow ? T.lrow[T.sn_lrow[k] + row0 + tid] : -1;
    __syncthreads();
    constexpr int LPC = 64 / NC;
    for (int q0 = 0; q0 < nrhs; q0 += RK) {
        if (q0) __syncthreads();                   // the previous block's readers are done
        for (int idx = tid; idx < SR * RK; idx += 256) {
            const int r = idx % SR, j = idx / SR;
            const int g = s_row[r];
            if (g >= 0) s_x[j][r] = x[g + (int64_t) min(q0 + j, nrhs - 1) * ldx]; else t_zero(s_x[j][r]);
        }
        __syncthreads();
        V xr[RB][RK];
#pragma unroll
        for (int q = 0; q < RB; ++q)
#pragma unroll
            for (int j = 0; j < RK; ++j) xr[q][j] = s_x[j][lane + 64 * q];
        for (int c0 = wave * NC; c0 < ns; c0 += 4 * NC) {
            V lv[NC][RB];
#pragma unroll
            for (int cc = 0; cc < NC; ++cc)
#pragma unroll
                for (int q = 0; q < RB; ++q) {
                    const int r = lane + 64 * q;
                    if (c0 + cc < ns && r < nrow) lv[cc][q] = t_op<CONJ>(t_ntload(L + r + (size_t) (c0 + cc) * lda)); else t_zero(lv[cc][q]);
                }
            V acc[RK][NC];
#pragma unroll
            for (int j = 0; j < RK; ++j)
#pragma unroll
                for (int cc = 0; cc < NC; ++cc) {
                    t_zero(acc[j][cc]);
#pragma unroll
                    for (int q = 0; q < RB; ++q) t_mad(acc[j][cc], lv[cc][q], xr[q][j]);
                }
            const int cmine = c0 + lane / LPC;
            const bool owner = (lane % LPC) == 0 && cmine < ns;
#pragma unroll
            for (int j = 0; j < RK; ++j) {
                const V sv = wave_colsum_v<NC>(acc[j], lane);
                if (owner && q0 + j < nrhs) {
                    V *d = x + fst + cmine + (int64_t) (q0 + j) * ldx;
                    if (single) t_plain_sub(d, sv); else t_atomic_sub(d, sv);
                }
            }
        }
    }
}

// ---- x_k <- Uinv_k^T x_k (LT = false) / Linv_k^T x_k (LT = true), double: one workgroup per supernode, in place ------------------------------------------------
// Output i is the dot product of COLUMN i of the inverse (contiguous, ld = ns; rows <= i of Uinv, >= i of Linv, explicit zeros elsewhere) with x_k: wave w takes
// the columns w 4 .. w 4 + 3 (mod 4 waves), lanes run along the column (RB blocks of 64 rows; blocks outside the triangle are not loaded).
template <bool LT, int NT, int RB, int RK>
__global__ __launch_bounds__(NT) void k_solve_diag_t(DevTables T, const int *__restrict__ nodes, double *__restrict__ x, int64_t ldx, int nrhs)
{
    extern __shared__ double t_lds[];
    double *xs = t_lds;                            // [right-hand side][ns]
    constexpr int NW = NT / 64, NC = 4, LPC = 64 / NC;
    const int k = nodes[blockIdx.x];
    if (!(T.sn_flags[k] & SNF_OWN_DIAG)) return;
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;
    const double *Ti = T.inv + T.sn_inv[k] + (LT ? 0 : (size_t) ns * ns);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int idx = tid; idx < ns * nrhs; idx += NT) xs[idx] = x[fst + (idx % ns) + (int64_t) (idx / ns) * ldx];
    __syncthreads();
    for (int i0 = wave * NC; i0 < ns; i0 += NW * NC) {
        double tv[NC][RB];
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int i = i0 + cc;
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                const int j = lane + 64 * q;
                const bool ok = i < ns && j < ns && (LT ? j >= i : j <= i);
                tv[cc][q] = ok ? t_ntload(Ti + j + (size_t) i * ns) : 0.0;
            }
        }
        const int imine = i0 + lane / LPC;
        const bool owner = (lane % LPC) == 0 && imine < ns;
        for (int q0 = 0; q0 < nrhs; q0 += RK) {
            double acc[RK][NC];
#pragma unroll
            for (int j = 0; j < RK; ++j)
#pragma unroll
                for (int cc = 0; cc < NC; ++cc) acc[j][cc] = 0.0;
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                const int r = min(lane + 64 * q, ns - 1);      // (rows past ns: the inverse's value is zero)
#pragma unroll
                for (int j = 0; j < RK; ++j) {
                    const double xv = xs[min(q0 + j, nrhs - 1) * ns + r];
#pragma unroll
                    for (int cc = 0; cc < NC; ++cc) acc[j][cc] += tv[cc][q] * xv;
                }
            }
#pragma unroll
            for (int j = 0; j < RK; ++j) {
                const double sv = wave_colsum_v<NC>(acc[j], lane);
                if (owner && q0 + j < nrhs) x[fst + imine + (int64_t) (q0 + j) * ldx] = sv;
            }
        }
    }
}

// ---- complex16 diagonal step: the complex path keeps no inverses -> blocked substitution on the factored block, transposed ------------------------------------
// M = op(A)^T with A the factored diagonal block (U_kk on and above the diagonal, L_kk below): UT = true solves M y = x with M = op(U_kk)^T (lower, its own
// diagonal), blocks ascending; UT = false with M = op(L_kk)^T (unit upper), blocks descending.  Per 32 columns, as kz_solve_diag: (a) one wave solves the 32 x 32
// triangle in registers (lane = row of M = COLUMN of A; the solved entries go round with v_readlane; wave w takes the right-hand sides w, w + 4, ...), (b) every
// thread subtracts the 32 solved entries from one of the remaining rows -- M(i, jb .. jb + 31) = op(A[jb .. jb + 31, i]) is CONTIGUOUS in column i of A.
template <bool UT, bool CONJ>
__global__ __launch_bounds__(256) void kz_solve_diag_t(DevTables T, const int *__restrict__ nodes, zc *__restrict__ x, int64_t ldx, int nrhs)
{
    extern __shared__ double t_lds[];
    zc *xs = reinterpret_cast<zc *>(t_lds);        // [right-hand side][ns]
    const int k = nodes[blockIdx.x];
    if (!(T.sn_flags[k] & SNF_OWN_DIAG)) return;
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;
    const int lda = T.sn_dlda[k];
    const zc *A = reinterpret_cast<const zc *>(T.val) + T.sn_dptr[k];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int idx = tid; idx < ns * nrhs; idx += 256) xs[idx] = x[fst + (idx % ns) + (int64_t) (idx / ns) * ldx];
    __syncthreads();
    const int nblk = (ns + DB - 1) / DB;
    for (int bi = 0; bi < nblk; ++bi) {
        const int jb = (UT ? bi : nblk - 1 - bi) * DB;
        const int nb = min(DB, ns - jb);
        {
            const int i = lane;
            const bool rok = i < nb;
            double cr[DB], ci[DB];                  // M(jb + i, jb + j) = op(A[jb + j, jb + i]): column jb + i of A, this lane's
#pragma unroll
            for (int j = 0; j < DB; ++j) {
                const zc v = (rok && j < nb && (UT ? j <= i : j > i)) ? t_op<CONJ>(A[jb + j + (size_t) (jb + i) * lda]) : make_double2(0.0, 0.0);
                cr[j] = v.x; ci[j] = v.y;
            }
            zc dinv = make_double2(1.0, 0.0);
            if (UT) {
                zc d = make_double2(1.0, 0.0);
#pragma unroll
                for (int j = 0; j < DB; ++j) if (i == j) d = make_double2(cr[j], ci[j]);
                if (rok) dinv = z_div(make_double2(1.0, 0.0), d);
            }
            for (int r = wave; r < nrhs; r += 4) {
                zc xv = rok ? xs[jb + i + r * ns] : make_double2(0.0, 0.0);
                if (UT) {
#pragma unroll
                    for (int j = 0; j < DB; ++j) {
                        if (j < nb) {              // wave-uniform
                            if (i == j) xv = z_mul(xv, dinv);
                            const zc xj = make_double2(lane_bcast(xv.x, j), lane_bcast(xv.y, j));
                            if (i > j) xv = z_fnma(xv, make_double2(cr[j], ci[j]), xj);
                        }
                    }
                } else {
#pragma unroll
                    for (int jj = 0; jj < DB; ++jj) {
                        const int j = DB - 1 - jj;
                        if (j < nb) {
                            const zc xj = make_double2(lane_bcast(xv.x, j), lane_bcast(xv.y, j));
                            if (i < j) xv = z_fnma(xv, make_double2(cr[j], ci[j]), xj);
                        }
                    }
                }
                if (rok) xs[jb + i + r * ns] = xv;
            }
        }
        __syncthreads();
        {
            const int r0 = UT ? jb + nb : 0, r1 = UT ? ns : jb;
            for (int idx = tid; idx < (r1 - r0) * nrhs; idx += 256) {
                const int i = r0 + idx % (r1 - r0), r = idx / (r1 - r0);
                zc acc = xs[i + r * ns];
                const zc *Ac = A + jb + (size_t) i * lda;
#pragma unroll 8
                for (int j = 0; j < nb; ++j) acc = z_fnma(acc, t_op<CONJ>(Ac[j]), xs[jb + j + r * ns]);
                xs[i + r * ns] = acc;
            }
        }
        __syncthreads();
    }
    for (int idx = tid; idx < ns * nrhs; idx += 256) x[fst + (idx % ns) + (int64_t) (idx / ns) * ldx] = xs[idx];
}

// ---- launch wrappers -----------------------------------------------------------------------------------------------------------------------------------
namespace eng {

constexpr int T_RK = 4;                            // right-hand sides per pass over the factor entries when nrhs >= 2
constexpr int T_DYN_LDS_MAX = 104 * 1024;          // x_k staged in LDS: up to max_rhs_chunk's 96 KiB

template <class K> static int t_attr(K kern) { HIPCHK(hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, T_DYN_LDS_MAX)); return 0; }
static int tsolve_attrs()
{
    int rc = 0;
    rc |= t_attr(k_solve_diag_t<false, 256, 1, 1>) | t_attr(k_solve_diag_t<true, 256, 1, 1>) | t_attr(k_solve_diag_t<false, 256, 1, T_RK>) | t_attr(k_solve_diag_t<true, 256, 1, T_RK>);
    rc |= t_attr(k_solve_diag_t<false, 1024, 4, 1>) | t_attr(k_solve_diag_t<true, 1024, 4, 1>) | t_attr(k_solve_diag_t<false, 1024, 4, T_RK>) | t_attr(k_solve_diag_t<true, 1024, 4, T_RK>);
    rc |= t_attr(k_fwd_update_t<double, false, 1, 16, 1>) | t_attr(k_fwd_update_t<double, false, 1, 8, T_RK>) | t_attr(k_fwd_update_t<double, false, 4, 4, 1>) | t_attr(k_fwd_update_t<double, false, 4, 4, T_RK>);
    rc |= t_attr(k_fwd_update_t<zc, false, 1, 8, 1>) | t_attr(k_fwd_update_t<zc, false, 1, 4, T_RK>) | t_attr(k_fwd_update_t<zc, false, 4, 4, 1>) | t_attr(k_fwd_update_t<zc, false, 4, 2, T_RK>);
    rc |= t_attr(k_fwd_update_t<zc, true, 1, 8, 1>) | t_attr(k_fwd_update_t<zc, true, 1, 4, T_RK>) | t_attr(k_fwd_update_t<zc, true, 4, 4, 1>) | t_attr(k_fwd_update_t<zc, true, 4, 2, T_RK>);
    rc |= t_attr(kz_solve_diag_t<true, false>) | t_attr(kz_solve_diag_t<true, true>) | t_attr(kz_solve_diag_t<false, false>) | t_attr(kz_solve_diag_t<false, true>);
    return rc;
}
// once per process, before the first transposed sweep (sluamd_tsolve.cpp): the dynamic-LDS limits of the kernels that stage x_k
int tsolve_setup() { static const int rc = tsolve_attrs(); return rc ? SLUAMD_EHIP : 0; }

void solve_diag_t(hipStream_t s, bool upper, const DevTables &T, const int *nodes, int nn, double *x, int64_t ldx, int nrhs, int mx)
{
    if (nn <= 0) return;
    const size_t lds = sizeof(double) * (size_t) mx * nrhs;
#define T_DIAG(LT, NT, RB) \
    do { if (nrhs >= 2) hipLaunchKernelGGL((k_solve_diag_t<LT, NT, RB, T_RK>), dim3(nn), dim3(NT), lds, s, T, nodes, x, ldx, nrhs); \
         else hipLaunchKernelGGL((k_solve_diag_t<LT, NT, RB, 1>), dim3(nn), dim3(NT), lds, s, T, nodes, x, ldx, nrhs); } while (0)
    if (mx <= 64) { if (upper) T_DIAG(false, 256, 1); else T_DIAG(true, 256, 1); }
    else { if (upper) T_DIAG(false, 1024, 4); else T_DIAG(true, 1024, 4); }
#undef T_DIAG
}

void fwd_update_t(hipStream_t s, const DevTables &T, const int *nodes, const int *prefix, int nn, int nwork, double *x, int64_t ldx, int nrhs, int mx)
{
    if (nwork <= 0) return;
    const size_t lds = sizeof(double) * (size_t) mx * nrhs;
    if (mx <= 64) {
        if (nrhs >= 2) hipLaunchKernelGGL((k_fwd_update_t<double, false, 1, 8, T_RK>), dim3(nwork), dim3(256), lds, s, T, nodes, prefix, nn, x, ldx, nrhs);
        else hipLaunchKernelGGL((k_fwd_update_t<double, false, 1, 16, 1>), dim3(nwork), dim3(256), lds, s, T, nodes, prefix, nn, x, ldx, nrhs);
    } else {
        if (nrhs >= 2) hipLaunchKernelGGL((k_fwd_update_t<double, false, 4, 4, T_RK>), dim3(nwork), dim3(256), lds, s, T, nodes, prefix, nn, x, ldx, nrhs);
        else hipLaunchKernelGGL((k_fwd_update_t<double, false, 4, 4, 1>), dim3(nwork), dim3(256), lds, s, T, nodes, prefix, nn, x, ldx, nrhs);
    }
}

void bwd_update_t(hipStream_t s, const DevTables &T, const int *nodes, const int *prefix, int nn, int nwork, double *x, int64_t ldx, int nrhs)
{
    if (nwork <= 0) return;
    if (nrhs >= 2) hipLaunchKernelGGL((k_bwd_update_t<double, false, 1, 8, T_RK>), dim3(nwork), dim3(256), 0, s, T, nodes, prefix, nn, x, ldx, nrhs);
    else hipLaunchKernelGGL((k_bwd_update_t<double, false, 1, 16, 1>), dim3(nwork), dim3(256), 0, s, T, nodes, prefix, nn, x, ldx, nrhs);
}

void zsolve_diag_t(hipStream_t s, bool upper, bool conj, const DevTables &T, const int *nodes, int nn, void *x, int64_t ldx, int nrhs, int mx)
{
    if (nn <= 0) return;
    const size_t lds = sizeof(zc) * (size_t) mx * nrhs;
    zc *xz = static_cast<zc *>(x);
    if (upper) { if (conj) hipLaunchKernelGGL((kz_solve_diag_t<true, true>), dim3(nn), dim3(256), lds, s, T, nodes, xz, ldx, nrhs);
                 else hipLaunchKernelGGL((kz_solve_diag_t<true, false>), dim3(nn), dim3(256), lds, s, T, nodes, xz, ldx, nrhs); }
    else { if (conj) hipLaunchKernelGGL((kz_solve_diag_t<false, true>), dim3(nn), dim3(256), lds, s, T, nodes, xz, ldx, nrhs);
           else hipLaunchKernelGGL((kz_solve_diag_t<false, false>), dim3(nn), dim3(256), lds, s, T, nodes, xz, ldx, nrhs); }
}

template <bool CONJ>
static void zfwd_update_t_launch(hipStream_t s, const DevTables &T, const int *nodes, const int *prefix, int nn, int nwork, zc *x, int64_t ldx, int nrhs, int mx)
{
    const size_t lds = sizeof(zc) * (size_t) mx * nrhs;
    if (mx <= 64) {
        if (nrhs >= 2) hipLaunchKernelGGL((k_fwd_update_t<zc, CONJ, 1, 4, T_RK>), dim3(nwork), dim3(256), lds, s, T, nodes, prefix, nn, x, ldx, nrhs);
        else hipLaunchKernelGGL((k_fwd_update_t<zc, CONJ, 1, 8, 1>), dim3(nwork), dim3(256), lds, s, T, nodes, prefix, nn, x, ldx, nrhs);
    } else {
        if (nrhs >= 2) hipLaunchKernelGGL((k_fwd_update_t<zc, CONJ, 4, 2, T_RK>), dim3(nwork), dim3(256), lds, s, T, nodes, prefix, nn, x, ldx, nrhs);
        else hipLaunchKernelGGL((k_fwd_update_t<zc, CONJ, 4, 4, 1>), dim3(nwork), dim3(256), lds, s, T, nodes, prefix, nn, x, ldx, nrhs);
    }
}
void zfwd_update_t(hipStream_t s, bool conj, const DevTables &T, const int *nodes, const int *prefix, int nn, int nwork, void *x, int64_t ldx, int nrhs, int mx)
{
    if (nwork <= 0) return;
    if (conj) zfwd_update_t_launch<true>(s, T, nodes, prefix, nn, nwork, static_cast<zc *>(x), ldx, nrhs, mx);
    else zfwd_update_t_launch<false>(s, T, nodes, prefix, nn, nwork, static_cast<zc *>(x), ldx, nrhs, mx);
}

template <bool CONJ>
static void zbwd_update_t_launch(hipStream_t s, const DevTables &T, const int *nodes, const int *prefix, int nn, int nwork, zc *x, int64_t ldx, int nrhs)
{
    if (nrhs >= 2) hipLaunchKernelGGL((k_bwd_update_t<zc, CONJ, 4, 2, T_RK>), dim3(nwork), dim3(256), 0, s, T, nodes, prefix, nn, x, ldx, nrhs);
    else hipLaunchKernelGGL((k_bwd_update_t<zc, CONJ, 4, 4, 1>), dim3(nwork), dim3(256), 0, s, T, nodes, prefix, nn, x, ldx, nrhs);
}
void zbwd_update_t(hipStream_t s, bool conj, const DevTables &T, const int *nodes, const int *prefix, int nn, int nwork, void *x, int64_t ldx, int nrhs)
{
    if (nwork <= 0) return;
    if (conj) zbwd_update_t_launch<true>(s, T, nodes, prefix, nn, nwork, static_cast<zc *>(x), ldx, nrhs);
    else zbwd_update_t_launch<false>(s, T, nodes, prefix, nn, nwork, static_cast<zc *>(x), ldx, nrhs);
}

}  // namespace eng
