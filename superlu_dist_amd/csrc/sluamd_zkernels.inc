// sluamd_zkernels.inc -- complex16 (doublecomplex) kernels of the hot path: pzgstrf3d / pzgstrs3d
// (SRC/complex16/pzgstrf3d.c, ztreeFactorization.c, pzgstrf2.c, ztrfCommWrapper.c, zscatter.c, zscatter3d.c,
// pzgstrs3d.c, pzgstrs_lsum.c -- SURVEY.md section 8(a) row a21).  Included inside namespace sluamd by sluamd_core.hip;
// shares the device tables, tile lists and level schedule of the double path (they are type independent).
//
// State of this file: the Schur update is NOT here -- the double kernel k_schur runs it through the real embedding of the complex
// product (k_schur<.., Z = true>: fused gather -> fp64 MFMA -> scatter, BASELINE.json config 5 "zgemm MFMA + complex scatter"); the
// panel kernels are blocked by 32 through LDS / registers on the vector ALUs (no MFMA yet); the diagonal solves are blocked
// substitutions (one wave per 32 x 32 triangle), the updates one thread per row.

typedef double2 zc;   // {x = re, y = im} == doublecomplex {r, i} (SRC/include/dcomplex.h)

__device__ __forceinline__ zc z_mul(zc a, zc b) { return make_double2(a.x * b.x - a.y * b.y, a.y * b.x + a.x * b.y); }   // zz_mult, dcomplex.h:66-73
__device__ __forceinline__ zc z_sub(zc a, zc b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ zc z_fnma(zc acc, zc a, zc b)   // acc - a*b
{
    return make_double2(fma(-a.x, b.x, fma(a.y, b.y, acc.x)), fma(-a.y, b.x, fma(-a.x, b.y, acc.y)));
}
__device__ __forceinline__ zc z_div(zc a, zc b)   // slud_z_div (Smith), SRC/complex16/dcomplex_dist.c:29-58
{
    double ratio, den, cr, ci;
    if (fabs(b.x) <= fabs(b.y)) {
        ratio = b.x / b.y; den = b.y * (1 + ratio * ratio);
        cr = (a.x * ratio + a.y) / den; ci = (a.y * ratio - a.x) / den;
    } else {
        ratio = b.y / b.x; den = b.x * (1 + ratio * ratio);
        cr = (a.x + a.y * ratio) / den; ci = (a.y - a.x * ratio) / den;
    }
    return make_double2(cr, ci);
}
// Reciprocal of a (non-zero) complex pivot off the division sequence: 1 / (a + i b) = (a - i b) / (a^2 + b^2) on the pivot scaled by a power of two
// (largest component in [0.5, 1): a^2 + b^2 can neither overflow nor lose the small component to underflow, what Smith's formula in z_div is for), with
// v_rcp_f64 + two Newton steps for the real reciprocal (as pivot_recip of the double kernels; relative error of a few ulp).  The pivot chain of the
// one-wave / four-wave complex LU kernels is latency: z_div's three dependent IEEE divisions were ~800 of the ~1900 cycles of an elimination step.
__device__ __forceinline__ zc z_recip(zc p)
{
    const int e = __builtin_amdgcn_frexp_exp(fmax(fabs(p.x), fabs(p.y)));
    const double a = __builtin_amdgcn_ldexp(p.x, -e), b = __builtin_amdgcn_ldexp(p.y, -e);
    const double d = __builtin_fma(a, a, b * b);
    double r = __builtin_amdgcn_rcp(d);
    double t = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, t, r);
    t = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, t, r);
    return make_double2(__builtin_amdgcn_ldexp(a * r, -e), __builtin_amdgcn_ldexp(-b * r, -e));
}
__device__ __forceinline__ void z_atomic_sub(zc *p, zc v)
{
    unsafeAtomicAdd(&p->x, -v.x);
    unsafeAtomicAdd(&p->y, -v.y);
}

// ---- diagonal block LU (Local_Zgstrf2, pzgstrf2.c): unpivoted right-looking elimination, one WG per supernode ----
// Blocked by 32 columns like the double kernel: the m x 32 column panel lives in LDS; its 32 x 32 head is factored in
// registers by one wave, the rows below are solved one per thread
// (pivot handling: |re|+|im| < thresh and both parts non-zero -> (sign(re)*thresh, 0); zero pivot -> info, column left
// unscaled), U12 = L11^-1 A12 one column per thread in registers, and the rank-32 trailing update A22 -= L21 U12 in
// 8-column register tiles with L21 read from the LDS panel and U12 staged 32 columns at a time.
// Unpivoted LU of the nb x nb (nb <= 32) complex head block at P (LDS, column-major, ld) by ONE wave in registers: lane r
// holds row r (identity-padded to 32), pivot rows are broadcast with v_readlane.  s_rinv[j] receives 1/U(j,j) ((1,0) for
// a zero pivot, which leaves the column unscaled like Local_Zgstrf2).  Same operation order as the rank-1 loop.
__device__ __forceinline__ void wave_zlu32(zc *P, int ld, int nb, int col1, int replace_tiny, double thresh, int *info, zc *s_rinv)
{
    const int lane = threadIdx.x & 63;
    double ar[DB], ai[DB];
#pragma unroll
    for (int c = 0; c < DB; ++c) {
        const bool in = lane < nb && c < nb;
        const zc v = in ? P[c * ld + lane] : make_double2((c == lane) ? 1.0 : 0.0, 0.0);
        ar[c] = v.x; ai[c] = v.y;
    }
#pragma unroll
    for (int j = 0; j < DB; ++j) {
        zc p = make_double2(lane_bcast(ar[j], j), lane_bcast(ai[j], j));
        if (j < nb) {
            if (replace_tiny && (fabs(p.x) + fabs(p.y)) < thresh && p.x != 0.0 && p.y != 0.0) {
                p = make_double2(p.x < 0 ? -thresh : thresh, 0.0);
                if (lane == j) { ar[j] = p.x; ai[j] = p.y; }
                if (lane == 0) atomicAdd(&info[1], 1);
            }
            if (p.x == 0.0 && p.y == 0.0 && lane == 0) { atomicMin(&info[0], col1 + j); atomicMax(&info[4], col1 + j); }
        }
        const bool zero = (p.x == 0.0 && p.y == 0.0);
        const zc rinv = zero ? make_double2(1.0, 0.0) : z_recip(p);
        if (lane == 0) s_rinv[j] = rinv;
        const bool below = lane > j;
        zc l = make_double2(ar[j], ai[j]);
        if (!zero) l = z_mul(l, rinv);
        if (below) { ar[j] = l.x; ai[j] = l.y; }
        const zc lm = below ? l : make_double2(0.0, 0.0);   // zero multiplier at and above the pivot row: no select per column
#pragma unroll
        for (int c = j + 1; c < DB; ++c) {
            const zc u = make_double2(lane_bcast(ar[c], j), lane_bcast(ai[c], j));
            { const zc t = z_fnma(make_double2(ar[c], ai[c]), lm, u); ar[c] = t.x; ai[c] = t.y; }
            if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int c = 0; c < DB; ++c) if (lane < nb && c < nb) P[c * ld + lane] = make_double2(ar[c], ai[c]);
}

// Diagonal blocks of at most 64 columns -- the leaves and the small separators at the bottom of the elimination DAG, tens of thousands per
// level -- ONE WAVE per block, in registers, no LDS, no barrier (the workgroup-per-block kernel below spends ~0.4 ms per block in barriers
// and L2 round trips whatever its size: 8 ms for the leaf level of the 1000 x 1000 grid operator).  Lane r holds row r.  64 complex
// columns do not fit the register file next to the temporaries, so the block is done in two column halves:
//   1. columns 0..31 of all rows: right-looking elimination, pivot rows broadcast with v_readlane (the L part of rows 32..63 comes with it);
//   2. columns 32..63: the 32 elimination steps of half 1 applied with the multipliers re-read from the block just written (L2 hits,
//      8 at a time), then the remaining 32 x 32 block is eliminated in the lanes 32..63.
// Arithmetic and pivot handling as kz_diag_lu / Local_Zgstrf2 (pzgstrf2.c): tiny pivot -> (sign(re) thresh, 0), zero pivot -> info, column unscaled.
__device__ __forceinline__ zc z_pivot(zc p, int lane, int j, int col1, int replace_tiny, double thresh, int *info, bool active, double &ar, double &ai)
{
    if (active) {
        if (replace_tiny && (fabs(p.x) + fabs(p.y)) < thresh && p.x != 0.0 && p.y != 0.0) {
            p = make_double2(p.x < 0 ? -thresh : thresh, 0.0);
            if (lane == j) { ar = p.x; ai = p.y; }
            if (lane == 0) atomicAdd(&info[1], 1);
        }
        if (p.x == 0.0 && p.y == 0.0 && lane == 0) { atomicMin(&info[0], col1 + j); atomicMax(&info[4], col1 + j); }
    }
    return p;
}

__global__ __launch_bounds__(256, 2) void kz_diag_lu_wave(DevTables T, const int *__restrict__ nodes, int nn, int replace_tiny, double thresh,
                                                          int *__restrict__ info)
{
    const int bi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bi >= nn) return;
    const int k = nodes[bi];
    if (!(T.sn_flags[k] & SNF_OWN_DIAG)) return;
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;
    const int lda = T.sn_dlda[k];
    zc *A = reinterpret_cast<zc *>(T.val) + T.sn_dptr[k];
    const int lane = threadIdx.x & 63;
    const bool rok = lane < ns;
    double ar[32], ai[32];
    // ---- half 1: columns 0..31 (identity-padded) ----
#pragma unroll
    for (int c = 0; c < 32; ++c) {
        const zc v = (rok && c < ns) ? A[lane + (size_t) c * lda] : make_double2((c == lane) ? 1.0 : 0.0, 0.0);
        ar[c] = v.x; ai[c] = v.y;
    }
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (j < ns) {                                   // wave-uniform
            zc p = make_double2(lane_bcast(ar[j], j), lane_bcast(ai[j], j));
            p = z_pivot(p, lane, j, fst + 1, replace_tiny, thresh, info, true, ar[j], ai[j]);
            const bool zero = (p.x == 0.0 && p.y == 0.0);
            const zc rinv = zero ? make_double2(1.0, 0.0) : z_recip(p);
            const bool below = lane > j;
            zc l = make_double2(ar[j], ai[j]);
            if (!zero) l = z_mul(l, rinv);
            if (below) { ar[j] = l.x; ai[j] = l.y; }
            const zc lm = below ? l : make_double2(0.0, 0.0);   // zero multiplier at and above the pivot row: no select per column
#pragma unroll
            for (int c = j + 1; c < 32; ++c) {
                const zc u = make_double2(lane_bcast(ar[c], j), lane_bcast(ai[c], j));
                { const zc t = z_fnma(make_double2(ar[c], ai[c]), lm, u); ar[c] = t.x; ai[c] = t.y; }
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int c = 0; c < 32; ++c) if (rok && c < ns) A[lane + (size_t) c * lda] = make_double2(ar[c], ai[c]);
    if (ns <= 32) return;                               // wave-uniform
    // ---- half 2: columns 32..63 ----
#pragma unroll
    for (int c = 0; c < 32; ++c) {
        const zc v = (rok && 32 + c < ns) ? A[lane + (size_t) (32 + c) * lda] : make_double2((32 + c == lane) ? 1.0 : 0.0, 0.0);
        ar[c] = v.x; ai[c] = v.y;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");     // the multipliers below are re-read from what this wave stored above
#pragma unroll
    for (int jg = 0; jg < 32; jg += 8) {
        zc l[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) l[t] = rok ? A[lane + (size_t) (jg + t) * lda] : make_double2(0.0, 0.0);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int j = jg + t;
            const bool below = lane > j;
            const zc lmt = below ? l[t] : make_double2(0.0, 0.0);
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                const zc u = make_double2(lane_bcast(ar[c], j), lane_bcast(ai[c], j));
                { const zc v = z_fnma(make_double2(ar[c], ai[c]), lmt, u); ar[c] = v.x; ai[c] = v.y; }
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int j = 32; j < 64; ++j) {
        if (j < ns) {
            const int cj = j - 32;
            zc p = make_double2(lane_bcast(ar[cj], j), lane_bcast(ai[cj], j));
            p = z_pivot(p, lane, j, fst + 1, replace_tiny, thresh, info, true, ar[cj], ai[cj]);
            const bool zero = (p.x == 0.0 && p.y == 0.0);
            const zc rinv = zero ? make_double2(1.0, 0.0) : z_recip(p);
            const bool below = lane > j;
            zc l = make_double2(ar[cj], ai[cj]);
            if (!zero) l = z_mul(l, rinv);
            if (below) { ar[cj] = l.x; ai[cj] = l.y; }
            const zc lm = below ? l : make_double2(0.0, 0.0);   // zero multiplier at and above the pivot row: no select per column
#pragma unroll
            for (int c = cj + 1; c < 32; ++c) {
                const zc u = make_double2(lane_bcast(ar[c], j), lane_bcast(ai[c], j));
                { const zc t = z_fnma(make_double2(ar[c], ai[c]), lm, u); ar[c] = t.x; ai[c] = t.y; }
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int c = 0; c < 32; ++c) if (rok && 32 + c < ns) A[lane + (size_t) (32 + c) * lda] = make_double2(ar[c], ai[c]);
}

// The same elimination with FOUR waves per block (round 5): the levels of few 33 .. 64-column blocks are the panel chain of the 2-D complex16 configuration
// (one block per level at the top: 52 us for a lone wave, 150 us beside the Schur tiles -- 21 % of the GPU time of pzgstrf3d), and a lone wave spends its
// time issuing: per elimination step 4 v_readlane + 4 v_fma_f64 for every later column.  Here wave w keeps columns 16 w .. 16 w + 15 of all 64 rows (lane = row,
// 32 VGPRs of data), so a step's column updates are dealt over the waves; what crosses waves is the multiplier column of the step, one complex value per row,
// through LDS (double-buffered by step parity: ONE barrier per step).  The owner of the NEXT step's column brings that column up to date first and has its
// multipliers in LDS before it turns to its other columns: the pivot chain (reciprocal, scaling) overlaps the other waves' updates.
// Same operations in the same order on every element as the one-wave kernel (bitwise equal factors); pivot handling as Local_Zgstrf2 (pzgstrf2.c).
__device__ __forceinline__ void z_make_multipliers(double &ar, double &ai, int j, int lane, int col1, int replace_tiny, double thresh, int *info, zc *s_l)
{
    zc p = make_double2(lane_bcast(ar, j), lane_bcast(ai, j));
    p = z_pivot(p, lane, j, col1, replace_tiny, thresh, info, true, ar, ai);
    const bool zero = (p.x == 0.0 && p.y == 0.0);
    const zc rinv = zero ? make_double2(1.0, 0.0) : z_recip(p);
    const bool below = lane > j;
    zc l = make_double2(ar, ai);
    if (!zero) l = z_mul(l, rinv);
    if (below) { ar = l.x; ai = l.y; }
    s_l[lane] = below ? l : make_double2(0.0, 0.0);     // zero multiplier at and above the pivot row
}

__global__ __launch_bounds__(256) void kz_diag_lu_wave4(DevTables T, const int *__restrict__ nodes, int nn, int replace_tiny, double thresh,
                                                        int *__restrict__ info)
{
    __shared__ zc s_l[2][64];
    const int bi = blockIdx.x;
    if (bi >= nn) return;
    const int k = nodes[bi];
    if (!(T.sn_flags[k] & SNF_OWN_DIAG)) return;        // workgroup-uniform
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;
    const int lda = T.sn_dlda[k];
    zc *A = reinterpret_cast<zc *>(T.val) + T.sn_dptr[k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool rok = lane < ns;
    double ar[16], ai[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int col = 16 * wave + c;
        const zc v = (rok && col < ns) ? A[lane + (size_t) col * lda] : make_double2((col == lane) ? 1.0 : 0.0, 0.0);
        ar[c] = v.x; ai[c] = v.y;
    }
    if (wave == 0) z_make_multipliers(ar[0], ai[0], 0, lane, fst + 1, replace_tiny, thresh, info, s_l[0]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        if (j < ns) {                                   // workgroup-uniform
            const int wj = j >> 4, jl = j & 15, wj1 = (j + 1) >> 4, jl1 = (j + 1) & 15;
            const zc lm = s_l[j & 1][lane];
            if (j + 1 < 64 && wave == wj1) {            // the next step's column first, then its multipliers (identity-padded steps past ns are skipped)
                const zc u = make_double2(lane_bcast(ar[jl1], j), lane_bcast(ai[jl1], j));
                const zc t = z_fnma(make_double2(ar[jl1], ai[jl1]), lm, u);
                ar[jl1] = t.x; ai[jl1] = t.y;
                if (j + 1 < ns) z_make_multipliers(ar[jl1], ai[jl1], j + 1, lane, fst + 1, replace_tiny, thresh, info, s_l[(j + 1) & 1]);
            }
            if (wave >= wj) {
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const bool later = wave > wj || c > jl;                       // column 16 wave + c > j
                    const bool done = wave == wj1 && c == jl1;                    // the look-ahead column above
                    if (later && !done) {
                        const zc u = make_double2(lane_bcast(ar[c], j), lane_bcast(ai[c], j));
                        const zc t = z_fnma(make_double2(ar[c], ai[c]), lm, u);
                        ar[c] = t.x; ai[c] = t.y;
                    }
                    if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int col = 16 * wave + c;
        if (rok && col < ns) A[lane + (size_t) col * lda] = make_double2(ar[c], ai[c]);
    }
}

// The same elimination for levels whose blocks have at most NC <= 32 columns (the small separators right above the leaves: 7, 15, 31
// columns), one 64-thread workgroup per block and NC columns in registers.  The point is the register footprint: these levels' diagonal
// kernels run on the look-ahead stream next to the bulk Schur tiles of the level below (5 waves x 88 VGPRs per SIMD), where a
// workgroup of four 237-VGPR waves waits until whole SIMDs drain -- measured 3.3 ms for a 0.07 ms kernel.
template <int NC>
__global__ __launch_bounds__(64) void kz_diag_lu_wave_small(DevTables T, const int *__restrict__ nodes, int nn, int replace_tiny, double thresh,
                                                            int *__restrict__ info)
{
    const int bi = blockIdx.x;
    if (bi >= nn) return;
    const int k = nodes[bi];
    if (!(T.sn_flags[k] & SNF_OWN_DIAG)) return;
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;
    const int lda = T.sn_dlda[k];
    zc *A = reinterpret_cast<zc *>(T.val) + T.sn_dptr[k];
    const int lane = threadIdx.x;
    const bool rok = lane < ns;
    double ar[NC], ai[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const zc v = (rok && c < ns) ? A[lane + (size_t) c * lda] : make_double2((c == lane) ? 1.0 : 0.0, 0.0);
        ar[c] = v.x; ai[c] = v.y;
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (j < ns) {                                   // wave-uniform
            zc p = make_double2(lane_bcast(ar[j], j), lane_bcast(ai[j], j));
            p = z_pivot(p, lane, j, fst + 1, replace_tiny, thresh, info, true, ar[j], ai[j]);
            const bool zero = (p.x == 0.0 && p.y == 0.0);
            const zc rinv = zero ? make_double2(1.0, 0.0) : z_recip(p);
            const bool below = lane > j;
            zc l = make_double2(ar[j], ai[j]);
            if (!zero) l = z_mul(l, rinv);
            if (below) { ar[j] = l.x; ai[j] = l.y; }
            const zc lm = below ? l : make_double2(0.0, 0.0);   // zero multiplier at and above the pivot row: no select per column
#pragma unroll
            for (int c = j + 1; c < NC; ++c) {
                const zc u = make_double2(lane_bcast(ar[c], j), lane_bcast(ai[c], j));
                { const zc t = z_fnma(make_double2(ar[c], ai[c]), lm, u); ar[c] = t.x; ai[c] = t.y; }
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) if (rok && c < ns) A[lane + (size_t) c * lda] = make_double2(ar[c], ai[c]);
}

constexpr int ZUC = 32;    // U12 columns staged per trailing-update slice
static inline size_t zdiag_lds_bytes(int nsmax) { return sizeof(double) * 2 * ((size_t) DB * (nsmax | 1) + (size_t) DB * ZUC) + 64; }

__global__ __launch_bounds__(256) void kz_diag_lu(DevTables T, const int *__restrict__ nodes,
                                                  int replace_tiny, double thresh, int *__restrict__ info, int ldp)
{
    extern __shared__ double zsm_raw[];
    __shared__ zc s_rinv[DB];
    zc *Ps = reinterpret_cast<zc *>(zsm_raw);       // panel: element (r, c) at Ps[c * ldp + r]
    zc *Us = Ps + (size_t) DB * ldp;                // U12 slice: element (kk, c) at Us[kk * ZUC + c]
    const int k = nodes[blockIdx.x];
    if (!(T.sn_flags[k] & SNF_OWN_DIAG)) return;     // XY layers: the owner of the diagonal block factors it (at the top of its own L slot)
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;
    const int lda = T.sn_dlda[k];
    zc *A = reinterpret_cast<zc *>(T.val) + T.sn_dptr[k];
    const int tid = threadIdx.x;
    for (int jb = 0; jb < ns; jb += DB) {
        const int nb = min(DB, ns - jb), m = ns - jb, nc = m - nb;
        for (int idx = tid; idx < m * nb; idx += 256) { const int r = idx % m, c = idx / m; Ps[c * ldp + r] = A[jb + r + (size_t) (jb + c) * lda]; }
        __syncthreads();
        if (tid < 64) wave_zlu32(Ps, ldp, nb, fst + jb + 1, replace_tiny, thresh, info, s_rinv);
        __syncthreads();
        // L21 rows: x U11 = a, one row per thread in registers (nc > 0 implies nb == 32); columns of a zero pivot stay
        // unscaled (s_rinv = 1), like the rank-1 formulation
        for (int r = tid; r < nc; r += 256) {
            zc x[DB];
#pragma unroll
            for (int c = 0; c < DB; ++c) x[c] = Ps[c * ldp + nb + r];
#pragma unroll
            for (int j = 0; j < DB; ++j) {
                zc acc = x[j];
#pragma unroll
                for (int kk = 0; kk < j; ++kk) acc = z_fnma(acc, x[kk], Ps[j * ldp + kk]);
                x[j] = z_mul(acc, s_rinv[j]);
            }
#pragma unroll
            for (int c = 0; c < DB; ++c) Ps[c * ldp + nb + r] = x[c];
        }
        __syncthreads();
        for (int idx = tid; idx < m * nb; idx += 256) { const int r = idx % m, c = idx / m; A[jb + r + (size_t) (jb + c) * lda] = Ps[c * ldp + r]; }
        if (nc > 0) {
            // U12 = L11^-1 A12 (unit lower): one thread per column, forward substitution in registers
            for (int c = tid; c < nc; c += 256) {
                zc *col = A + jb + (size_t) (jb + nb + c) * lda;
                zc x[DB];
#pragma unroll
                for (int i = 0; i < DB; ++i) x[i] = col[i];
#pragma unroll
                for (int i = 1; i < DB; ++i) {
                    zc acc = x[i];
#pragma unroll
                    for (int kk = 0; kk < i; ++kk) acc = z_fnma(acc, Ps[kk * ldp + i], x[kk]);
                    x[i] = acc;
                }
#pragma unroll
                for (int i = 0; i < DB; ++i) col[i] = x[i];
            }
            __syncthreads();
            // A22 -= L21 U12: thread (tr, tc) owns rows tr + 64 q and the 8 columns tc*8.. of the 32-column slice
            const int tr = tid & 63, tc = tid >> 6;
            for (int c0 = 0; c0 < nc; c0 += ZUC) {
                const int ncc = min(ZUC, nc - c0);
                for (int idx = tid; idx < DB * ZUC; idx += 256) {
                    const int i = idx & 31, c = idx >> 5;
                    Us[i * ZUC + c] = (c < ncc) ? A[jb + i + (size_t) (jb + nb + c0 + c) * lda] : make_double2(0.0, 0.0);
                }
                __syncthreads();
                // 2 rows x 8 columns per thread: 10 LDS reads per 16 complex multiply-adds
                for (int r = tr; r < nc; r += 128) {
                    const int r1 = r + 64;
                    const bool two = r1 < nc;
                    zc acc0[8], acc1[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) { acc0[q] = make_double2(0.0, 0.0); acc1[q] = make_double2(0.0, 0.0); }
#pragma unroll 4
                    for (int kk = 0; kk < DB; ++kk) {
                        const zc l0 = Ps[kk * ldp + nb + r];
                        const zc l1 = Ps[kk * ldp + nb + (two ? r1 : r)];
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const zc u = Us[kk * ZUC + tc * 8 + q];
                            acc0[q] = z_fnma(acc0[q], l0, u);
                            acc1[q] = z_fnma(acc1[q], l1, u);
                        }
                    }
                    // 16 loads, then 16 stores: one L2 round trip per row pair instead of dependent ones
                    zc *e0[8], *e1[8]; zc o0[8], o1[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int c = min(tc * 8 + q, ncc - 1);
                        e0[q] = A + jb + nb + r + (size_t) (jb + nb + c0 + c) * lda;
                        e1[q] = A + jb + nb + (two ? r1 : r) + (size_t) (jb + nb + c0 + c) * lda;
                        o0[q] = *e0[q]; o1[q] = *e1[q];
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (tc * 8 + q < ncc) {     // acc holds -(L21 U12)
                            *e0[q] = make_double2(o0[q].x + acc0[q].x, o0[q].y + acc0[q].y);
                            if (two) *e1[q] = make_double2(o1[q].x + acc1[q].x, o1[q].y + acc1[q].y);
                        }
                }
                __syncthreads();
            }
        }
        __syncthreads();
    }
}

// ---- panel TRSMs, one thread per panel row (L) / per non-empty skyline column (U), blocked by 32 ----------------------
// The thread keeps the 32 unknowns of the current block in registers; the 32x32 operand blocks of U_kk / L_kk are staged
// through LDS once per workgroup (instead of one global load per multiply), earlier blocks of the thread's own row /
// column are re-read from L2.  L strips first (blocks [0, nl)), then U column chunks.
// The same two panel solves for levels of <= 64-column supernodes (round 4), FOUR LANES PER ROW / skyline column.  kz_panel_trsm below gives a row to one thread:
// 2 048 complex multiply-adds in sequence, ~8 round trips (the 32-column blocks go through global memory), 71 us however few strips a level has -- and on the
// 1000^2 complex16 configuration the panel chain is what bounds the factorisation (NOTEBOOK.md section 5).  Here a quad owns a row: lane q holds its columns
// 4 i + q (16 values), the whole triangle is staged in LDS once per workgroup, and the substitution is right-looking -- the owner of column j finishes
// x_j, a DPP quad broadcast hands it to the other three lanes, every lane updates its later columns: the dependent chain per column is one multiply, one
// broadcast, one multiply-add.  Workgroup = the same 64-row strip / 64-column chunk as before, 256 threads.
template <int Q> __device__ __forceinline__ double quad_bcast(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, Q * 0x55, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, Q * 0x55, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <int Q> __device__ __forceinline__ zc quad_bcast_z(zc v) { return make_double2(quad_bcast<Q>(v.x), quad_bcast<Q>(v.y)); }

// NI = values per lane (columns 4 i + q): 16 -> supernodes of up to 64 columns, 8 -> 32, 4 -> 16 (round 5: the levels of small separators right above the leaves
// -- 7, 15, 31 columns, thousands of panels -- ran the 64-column build: 66.6 KB of LDS = two workgroups per CU, 1.2 ms for a level whose triangles are 8 x 8).
// The staged triangle is (4 NI) x (4 NI + 1) complex values: 66.6 / 16.9 / 4.4 KB.
// one step of the right-looking substitution: column / row j = 4 JJ + TT.  UPPER (L branch, X U = B): x_j *= 1 / U_jj, then x_c -= x_j U[j][c] for the lane's
// columns c > j;  !UPPER (U branch, L x = u, unit diagonal): x_i -= L[i][j] x_j for the lane's rows i > j.  Ts[zq_off(j) + c] (packed rows, c > j) holds U[j][c] resp. L[c][j].
template <bool UPPER, int JJ, int TT, int NI>
__device__ __forceinline__ void zq_step(zc (&x)[NI], const zc *Ts, const zc *s_tinv, int q, int ns)
{
    constexpr int j = 4 * JJ + TT;
    if (j >= ns) return;
    zc xj = x[JJ];
    if (UPPER) xj = z_mul(xj, s_tinv[j]);
    xj = quad_bcast_z<TT>(xj);
    if (UPPER && q == TT) x[JJ] = xj;
    constexpr int ZN = 4 * NI;
    const zc *Tj = Ts + (j * ZN - j * (j + 1) / 2) + q;        // packed row j of the triangle: element (j, c), c >= j, at zq_off(j) + c
    if (q > TT) x[JJ] = z_fnma(x[JJ], xj, Tj[4 * JJ]);
#pragma unroll
    for (int i = JJ + 1; i < NI; ++i) x[i] = z_fnma(x[i], xj, Tj[4 * i]);
}
template <bool UPPER, int JJ, int NI>
__device__ __forceinline__ void zq_steps(zc (&x)[NI], const zc *Ts, const zc *s_tinv, int q, int ns)
{
    if constexpr (JJ < NI) {
        if (4 * JJ < ns) {
            zq_step<UPPER, JJ, 0, NI>(x, Ts, s_tinv, q, ns); zq_step<UPPER, JJ, 1, NI>(x, Ts, s_tinv, q, ns);
            zq_step<UPPER, JJ, 2, NI>(x, Ts, s_tinv, q, ns); zq_step<UPPER, JJ, 3, NI>(x, Ts, s_tinv, q, ns);
            zq_steps<UPPER, JJ + 1, NI>(x, Ts, s_tinv, q, ns);
        }
    }
}

template <int NI>
__global__ __launch_bounds__(256) void kz_panel_trsm_quad(DevTables T, const int *__restrict__ nodes, const int *__restrict__ lprefix, const int *__restrict__ uprefix,
                                                          int nn, int nl)
{
    constexpr int ZN = 4 * NI;
    // the triangle PACKED by rows (row j holds its columns j .. ZN - 1 at j ZN - j (j + 1) / 2 + c): 33.3 KB for 64 columns instead of the 66.6 KB of the
    // square 64 x 65 image -- four workgroups per CU instead of two on the leaf level, whose tens of thousands of strips mostly stage and leave
    auto zq_off = [](int j) { return j * ZN - j * (j + 1) / 2; };
    __shared__ zc Ts[ZN * (ZN + 1) / 2];
    __shared__ zc s_tinv[ZN];
    zc *V = reinterpret_cast<zc *>(T.val);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 2, q = lane & 3;
    const bool lbranch = (int) blockIdx.x < nl;
    const int id = lbranch ? (int) blockIdx.x : (int) blockIdx.x - nl;
    const int ni = find_node_wave(lbranch ? lprefix : uprefix, nn, id);
    const int k = nodes[ni];
    const int unit = id - (lbranch ? lprefix : uprefix)[ni];
    const int ns = T.xsup[k + 1] - T.xsup[k];
    const zc *D = V + T.sn_dptr[k];                // factored diagonal block: own slot, or the image received in exchange phase 1
    const int ldd = T.sn_dlda[k];
    // the triangle: element (jj, cc) of the block at D[jj + cc * ldd]; L branch keeps U[jj][cc] (jj <= cc) at Ts[zq_off(jj) + cc], U branch L[cc'][jj'] ... i.e.
    // BOTH read Ts[zq_off(j) + c] in the steps: L branch j = row of U, c = column; U branch j = column of L, c = row
    // only the triangle the branch reads, only ns x ns of it: a leaf level launches tens of thousands of these workgroups for supernodes of a few dozen columns,
    // and the staging is most of what they do.  (Entries outside it stay unwritten: they only ever meet the zero-initialised x of columns / rows >= ns or of the
    // other triangle's positions, whose results are neither stored nor broadcast.)  Columns / rows ns .. 63 of the staged rows ARE read by the steps (the
    // lane's later columns run to 63 whatever ns is): zero-filled, so that no lane ever computes on uninitialised LDS -- ns (64 - ns) writes per workgroup.
    static_assert(sizeof(zc) * (ZN * (ZN + 1) / 2 + ZN) <= 40 * 1024, "kz_panel_trsm_quad: the packed triangle is sized for four workgroups per CU of gfx950's 160 KB of LDS");
    for (int idx = tid; idx < ns * (ZN - ns); idx += 256) {
        const int j = idx / (ZN - ns), c = ns + idx - j * (ZN - ns);
        Ts[zq_off(j) + c] = make_double2(0.0, 0.0);
    }
    for (int idx = tid; idx < ns * ns; idx += 256) {
        const int cc = idx / ns, jj = idx - cc * ns;
        if (lbranch ? jj <= cc : jj > cc) {
            const zc v = D[jj + (size_t) cc * ldd];
            if (lbranch) Ts[zq_off(jj) + cc] = v;      // U[jj][cc]
            else Ts[zq_off(cc) + jj] = v;              // L[jj][cc] at (column cc, row jj): strictly above the diagonal of the packed image
        }
    }
    __syncthreads();
    if (lbranch && tid < ns) s_tinv[tid] = z_div(make_double2(1.0, 0.0), Ts[zq_off(tid) + tid]);
    if (lbranch) {   // L(:,k) <- L(:,k) inv(U_kk)   (zLPanelTrSolve, ztrfCommWrapper.c)
        const int lda = T.sn_nsupr[k];
        const int ldiag = T.sn_ldiag[k];
        const int row = ldiag + unit * 64 + wave * 16 + grp;
        const bool ok = row < lda;
        zc *B = V + T.sn_lval[k] + (ok ? row : ldiag);
        zc x[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) x[i] = (ok && 4 * i + q < ns) ? B[(size_t) (4 * i + q) * lda] : make_double2(0.0, 0.0);
        __syncthreads();      // s_tinv
        zq_steps<true, 0, NI>(x, Ts, s_tinv, q, ns);
#pragma unroll
        for (int i = 0; i < NI; ++i) if (ok && 4 * i + q < ns) B[(size_t) (4 * i + q) * lda] = x[i];
    } else {         // U(k,:) <- inv(L_kk) U(k,:) on the skyline   (zTrs2_GatherTrsmScatter, pzgstrf2.c)
        const int c = unit * 64 + wave * 16 + grp;
        const bool ok = c < T.sn_ncolu[k];
        int lead = ns;
        zc *u = V + T.sn_uval[k];
        if (ok) {
            const int64_t ci = T.sn_ucol[k] + c;
            lead = T.ucol_ld[ci];                  // implicit zeros above the segment
            u += T.ucol_cp[ci];
        }
        zc x[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) { const int a = 4 * i + q; x[i] = (a >= lead && a < ns) ? u[a - lead] : make_double2(0.0, 0.0); }
        zq_steps<false, 0, NI>(x, Ts, s_tinv, q, ns);
#pragma unroll
        for (int i = 0; i < NI; ++i) { const int a = 4 * i + q; if (a >= lead && a < ns) u[a - lead] = x[i]; }
    }
}

__global__ __launch_bounds__(64) void kz_panel_trsm(DevTables T, const int *__restrict__ nodes,
                                                    const int *__restrict__ lprefix, const int *__restrict__ uprefix,
                                                    int nn, int nl)
{
    __shared__ zc Tb[DB * (DB + 1)];
    __shared__ zc s_tinv[DB];          // reciprocals of the staged diagonal: one complex division per column of U_kk instead of one per row and column
    zc *V = reinterpret_cast<zc *>(T.val);
    const int tid = threadIdx.x;
    if ((int) blockIdx.x < nl) {   // L(:,k) <- L(:,k) inv(U_kk)   (zLPanelTrSolve, ztrfCommWrapper.c)
        const int ni = find_node_wave(lprefix, nn, blockIdx.x);
        const int k = nodes[ni];
        const int strip = blockIdx.x - lprefix[ni];
        const int ns = T.xsup[k + 1] - T.xsup[k];
        const int lda = T.sn_nsupr[k];
        const int ldiag = T.sn_ldiag[k];               // rows of the diagonal block at the top of this slot (XY layers: 0 off the process row of k)
        const int row = ldiag + strip * 64 + tid;
        const bool ok = row < lda;
        const zc *D = V + T.sn_dptr[k];                // factored diagonal block: own slot, or the image received in exchange phase 1
        const int ldd = T.sn_dlda[k];
        zc *B = V + T.sn_lval[k] + (ok ? row : ldiag);
        for (int jb = 0; jb < ns; jb += DB) {
            zc x[DB];
#pragma unroll
            for (int c = 0; c < DB; ++c) x[c] = (ok && jb + c < ns) ? B[(size_t) (jb + c) * lda] : make_double2(0.0, 0.0);
            for (int kc = 0; kc <= jb; kc += DB) {
                // stage U_kk(kc.., jb..): element (kk, cc) at Tb[cc * 33 + kk]; identity-padded past ns
                __syncthreads();
                for (int idx = tid; idx < DB * DB; idx += 64) {
                    const int kk = idx & 31, cc = idx >> 5;
                    zc v = make_double2((kc == jb && kk == cc) ? 1.0 : 0.0, 0.0);
                    if (kc + kk < ns && jb + cc < ns) v = D[kc + kk + (size_t) (jb + cc) * ldd];
                    Tb[cc * (DB + 1) + kk] = v;
                }
                __syncthreads();
                if (kc == jb) {
                    if (tid < DB) s_tinv[tid] = z_div(make_double2(1.0, 0.0), Tb[tid * (DB + 1) + tid]);
                    __syncthreads();
                }
                if (kc < jb) {
                    for (int kk = 0; kk < DB; ++kk) {
                        const zc b = ok ? B[(size_t) (kc + kk) * lda] : make_double2(0.0, 0.0);
#pragma unroll
                        for (int c = 0; c < DB; ++c) x[c] = z_fnma(x[c], b, Tb[c * (DB + 1) + kk]);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < DB; ++j) {
                        zc acc = x[j];
#pragma unroll
                        for (int kk = 0; kk < j; ++kk) acc = z_fnma(acc, x[kk], Tb[j * (DB + 1) + kk]);
                        x[j] = z_mul(acc, s_tinv[j]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < DB; ++c) if (ok && jb + c < ns) B[(size_t) (jb + c) * lda] = x[c];
        }
    } else {                        // U(k,:) <- inv(L_kk) U(k,:) on the skyline   (zTrs2_GatherTrsmScatter, pzgstrf2.c)
        const int id = blockIdx.x - nl;
        const int ni = find_node_wave(uprefix, nn, id);
        const int k = nodes[ni];
        const int c = (id - uprefix[ni]) * 64 + tid;
        const bool ok = c < T.sn_ncolu[k];
        const int klst = T.xsup[k + 1], ns = klst - T.xsup[k];
        const int lda = T.sn_nsupr[k];
        int lead = ns;
        zc *u = V + T.sn_uval[k];
        if (ok) {     // flat per-non-empty-column maps instead of a search over the block descriptors
            const int64_t ci = T.sn_ucol[k] + c;
            lead = T.ucol_ld[ci];                          // implicit zeros above the segment
            u += T.ucol_cp[ci];
        }
        const zc *Lkk = V + T.sn_dptr[k];
        const int ldd = T.sn_dlda[k];
        for (int ib = 0; ib < ns; ib += DB) {
            zc x[DB];
#pragma unroll
            for (int i = 0; i < DB; ++i) { const int a = ib + i; x[i] = (a >= lead && a < ns) ? u[a - lead] : make_double2(0.0, 0.0); }
            for (int kb = 0; kb <= ib; kb += DB) {
                // stage L_kk(ib.., kb..): element (i, kk) at Tb[kk * 33 + i]
                __syncthreads();
                for (int idx = tid; idx < DB * DB; idx += 64) {
                    const int i = idx & 31, kk = idx >> 5;
                    zc v = make_double2(0.0, 0.0);
                    if (ib + i < ns && kb + kk < ns) v = Lkk[ib + i + (size_t) (kb + kk) * ldd];
                    Tb[kk * (DB + 1) + i] = v;
                }
                __syncthreads();
                if (kb < ib) {
                    for (int kk = 0; kk < DB; ++kk) {
                        const int a = kb + kk;
                        const zc b = (a >= lead && a < ns) ? u[a - lead] : make_double2(0.0, 0.0);
#pragma unroll
                        for (int i = 0; i < DB; ++i) x[i] = z_fnma(x[i], Tb[kk * (DB + 1) + i], b);
                    }
                } else {
#pragma unroll
                    for (int i = 1; i < DB; ++i) {
                        zc acc = x[i];
#pragma unroll
                        for (int kk = 0; kk < i; ++kk) acc = z_fnma(acc, Tb[kk * (DB + 1) + i], x[kk]);
                        x[i] = acc;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < DB; ++i) { const int a = ib + i; if (a >= lead && a < ns) u[a - lead] = x[i]; }
        }
    }
}

// ---- Schur update: k_schur<.., Z = true> (sluamd_kernels.hip) runs the complex update through its real embedding ----

// ---- triangular solves (zlsum_fmod_inv / zlsum_bmod_inv, pzgstrs_lsum.c) ---------------------------------------------
// x_k <- inv(L_kk) x_k (unit lower) / inv(U_kk) x_k by BLOCKED substitution on the factored diagonal block (the complex path keeps no
// inverses): per 32 columns, (a) the 32 x 32 triangular block is solved by ONE wave in registers -- lane = row, the solved value of
// each column broadcast with v_readlane, no barrier (wave w takes the right-hand sides w, w + 4, ...) -- then (b) every thread
// subtracts the 32 solved columns from its row of the rest.  Two barriers per 32 columns instead of one per column (round 1's
// form: 174 us per 256-column block; the diagonal solves were 5.9 of the 7.3 ms of a solve of the 1000 x 1000 grid operator).
template <bool LOWER>
__global__ __launch_bounds__(256) void kz_solve_diag(DevTables T, const int *__restrict__ nodes, zc *__restrict__ x,
                                                     int64_t ldx, int nrhs)
{
    extern __shared__ double xs_raw[];
    zc *xs = reinterpret_cast<zc *>(xs_raw);   // ns x nrhs
    const int k = nodes[blockIdx.x];
    if (!(T.sn_flags[k] & SNF_OWN_DIAG)) return;           // x_k is solved by the owner of the diagonal block
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;
    const int lda = T.sn_dlda[k];
    const zc *A = reinterpret_cast<const zc *>(T.val) + T.sn_dptr[k];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int idx = tid; idx < ns * nrhs; idx += 256) xs[idx] = x[fst + (idx % ns) + (int64_t) (idx / ns) * ldx];
    __syncthreads();
    const int nblk = (ns + DB - 1) / DB;
    for (int bi = 0; bi < nblk; ++bi) {
        const int jb = (LOWER ? bi : nblk - 1 - bi) * DB;
        const int nb = min(DB, ns - jb);
        // (a) the triangular block: lane i = row jb + i; column values in registers
        {
            const int i = lane;
            const bool rok = i < nb;
            double cr[DB], ci[DB];          // column j of the block, this lane's row
#pragma unroll
            for (int j = 0; j < DB; ++j) {
                const zc v = (rok && j < nb) ? A[jb + i + (size_t) (jb + j) * lda] : make_double2(0.0, 0.0);
                cr[j] = v.x; ci[j] = v.y;
            }
            // 1 / U_ii once per block (the substitution then multiplies: one complex division per row, not one per row and rhs)
            zc dinv = make_double2(1.0, 0.0);
            if (!LOWER) {
                zc d = make_double2(1.0, 0.0);
#pragma unroll
                for (int j = 0; j < DB; ++j) if (i == j) d = make_double2(cr[j], ci[j]);
                if (rok) dinv = z_div(make_double2(1.0, 0.0), d);
            }
            for (int r = wave; r < nrhs; r += 4) {
                zc xv = rok ? xs[jb + i + r * ns] : make_double2(0.0, 0.0);
                if (LOWER) {
#pragma unroll
                    for (int j = 0; j < DB; ++j) {
                        if (j < nb) {      // wave-uniform
                            const zc xj = make_double2(lane_bcast(xv.x, j), lane_bcast(xv.y, j));
                            if (i > j) xv = z_fnma(xv, make_double2(cr[j], ci[j]), xj);
                        }
                    }
                } else {
#pragma unroll
                    for (int jj = 0; jj < DB; ++jj) {
                        const int j = DB - 1 - jj;
                        if (j < nb) {
                            if (i == j) xv = z_mul(xv, dinv);
                            const zc xj = make_double2(lane_bcast(xv.x, j), lane_bcast(xv.y, j));
                            if (i < j) xv = z_fnma(xv, make_double2(cr[j], ci[j]), xj);
                        }
                    }
                }
                if (rok) xs[jb + i + r * ns] = xv;
            }
        }
        __syncthreads();
        // (b) the rest of the rows: below the block (lower) / above it (upper)
        {
            const int r0 = LOWER ? jb + nb : 0, r1 = LOWER ? ns : jb;
            for (int idx = tid; idx < (r1 - r0) * nrhs; idx += 256) {
                const int i = r0 + idx % (r1 - r0), r = idx / (r1 - r0);
                zc acc = xs[i + r * ns];
                const zc *Ar = A + i + (size_t) jb * lda;
#pragma unroll 8
                for (int j = 0; j < nb; ++j) acc = z_fnma(acc, Ar[(size_t) j * lda], xs[jb + j + r * ns]);
                xs[i + r * ns] = acc;
            }
        }
        __syncthreads();
    }
    for (int idx = tid; idx < ns * nrhs; idx += 256) x[fst + (idx % ns) + (int64_t) (idx / ns) * ldx] = xs[idx];
}

// The diagonal solve of supernodes of at most 64 columns (every level at the supernode width the complex path runs best with) by ONE
// WAVE per supernode in registers: lane = row; the columns of the triangle stream through eight-column register batches -- their loads
// do not depend on x, the next batch is in flight while the current one is applied -- and every step is a v_readlane broadcast of the
// solved entry plus one complex multiply-add per lane.  No LDS, no barrier (the blocked kernel above spends 18-21 us per launch in four
// barriers and three dependent load phases for the same 64 x 64 triangle).  Upper: the reciprocals of the diagonal are taken once, in parallel.
template <bool LOWER>
__global__ __launch_bounds__(256) void kz_solve_diag_wave(DevTables T, const int *__restrict__ nodes, int nn, zc *__restrict__ x, int64_t ldx, int nrhs)
{
    const int bi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bi >= nn) return;
    const int k = nodes[bi];
    if (!(T.sn_flags[k] & SNF_OWN_DIAG)) return;           // x_k is solved by the owner of the diagonal block
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;   // <= 64
    const int lda = T.sn_dlda[k];
    const zc *A = reinterpret_cast<const zc *>(T.val) + T.sn_dptr[k];
    const int lane = threadIdx.x & 63;
    const bool rok = lane < ns;
    const zc zero = make_double2(0.0, 0.0);
    zc dinv = make_double2(1.0, 0.0);
    if (!LOWER && rok) dinv = z_div(make_double2(1.0, 0.0), A[lane + (size_t) lane * lda]);
    const int nbat = (ns + 7) >> 3;
    // column batch t (processing order): columns 8 t .. 8 t + 7 (lower, ascending) or the mirror image (upper, descending)
    auto load_batch = [&](int t, zc (&col)[8]) {
        const int j0 = LOWER ? 8 * t : 8 * (nbat - 1 - t);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + u;
            col[u] = (rok && j < ns && (LOWER ? lane > j : lane < j)) ? A[lane + (size_t) j * lda] : zero;   // zero where the row must not change
        }
    };
    for (int r = 0; r < nrhs; ++r) {
        zc b = rok ? x[fst + lane + (int64_t) r * ldx] : zero;
        zc cur[8], nxt[8];
        load_batch(0, cur);
        for (int t = 0; t < nbat; ++t) {
            if (t + 1 < nbat) load_batch(t + 1, nxt);
            const int j0 = LOWER ? 8 * t : 8 * (nbat - 1 - t);
#pragma unroll
            for (int uu = 0; uu < 8; ++uu) {
                const int u = LOWER ? uu : 7 - uu;
                const int j = j0 + u;
                if (j < ns) {      // wave-uniform
                    if (!LOWER && lane == j) b = z_mul(b, dinv);
                    const zc xj = make_double2(lane_bcast(b.x, j), lane_bcast(b.y, j));
                    b = z_fnma(b, cur[u], xj);
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) cur[u] = nxt[u];
        }
        if (rok) x[fst + lane + (int64_t) r * ldx] = b;
    }
}

__global__ __launch_bounds__(256) void kz_fwd_update(DevTables T, const int *__restrict__ nodes, const int *__restrict__ prefix,
                                                     int nn, zc *__restrict__ x, int64_t ldx, int nrhs)
{
    extern __shared__ double xk_raw[];
    zc *xk = reinterpret_cast<zc *>(xk_raw);
    const int ni = find_node_wave(prefix, nn, blockIdx.x);
    const int k = nodes[ni];
    const int strip = blockIdx.x - prefix[ni];
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;
    const int lda = T.sn_nsupr[k];
    const int row = T.sn_ldiag[k] + strip * 256 + threadIdx.x;
    const bool rvalid = row < lda;
    const zc *L = reinterpret_cast<const zc *>(T.val) + T.sn_lval[k] + (rvalid ? row : T.sn_ldiag[k]);
    const int grow = rvalid ? T.lrow[T.sn_lrow[k] + row] : 0;           // flat map: global row of every slot row
    // the first eight columns of the row go in flight before x_k is staged (they do not depend on x): one round trip less per workgroup
    zc l0[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) l0[u] = (rvalid && u < ns) ? L[(size_t) u * lda] : make_double2(0.0, 0.0);
    for (int idx = threadIdx.x; idx < ns * nrhs; idx += 256) xk[idx] = x[fst + (idx % ns) + (int64_t) (idx / ns) * ldx];
    __syncthreads();
    if (!rvalid) return;
    for (int r = 0; r < nrhs; ++r) {
        const zc *xq = xk + r * ns;
        zc acc0 = make_double2(0.0, 0.0), acc1 = acc0;
#pragma unroll
        for (int u = 0; u < 8; ++u) { if (u & 1) acc1 = z_fnma(acc1, l0[u], xq[min(u, ns - 1)]); else acc0 = z_fnma(acc0, l0[u], xq[min(u, ns - 1)]); }   // l0 is zero past ns
        int kk = 8;
        for (; kk + 8 <= ns; kk += 8) {      // batches of eight independent 16-byte loads
            zc lv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) lv[u] = L[(size_t) (kk + u) * lda];
#pragma unroll
            for (int u = 0; u < 8; ++u) { if (u & 1) acc1 = z_fnma(acc1, lv[u], xq[kk + u]); else acc0 = z_fnma(acc0, lv[u], xq[kk + u]); }
        }
        for (; kk < ns; ++kk) acc0 = z_fnma(acc0, L[(size_t) kk * lda], xq[kk]);
        zc *d = x + grow + (int64_t) r * ldx;          // acc = -sum
        unsafeAtomicAdd(&d->x, acc0.x + acc1.x);
        unsafeAtomicAdd(&d->y, acc0.y + acc1.y);
    }
}

__global__ __launch_bounds__(256) void kz_bwd_update(DevTables T, const int *__restrict__ nodes, const int *__restrict__ prefix,
                                                     int nn, zc *__restrict__ x, int64_t ldx, int nrhs)
{
    __shared__ int s_cp[64], s_ld[64], s_gc[64];
    __shared__ double s_rr[4][64], s_ri[4][64];
    const int ni = find_node_wave(prefix, nn, blockIdx.x);
    const int k = nodes[ni];
    const int chunk = blockIdx.x - prefix[ni];
    const int fst = T.xsup[k], klst = T.xsup[k + 1], ns = klst - fst;
    const int ncol = min(64, T.sn_ncolu[k] - chunk * 64);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < 64) {
        int cp = 0, ld = ns, gc = 0;
        if (tid < ncol) {     // flat per-non-empty-column maps (value offset, leading zeros, global column): no search over the block descriptors
            const int64_t ci = T.sn_ucol[k] + chunk * 64 + tid;
            ld = T.ucol_ld[ci]; cp = T.ucol_cp[ci]; gc = T.ucol_gc[ci];
        }
        s_cp[tid] = cp; s_ld[tid] = ld; s_gc[tid] = gc;
    }
    __syncthreads();
    const zc *Uv = reinterpret_cast<const zc *>(T.val) + T.sn_uval[k];
    for (int r = 0; r < nrhs; ++r) {
        for (int rb = 0; rb < ns; rb += 64) {
            const int i = rb + lane;
            zc acc = make_double2(0.0, 0.0);
            for (int c = wave; c < ncol; c += 4) {
                const int ld = s_ld[c];
                if (i < ns && i >= ld) acc = z_fnma(acc, Uv[s_cp[c] + (i - ld)], x[s_gc[c] + (int64_t) r * ldx]);   // -sum
            }
            s_rr[wave][lane] = acc.x; s_ri[wave][lane] = acc.y;
            __syncthreads();
            if (wave == 0 && i < ns) {
                const double sr = s_rr[0][lane] + s_rr[1][lane] + s_rr[2][lane] + s_rr[3][lane];
                const double si = s_ri[0][lane] + s_ri[1][lane] + s_ri[2][lane] + s_ri[3][lane];
                zc *d = x + fst + i + (int64_t) r * ldx;
                if (sr != 0.0) unsafeAtomicAdd(&d->x, sr);
                if (si != 0.0) unsafeAtomicAdd(&d->y, si);
            }
            __syncthreads();
        }
    }
}

// ---- fused links of the complex16 sweeps (round 5; 1 x 1 x 1 grids, every supernode <= 64 columns) -------------------------------------------------------
// The level-set form above pays two dependent launches per level and sweep (diagonal solves, updates): 212 launches of ~15 us for the 53 levels of the 2-D
// configuration, 0.10 of the HBM peak.  ONE launch per level and sweep instead, out of place like the double path's links (x = accumulators, w = solved blocks
// forward; w = accumulators, x = final solution backward):
//   forward  unit (k, 256-row strip): EVERY strip's workgroup solves y_k = inv(L_kk) x_k itself -- one wave, in registers, the whole triangle loaded in one
//            round trip (zsolve64_wave) -- while the other waves already have the first columns of their panel rows in flight; strip 0 stores y_k to w;
//            then x[rows] -= L(rows, k) y_k as kz_fwd_update.  (A supernode without off-diagonal rows still gets one unit: LevelSched::zffu_prefix.)
//   backward unit (k, 64-column chunk): w_k -= U(k, chunk) x[columns] as kz_bwd_update (fp64 atomics), then every wave drains, ONE lane releases at agent
//            scope and takes a ticket of supernode k; the workgroup that takes the LAST ticket acquires, reads the completed w_k and solves
//            x_k = inv(U_kk) w_k (and resets the ticket counter for the next sweep).  Few workgroups per level here: the agent-scope hand-off that was too
//            expensive for the double path at 100^3 (NOTEBOOK.md section 5) costs less than the launch it replaces.
template <bool LOWER>
__device__ __forceinline__ zc zsolve64_wave(const zc *A, int lda, int ns, int lane, zc b)
{   // one wave: b = row `lane` of the right-hand side; returns row `lane` of inv(L) b (unit lower) or inv(U) b
    const bool rok = lane < ns;
    const zc zero = make_double2(0.0, 0.0);
    zc dinv = make_double2(1.0, 0.0);
    if (!LOWER && rok) dinv = z_div(make_double2(1.0, 0.0), A[lane + (size_t) lane * lda]);
    // the whole triangle in ONE round trip: row `lane` of every column, in registers (the substitution itself is ~1 us; eight dependent batches were ~8)
    zc col[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) col[j] = (rok && j < ns && (LOWER ? lane > j : lane < j)) ? A[lane + (size_t) j * lda] : zero;
#pragma unroll
    for (int jj = 0; jj < 64; ++jj) {
        const int j = LOWER ? jj : 63 - jj;
        if (j < ns) {      // wave-uniform
            if (!LOWER && lane == j) b = z_mul(b, dinv);
            const zc xj = make_double2(lane_bcast(b.x, j), lane_bcast(b.y, j));
            b = z_fnma(b, col[j], xj);
        }
    }
    return b;
}

// Wave `wave` of a 64-column chunk of U(k, :) on a latency-bound level: its sixteen columns (wave, wave + 4, ...) with ALL their loads in flight at once --
// skyline value of row i and the solved x of the column -- instead of sixteen dependent iterations (kz_bwd_fused 25 -> 19 us per level; the level-set
// kernel of the wide levels keeps the loop: at 142 registers it loses more occupancy than it gains).  Returns -sum_c U(i, c) x[c] of those columns.
__device__ __forceinline__ zc z_bwd_cols(const zc *Uv, const zc *xr, const int *s_cp, const int *s_ld, const int *s_gc, int ncol, int wave, int i, int ns)
{
    zc uv[16], xv[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int c = wave + 4 * u;
        const bool on = c < ncol && i < ns && i >= s_ld[c];        // s_* hold neutral entries past ncol
        uv[u] = Uv[on ? s_cp[c] + (i - s_ld[c]) : 0];               // unconditional loads from always-valid addresses; `on` applied below
        xv[u] = xr[on ? s_gc[c] : 0];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int c = wave + 4 * u;
        if (!(c < ncol && i < ns && i >= s_ld[c])) uv[u] = make_double2(0.0, 0.0);
    }
    zc acc0 = make_double2(0.0, 0.0), acc1 = acc0;
#pragma unroll
    for (int u = 0; u < 16; ++u) { if (u & 1) acc1 = z_fnma(acc1, uv[u], xv[u]); else acc0 = z_fnma(acc0, uv[u], xv[u]); }
    return make_double2(acc0.x + acc1.x, acc0.y + acc1.y);
}

constexpr int ZFW = 8;     // panel columns per batch of a thread's loads in the fused forward unit
__global__ __launch_bounds__(256) void kz_fwd_fused(DevTables T, const int *__restrict__ nodes, const int *__restrict__ prefix, int nn,
                                                    zc *__restrict__ x, zc *__restrict__ w, int64_t ldx, int nrhs)
{
    extern __shared__ double xk_raw[];
    zc *xk = reinterpret_cast<zc *>(xk_raw);           // ns x nrhs: y_k
    const int ni = find_node_wave(prefix, nn, blockIdx.x);
    const int k = nodes[ni];
    const int strip = blockIdx.x - prefix[ni];
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;   // <= 64
    const int lda = T.sn_nsupr[k];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = T.sn_ldiag[k] + strip * 256 + tid;
    const bool rvalid = row < lda;
    const zc *V = reinterpret_cast<const zc *>(T.val);
    const zc *L = V + T.sn_lval[k] + (rvalid ? row : T.sn_ldiag[k]);
    const int grow = rvalid ? T.lrow[T.sn_lrow[k] + row] : 0;
    zc l0[ZFW];
#pragma unroll
    for (int u = 0; u < ZFW; ++u) l0[u] = (rvalid && u < ns) ? L[(size_t) u * lda] : make_double2(0.0, 0.0);
    if (wave == 0) {       // y_k = inv(L_kk) x_k, every right-hand side
        const zc *A = V + T.sn_dptr[k];
        const int ldd = T.sn_dlda[k];
        for (int r = 0; r < nrhs; ++r) {
            zc b = lane < ns ? x[fst + lane + (int64_t) r * ldx] : make_double2(0.0, 0.0);
            b = zsolve64_wave<true>(A, ldd, ns, lane, b);
            if (lane < ns) { xk[lane + r * ns] = b; if (strip == 0) w[fst + lane + (int64_t) r * ldx] = b; }
        }
    }
    __syncthreads();
    if (!rvalid) return;
    for (int r = 0; r < nrhs; ++r) {
        const zc *xq = xk + r * ns;
        zc acc0 = make_double2(0.0, 0.0), acc1 = acc0;
#pragma unroll
        for (int u = 0; u < ZFW; ++u) { if (u & 1) acc1 = z_fnma(acc1, l0[u], xq[min(u, ns - 1)]); else acc0 = z_fnma(acc0, l0[u], xq[min(u, ns - 1)]); }   // l0 is zero past ns
        int kk = ZFW;
        for (; kk + ZFW <= ns; kk += ZFW) {
            zc lv[ZFW];
#pragma unroll
            for (int u = 0; u < ZFW; ++u) lv[u] = L[(size_t) (kk + u) * lda];
#pragma unroll
            for (int u = 0; u < ZFW; ++u) { if (u & 1) acc1 = z_fnma(acc1, lv[u], xq[kk + u]); else acc0 = z_fnma(acc0, lv[u], xq[kk + u]); }
        }
        for (; kk < ns; ++kk) acc0 = z_fnma(acc0, L[(size_t) kk * lda], xq[kk]);
        zc *d = x + grow + (int64_t) r * ldx;          // acc = -sum
        unsafeAtomicAdd(&d->x, acc0.x + acc1.x);
        unsafeAtomicAdd(&d->y, acc0.y + acc1.y);
    }
}

__global__ __launch_bounds__(256) void kz_bwd_fused(DevTables T, const int *__restrict__ nodes, const int *__restrict__ prefix, int nn,
                                                    zc *__restrict__ x, zc *__restrict__ w, int64_t ldx, int nrhs, int *__restrict__ tickets)
{
    __shared__ int s_cp[64], s_ld[64], s_gc[64];
    __shared__ double s_rr[4][64], s_ri[4][64];
    __shared__ int s_last;
    const int ni = find_node_wave(prefix, nn, blockIdx.x);
    const int k = nodes[ni];
    const int chunk = blockIdx.x - prefix[ni];
    const int nunits = prefix[ni + 1] - prefix[ni];
    const int fst = T.xsup[k], ns = T.xsup[k + 1] - fst;     // <= 64
    const int ncol = max(0, min(64, T.sn_ncolu[k] - chunk * 64));
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < 64) {
        int cp = 0, ld = ns, gc = 0;
        if (tid < ncol) {
            const int64_t ci = T.sn_ucol[k] + chunk * 64 + tid;
            ld = T.ucol_ld[ci]; cp = T.ucol_cp[ci]; gc = T.ucol_gc[ci];
        }
        s_cp[tid] = cp; s_ld[tid] = ld; s_gc[tid] = gc;
    }
    __syncthreads();
    const zc *V = reinterpret_cast<const zc *>(T.val);
    const zc *Uv = V + T.sn_uval[k];
    if (ncol > 0)
        for (int r = 0; r < nrhs; ++r) {
            const zc acc = z_bwd_cols(Uv, x + (int64_t) r * ldx, s_cp, s_ld, s_gc, ncol, wave, lane, ns);   // -sum
            s_rr[wave][lane] = acc.x; s_ri[wave][lane] = acc.y;
            __syncthreads();
            if (wave == 0 && lane < ns) {
                const double sr = s_rr[0][lane] + s_rr[1][lane] + s_rr[2][lane] + s_rr[3][lane];
                const double si = s_ri[0][lane] + s_ri[1][lane] + s_ri[2][lane] + s_ri[3][lane];
                zc *d = w + fst + lane + (int64_t) r * ldx;
                if (sr != 0.0) unsafeAtomicAdd(&d->x, sr);
                if (si != 0.0) unsafeAtomicAdd(&d->y, si);
            }
            __syncthreads();
        }
    // ticket of supernode k: every wave's atomics are complete (release at agent scope) before the counter moves
    __atomic_thread_fence(__ATOMIC_RELEASE);
    __syncthreads();
    if (tid == 0) {
        const int old = __hip_atomic_fetch_add(&tickets[k], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (old == nunits - 1);
        if (s_last) __hip_atomic_store(&tickets[k], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // for the next sweep
    }
    __syncthreads();
    if (!s_last || wave != 0) return;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const zc *A = V + T.sn_dptr[k];
    const int ldd = T.sn_dlda[k];
    for (int r = 0; r < nrhs; ++r) {
        zc b = make_double2(0.0, 0.0);
        if (lane < ns) {    // completed by other workgroups' atomics: read past this CU's caches
            zc *p = w + fst + lane + (int64_t) r * ldx;
            b.x = __hip_atomic_load(&p->x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            b.y = __hip_atomic_load(&p->y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        b = zsolve64_wave<false>(A, ldd, ns, lane, b);
        if (lane < ns) x[fst + lane + (int64_t) r * ldx] = b;
    }
}

__global__ void kz_scatter_values(zc *__restrict__ val, const int64_t *__restrict__ pos, const zc *__restrict__ a, int64_t nnz)
{
    int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nnz) val[pos[e]] = a[e];
}
