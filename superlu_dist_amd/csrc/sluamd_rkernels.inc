// sluamd_rkernels.inc -- the kernels of iterative refinement (pdgsrfs3d, SRC/double/pdgsrfs.c:345-510; pzgsrfs3d, SRC/complex16/pzgsrfs.c:365-514), written once
// for double and complex16, A x = b / A^T x = b / A^H x = b, one matrix and batches.  Included by sluamd_kernels.hip (k_rfs_residual, k_rfs_update behind
// eng::rfs_residual / eng::rfs_update), by sluamd_bkernels.inc (k_batch_residual, k_batch_update call rfs_row / rfs_add) and by sluamd_mkernels.inc (the block
// kernels call rfs_term / rfs_quot / rfs_block_max / rfs_add): everything here is a template or
// forced inline, V = double or double2 {x = re, y = im}.
//
// One pass over the matrix does both of the reference's p[dz]gsmv calls (abs = 0 and abs = 1): the residual r = b - op(A) x, stored permuted by the caller
// (r_perm[perm_c[i]] = r_i: the right-hand side of the triangular solves on Pc A Pc^T; A^T d = r is A1^T (Pc d) = Pc r, the same permutation), the weight
// temp_i = sum_j |a_ij| |x_j| + |b_i| (complex16: abs1(z) = |re| + |im|, slud_z_abs1, which the conjugate leaves alone) and the componentwise backward
// error max_i |r_i| / temp_i with the SAFE1 / SAFE2 guards (pdgsrfs.c:463-469, pzgsrfs.c:466-471).
// A row of op(A) is the entries [e0, e1) of
//   the attached CSR itself (POS = false):  a = av[e],        x index ci[e]                     12 B (complex16 20 B) per nonzero, HBM-bound
//   its transposed index (POS = true):      a = av[tpos[e]],  x index tri[e]                    one more dependent gather: 8 B of index + a scattered value
// The transposed index (tcp[n + 1] column pointers; per entry in column order, rows ascending inside a column -- a fixed summation order, results repeat run to
// run -- tri[e] its row and tpos[e] its position in the CSR value array) copies NO values, so whatever rewrites or scales the attached values in place
// (sluamd_[dz]UpdateValues, sluamd_[dz]Equilibrate) is seen by the next pass.  A refinement step reads the factors beside either pass, three orders of
// magnitude more.
// The expressions below and their operand order are what every form computes: the compiler contracts them into multiply-adds, a reshaped expression can
// round differently, and "a batch is bitwise one matrix alone" holds because the batch kernels call this text.
template <bool CONJ> __device__ __forceinline__ double rfs_op(double a) { return a; }
template <bool CONJ> __device__ __forceinline__ double2 rfs_op(double2 a) { if (CONJ) a.y = -a.y; return a; }
__device__ __forceinline__ void rfs_mad(double &acc, double a, double xv) { acc += a * xv; }
__device__ __forceinline__ void rfs_mad(double2 &acc, double2 a, double2 xv) { acc.x += a.x * xv.x - a.y * xv.y; acc.y += a.x * xv.y + a.y * xv.x; }
__device__ __forceinline__ double rfs_abs1(double v) { return fabs(v); }
__device__ __forceinline__ double rfs_abs1(double2 v) { return fabs(v.x) + fabs(v.y); }
__device__ __forceinline__ double rfs_sub(double b, double ax) { return b - ax; }
__device__ __forceinline__ double2 rfs_sub(double2 b, double2 ax) { return make_double2(b.x - ax.x, b.y - ax.y); }
__device__ __forceinline__ void rfs_add(double &v, double d) { v += d; }
__device__ __forceinline__ void rfs_add(double2 &v, double2 d) { v.x += d.x; v.y += d.y; }

// The two halves of a row, shared by the column form (rfs_row) and the block form (k_rfs_residual_block, sluamd_mkernels.inc, one pair of accumulators per
// column): one entry into (ax, t), and the end of the row -- b last, then the three-branch quotient
template <class V> __device__ __forceinline__ void rfs_term(V &ax, double &t, const V a, const V xv)
{
    rfs_mad(ax, a, xv);
    t += rfs_abs1(a) * rfs_abs1(xv);
}
// (rfs_ratio: the end of the row for a residual r that is already formed -- the extra-precise pass, sluamd_xkernels.inc, rounds its own)
template <class V> __device__ __forceinline__ double rfs_ratio(const V r, double t, const V bval, double safe1, double safe2)
{
    t += rfs_abs1(bval);
    const double ar = rfs_abs1(r);
    if (t > safe2) return ar / t;
    if (t != 0.0) return (safe1 + ar) / t;
    return 0.0;
}
template <class V> __device__ __forceinline__ double rfs_quot(const V ax, double t, const V bval, double safe1, double safe2, V &r)
{
    r = rfs_sub(bval, ax);
    return rfs_ratio(r, t, bval, safe1, safe2);
}

// r = bval - sum_e op(a_e) x[xi[e]] over the entries [e0, e1); returns the row's backward error q (0 for a row whose weight is 0).  ap (POS only): the
// position of entry e in av
template <class V, bool CONJ, bool POS>
__device__ __forceinline__ double rfs_row(int e0, int e1, const int *__restrict__ xi, const int *__restrict__ ap, const V *__restrict__ av,
                                          const V *__restrict__ x, V bval, double safe1, double safe2, V &r)
{
    V ax = V();
    double t = 0.0;
    for (int e = e0; e < e1; ++e) {
        const V a = rfs_op<CONJ>(av[POS ? ap[e] : e]), xv = x[xi[e]];
        rfs_term(ax, t, a, xv);
    }
    return rfs_quot(ax, t, bval, safe1, safe2, r);
}

// max of q over the workgroup (256 threads, all of them call it) into *s_out: wave, LDS, ONE integer atomicMax on the bit pattern -- non-negative doubles
// order like their bit patterns, so the result does not depend on the order of the workgroups
__device__ __forceinline__ void rfs_block_max(double q, unsigned long long *__restrict__ s_out)
{
    __shared__ double red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q = fmax(q, __shfl_xor(q, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
        q = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        atomicMax(s_out, (unsigned long long) __double_as_longlong(q));
    }
}

// one thread per row i of op(A); TRANS: (ptr, idx, pos) = the transposed index, else the CSR (pos unused)
template <class V, bool TRANS, bool CONJ>
__global__ __launch_bounds__(256) void k_rfs_residual(int n, const int *__restrict__ ptr, const int *__restrict__ idx, const int *__restrict__ pos,
                                                      const V *__restrict__ av, const V *__restrict__ x, const V *__restrict__ b,
                                                      const int *__restrict__ pc, V *__restrict__ r_perm, unsigned long long *__restrict__ s_out,
                                                      double safe1, double safe2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    double q = 0.0;
    if (i < n) {
        V r;
        q = rfs_row<V, CONJ, TRANS>(ptr[i], ptr[i + 1], idx, pos, av, x, b[i], safe1, safe2, r);
        r_perm[pc[i]] = r;
    }
    rfs_block_max(q, s_out);
}

// x_i += dx_perm[perm_c[i]] (pdgsrfs.c:490-496 after the solve), one value per thread
template <class V>
__global__ __launch_bounds__(256) void k_rfs_update(int n, const int *__restrict__ pc, const V *__restrict__ dx_perm, V *__restrict__ x)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        V v = x[i];
        rfs_add(v, dx_perm[pc[i]]);
        x[i] = v;
    }
}
