// sluamd_rkernels.inc -- residual / backward-error kernels of the TRANSPOSED and CONJUGATE-TRANSPOSED refinement (sluamd_trefine.cpp), included by
// sluamd_kernels.hip behind sluamd_zkernels.inc (zc).  The twins of k_rfs_residual / k_zrfs_residual over the transposed index of the attached CSR matrix:
// tcp[n + 1] column pointers, and per entry in column order (rows ascending inside a column: a fixed summation order, results repeat run to run) tri[e] its
// row and tpos[e] its position in the CSR value array.  The values are NOT copied: a = av[tpos[e]], so whatever rewrites or scales the attached values in
// place (sluamd_[dz]UpdateValues, sluamd_[dz]Equilibrate) is seen by the next pass.
// One thread per column j of A = row j of op(A): r_j = b_j - sum_e op(a_e) x[tri[e]] stored permuted (r_perm[perm_c[j]] = r_j: A^T d = r is
// A1^T (Pc d) = Pc r on the factors of A1 = Pc A Pc^T), temp_j = sum_e |a_e| |x| + |b_j| (complex16: abs1(z) = |re| + |im|, which the conjugate leaves
// alone), q_j with the SAFE1 / SAFE2 guards, then the wave, workgroup and integer atomicMax reduction of the untransposed kernels.
// HBM-bound, with one more dependent gather than the CSR pass: 8 B of index + a scattered value (a 64 B line at worst) per nonzero; a refinement step reads
// the factors beside it, three orders of magnitude more, so the index trades SpMV speed for values that cannot go stale.
__global__ __launch_bounds__(256) void k_rfs_residual_t(int n, const int *__restrict__ tcp, const int *__restrict__ tri, const int *__restrict__ tpos,
                                                        const double *__restrict__ av, const double *__restrict__ x,
                                                        const double *__restrict__ b, const int *__restrict__ pc,
                                                        double *__restrict__ r_perm, unsigned long long *__restrict__ s_out,
                                                        double safe1, double safe2)
{
    __shared__ double red[4];
    const int j = blockIdx.x * 256 + threadIdx.x;
    double q = 0.0;
    if (j < n) {
        double ax = 0.0, t = 0.0;
        for (int e = tcp[j]; e < tcp[j + 1]; ++e) {
            const double a = av[tpos[e]], xv = x[tri[e]];
            ax += a * xv;
            t += fabs(a) * fabs(xv);
        }
        const double r = b[j] - ax;
        t += fabs(b[j]);
        r_perm[pc[j]] = r;
        if (t > safe2) q = fabs(r) / t;
        else if (t != 0.0) q = (safe1 + fabs(r)) / t;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q = fmax(q, __shfl_xor(q, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
        q = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        atomicMax(s_out, (unsigned long long) __double_as_longlong(q));
    }
}

// complex16; CONJ: op(a) = conj(a) (A^H x = b)
template <bool CONJ>
__global__ __launch_bounds__(256) void kz_rfs_residual_t(int n, const int *__restrict__ tcp, const int *__restrict__ tri, const int *__restrict__ tpos,
                                                         const zc *__restrict__ av, const zc *__restrict__ x,
                                                         const zc *__restrict__ b, const int *__restrict__ pc,
                                                         zc *__restrict__ r_perm, unsigned long long *__restrict__ s_out,
                                                         double safe1, double safe2)
{
    __shared__ double red[4];
    const int j = blockIdx.x * 256 + threadIdx.x;
    double q = 0.0;
    if (j < n) {
        double axr = 0.0, axi = 0.0, t = 0.0;
        for (int e = tcp[j]; e < tcp[j + 1]; ++e) {
            zc a = av[tpos[e]];
            const zc xv = x[tri[e]];
            if (CONJ) a.y = -a.y;
            axr += a.x * xv.x - a.y * xv.y;
            axi += a.x * xv.y + a.y * xv.x;
            t += (fabs(a.x) + fabs(a.y)) * (fabs(xv.x) + fabs(xv.y));
        }
        const zc bj = b[j];
        const zc r = make_double2(bj.x - axr, bj.y - axi);
        t += fabs(bj.x) + fabs(bj.y);
        r_perm[pc[j]] = r;
        const double ar = fabs(r.x) + fabs(r.y);
        if (t > safe2) q = ar / t;
        else if (t != 0.0) q = (safe1 + ar) / t;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q = fmax(q, __shfl_xor(q, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
        q = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        atomicMax(s_out, (unsigned long long) __double_as_longlong(q));
    }
}
