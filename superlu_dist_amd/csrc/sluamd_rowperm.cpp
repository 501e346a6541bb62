// sluamd_rowperm.cpp -- RowPerm = LargeDiag_MC64: the row permutation that maximises the product of the diagonal moduli, and the scalings that come with it
// (the role of dldperm_dist / mc64ad_dist at pdgssvx3d.c:779-870; written from Duff & Koster, SIAM J. Matrix Anal. Appl. 22 (2001), not from that code).
// Contract: include/superlu_dist_amd.h.  A hybrid: the device computes the logarithmic costs, the initial duals and a first matching by proposal rounds on the
// tight entries (sluamd_pkernels.inc); the host finds a shortest augmenting path for every row the rounds left unmatched (sluamd_match.cpp).
// A file of its own: the CPU test build (oracle/Makefile) links a fixed list of the host sources against a CPU restatement of the older kernels only, so no
// file of that list may reference these kernels (eng::rp_*).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "sluamd_internal.h"
#include "sluamd_match.h"

using namespace sluamd;

namespace {

struct OwnStream { hipStream_t s = nullptr; ~OwnStream() { if (s) hipStreamDestroy(s); } };

double exp2_exact(double x) { return x == std::floor(x) && std::fabs(x) < 1000.0 ? std::ldexp(1.0, (int) x) : std::exp2(x); }

int large_diag(int device, int64_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const void *nzval, sluamd_int_t *perm_r, double *r, double *c,
               sluamd_rowperm_t *out, bool z, const char *who)
{
    const std::string me = std::string(who) + ": ";
    if (n < 0 || n >= INT32_MAX) { set_error(me + "n must be in [0, 2^31 - 1)"); return SLUAMD_EINVAL; }      // (indices are sluamd_int_t: rowptr[n] < 2^31 with it)
    if (!rowptr || !perm_r || !out || (n > 0 && rowptr[n] > 0 && (!colind || !nzval))) { set_error(me + "null argument"); return SLUAMD_EINVAL; }
    if (rowptr[0] != 0) { set_error(me + "rowptr[0] must be 0 (CSR, 0-based)"); return SLUAMD_EINVAL; }
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) { set_error(me + "rowptr is not ascending"); return SLUAMD_EINVAL; }
    const int64_t nnz = rowptr[n];
    for (int64_t e = 0; e < nnz; ++e)
        if (colind[e] < 0 || colind[e] >= n) { set_error(me + "column index outside [0, n)"); return SLUAMD_EINVAL; }
    *out = sluamd_rowperm_t{0, 0, 0, 0};
    if (n == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error(me + "no HIP device visible; the matching's device phase has no CPU fallback"); return SLUAMD_ENODEVICE; }
    if (device >= ndev) { set_error(me + "no such device"); return SLUAMD_EINVAL; }
    if (device >= 0) HIPCHK(hipSetDevice(device));
    const char *env = getenv("SLUAMD_ROWPERM_HOST");
    const bool host_only = env && atoi(env) != 0;
    env = getenv("SLUAMD_ROWPERM_ROUNDS");
    const int max_rounds = env && atoi(env) >= 0 ? atoi(env) : 32;

    // SLUAMD_ROWPERM_VERBOSE=1: one line of per-phase wall-clock times on stderr (scripts/ab_rowperm.py reads it)
    env = getenv("SLUAMD_ROWPERM_VERBOSE");
    const bool verbose = env && atoi(env) != 0;
    double t_ms[5] = {0, 0, 0, 0, 0};                                 // upload + costs + duals | rounds | download | host paths | scalings
    auto now = []() { return std::chrono::steady_clock::now(); };
    auto lap = [&](int k, std::chrono::steady_clock::time_point &t0) { const auto t1 = now(); t_ms[k] += std::chrono::duration<double, std::milli>(t1 - t0).count(); t0 = t1; };
    auto t0 = now();

    DevBag D;                   // every device allocation of this call, freed on any way out
    D.device = device;
    OwnStream own;
    HIPCHK(hipStreamCreate(&own.s));
    hipStream_t s = own.s;
    const int ni = (int) n;
    int *d_rp, *d_ci, *d_rowmatch, *d_colmatch, *d_prop, *d_count;
    double *d_av, *d_cmax, *d_cost, *d_u, *d_v;
    int rc;
    if ((rc = D.alloc(&d_rp, (size_t) n + 1, "the matching's copy of A (row pointers)")) || (rc = D.alloc(&d_ci, (size_t) nnz, "the matching's copy of A (column indices)")) ||
        (rc = D.alloc(&d_av, (size_t) nnz * (z ? 2 : 1), "the matching's copy of A (values)")) || (rc = D.alloc(&d_cmax, (size_t) n, "the matching's column maxima")) ||
        (rc = D.alloc(&d_cost, (size_t) nnz, "the matching's costs")) || (rc = D.alloc(&d_u, (size_t) n, "the matching's row duals")) ||
        (rc = D.alloc(&d_v, (size_t) n, "the matching's column duals")) || (rc = D.alloc(&d_rowmatch, (size_t) n, "the matching's row matches")) ||
        (rc = D.alloc(&d_colmatch, (size_t) n, "the matching's column matches")) || (rc = D.alloc(&d_prop, (size_t) n, "the matching's proposals")) ||
        (rc = D.alloc(&d_count, 1, "the matching's counter"))) return rc;
    HIPCHK(hipMemcpyAsync(d_rp, rowptr, sizeof(int) * ((size_t) n + 1), hipMemcpyHostToDevice, s));
    if (nnz) {
        HIPCHK(hipMemcpyAsync(d_ci, colind, sizeof(int) * (size_t) nnz, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_av, nzval, sizeof(double) * (size_t) nnz * (z ? 2 : 1), hipMemcpyHostToDevice, s));
    }
    // costs and the initial duals
    HIPCHK(hipMemsetAsync(d_cmax, 0, sizeof(double) * (size_t) n, s));
    eng::rp_colmax(s, z, ni, nnz, d_rp, d_ci, d_av, d_cmax);
    eng::rp_cost_u(s, z, ni, nnz, d_rp, d_ci, d_av, d_cmax, d_cost, d_u);
    eng::rp_fill_inf(s, n, d_v);
    eng::rp_v(s, ni, nnz, d_rp, d_ci, d_cost, d_u, d_v);
    // proposal rounds on the tight entries; the host reads one counter per round
    eng::rp_fill(s, n, d_rowmatch, -1); eng::rp_fill(s, n, d_colmatch, -1); eng::rp_fill(s, n, d_prop, INT32_MAX);
    HIPCHK(hipMemsetAsync(d_count, 0, sizeof(int), s));
    HIPCHK(hipGetLastError());
    if (verbose) { HIPCHK(hipStreamSynchronize(s)); lap(0, t0); }
    int64_t matched = 0;
    int rounds = 0;
    while (!host_only && rounds < max_rounds && matched < n) {
        eng::rp_propose(s, ni, nnz, d_rp, d_ci, d_cost, d_u, d_v, d_rowmatch, d_colmatch, d_prop);
        eng::rp_accept(s, ni, d_prop, d_rowmatch, d_colmatch, d_count);
        int total = 0;
        HIPCHK(hipMemcpyAsync(&total, d_count, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ++rounds;
        if (total == matched) break;
        matched = total;
    }
    out->rounds = rounds; out->matched_device = matched;
    lap(1, t0);
    std::vector<double> u((size_t) n), v((size_t) n), cmax((size_t) n);
    std::vector<int32_t> rowmatch((size_t) n), colmatch((size_t) n);
    HIPCHK(hipMemcpyAsync(u.data(), d_u, sizeof(double) * (size_t) n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(v.data(), d_v, sizeof(double) * (size_t) n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cmax.data(), d_cmax, sizeof(double) * (size_t) n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(rowmatch.data(), d_rowmatch, sizeof(int) * (size_t) n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(colmatch.data(), d_colmatch, sizeof(int) * (size_t) n, hipMemcpyDeviceToHost, s));
    std::vector<double> cost;
    if (matched < n) {          // the host phase needs the costs; a matching the device completed does not
        cost.resize((size_t) std::max<int64_t>(nnz, 1));
        if (nnz) HIPCHK(hipMemcpyAsync(cost.data(), d_cost, sizeof(double) * (size_t) nnz, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    lap(2, t0);
    int64_t left = 0;
    if (matched < n) left = match_augment(n, rowptr, colind, cost.data(), u.data(), v.data(), rowmatch.data(), colmatch.data(), &out->augmentations);
    lap(3, t0);
    if (left > 0) out->info = (int32_t) left;
    else {
        for (int64_t i = 0; i < n; ++i) perm_r[i] = rowmatch[i];
        if (r) for (int64_t i = 0; i < n; ++i) r[i] = exp2_exact(u[i]);
        if (c) for (int64_t j = 0; j < n; ++j) c[j] = exp2_exact(v[j]) / cmax[j];
    }
    lap(4, t0);
    if (verbose)
        fprintf(stderr, "%s: n %lld nnz %lld | costs+duals %.2f ms | %d rounds %.2f ms | download %.2f ms | host paths %.2f ms | scalings %.2f ms | matched_device %lld augmentations %lld info %d\n",
                who, (long long) n, (long long) nnz, t_ms[0], rounds, t_ms[1], t_ms[2], t_ms[3], t_ms[4], (long long) matched, (long long) out->augmentations, (int) out->info);
    return 0;
}

}  // namespace

extern "C" {

int sluamd_dLargeDiag(int device, int64_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const double *nzval, sluamd_int_t *perm_r, double *r,
                      double *c, sluamd_rowperm_t *out)
{
    return large_diag(device, n, rowptr, colind, nzval, perm_r, r, c, out, false, "sluamd_dLargeDiag");
}

int sluamd_zLargeDiag(int device, int64_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const sluamd_doublecomplex *nzval, sluamd_int_t *perm_r,
                      double *r, double *c, sluamd_rowperm_t *out)
{
    return large_diag(device, n, rowptr, colind, nzval, perm_r, r, c, out, true, "sluamd_zLargeDiag");
}

}  // extern "C"
