/*
 * pddrive3d_amd.c -- plain C driver over the C ABI of libsluamd.so (include/superlu_dist_amd.h), no Python involved:
 * the counterpart of the reference's EXAMPLE/pddrive3d.c for the part of the pipeline this library covers
 * (Equil = NO, RowPerm = NOROWPERM, ColPerm = NATURAL or MY_PERMC, 1 x 1 x 1 grid).
 *
 *   pddrive3d_amd N            7-point Poisson on an N^3 grid (what EXAMPLE/pddrive3d reads as a generated .dat), natural order
 *   pddrive3d_amd file.dat     triplet file, the format dreadtriple.c reads: "m n nnz" then "row col value", 0- or 1-based
 *   pddrive3d_amd file.mtx     MatrixMarket coordinate file (real / integer / pattern; general / symmetric / skew-symmetric), what
 *                              dreadMM.c reads (SRC/double/dreadMM.c: symmetric storage is expanded to the full pattern) -- e.g.
 *                              SuiteSparse audikw_1.mtx (BASELINE.json configs[3]; not shipped: no network)
 * Files are ordered with sluamd_order_nd (nested dissection of the pattern of A + A^T; the generated grid keeps its natural order
 * unless -nd is given).
 *
 * Pipeline: symbolic factorisation (sluamd_dsymbfact) -> device-resident distribution + handle
 * (sluamd_dCreateLUHandleFromSymb) -> sluamd_pdgstrf3d -> sluamd_pdgstrs3d -> sluamd_pdgsrfs3d (IterRefine = SLU_DOUBLE),
 * with xtrue_i = +-1 and b = A xtrue like dGenXtrue_dist / dFillRHS_dist (dutil_dist.c:598).  Prints what pddrive3d
 * prints at the end: ||X - Xtrue||_inf / ||X||_inf, plus the residual and the timings.  Exit code 0 iff residual < 1e-10.
 *
 *   --steps K   after the first solve, K more systems on the SAME pattern (Fact = SamePattern_SameRowPerm): the values are perturbed
 *               deterministically, sluamd_dUpdateValues hands them to the handle (an equilibrated handle reuses R and C), then factor and
 *               solve as before; one "STEP k" line with the residual against the perturbed matrix each, all of them < 1e-10 for exit code 0.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "superlu_dist_amd.h"

#define CHECK(call)                                                                      \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_) { fprintf(stderr, "%s failed (rc=%d): %s\n", #call, rc_, sluamd_last_error()); return 2; } \
    } while (0)

static int poisson3d(int N, int64_t *n_out, int **rp_out, int **ci_out, double **v_out)
{
    const int64_t n = (int64_t) N * N * N;
    int *rp = (int *) malloc(sizeof(int) * (n + 1)), *ci = (int *) malloc(sizeof(int) * 7 * n);
    double *v = (double *) malloc(sizeof(double) * 7 * n);
    if (!rp || !ci || !v) return 1;
    int64_t p = 0;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < N; ++k) {
                const int64_t r = ((int64_t) i * N + j) * N + k;
                rp[r] = (int) p;
                if (i > 0) { ci[p] = (int) (r - (int64_t) N * N); v[p++] = -1.0; }
                if (j > 0) { ci[p] = (int) (r - N); v[p++] = -1.0; }
                if (k > 0) { ci[p] = (int) (r - 1); v[p++] = -1.0; }
                ci[p] = (int) r; v[p++] = 6.0;
                if (k < N - 1) { ci[p] = (int) (r + 1); v[p++] = -1.0; }
                if (j < N - 1) { ci[p] = (int) (r + N); v[p++] = -1.0; }
                if (i < N - 1) { ci[p] = (int) (r + (int64_t) N * N); v[p++] = -1.0; }
            }
    rp[n] = (int) p;
    *n_out = n; *rp_out = rp; *ci_out = ci; *v_out = v;
    return 0;
}

typedef struct { int r, c; double v; } trip_t;
static int cmp_trip(const void *a, const void *b)
{
    const trip_t *x = (const trip_t *) a, *y = (const trip_t *) b;
    if (x->r != y->r) return x->r < y->r ? -1 : 1;
    return x->c < y->c ? -1 : (x->c > y->c);
}

static int read_triplets(const char *path, int64_t *n_out, int **rp_out, int **ci_out, double **v_out)
{
    FILE *f = fopen(path, "r");
    if (!f) return 1;
    long m, n, nnz;
    if (fscanf(f, "%ld %ld %ld", &m, &n, &nnz) != 3 || m != n) { fclose(f); return 1; }
    trip_t *t = (trip_t *) malloc(sizeof(trip_t) * (size_t) nnz);
    int minidx = 1 << 30;
    for (long e = 0; e < nnz; ++e) {
        if (fscanf(f, "%d %d %lf", &t[e].r, &t[e].c, &t[e].v) != 3) { fclose(f); free(t); return 1; }
        if (t[e].r < minidx) minidx = t[e].r;
        if (t[e].c < minidx) minidx = t[e].c;
    }
    fclose(f);
    for (long e = 0; e < nnz; ++e) { t[e].r -= minidx; t[e].c -= minidx; }   /* 0/1-based auto-detect, dreadtriple.c:85-92 */
    qsort(t, (size_t) nnz, sizeof(trip_t), cmp_trip);
    int *rp = (int *) calloc((size_t) n + 1, sizeof(int)), *ci = (int *) malloc(sizeof(int) * (size_t) nnz);
    double *v = (double *) malloc(sizeof(double) * (size_t) nnz);
    for (long e = 0; e < nnz; ++e) { rp[t[e].r + 1]++; ci[e] = t[e].c; v[e] = t[e].v; }
    for (long i = 0; i < n; ++i) rp[i + 1] += rp[i];
    free(t);
    *n_out = n; *rp_out = rp; *ci_out = ci; *v_out = v;
    return 0;
}

/* MatrixMarket coordinate format (what dreadMM_dist reads, SRC/double/dreadMM.c:40-230): banner "%%MatrixMarket matrix coordinate
 * <real|integer|pattern> <general|symmetric|skew-symmetric>", comment lines, "m n nnz", then 1-based "row col [value]" lines;
 * symmetric / skew-symmetric files store one triangle and are expanded; pattern files get value 1 (diagonal: row degree + 1, so
 * that the unpivoted factorisation is defined).  Duplicates are summed. */
static int read_matrix_market(const char *path, int64_t *n_out, int **rp_out, int **ci_out, double **v_out)
{
    FILE *f = fopen(path, "r");
    if (!f) return 1;
    char line[1024], obj[64], fmt[64], field[64], sym[64];
    if (!fgets(line, sizeof line, f) || sscanf(line, "%%%%MatrixMarket %63s %63s %63s %63s", obj, fmt, field, sym) != 4) { fclose(f); return 1; }
    for (char *c = field; *c; ++c) if (*c >= 'A' && *c <= 'Z') *c += 32;
    for (char *c = sym; *c; ++c) if (*c >= 'A' && *c <= 'Z') *c += 32;
    if (strcmp(fmt, "coordinate") || (strcmp(field, "real") && strcmp(field, "integer") && strcmp(field, "pattern"))) { fclose(f); return 1; }
    const int pattern = !strcmp(field, "pattern");
    const int symm = !strcmp(sym, "symmetric"), skew = !strcmp(sym, "skew-symmetric");
    if (!symm && !skew && strcmp(sym, "general")) { fclose(f); return 1; }
    do { if (!fgets(line, sizeof line, f)) { fclose(f); return 1; } } while (line[0] == '%');
    long m, n, nz;
    if (sscanf(line, "%ld %ld %ld", &m, &n, &nz) != 3 || m != n) { fclose(f); return 1; }
    trip_t *t = (trip_t *) malloc(sizeof(trip_t) * (size_t) (2 * nz + 1));
    if (!t) { fclose(f); return 1; }
    long k = 0;
    for (long e = 0; e < nz; ++e) {
        int r, c; double val = 1.0;
        if (pattern ? fscanf(f, "%d %d", &r, &c) != 2 : fscanf(f, "%d %d %lf", &r, &c, &val) != 3) { fclose(f); free(t); return 1; }
        if (r < 1 || r > n || c < 1 || c > n) { fclose(f); free(t); return 1; }
        t[k].r = r - 1; t[k].c = c - 1; t[k].v = val; ++k;
        if ((symm || skew) && r != c) { t[k].r = c - 1; t[k].c = r - 1; t[k].v = skew ? -val : val; ++k; }
    }
    fclose(f);
    qsort(t, (size_t) k, sizeof(trip_t), cmp_trip);
    long u = 0;                                          /* sum duplicates */
    for (long e = 0; e < k; ++e) { if (u && t[u - 1].r == t[e].r && t[u - 1].c == t[e].c) t[u - 1].v += t[e].v; else t[u++] = t[e]; }
    int *rp = (int *) calloc((size_t) n + 1, sizeof(int)), *ci = (int *) malloc(sizeof(int) * (size_t) (u ? u : 1));
    double *v = (double *) malloc(sizeof(double) * (size_t) (u ? u : 1));
    for (long e = 0; e < u; ++e) { rp[t[e].r + 1]++; ci[e] = t[e].c; v[e] = t[e].v; }
    for (long i = 0; i < n; ++i) rp[i + 1] += rp[i];
    if (pattern) for (long i = 0; i < n; ++i) for (int e = rp[i]; e < rp[i + 1]; ++e) if (ci[e] == i) v[e] = (double) (rp[i + 1] - rp[i]) + 1.0;
    free(t);
    *n_out = n; *rp_out = rp; *ci_out = ci; *v_out = v;
    return 0;
}

/* --batch K: K Poisson operators with shifted diagonals, A_k = A + (k / 4) I, as ONE batch (sluamd_dBatch*): one ordering and one symbolic factorisation of
 * one matrix, one plan; per matrix info and the maximum residual over the right-hand side b_k = A_k xtrue */
static int run_batch(int64_t n, const int *rp, const int *ci, const double *v, long K)
{
    const int64_t nnz = rp[n];
    double *vals = (double *) malloc(sizeof(double) * (size_t) (nnz * K)), *B = (double *) malloc(sizeof(double) * (size_t) (n * K));
    double *X = (double *) calloc((size_t) (n * K), sizeof(double));
    int *perm = (int *) malloc(sizeof(int) * n), *permo = (int *) malloc(sizeof(int) * n), *info = (int *) malloc(sizeof(int) * K);
    if (!vals || !B || !X || !perm || !permo || !info) return 2;
    for (long k = 0; k < K; ++k)
        for (int64_t i = 0; i < n; ++i) {
            double s = 0.0;
            for (int e = rp[i]; e < rp[i + 1]; ++e) {
                const double a = v[e] + (ci[e] == i ? 0.25 * (double) k : 0.0);
                vals[k * nnz + e] = a;
                s += a * ((ci[e] % 2) ? 1.0 : -1.0);
            }
            B[k * n + i] = s;
        }
    sluamd_symb_t symb; sluamd_batch_t bt;
    CHECK(sluamd_order_nd(n, rp, ci, 64, perm));
    CHECK(sluamd_dsymbfact(&symb, n, rp, ci, perm, 32, 256, permo));
    CHECK(sluamd_dBatchCreate(&bt, symb, (int32_t) K, rp, ci, vals, nnz, permo, NULL));
    sluamd_symb_free(symb);
    CHECK(sluamd_dBatchFactor(bt, info));
    CHECK(sluamd_dBatchSolve(bt, SLUAMD_NOTRANS, B, n, n, X, n, n, 1, 0, NULL, NULL));
    double worst = 0.0; int bad = 0;
    for (long k = 0; k < K; ++k) {
        double res = 0.0, bn = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            double s = 0.0;
            for (int e = rp[i]; e < rp[i + 1]; ++e) s += vals[k * nnz + e] * X[k * n + ci[e]];
            if (fabs(s - B[k * n + i]) > res) res = fabs(s - B[k * n + i]);
            if (fabs(B[k * n + i]) > bn) bn = fabs(B[k * n + i]);
        }
        res /= bn > 0.0 ? bn : 1.0;
        printf("BATCH matrix %ld: info %d  max residual %.3e\n", k, info[k], res);
        if (res > worst) worst = res;
        if (info[k]) bad = 1;
    }
    sluamd_stats_t st;
    CHECK(sluamd_get_stats(sluamd_BatchHandle(bt), &st));
    printf("BATCH %ld matrices of order %lld: factor %.3f ms  solve %.3f ms  levels %d  max residual %.3e\n", K, (long long) n, st.t_factor_ms, st.t_solve_ms,
           st.num_levels, worst);
    sluamd_BatchDestroy(bt);
    free(vals); free(B); free(X); free(perm); free(permo); free(info);
    if (bad || !(worst < 1e-10)) { printf("FAILED\n"); return 1; }
    printf("PASSED\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s N [-nd] [--equil] [--rowperm] [--refine gmres|extra] [--steps K] | N --batch K | file.dat [--equil] [--rowperm] [--steps K] | file.mtx [--equil] [--rowperm] [--steps K]\n", argv[0]); return 2; }
    if (sluamd_device_count() < 1) { fprintf(stderr, "no HIP device: this library has no CPU fallback\n"); return 3; }
    int64_t n; int *rp, *ci; double *v;
    char *end;
    const long N = strtol(argv[1], &end, 10);
    int use_nd = argc > 2 && !strcmp(argv[2], "-nd");
    int equil = 0;                                            /* --equil: Equil = YES (pdgsequ + pdlaqgs on the device, scaled solve) */
    for (int a = 2; a < argc; ++a) if (!strcmp(argv[a], "--equil")) equil = 1;
    int gmres = 0;                                            /* --refine gmres: the refinement of the first solve is sluamd_pdgsrfs3d_gmres (GMRES preconditioned by the factors) */
    int extra = 0;                                            /* --refine extra: sluamd_pdgsrfs3d_extra (IterRefine = SLU_EXTRA: the residual in twice the working precision) */
    for (int a = 2; a + 1 < argc; ++a) if (!strcmp(argv[a], "--refine")) {
        if (!strcmp(argv[a + 1], "gmres")) gmres = 1;
        else if (!strcmp(argv[a + 1], "extra")) extra = 1;
        else { fprintf(stderr, "--refine takes gmres or extra\n"); return 2; }
    }
    int rowperm = 0;                                          /* --rowperm: RowPerm = LargeDiag_MC64 (matching on the device + host, its scalings, solve in A's ordering) */
    for (int a = 2; a < argc; ++a) if (!strcmp(argv[a], "--rowperm")) rowperm = 1;
    long nsteps = 0;                                          /* --steps K: K same-pattern value updates after the first solve */
    for (int a = 2; a + 1 < argc; ++a) if (!strcmp(argv[a], "--steps")) nsteps = strtol(argv[a + 1], NULL, 10);
    const size_t len = strlen(argv[1]);
    if (*end == '\0' && N > 0) { if (poisson3d((int) N, &n, &rp, &ci, &v)) return 2; }
    else if (len > 4 && !strcmp(argv[1] + len - 4, ".mtx")) {
        if (read_matrix_market(argv[1], &n, &rp, &ci, &v)) { fprintf(stderr, "cannot read MatrixMarket file %s\n", argv[1]); return 2; }
        use_nd = 1;
    } else {
        if (read_triplets(argv[1], &n, &rp, &ci, &v)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        use_nd = 1;
    }
    for (int a = 2; a + 1 < argc; ++a)                         /* --batch K: K shifted operators of the same pattern as one batch */
        if (!strcmp(argv[a], "--batch")) {
            const long K = strtol(argv[a + 1], NULL, 10);
            if (K < 1) { fprintf(stderr, "--batch needs a positive count\n"); return 2; }
            return run_batch(n, rp, ci, v, K);
        }

    /* xtrue, b = A xtrue, anorm (infinity norm, what pdgssvx3d passes to pdgstrf3d) */
    double *xt = (double *) malloc(sizeof(double) * n), *b = (double *) malloc(sizeof(double) * n), anorm = 0.0;
    for (int64_t i = 0; i < n; ++i) xt[i] = (i % 2) ? 1.0 : -1.0;
    for (int64_t i = 0; i < n; ++i) {
        double s = 0.0, rs = 0.0;
        for (int e = rp[i]; e < rp[i + 1]; ++e) { s += v[e] * xt[ci[e]]; rs += fabs(v[e]); }
        b[i] = s; if (rs > anorm) anorm = rs;
    }

    /* RowPerm = LargeDiag_MC64: perm_r[i] = row of Pr A that row i of A becomes; the handle is built from A1 = Pr A (rpF / ciF / vF, vF[e] = v[pos[e]]) */
    int *rpF = rp, *ciF = ci, *perm_r = NULL, *pos = NULL; double *vF = v, *rs = NULL, *cs = NULL;
    if (rowperm) {
        sluamd_rowperm_t m;
        perm_r = (int *) malloc(sizeof(int) * n); rs = (double *) malloc(sizeof(double) * n); cs = (double *) malloc(sizeof(double) * n);
        CHECK(sluamd_dLargeDiag(-1, n, rp, ci, v, perm_r, rs, cs, &m));
        printf("ROWPERM: rounds %d  matched on the device %lld of %lld  augmenting paths on the host %lld  info %d\n", m.rounds, (long long) m.matched_device,
               (long long) n, (long long) m.augmentations, m.info);
        if (m.info) { printf("structurally singular: %d rows cannot be matched\n", m.info); return 1; }
        const size_t nz = (size_t) (rp[n] ? rp[n] : 1);
        rpF = (int *) calloc((size_t) n + 1, sizeof(int)); ciF = (int *) malloc(sizeof(int) * nz); vF = (double *) malloc(sizeof(double) * nz);
        pos = (int *) malloc(sizeof(int) * nz);
        double *r1 = (double *) malloc(sizeof(double) * n);                        /* R by the rows of Pr A */
        for (int64_t i = 0; i < n; ++i) { rpF[perm_r[i] + 1] = rp[i + 1] - rp[i]; r1[perm_r[i]] = rs[i]; }
        for (int64_t i = 0; i < n; ++i) rpF[i + 1] += rpF[i];
        for (int64_t i = 0; i < n; ++i)
            for (int e = rp[i], q = rpF[perm_r[i]]; e < rp[i + 1]; ++e, ++q) { pos[q] = e; ciF[q] = ci[e]; vF[q] = v[e]; }
        free(rs); rs = r1;
        use_nd = use_nd || N <= 0;
    }

    /* ColPerm: NATURAL (generated grid) or our nested dissection (files), MY_PERMC in the reference's terms; the etree postorder of
     * the symbolic factorisation is composed into perm_c */
    int *perm_c = (int *) malloc(sizeof(int) * n), *perm_c_in = (int *) malloc(sizeof(int) * n);
    if (use_nd) CHECK(sluamd_order_nd(n, rpF, ciF, 64, perm_c_in));
    else for (int64_t i = 0; i < n; ++i) perm_c_in[i] = (int) i;
    sluamd_symb_t symb;
    CHECK(sluamd_dsymbfact(&symb, n, rpF, ciF, perm_c_in, 32, 256, perm_c));
    int32_t nsupers; int64_t nnzL, nnzU; double flops;
    CHECK(sluamd_symb_info(symb, &nsupers, &nnzL, &nnzU, NULL, NULL, &flops));

    sluamd_options_t opt; sluamd_default_options(&opt);
    sluamd_handle_t h;
    CHECK(sluamd_dCreateLUHandleFromSymb(&h, symb, rpF, ciF, vF, perm_c, &opt));

    int info = 0;
    sluamd_equil_t eq;
    if (rowperm) {   /* the matching's scalings alone (with --equil; else none: the call attaches A1), then B and X in A's ordering */
        CHECK(sluamd_dEquilibrateWith(h, (sluamd_int_t) n, rpF, ciF, vF, perm_c, equil ? rs : NULL, equil ? cs : NULL, &eq));
        CHECK(sluamd_SetRowPerm(h, perm_r));
        printf("EQUIL: equed = %c  rowcnd %.3e  colcnd %.3e  amax %.3e  info %d\n", "NRCB"[eq.equed], eq.rowcnd, eq.colcnd, eq.amax, eq.info);
        anorm = eq.anorm;
    } else if (equil) {   /* scales the handle's matrix; anorm of the scaled matrix comes back (pdgssvx3d.c:673-729) */
        CHECK(sluamd_dEquilibrate(h, (sluamd_int_t) n, rp, ci, v, perm_c, &eq));
        printf("EQUIL: equed = %c  rowcnd %.3e  colcnd %.3e  amax %.3e  info %d\n", "NRCB"[eq.equed], eq.rowcnd, eq.colcnd, eq.amax, eq.info);
        anorm = eq.anorm;
    }
    const double thresh = 1.1920928955078125e-07 * anorm;   /* smach_dist("Epsilon") * anorm, pdgstrf3d.c:132 */
    CHECK(sluamd_pdgstrf3d(h, thresh, &info));
    if (info) { printf("INFO = %d returned from pdgstrf3d (zero pivot)\n", info); return 1; }

    /* solve through pdgstrs3d's own boundary: b in the ORIGINAL row order in, x in the original order out (B_to_X / X_to_B with
     * perm_c run inside the library; a single rank holds all n rows) */
    double *x = (double *) malloc(sizeof(double) * n);
    double berr = 0.0; int32_t steps = 0, gsolves = 0;
    sluamd_xrefine_t xr = {0.0, 0.0, 0, 0};
    if (extra && (equil || rowperm)) { fprintf(stderr, "--refine extra: not with --equil / --rowperm in this example (solve with refine = 0, then refine the scaled system)\n"); return 2; }
    if (gmres && (equil || rowperm)) { fprintf(stderr, "--refine gmres: not with --equil / --rowperm in this example (solve with refine = 0, then refine the scaled system)\n"); return 2; }
    if (equil || rowperm) {   /* the expert driver's solve phase: B scaled by R, solve, refinement on the scaled system, X scaled by C */
        CHECK(sluamd_pdgssvx3d_solve(h, SLUAMD_NOTRANS, b, n, x, n, 1, 1, &berr, &steps));
    } else {
        memcpy(x, b, sizeof(double) * n);
        CHECK(sluamd_pdgstrs3d_dist(h, x, n, 1, n, 0, perm_c, perm_c));
        /* IterRefine = SLU_DOUBLE */
        CHECK(sluamd_dAttachMatrix(h, (sluamd_int_t) n, rp, ci, v, perm_c));
        if (gmres) CHECK(sluamd_pdgsrfs3d_gmres(h, SLUAMD_NOTRANS, b, n, x, n, 1, NULL, &berr, &steps, &gsolves));   /* NULL: restart 20, 100 solves, 2^-30 */
        else if (extra) { CHECK(sluamd_pdgsrfs3d_extra(h, SLUAMD_NOTRANS, b, n, x, n, 1, &berr, &xr)); steps = xr.steps; }
        else CHECK(sluamd_pdgsrfs3d(h, b, n, x, n, 1, &berr, &steps));
    }

    double err = 0.0, xn = 0.0, rn = 0.0, bn = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        double s = b[i];
        for (int e = rp[i]; e < rp[i + 1]; ++e) s -= v[e] * x[ci[e]];
        rn += s * s; bn += b[i] * b[i];
        if (fabs(x[i] - xt[i]) > err) err = fabs(x[i] - xt[i]);
        if (fabs(x[i]) > xn) xn = fabs(x[i]);
    }
    sluamd_stats_t st;
    sluamd_get_stats(h, &st);
    printf("n = %lld  nnz(A) = %d  nsupers = %d  nnz(L+U) = %lld  flops = %.3e\n", (long long) n, rp[n], nsupers,
           (long long) (nnzL + nnzU), flops);
    printf("FACTOR time %.3f ms  (%.1f GFLOP/s)   SOLVE time %.3f ms   refinement steps %d  berr %.2e\n", st.t_factor_ms,
           flops / (st.t_factor_ms * 1e-3) / 1e9, st.t_solve_ms, steps, berr);
    printf("||X-Xtrue||/||X|| = %e   ||b-Ax||_2/||b||_2 = %e\n", err / xn, sqrt(rn / bn));
    if (extra) printf("extra-precise refinement: berr %.2e  steps %d  dxrel %.3e  state %s  (forward error estimate dxrel / (1 - rho) = %.3e)\n", berr, xr.steps, xr.dxrel,
                      xr.state == SLUAMD_XR_CONVERGED ? "CONVERGED" : xr.state == SLUAMD_XR_NO_PROGRESS ? "NO_PROGRESS" : "LIMIT", xr.dxrel / (1.0 - xr.rho));
    if (gmres) printf("GMRES refinement: outer steps %d  applications of the factors %d\n", steps, gsolves);
    int bad_steps = 0;
    double *v2 = nsteps > 0 ? (double *) malloc(sizeof(double) * (size_t) (rp[n] ? rp[n] : 1)) : NULL;
    for (long s = 1; s <= nsteps; ++s) {
        /* same pattern, new values: the diagonal grows by up to 1/2, the rest shrinks by up to 3/8 (a diagonally dominant A stays so) */
        for (int64_t i = 0; i < n; ++i)
            for (int e = rp[i]; e < rp[i + 1]; ++e)
                v2[e] = ci[e] == i ? v[e] * (1.0 + 0.125 * (double) ((i + s) % 5)) : v[e] * (1.0 - 0.0625 * (double) ((e + 3 * s) % 7));
        for (int64_t i = 0; i < n; ++i) {
            double t = 0.0;
            for (int e = rp[i]; e < rp[i + 1]; ++e) t += v2[e] * xt[ci[e]];
            b[i] = t;
        }
        sluamd_update_t up;                                   /* a matrix is attached by now (sluamd_dEquilibrate / sluamd_dAttachMatrix): it takes the new values, and anorm comes back */
        if (rowperm) { for (int e = 0; e < rp[n]; ++e) vF[e] = v2[pos[e]]; }   /* the handle's CSR is that of Pr A */
        CHECK(sluamd_dUpdateValues(h, rowperm ? vF : v2, &up));
        CHECK(sluamd_pdgstrf3d(h, 1.1920928955078125e-07 * up.anorm, &info));
        if (info) { printf("STEP %ld: INFO = %d returned from pdgstrf3d (zero pivot)\n", s, info); return 1; }
        if (equil || rowperm) {
            CHECK(sluamd_pdgssvx3d_solve(h, SLUAMD_NOTRANS, b, n, x, n, 1, 1, &berr, &steps));
        } else {
            memcpy(x, b, sizeof(double) * n);
            CHECK(sluamd_pdgstrs3d_dist(h, x, n, 1, n, 0, perm_c, perm_c));
            CHECK(sluamd_pdgsrfs3d(h, b, n, x, n, 1, &berr, &steps));
        }
        double r2 = 0.0, b2 = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            double t = b[i];
            for (int e = rp[i]; e < rp[i + 1]; ++e) t -= v2[e] * x[ci[e]];
            r2 += t * t; b2 += b[i] * b[i];
        }
        printf("STEP %ld: equed = %c  anorm %.6e  refinement steps %d  berr %.2e  ||b-Ax||_2/||b||_2 = %e\n", s, "NRCB"[up.equed], up.anorm, steps, berr, sqrt(r2 / b2));
        if (!(sqrt(r2 / b2) < 1e-10)) bad_steps++;
    }
    free(v2);
    sluamd_dDestroyLUHandle(h);
    sluamd_symb_free(symb);
    return sqrt(rn / bn) < 1e-10 && !bad_steps ? 0 : 1;
}
