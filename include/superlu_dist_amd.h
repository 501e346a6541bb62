/*
 * superlu_dist_amd.h -- C ABI of the MI355X (gfx950) implementation of SuperLU_DIST's 3D supernodal
 * LU hot path: numeric factorisation (pdgstrf3d) and block triangular solve (pdgstrs3d).
 *
 * Drop-in boundary.  The reference is plain C; its GPU factorisation is
 * reached through an opaque-handle hook set called from pdgssvx3d
 * (/root/reference/SRC/double/pdgssvx3d.c:1013-1021):
 *
 *     dCreateLUgpuHandle / pdgstrf3d_LUv1 / dCopyLUGPU2Host / dDestroyLUgpuHandle
 *     (/root/reference/SRC/include/superlu_upacked.h:16-29,
 *      /root/reference/SRC/CplusplusFactor/LUgpuCHandle_interface_impl.cu:11-73)
 *
 * The entry points below replace exactly that set (plus the solve hooks), with the reference's
 * struct arguments flattened to plain pointers and sizes so that the library has no dependency on the
 * reference headers.  INTEGRATION.md shows the ~40-line stub a maintainer adds to pdgssvx3d.c to bind
 * dLUstruct_t / gridinfo3d_t / dtrf3Dpartition_t to these calls.
 *
 * All functions return 0 on success, a negative SLUAMD_E* code on failure; none of them falls back to
 * a CPU path: without a HIP device they fail with SLUAMD_ENODEVICE.
 */
#ifndef SUPERLU_DIST_AMD_H
#define SUPERLU_DIST_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* reference int_t (superlu_defs.h:121-129): 32-bit in the default build, 64-bit with _LONGINT.
 * The ABI carries 32-bit indices (one rank's panels are far below 2^31 rows / columns); value offsets are 64-bit internally.
 * An application built with 64-bit int_t passes narrowed copies of its index arrays -- oracle/ref/sluamd_binding.c does it under
 * #if defined(_LONGINT), range-checked; the value arrays are used in place. */
typedef int32_t sluamd_int_t;

#define SLUAMD_OK 0
#define SLUAMD_EINVAL (-1)
#define SLUAMD_ENODEVICE (-2)
#define SLUAMD_EHIP (-3)
#define SLUAMD_ENOMEM (-4)
#define SLUAMD_ESTRUCT (-5) /* malformed L/U index structure */

/* One rank's view of dLUstruct_t->Llu + Glu_persist + gridinfo3d_t
 * (superlu_ddefs.h:97-172, superlu_defs.h:454-457, :385-420).  Index formats are the reference's own
 * (superlu_defs.h:156-198).  Pointer arrays have ceil(nsupers/npcol) and
 * ceil(nsupers/nprow) entries; absent panels are NULL. */
typedef struct sluamd_dLUview {
    int64_t n;                      /* order of the matrix                                  */
    int32_t nsupers;                /* Glu_persist->supno[n-1]+1                             */
    const sluamd_int_t *xsup;       /* Glu_persist->xsup[nsupers+1]                          */
    int32_t nprow, npcol, npdep;    /* gridinfo3d_t: grid2d.nprow, grid2d.npcol, npdep       */
    int32_t myrow, mycol, myzlayer; /* MYROW(iam), MYCOL(iam), zscp.Iam                      */
    sluamd_int_t **Lrowind_bc_ptr;  /* Llu->Lrowind_bc_ptr                                   */
    double **Lnzval_bc_ptr;         /* Llu->Lnzval_bc_ptr                                    */
    sluamd_int_t **Ufstnz_br_ptr;   /* Llu->Ufstnz_br_ptr                                    */
    double **Unzval_br_ptr;         /* Llu->Unzval_br_ptr                                    */
} sluamd_dLUview_t;

/* complex16 twin (zLUstruct_t->Llu, superlu_zdefs.h): same layout, values are doublecomplex {r, i} (dcomplex.h) */
typedef struct { double r, i; } sluamd_doublecomplex;
typedef struct sluamd_zLUview {
    int64_t n;
    int32_t nsupers;
    const sluamd_int_t *xsup;
    int32_t nprow, npcol, npdep;
    int32_t myrow, mycol, myzlayer;
    sluamd_int_t **Lrowind_bc_ptr;
    sluamd_doublecomplex **Lnzval_bc_ptr;
    sluamd_int_t **Ufstnz_br_ptr;
    sluamd_doublecomplex **Unzval_br_ptr;
} sluamd_zLUview_t;

/* dtrf3Dpartition_t (superlu_ddefs.h:317-337) flattened: elimination forests of this rank's Z layer.
 * May be NULL for a 1x1x1 grid: the library then derives a level schedule from the block structure. */
typedef struct sluamd_forest_view {
    int32_t maxLvl;                   /* log2(npdep)+1                                        */
    const sluamd_int_t *myTreeIdxs;   /* [maxLvl] forest id handled at each Z level           */
    const sluamd_int_t *myZeroTrIdxs; /* [maxLvl] 1 = this layer does not factor that level   */
    int32_t numForests;               /* 2^maxLvl - 1                                         */
    const int32_t *nNodes;            /* [numForests] sForest_t.nNodes                        */
    const sluamd_int_t *const *nodeList; /* [numForests] sForest_t.nodeList (elimination order) */
} sluamd_forest_view_t;

typedef struct sluamd_options {
    int32_t device;             /* HIP device ordinal (-1 = current device)                      */
    int32_t replace_tiny_pivot; /* options->ReplaceTinyPivot == YES (superlu_defs.h:697)         */
    int32_t deterministic;      /* 1: one supernode per Schur launch -> fixed summation order of the factors; the sweeps of
                                 *    sluamd_pdgstrs3d on a one-rank double handle run one update unit per launch, so a solve
                                 *    repeats bit for bit too (grids, complex16 and the transposed sweeps still accumulate
                                 *    with fp64 atomics in arrival order)                          */
    int32_t verbose;
    int32_t info_rule;          /* which zero pivot `info` names on an exactly singular matrix (round 6; a former reserved slot -- the struct's size and the
                                 * offsets of the fields above are unchanged):
                                 *   SLUAMD_INFO_FIRST (0, sluamd_default_options): the smallest zero-pivot column -- the DOCUMENTED meaning (pdgstrf2.c:493-497)
                                 *   SLUAMD_INFO_REFERENCE (1): what the reference's CODE leaves -- Local_Dgstrf2 overwrites *info at every zero pivot
                                 *     (pdgstrf2.c:568-571), so a rank keeps the one it met LAST; pdgstrf3d takes the MIN over the ranks (pdgstrf3d.c:388-392).
                                 *     The reference-side binding (bindings/superlu_dist/sluamd_binding.c) selects this one. */
    int32_t reserved_i;
    double  reserved[3];
} sluamd_options_t;
#define SLUAMD_INFO_FIRST 0
#define SLUAMD_INFO_REFERENCE 1

typedef struct sluamd_stats {
    double flops_schur_padded; /* reference tally 2*nbrow*ldu*ncols (sec_structs.c:692-693), in double */
    double flops_schur_exact;  /* 2*nbrow*segsize per U column                                        */
    double flops_panel;        /* diag LU + the two panel TRSMs                                       */
    double t_factor_ms;        /* last sluamd_pdgstrf3d: HIP-event time of the numeric phase          */
    double t_schur_ms, t_panel_ms; /* split by kernel family (events on the compute stream)           */
    double t_solve_ms;         /* last sluamd_pdgstrs3d                                               */
    double t_h2d_ms, t_d2h_ms;
    int64_t nnz_L, nnz_U;      /* stored entries (incl. explicit zeros of the supernodal format)      */
    int64_t bytes_device;
    int32_t num_levels, num_launches;
    int32_t tiny_pivots;
    int32_t reserved_i;
    int64_t schur_launches, schur_tiles;
    double  schur_bytes_alg;   /* algorithmic HBM bytes of all Schur launches             */
    int64_t chain_units;       /* always 0 (the opt-in persistent dataflow sweeps of rounds 3-5 were removed: slower, NOTEBOOK.md); kept for layout */
    int32_t chain_levels;      /* always 0, as above                                                  */
    int32_t solve_launches;    /* kernel launches of the last sluamd_pdgstrs3d (one right-hand-side chunk) */
    double  t_exchange_ms;     /* grid handles, profiling on: time of the XY panel-exchange phases ... */
    double  t_reduce_ms;       /* ... and of the Z ancestor reduction inside the last sluamd_pdgstrf3d */
    /* the Schur update by tile configuration (round 4): k_schur<128,128,8> -- supernodes of >= 96 columns whose block pairs fill 128 x 128
     * tiles, the MFMA-bound part -- against the 64 x 64 configuration of the narrow supernodes at the bottom of the tree (HBM / latency-bound,
     * "MFMA-bound only when s_k >~ 120") */
    double  t_schur_big_ms;        /* profiling on: HIP-event time of the 128 x 128 launches (part of t_schur_ms) */
    double  flops_schur_exact_big; /* exact-segment flops of the supernodes that use that configuration (part of flops_schur_exact) */
    double  schur_bytes_alg_big;   /* ... and their algorithmic destination bytes (part of schur_bytes_alg) */
} sluamd_stats_t;

typedef struct sluamd_lu_handle_s *sluamd_handle_t;

void sluamd_default_options(sluamd_options_t *opt);

/* Replaces dCreateLUgpuHandle (LUgpuCHandle_interface_impl.cu:11): uploads this rank's L/U index and
 * value arrays to HBM (kept resident for factor + solve), builds the device-side block directories and
 * the level schedule.  `forests` may be NULL (see above). */
int sluamd_dCreateLUHandle(sluamd_handle_t *h, const sluamd_dLUview_t *lu, const sluamd_forest_view_t *forests,
                           const sluamd_options_t *opt);

/* Re-upload numeric values only (same structure): the SamePattern_SameRowPerm refactor path
 * (superlu_defs.h:545-566). */
int sluamd_dSetValues(sluamd_handle_t h, const sluamd_dLUview_t *lu);

/* Replaces pdgstrf3d_LUv1 (LUgpuCHandle_interface_impl.cu:66) == the numeric work of pdgstrf3d
 * (pdgstrf3d.c:121-439): factors L\U in place in HBM.  thresh = smach("Epsilon")*anorm
 * (pdgstrf3d.c:132-133).  *info: 0, or 1-based column of a zero pivot (pdgstrf2.c:568-571). */
int sluamd_pdgstrf3d(sluamd_handle_t h, double thresh, int *info);

/* Replaces dCopyLUGPU2Host (LUgpuCHandle_interface_impl.cu:43): writes the factored values back into
 * the caller's Lnzval_bc_ptr / Unzval_br_ptr arrays in the reference panel / skyline formats. */
int sluamd_dCopyLU2Host(sluamd_handle_t h, const sluamd_dLUview_t *lu);

/* Replaces the L- and U-solves of pdgstrs3d / pdgstrs3d_newsolve (pdgstrs3d.c:6604, :6935) between
 * pdReDistribute3d_B_to_X and pdReDistribute3d_X_to_B: x is the right-hand side already permuted by
 * Pc*Pr (row index = global row of the factored matrix), n x nrhs column-major with leading dimension
 * ldx, overwritten by the solution of L U y = x.  Host-pointer and device-pointer variants. */
int sluamd_pdgstrs3d(sluamd_handle_t h, double *x, int64_t ldx, int32_t nrhs);
int sluamd_pdgstrs3d_dev(sluamd_handle_t h, double *d_x, int64_t ldx, int32_t nrhs);

/* complex16 twins of the four entry points above and of the solve (pzgstrf3d, SRC/complex16/pzgstrf3d.c; pzgstrs3d,
 * SRC/complex16/pzgstrs3d.c): same semantics on doublecomplex values.  Handles are shared with the double API for
 * sluamd_dDestroyLUHandle / sluamd_get_stats. */
int sluamd_zCreateLUHandle(sluamd_handle_t *h, const sluamd_zLUview_t *lu, const sluamd_forest_view_t *forests,
                           const sluamd_options_t *opt);
int sluamd_zSetValues(sluamd_handle_t h, const sluamd_zLUview_t *lu);
int sluamd_pzgstrf3d(sluamd_handle_t h, double thresh, int *info);
int sluamd_zCopyLU2Host(sluamd_handle_t h, const sluamd_zLUview_t *lu);
int sluamd_pzgstrs3d(sluamd_handle_t h, sluamd_doublecomplex *x, int64_t ldx, int32_t nrhs);

/* Transposed and conjugate-transposed solves with the resident factors: x (n x nrhs, column-major, leading dimension ldx, rows in
 * the ordering of the factored matrix -- the convention of sluamd_pdgstrs3d) is overwritten by the solution of (L U)^T y = x
 * (SLUAMD_TRANS) or (L U)^H y = x (SLUAMD_CONJ; the same as SLUAMD_TRANS on a double handle).  No second factorisation and no copy
 * of the factors: the sweeps read the panels and skylines along their columns (U^T forward over the DAG levels ascending, L^T
 * backward over them descending; the levels are longest paths over the L and the U blocks, so one schedule orders both systems).
 * The reference's pdgstrs3d has no such solve (pdgssvx3d reads options->Trans for the equilibration only).
 * SLUAMD_NOTRANS calls sluamd_pdgstrs3d[_dev] / sluamd_pzgstrs3d and nothing else; it also gives complex16 handles a
 * device-pointer solve.  Errors: trans outside {0, 1, 2} or a handle of the other precision: SLUAMD_EINVAL.  GRID HANDLES of
 * more than one rank, after sluamd_PlanTransposedSweeps (below): the replicated form of sluamd_pdgstrs3d -- every rank passes the
 * complete x, the call is collective, every rank returns the complete solution.  The transposed sweeps reduce the partial sums of
 * x_k along process COLUMN k % Pc and broadcast x_k along process ROW k % Pr (the untransposed ones the other way round), through
 * exchange lists of their own.  A grid handle whose lists were not planned returns SLUAMD_EINVAL for SLUAMD_TRANS / SLUAMD_CONJ, as
 * every grid handle did before these lists existed (sluamd_last_error() names the call); that and the argument errors above are
 * decided on state that is the same on all ranks, before the first exchange, so every rank returns them alike.
 * sluamd_p[dz]gstrs3d_dist (B distributed by rows) stays untransposed.
 * nrhs == 0 returns 0.  stats.t_solve_ms and stats.solve_launches are filled as by the untransposed solve: per chunk of
 * right-hand sides one diagonal and one update launch per DAG level and sweep (4 x levels; on a grid: of the forests this rank sweeps). */
#define SLUAMD_NOTRANS 0
#define SLUAMD_TRANS   1
#define SLUAMD_CONJ    2   /* conjugate transpose; identical to SLUAMD_TRANS on double handles */
int sluamd_pdgstrs3d_trans(sluamd_handle_t h, int trans, double *x, int64_t ldx, int32_t nrhs);
/* Plans the exchange lists of the transposed sweeps on a handle of more than one rank: from then on sluamd_p[dz]gstrs3d_trans,
 * sluamd_p[dz]gsrfs3d_trans and sluamd_p[dz]gssvx3d_solve take SLUAMD_TRANS / SLUAMD_CONJ on it.  EVERY rank of the grid calls it,
 * any time after the handle was created; it is local (the handle's own level lists and grid position, no communication, no device
 * work), costs a few run lists per level, and may be repeated.  A handle that never asks plans nothing.  1 x 1 x 1 handles: returns 0,
 * nothing to plan. */
int sluamd_PlanTransposedSweeps(sluamd_handle_t h);
int sluamd_pdgstrs3d_trans_dev(sluamd_handle_t h, int trans, double *d_x, int64_t ldx, int32_t nrhs);
int sluamd_pzgstrs3d_trans(sluamd_handle_t h, int trans, sluamd_doublecomplex *x, int64_t ldx, int32_t nrhs);
int sluamd_pzgstrs3d_trans_dev(sluamd_handle_t h, int trans, sluamd_doublecomplex *d_x, int64_t ldx, int32_t nrhs);

/* Replaces dDestroyLUgpuHandle (LUgpuCHandle_interface_impl.cu:30). */
void sluamd_dDestroyLUHandle(sluamd_handle_t h);

int sluamd_get_stats(sluamd_handle_t h, sluamd_stats_t *out);
/* wall-clock breakdown of the handle's creation as "phase=seconds;phase=seconds;..." (host planner phases, arena allocation, table uploads,
 * distribution of A): the pre-processing a caller pays once per sparsity structure (pddistribute3d + the GPU handle set-up of the reference) */
int sluamd_setup_times(sluamd_handle_t h, char *buf, int32_t cap);
/* Diagnostics: how many device allocations the library has requested in this process so far (every one goes through one helper; the pool's chunks and
 * the caller's own allocations are not counted).  Two reads around a call tell whether the call allocated. */
int64_t sluamd_device_alloc_count(void);
/* The plan of this rank, one row of SLUAMD_PLAN_COLS doubles per (Z level, DAG level): supernodes, Schur / panel flops of THIS rank, bytes and messages of the two XY
 * exchange phases, bytes of the Z reduction that follows the Z level (column list at the definition, sluamd_api.cpp).  buf may be NULL: *rows = rows needed.
 * Host data only (no device work): what a scaling model needs from the library (scripts/scale_model.py; the reference prints the same quantities as its
 * SCT counters commVolFactor / commVolRed, sec_structs.c). */
#define SLUAMD_PLAN_COLS 20
int sluamd_plan_table(sluamd_handle_t h, double *buf, int64_t cap_rows, int64_t *rows);
/* The x-segment exchange lists of the solve sweeps on this rank's plan, read-only (tests compare the two sides of every message).  which: 0 .. 3 = the
 * untransposed sweeps' reduce-send, reduce-receive, broadcast-send, broadcast-receive lists, 4 .. 7 = the same of the transposed sweeps.  One row of 5 ints
 * per run, in list order: Z level, DAG level, peer (world rank), first row, rows (in doubles: complex16 rows count twice).  buf may be NULL: *rows = rows needed. */
int sluamd_plan_xlists(sluamd_handle_t h, int which, int32_t *buf, int64_t cap_rows, int64_t *rows);
const char *sluamd_last_error(void);
/* number of visible HIP devices (0 when none) -- lets callers fail loudly instead of falling back */
int sluamd_device_count(void);
/* The value arenas of 1 x 1 x 1 handles come from a process-level pool of physical device chunks (destroyed handles return their chunks to it, later
 * handles re-map them: no driver-side clearing of re-used memory).  This call returns the chunks no handle uses to the driver (dev < 0: every device);
 * result = the bytes the pool held.  The library trims by itself when one of its allocations fails.  SLUAMD_NO_DEVPOOL=1: plain hipMalloc. */
int64_t sluamd_device_pool_trim(int dev);
/* "domain:bus:device.function" of HIP device `dev` (hipDeviceGetPCIBusId): lets a harness find the device's sysfs node, e.g. to sample its clock beside a
 * measurement (bench.py `device_clock`).  buf of at least 16 bytes. */
int sluamd_device_pci_bus_id(int dev, char *buf, int len);

/* ------------------------------------------------------------------------------------------------
 * Host-side producers of the L/U store (rows of SURVEY.md section 8(f) that the hot path needs when the
 * reference's pre-processing is not linked): symmetric-pattern symbolic factorisation + distribution
 * for a 1 x 1 x npdep grid.  Mirrors symbfact_dist / pddistribute3d (symbfact.c, pddistribute3d.c:1357)
 * in effect (same store formats), not in algorithm.
 * ------------------------------------------------------------------------------------------------ */
typedef struct sluamd_symb_s *sluamd_symb_t;

/* A: n x n CSR (rowptr/colind/nzval) of the ORIGINAL matrix; perm_c[old] = new is applied symmetrically
 * (A1 = Pc A Pc^T, i.e. RowPerm = NOROWPERM, ColPerm = MY_PERMC; pdgssvx3d.c:749-791); the etree
 * postorder is composed into perm_c_out like sp_colorder does (sp_colorder.c).  relax / maxsup play the
 * roles of sp_ienv_dist(2) / sp_ienv_dist(3) (sp_ienv.c:95-110). */
int sluamd_dsymbfact(sluamd_symb_t *s, int64_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                     const sluamd_int_t *perm_c, int32_t relax, int32_t maxsup, sluamd_int_t *perm_c_out);
/* The same producer for UNSYMMETRIC patterns with the reference's own supernode rules (symbfact.c:83-200: relax_snode :221-265, the
 * T2 / subset / maxsup boundary test of column_dfs :598-672): the exact structure of L and U of Pc A Pc^T under elimination without
 * pivoting, U as per-column skyline segments -- the store the reference's symbfact + pddistribute3d build for the same perm_c, relax
 * (sp_ienv_dist(2)) and maxsup (sp_ienv_dist(3)): xsup, every L block's row set and every Ufstnz entry agree (tests/test_symbolic_parity.py).
 * The result feeds the same consumers as sluamd_dsymbfact (sluamd_symb_view, sluamd_ddistribute_host, sluamd_dCreateLUHandleFromSymb[Grid],
 * sluamd_symb_partition, sluamd_symb_grid_footprint). */
int sluamd_dsymbfact_unsym(sluamd_symb_t *s, int64_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                           const sluamd_int_t *perm_c, int32_t relax, int32_t maxsup, sluamd_int_t *perm_c_out);
/* Fill-reducing ordering for matrices without geometry (the role of get_perm_c / METIS in the reference,
 * SRC/prec-independent/get_perm_c.c): nested dissection of the pattern of A + A^T by BFS level structures; perm_c[old] = new,
 * to be passed to sluamd_dsymbfact.  leaf = component size below which no further separator is sought (<= 0: 64). */
int sluamd_order_nd(int64_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, int32_t leaf, sluamd_int_t *perm_c);
/* The synthetic operator of SURVEY.md 8(d) / BASELINE.json configs[1-2] for harnesses: 7-point Poisson on an nx x ny x nz grid, natural index (i ny + j) nz + k,
 * diagonal 6, off-diagonals -1, Dirichlet truncation, CSR with ascending column indices.  rowptr: nx ny nz + 1 entries, colind / nzval:
 * 7 n - 2 (nx ny + ny nz + nx nz) entries; returns that count (or a negative error code). */
int64_t sluamd_poisson3d(int32_t nx, int32_t ny, int32_t nz, sluamd_int_t *rowptr, sluamd_int_t *colind, double *nzval);
int sluamd_symb_info(sluamd_symb_t s, int32_t *nsupers, int64_t *nnzL, int64_t *nnzU, int64_t *lidx_len,
                     int64_t *uidx_len, double *flops);
/* borrow the store in the reference's formats (valid until sluamd_symb_free) */
int sluamd_symb_view(sluamd_symb_t s, sluamd_dLUview_t *view);
/* scatter A's values (original CSR + the same perm_c_out) into the zero-initialised store held by `s`
 * (host) -- what pddistribute3d does for a 1x1x1 grid */
int sluamd_ddistribute_host(sluamd_symb_t s, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                            const double *nzval, const sluamd_int_t *perm_c_final);
/* device-resident variant: create the LU handle straight from the symbolic structure; values are
 * zero-filled in HBM and A's entries scattered by a kernel (no host copy of the factors exists) */
int sluamd_dCreateLUHandleFromSymb(sluamd_handle_t *h, sluamd_symb_t s, const sluamd_int_t *rowptr,
                                   const sluamd_int_t *colind, const double *nzval,
                                   const sluamd_int_t *perm_c_final, const sluamd_options_t *opt);
/* copy the store out as flat arrays + offsets (any pointer may be NULL) */
int sluamd_symb_export(sluamd_symb_t s, sluamd_int_t *xsup, int64_t *lidx_off, sluamd_int_t *lidx, int64_t *lval_off,
                       double *lval, int64_t *uidx_off, sluamd_int_t *uidx, int64_t *uval_off, double *uval);
int sluamd_zCreateLUHandleFromSymb(sluamd_handle_t *h, sluamd_symb_t s, const sluamd_int_t *rowptr,
                                   const sluamd_int_t *colind, const sluamd_doublecomplex *nzval,
                                   const sluamd_int_t *perm_c_final, const sluamd_options_t *opt);
void sluamd_symb_free(sluamd_symb_t s);
/* elimination-forest partition for npdep Z layers (getForests' job, supernodalForest.c; tree ids in heap order like
 * getGridTrees, supernodal_etree.c:840-851): sn_tree[k] = forest of supernode k (see sluamd_dCreateLUHandleFromSymbGrid) */
int sluamd_symb_partition(sluamd_symb_t s, int32_t npdep, int32_t *sn_tree);
/* Capacity planning: stored factor values per world rank of an nprow x npcol x npdep grid (own slots, including the ancestor
 * panels every layer below a forest replicates -- dinit3DLUstructForest, pd3dcomm.c:334-800), the part of them that is such a
 * replica, and the index entries, from the symbolic structure alone.  Arrays of nprow*npcol*npdep entries; `replicated` /
 * `index_entries` may be NULL; sn_tree as for sluamd_dCreateLUHandleFromSymbGrid (NULL when npdep == 1). */
int sluamd_symb_grid_footprint(sluamd_symb_t s, int32_t nprow, int32_t npcol, int32_t npdep, const int32_t *sn_tree,
                               int64_t *values, int64_t *replicated, int64_t *index_entries);
/* The symbolic structure of the block-diagonal matrix diag(A, ..., A) with `count` copies of the m x m pattern `s` was made for (sluamd_dsymbfact[_unsym]),
 * matrix-major: xsup, every L block's row set and every Ufstnz entry are those of `s` shifted by k m for copy k, supernode ids by k nsupers; the final
 * column permutation is perm_big[k m + i] = k m + perm_c_out[i].  `*out` is a full sluamd_symb_t (sluamd_symb_info, _export, _view, _partition,
 * sluamd_dCreateLUHandleFromSymb, sluamd_symb_free); `s` is not modified and may be freed first.  The cost is linear in the output: no symbolic
 * factorisation of count m columns runs.  Errors (SLUAMD_EINVAL): null arguments, count <= 0, count m beyond the 32-bit indices of the ABI. */
int sluamd_symb_replicate(sluamd_symb_t s, int32_t count, sluamd_symb_t *out);
/* re-run the device-side distribution (zero-fill + scatter of A) on such a handle: refactor loops */
int sluamd_dResetValues(sluamd_handle_t h);

/* ---- auxiliary (timing / tests) ---- */
int sluamd_device_synchronize(void);
int sluamd_set_profile(sluamd_handle_t h, int on);         /* per-kernel-family HIP-event timing in stats */
int sluamd_factor_info(sluamd_handle_t h, int *info, int *tiny_pivots);
/* Linv / Uinv of the diagonal block of supernode k as the handle keeps them for the panel solves and the triangular sweeps -- what pdCompute_Diag_Inv
 * (SRC/double/pdgstrs.c:842-959: dtrtri on the factored block) leaves in Llu->Linv_bc_ptr / Uinv_bc_ptr: column-major nsupc x nsupc each, unit-lower and
 * upper inverse with explicit zeros in the other triangle.  Host buffers; the rank must own the diagonal block; double handles after a factorisation. */
int sluamd_dGetDiagInv(sluamd_handle_t h, int32_t k, double *Linv, double *Uinv);
int sluamd_mfma_selftest(const double *A16x4, const double *B4x16, double *D16x16);

/* ---- iterative refinement: pdgsrfs3d (SRC/double/pdgsrfs.c:345-510) with its SpMV pdgsmv (SRC/double/pdgsmv.c) on the
 * device, SURVEY 8(f)-2.  The ORIGINAL matrix (CSR, 0-based) and perm_c are attached once; the factors in the handle are
 * those of Pc A Pc^T (Equil=NO, NOROWPERM -- the boundary's convention; Equil = YES and RowPerm = LargeDiag_MC64 are the sections below).  B, X: original ordering, column-major; X holds
 * the initial solution and is refined in place; berr[nrhs] = componentwise backward errors; *steps = refinement steps of
 * the last right-hand side (stat->RefineSteps).  Stopping rule as the reference: berr > eps, berr*2 <= previous, < 20. */
int sluamd_dAttachMatrix(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                         const double *nzval, const sluamd_int_t *perm_c);
int sluamd_pdgsrfs3d(sluamd_handle_t h, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, double *berr,
                     int32_t *steps);
int sluamd_pdgsrfs3d_dev(sluamd_handle_t h, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs,
                         double *berr, int32_t *steps);
/* complex16 twins: pzgsrfs3d (SRC/complex16/pzgsrfs.c:365-514), the residual with abs1(z) = |re| + |im| as in pzgsmv.  Same
 * semantics as the double calls; nzval, B, X are doublecomplex, ldb / ldx counted in complex elements.  zAttachMatrix needs a
 * complex16 handle (dAttachMatrix a double one); a refinement call whose precision is not that of the handle and of the attached
 * matrix, or with no matrix attached, returns SLUAMD_EINVAL.  nrhs == 0 returns 0 with *steps = 0.
 * Grid handles (both precisions): the replicated form of sluamd_pdgstrs3d -- every rank attaches the complete matrix, passes the
 * complete B and X and gets the complete refined X back; the calls are collective, and each step's continue / stop decision is a
 * min-all-reduce over the grid, so all ranks take the same number of steps. */
int sluamd_zAttachMatrix(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                         const sluamd_doublecomplex *nzval, const sluamd_int_t *perm_c);
int sluamd_pzgsrfs3d(sluamd_handle_t h, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X, int64_t ldx,
                     int32_t nrhs, double *berr, int32_t *steps);
int sluamd_pzgsrfs3d_dev(sluamd_handle_t h, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X,
                         int64_t ldx, int32_t nrhs, double *berr, int32_t *steps);
/* Refinement of the transposed and conjugate-transposed systems (xGERFS with trans): op(A) x = b for the ATTACHED matrix, op(A) = A^T
 * (SLUAMD_TRANS) or A^H (SLUAMD_CONJ; the same as SLUAMD_TRANS on a double handle), with the contract of sluamd_p[dz]gsrfs3d[_dev]:
 * B, X in the original ordering, X holds the initial solution (e.g. of sluamd_p[dz]gstrs3d_trans on Pc b) and is refined in place,
 * berr[j] = max_i |r_i| / (|op(A)| |x| + |b|)_i with the SAFE1 / SAFE2 guards (complex16: abs1), the same stopping rule, the same limit
 * of 20 steps, *steps = those of the last right-hand side.  The correction of a step is the transposed solve with the resident factors:
 * with the factors of Pc A Pc^T, A^T d = r is (Pc A Pc^T)^T (Pc d) = Pc r, the same permutation on both sides.  The residual reads the
 * attached values through a transposed index of the CSR pattern (column pointers, rows, positions -- no second copy of the values, so
 * sluamd_[dz]UpdateValues and sluamd_[dz]Equilibrate need nothing new), built on the host at the first transposed call after a matrix
 * was attached (its time appears in sluamd_setup_times as refine.transposed_index) and dropped with that matrix.
 * SLUAMD_NOTRANS calls sluamd_p[dz]gsrfs3d[_dev] and nothing else.  nrhs == 0 returns 0 with *steps = 0.
 * Errors, all SLUAMD_EINVAL with a message: trans outside {0, 1, 2}; a handle of the other precision; no attached matrix, or one of the
 * other precision; a grid handle without sluamd_PlanTransposedSweeps.  Grid handles: the replicated form of sluamd_p[dz]gsrfs3d (the complete attached matrix, B and X on every rank,
 * collective); berr and the step count come from replicated data and are the same on every rank, the continue / stop decision is agreed
 * by a min-all-reduce.
 * After sluamd_[dz]Equilibrate the attached matrix is the scaled one, A' = R A C, and these calls refine op(A') x' = b': for
 * op(A) x = b pass b' = C o b and the scaled solution x' (op(A') x' = b' with x = R o x'), then unscale x = R o x' -- the roles of R and C
 * swapped against the untransposed system, see sluamd_p[dz]gssvx3d_solve. */
int sluamd_pdgsrfs3d_trans(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs,
                           double *berr, int32_t *steps);
int sluamd_pdgsrfs3d_trans_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs,
                               double *berr, int32_t *steps);
int sluamd_pzgsrfs3d_trans(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X,
                           int64_t ldx, int32_t nrhs, double *berr, int32_t *steps);
int sluamd_pzgsrfs3d_trans_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X,
                               int64_t ldx, int32_t nrhs, double *berr, int32_t *steps);

/* GMRES refinement preconditioned by the resident factors (GMRES-IR: Carson & Higham; the fallback Li & Demmel name for static pivoting): for systems on
 * which the stationary loop above stalls or diverges because the spectral radius of I - (L U)^-1 A reaches one -- replaced tiny pivots, factors of an
 * earlier matrix kept as a lagged preconditioner (sluamd_[dz]UpdateValues / sluamd_[dz]AttachMatrix with another matrix), growth.  The outer loop is that of
 * sluamd_p[dz]gsrfs3d[_trans]: the same residual and berr kernels, the same stopping rule (berr > eps, 2 berr <= previous, < 20 outer steps), the same
 * update; the correction of a step is one cycle of right-preconditioned GMRES on A1 d = r, A1 = Pc op(A) Pc^T, M = L U, d_0 = 0, instead of one
 * application of (L U)^-1: classical Gram-Schmidt with one reorthogonalisation on the device, Hessenberg matrix and Givens rotations on the host.  A cycle
 * ends when the residual estimate is <= inner_tol ||r||_2, on a breakdown, after `restart` iterations, or when the budget leaves one application of the
 * factors; its correction d = M^-1 V y costs that last application.  The accuracy reported is computed by the refinement's own kernels from the true
 * residual; GMRES only proposes corrections.  Reductions use no floating-point atomics: on a deterministic handle two calls return the same bits.
 * trans, B, X, ldb, ldx, nrhs, berr, the ordering, equilibrated handles (the attached, scaled system is refined) and nrhs == 0: the contract of
 * sluamd_p[dz]gsrfs3d_trans[_dev].  *steps = OUTER steps (cycles) of the last right-hand side; solves[j] (may be NULL) = applications of the factors spent
 * on right-hand side j: iterations + 1 per cycle.  When max_solves is reached the cycle in hand is finished into X, the true berr is computed and the call
 * returns 0 with solves[j] == max_solves (a single remaining application is spent on one plain refinement step: a cycle needs two).
 * A residual whose 2-norm is not a positive finite double (its square under- or overflows) gets the plain step instead of a cycle; a residual that
 * op(A) (L U)^-1 maps to zero ends the refinement of that right-hand side with X untouched and the berr reached so far (one application spent), return 0.
 * opt == NULL: the defaults.  Device memory: restart + 5 vectors of n values and 1 MiB of partial sums, allocated on the first call of a handle, regrown
 * when restart grows, released with the attached matrix.
 * Errors beyond those of sluamd_p[dz]gsrfs3d_trans, all SLUAMD_EINVAL with a message: restart outside [1, 64], max_solves < 1, inner_tol outside (0, 1);
 * a handle of a multi-rank grid; the handle of a batch (sluamd_BatchHandle). */
typedef struct sluamd_gmres {
    int32_t restart;      /* basis vectors per cycle, 1..64; default 20 (the limit of the outer loop) */
    int32_t max_solves;   /* cap on applications of the factors per right-hand side, >= 1; default 100 */
    double  inner_tol;    /* cycle ends at estimate <= inner_tol * ||r||_2, in (0,1); default 2^-30: two outer steps reach eps */
} sluamd_gmres_t;
void sluamd_default_gmres(sluamd_gmres_t *opt);
int sluamd_pdgsrfs3d_gmres(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs,
                           const sluamd_gmres_t *opt, double *berr, int32_t *steps, int32_t *solves);
int sluamd_pdgsrfs3d_gmres_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs,
                               const sluamd_gmres_t *opt, double *berr, int32_t *steps, int32_t *solves);
int sluamd_pzgsrfs3d_gmres(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X,
                           int64_t ldx, int32_t nrhs, const sluamd_gmres_t *opt, double *berr, int32_t *steps, int32_t *solves);
int sluamd_pzgsrfs3d_gmres_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X,
                               int64_t ldx, int32_t nrhs, const sluamd_gmres_t *opt, double *berr, int32_t *steps, int32_t *solves);
/* test hook: ONE operation of the Krylov kernels of the GMRES refinement, through the chunk loops the cycle itself runs, on vectors laid out as the cycle's
 * workspace (16-byte aligned, zero-filled; a double vector of odd order padded to an even count).  No handle: host pointers, the current device, its null
 * stream.  z: 0 double, 1 complex16; vs = 1 or 2 doubles per value; ns = doubles per padded vector = z ? 2 n : n + (n & 1).  V: nv vectors of n values,
 * contiguous; placed vstride doubles apart on the device (even, >= ns; the gap behind a vector holds NaN).  x: n values.  xout: ns doubles, the pad
 * included.  coef: nv coefficients of vs doubles.  The partial sums and the result words hold NaN before the operation.
 *   SLUAMD_KRYLOV_DOTS     nv in [0, 64]: res[vs k ..] = v_k^H x, res[vs nv] = ||x||^2 (partials of the first chunk's launch); xout = x as the kernels left it
 *   SLUAMD_KRYLOV_AXPYS    nv in [1, 64]: x -= sum_k v_k coef_k, coef read from device memory; xout = x, res[0] = ||x||^2 of the new x
 *   SLUAMD_KRYLOV_SCALE    xout = x / h into a vector of its own that held NaN (nv, V, coef, res unused)
 *   SLUAMD_KRYLOV_COMBINE  nv in [1, 64]: x = (add ? x : 0) + sum_k v_k coef_k; xout = x (res unused)
 * Errors, SLUAMD_EINVAL with a message: an unknown op, n < 1, nv outside the range of the op, vstride odd or < ns, a null pointer the op uses. */
#define SLUAMD_KRYLOV_DOTS 0
#define SLUAMD_KRYLOV_AXPYS 1
#define SLUAMD_KRYLOV_SCALE 2
#define SLUAMD_KRYLOV_COMBINE 3
int sluamd_krylov_selftest(int op, int z, int64_t n, int32_t nv, int64_t vstride, const double *V, const double *x, const double *coef, double h, int add,
                           double *xout, double *res);

/* Blocked refinement: the contract of sluamd_p[dz]gsrfs3d_trans[_dev] -- trans, B, X, ldb, ldx, nrhs, the ordering, berr[j], equilibrated handles, grid
 * handles (replicated form, collective; transposed calls after sluamd_PlanTransposedSweeps) -- with all right-hand sides carried through the loop TOGETHER,
 * in panels of 16 columns (the block that one pass of the fp64 MFMA sweeps over the factors serves): per step one residual pass over the columns of the
 * panel that are still active, ONE solve with the resident factors for all columns that continue, one update of exactly those.  The calls above pay one
 * pass over the factors per column and step.  Per column nothing differs from those calls: the same residual and berr (the same kernel text, bitwise), the
 * same continue / stop decision from that column's own previous berr and step count, the same update; a column that has stopped is not touched again, so
 * X, berr and the step counts are those of sluamd_p[dz]gsrfs3d[_trans] column by column wherever the sweeps return the same correction for a column alone
 * and inside a block (exactly representable data, deterministic handles).
 * steps (may be NULL): nrhs entries, steps[j] = the steps of right-hand side j itself.  nrhs == 0 returns 0 and writes nothing.
 * Device memory: 16 n values and 16 words on the first block call of a handle, 32 n values more on the first call of the host form; released with the
 * attached matrix.  On grids the decisions of a panel are agreed by one min-all-reduce per step.
 * Errors beyond those of sluamd_p[dz]gsrfs3d_trans: the handle of a batch (sluamd_BatchHandle), SLUAMD_EINVAL. */
int sluamd_pdgsrfs3d_block(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs,
                           double *berr, int32_t *steps);
int sluamd_pdgsrfs3d_block_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs,
                               double *berr, int32_t *steps);
int sluamd_pzgsrfs3d_block(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X,
                           int64_t ldx, int32_t nrhs, double *berr, int32_t *steps);
int sluamd_pzgsrfs3d_block_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X,
                               int64_t ldx, int32_t nrhs, double *berr, int32_t *steps);

/* Extra-precise refinement, IterRefine = SLU_EXTRA ("accumulate residual in extra precision"): for systems whose condition number approaches 1 / eps.  The
 * calls above stop on the backward error, and berr <= eps is reached while the forward error is still about cond(A) eps: the rounded fp64 residual limits
 * what a correction can gain.  Here the residual of every step is accumulated in twice the working precision (per entry the product's error by a fused
 * multiply-add and the sum's by TwoSum, carried in a compensation word; one rounding at the end of the row), the correction is the solve with the resident
 * factors, and the loop watches the corrections.  With ndx = max_i abs1(dx_i) and nx = max_i abs1(x_i) of the x the correction belongs to (abs1 = |re| + |im|),
 * per right-hand side:
 *     residual (extra) -> berr;  after 20 steps: LIMIT.  dx = solve;  ndx == 0: CONVERGED.  After the first step, 2 ndx > the previous ndx (or at any step
 *     an ndx that is not finite): NO_PROGRESS, dx is dropped.  x += dx;  ndx <= eps nx (eps = 2^-53): one closing residual pass, CONVERGED.
 * The factor 2 is the one the reference's rule applies to berr.  berr[j] always belongs to the returned X.  x itself stays fp64: the result is the fp64
 * neighbourhood of the solution, a few ulps in the largest component for cond(A) up to about 1 / eps, not a doubled x.
 * out (may be NULL): nrhs entries.  steps = corrections applied; state as below; dxrel = ndx / nx of the last correction COMPUTED (a dropped one included;
 * 0 when ndx == 0); rho = the largest ratio of successive ndx among the corrections applied (0 with fewer than two).  dxrel / (1 - rho) ESTIMATES the
 * relative forward error max|x - x*| / max|x| of the returned X (the tail of a geometric series of corrections); it is an estimate, not a bound.
 * trans, B, X, ldb, ldx, nrhs, berr, the ordering, equilibrated handles (the attached, scaled system is refined): the contract of
 * sluamd_p[dz]gsrfs3d_trans[_dev].  nrhs == 0 returns 0 and writes nothing.  Device memory: two words on the first call of a handle, released with the
 * attached matrix.  No floating-point atomics: two calls return the same bits wherever the solves do.
 * Errors beyond those of sluamd_p[dz]gsrfs3d_trans, SLUAMD_EINVAL with a message: a handle of a multi-rank grid; the handle of a batch. */
#define SLUAMD_XR_CONVERGED 0
#define SLUAMD_XR_NO_PROGRESS 1
#define SLUAMD_XR_LIMIT 2
typedef struct sluamd_xrefine {
    double  dxrel, rho;
    int32_t steps, state;
} sluamd_xrefine_t;
int sluamd_pdgsrfs3d_extra(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs, double *berr,
                           sluamd_xrefine_t *out);
int sluamd_pdgsrfs3d_extra_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs,
                               double *berr, sluamd_xrefine_t *out);
int sluamd_pzgsrfs3d_extra(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X,
                           int64_t ldx, int32_t nrhs, double *berr, sluamd_xrefine_t *out);
int sluamd_pzgsrfs3d_extra_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X,
                               int64_t ldx, int32_t nrhs, double *berr, sluamd_xrefine_t *out);
/* R = B - op(A) X of the ATTACHED matrix in the caller's ordering (B, X, R column-major, ld in values, R apart from B and X), and berr[j] (may be NULL) =
 * the componentwise backward error of column j as the refinement computes it.  extra = 0: the refinement's fp64 pass, bitwise (the same row text);
 * extra != 0: the pass of sluamd_p[dz]gsrfs3d_extra, every r_i one rounding of the exact residual up to second-order terms.  Any handle with an attached
 * matrix (on a grid every rank holds the complete matrix and computes the same).  nrhs == 0 returns 0.
 * Errors, SLUAMD_EINVAL with a message: null B, X or R, a leading dimension below n, trans outside {0, 1, 2}, a handle of the other precision, no
 * attached matrix. */
int sluamd_dResidual(sluamd_handle_t h, int trans, int extra, const double *B, int64_t ldb, const double *X, int64_t ldx, int32_t nrhs, double *R,
                     int64_t ldr, double *berr);
int sluamd_dResidual_dev(sluamd_handle_t h, int trans, int extra, const double *d_B, int64_t ldb, const double *d_X, int64_t ldx, int32_t nrhs,
                         double *d_R, int64_t ldr, double *berr);
int sluamd_zResidual(sluamd_handle_t h, int trans, int extra, const sluamd_doublecomplex *B, int64_t ldb, const sluamd_doublecomplex *X, int64_t ldx,
                     int32_t nrhs, sluamd_doublecomplex *R, int64_t ldr, double *berr);
int sluamd_zResidual_dev(sluamd_handle_t h, int trans, int extra, const sluamd_doublecomplex *d_B, int64_t ldb, const sluamd_doublecomplex *d_X,
                         int64_t ldx, int32_t nrhs, sluamd_doublecomplex *d_R, int64_t ldr, double *berr);

/* ---- Equil = YES: row / column equilibration on the device and the solve phase of the expert driver in the caller's ordering and
 * scaling (pdgsequ + pdlaqgs at the head of pdgssvx3d, SRC/double/pdgssvx3d.c:673-729; B scaled by R before the solve, :1450-1465;
 * X scaled by C after it, :1806-1821, the roles swapped for a transposed system).  For handles made by
 * sluamd_[dz]CreateLUHandleFromSymb[Grid]: there A's values exist on the host only in the caller's CSR, not in store form.
 *
 * sluamd_[dz]Equilibrate takes the arrays the handle was created from and attaches them like sluamd_[dz]AttachMatrix.  It computes
 * R[i] = 1 / max_j |a_ij| and C[j] = 1 / max_i |a_ij| R[i] with the smlnum / bignum clamps, rowcnd, colcnd and amax (pdgsequ.c:126-215;
 * complex16: abs1(z) = |re| + |im|, pzgsequ.c:136, :182), bit for bit what the host routine computes (maxima are exact).  info > 0 (row
 * i exactly zero: i + 1; column j: n + j + 1; pdgsequ.c:158-164, :202-208): it stops there with equed = SLUAMD_EQUED_N, nothing scaled,
 * and returns 0 like the reference.  Otherwise equed is decided as pdlaqgs does (THRESH = 0.1, small = 2^-1022 / 2^-52, large = 1 / small;
 * pdlaqgs.c:89-146), the ATTACHED values are scaled in place -- R: a r[i]; C: a c[j]; B: (a r[i]) c[j] in exactly that order, both
 * precisions (pzlaqgs.c:141 forms r[i] c[j] first; the order here cannot overflow in the product of the two scalings) --, R and C stay
 * on the device, and the scaled values are distributed into the store: the handle is then UNFACTORED and holds the scaled matrix, and a
 * later sluamd_dResetValues restores the scaled values, not the original ones.  anorm: the 1-norm (maximum column sum of the moduli;
 * complex16: the true modulus, as pzlangs) of the matrix the handle now holds, for thresh = eps_single * anorm; it is summed with fp64
 * atomics, so its low bits depend on the order: relative error of the summation <= k 2^-52 for a longest column of k entries; the
 * complex16 moduli come from the device's hypot, each within about one unit in the last place (2^-52) on top of that.
 * Errors, all SLUAMD_EINVAL with a message: a handle not created from the symbolic structure, n or rowptr[n] not those of the creation,
 * a handle of the other precision, a second call on the same handle.
 * Grid handles: every rank holds the complete A and computes the same R and C on its own (no communication; bitwise equal results).
 * After an equilibration the refinement entry points sluamd_p[dz]gsrfs3d[_dev] keep their contract: they refine the ATTACHED system,
 * which is now the scaled one (B' = R o B, X = C o X'); sluamd_[dz]AttachMatrix afterwards replaces the attached matrix. */
#define SLUAMD_EQUED_N 0
#define SLUAMD_EQUED_R 1
#define SLUAMD_EQUED_C 2
#define SLUAMD_EQUED_B 3
typedef struct sluamd_equil {
    int32_t equed;            /* SLUAMD_EQUED_N / _R / _C / _B */
    int32_t info;             /* 0; i+1: row i is exactly zero; n+j+1: column j is */
    double rowcnd, colcnd, amax;   /* what pdgsequ returns; a ratio it did not reach (info > 0) is 0 */
    double anorm;             /* 1-norm of the matrix the handle now holds (scaled unless equed == N) */
} sluamd_equil_t;
int sluamd_dEquilibrate(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                        const double *nzval, const sluamd_int_t *perm_c, sluamd_equil_t *out);
int sluamd_zEquilibrate(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                        const sluamd_doublecomplex *nzval, const sluamd_int_t *perm_c, sluamd_equil_t *out);
/* The same with R and C as INPUTS (host arrays of n positive finite values; either may be NULL): for scalings that come from elsewhere, above all from
 * sluamd_[dz]LargeDiag.  equed follows from which of them is non-NULL (both NULL: SLUAMD_EQUED_N, the call attaches the matrix and returns its norm).
 * Everything else is the contract of sluamd_[dz]Equilibrate: the attached values are scaled in place as (a r[i]) c[j] in exactly that order and distributed
 * into the store, the handle is UNFACTORED, anorm is that of the matrix the handle now holds, and a handle takes ONE equilibration of either kind.
 * rowcnd / colcnd are what pdgsequ defines, formed from the given vectors: max(min r, smlnum) / min(max r, bignum), 1 for a NULL vector; amax is that of
 * the unscaled matrix; info = 0.  Additional error (SLUAMD_EINVAL): a value of r or c that is not positive and finite. */
int sluamd_dEquilibrateWith(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                            const double *nzval, const sluamd_int_t *perm_c, const double *r, const double *c, sluamd_equil_t *out);
int sluamd_zEquilibrateWith(sluamd_handle_t h, sluamd_int_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                            const sluamd_doublecomplex *nzval, const sluamd_int_t *perm_c, const double *r, const double *c,
                            sluamd_equil_t *out);
/* R[n] and C[n] to the host (either may be NULL); both precisions; all ones where that side was not scaled (also before any
 * equilibration) */
int sluamd_GetScalings(sluamd_handle_t h, double *r, double *c);
/* The solve phase of the expert driver: B and X in the ORIGINAL ordering and scaling, column-major, ld in values; B is not modified.
 * Needs an attached matrix (for perm_c: sluamd_[dz]Equilibrate or sluamd_[dz]AttachMatrix); works with or without equilibration.
 *   xp[perm_c[i], j] = s_in[i] B[i, j];  the existing solve (sluamd_p[dz]gstrs3d_trans_dev) on xp;  X[i, j] = s_out[i] y[perm_c[i], j]
 * with SLUAMD_NOTRANS: s_in = R (if row-scaled), s_out = C (if column-scaled); SLUAMD_TRANS / SLUAMD_CONJ: s_in = C, s_out = R.
 * refine != 0: the refinement loop of sluamd_p[dz]gsrfs3d runs on the scaled system between solve and unscaling, as in the reference
 * (this path makes five passes over the n x nrhs block instead of two: X' gathered unscaled, B' = s_in o B formed in the work block for
 * the residuals, X unscaled in place at the end; each entry point also synchronises its stream once beside the waits of the wrapped calls);
 * berr[nrhs] and *steps as there (both may be NULL when refine == 0).  refine with SLUAMD_TRANS / SLUAMD_CONJ: SLUAMD_EINVAL here -- solve
 * with refine == 0, then refine the scaled system with sluamd_p[dz]gsrfs3d_trans[_dev] (b' = C o b, x' = x / R; the recipe is at their
 * declaration).  Grid handles: the replicated form (complete B in, complete X out, collective); SLUAMD_TRANS / SLUAMD_CONJ there after sluamd_PlanTransposedSweeps, else SLUAMD_EINVAL.
 * nrhs == 0 returns 0. */
int sluamd_pdgssvx3d_solve(sluamd_handle_t h, int trans, const double *B, int64_t ldb, double *X, int64_t ldx, int32_t nrhs,
                           int refine, double *berr, int32_t *steps);
int sluamd_pdgssvx3d_solve_dev(sluamd_handle_t h, int trans, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t nrhs,
                               int refine, double *berr, int32_t *steps);
int sluamd_pzgssvx3d_solve(sluamd_handle_t h, int trans, const sluamd_doublecomplex *B, int64_t ldb, sluamd_doublecomplex *X,
                           int64_t ldx, int32_t nrhs, int refine, double *berr, int32_t *steps);
int sluamd_pzgssvx3d_solve_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, sluamd_doublecomplex *d_X,
                               int64_t ldx, int32_t nrhs, int refine, double *berr, int32_t *steps);

/* ---- RowPerm = LargeDiag_MC64: the row permutation that maximises the product of the moduli on the diagonal, and the scalings that come with it (the
 * reference's default, dldperm_dist at pdgssvx3d.c:779-870).  This library pivots statically: a matrix whose large entries lie off the diagonal (zeros on
 * the diagonal: saddle-point and circuit matrices; rows that arrive in another order) needs this step before the symbolic factorisation.
 *
 * sluamd_[dz]LargeDiag takes no handle, like sluamd_order_nd.  A: n x n CSR, 0-based, n and rowptr[n] below 2^31 (else SLUAMD_EINVAL, as a column index
 * outside [0, n) or a descending rowptr); stored entries equal to zero are not edges; device = -1: the current device.  complex16: the modulus by hypot.
 *   perm_r[i] = j: row i of A is row j of Pr A (the reference's convention, pdgssvx3d.c:406) -- row i is matched to column j, a(i, j) lands on the diagonal.
 *   r[n] by original row, c[n] by column (either may be NULL): |r[i] a(i,j) c[j]| <= 1 for every entry, = 1 where j = perm_r[i].
 * Algorithm (Duff & Koster, SIAM J. Matrix Anal. Appl. 22, 2001: shortest augmenting paths on logarithmic costs), a hybrid:
 *   cost(i,j) = lg(cmax_j) - lg|a(i,j)| >= 0, cmax_j the largest modulus of column j; lg(x) = e + log2(m) for x = m 2^e, 1/2 <= m < 1 (frexp), so the
 *   logarithm of a power of two is an exact integer on the device and on any host.  Duals u, v: u_i + v_j <= cost(i,j), equality on the matched entries;
 *   r[i] = 2^u_i, c[j] = 2^v_j / cmax_j.
 *   Device: column maxima, costs, u_i = min_j cost(i,j), v_j = min_i (cost(i,j) - u_i); then proposal rounds on the tight entries ((cost - u_i) == v_j):
 *   every unmatched row proposes to its free tight column of lowest index, a column accepts the proposing row of lowest index; the rounds stop after one
 *   that matches nothing, when every row is matched, or after SLUAMD_ROWPERM_ROUNDS of them (environment, default 32).  All atomics are integer minima /
 *   maxima / sums and a launch only reads what an earlier launch wrote: the outcome does not depend on scheduling, two calls on the same input return
 *   bitwise equal perm_r, r, c and counters -- every rank of a grid may compute them on its own, as with sluamd_[dz]Equilibrate.
 *   Host: for every row still unmatched, in ascending order, a shortest augmenting path (Dijkstra on the reduced costs, binary heap, ties to the lower
 *   column), the dual update and the augmentation.  SLUAMD_ROWPERM_HOST=1 (environment) skips the proposal rounds, so the host matches every row: for A/B
 *   timing and tests; the optimum's value is the same, perm_r too where the optimum is unique.
 * out->info = k > 0: structurally singular, k rows cannot be matched; perm_r, r, c are not written; the call still returns 0.
 * A matrix whose moduli span more than 2^1000 can overflow r or c.
 * With the matching's scalings the scaled matrix has a unit diagonal (in modulus) and entries <= 1.  The reference composes them with pdgsequ's scalings;
 * this library applies them alone (sluamd_[dz]EquilibrateWith): a second equilibration of such a matrix has nothing left to balance. */
typedef struct sluamd_rowperm {
    int32_t info;            /* 0; k > 0: structurally singular, k rows cannot be matched (perm_r, r, c not written) */
    int32_t rounds;          /* proposal rounds run on the device */
    int64_t matched_device;  /* rows matched by the device phase */
    int64_t augmentations;   /* shortest augmenting paths found on the host */
} sluamd_rowperm_t;
int sluamd_dLargeDiag(int device, int64_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const double *nzval,
                      sluamd_int_t *perm_r, double *r, double *c, sluamd_rowperm_t *out);
int sluamd_zLargeDiag(int device, int64_t n, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const sluamd_doublecomplex *nzval,
                      sluamd_int_t *perm_r, double *r, double *c, sluamd_rowperm_t *out);
/* The handle was created from A1 = Pr A (and equilibrated with R indexed by A1's rows, R1[perm_r[i]] = r[i]): perm_r[n] (host) tells
 * sluamd_p[dz]gssvx3d_solve[_dev] that B and X are in A's ordering.  Either precision; with R, C, perm_c the handle's:
 *   SLUAMD_NOTRANS:          xp[perm_c[perm_r[i]]] = R[perm_r[i]] B[i];   X[j] = C[j] y[perm_c[j]]
 *   SLUAMD_TRANS / _CONJ:    xp[perm_c[j]] = C[j] B[j];                   X[i] = R[perm_r[i]] y[perm_c[perm_r[i]]]
 * With refine = 1 the loop runs on the attached (permuted, scaled) system, as without a row permutation.  The composed index and scaling vectors are built
 * once, on the device, by this call; they belong to the attached matrix: call it AFTER sluamd_[dz]EquilibrateWith / sluamd_[dz]AttachMatrix (a later
 * attach or equilibration drops the permutation) and before the factorisation.  sluamd_[dz]UpdateValues is unchanged: its values are those of the CSR the
 * handle was created from, that is A1.  Errors, all SLUAMD_EINVAL with a message: perm_r is not a permutation of 0 .. n-1; no matrix is attached; the
 * handle holds factors. */
int sluamd_SetRowPerm(sluamd_handle_t h, const sluamd_int_t *perm_r);

/* ---- Fact = SamePattern_SameRowPerm: new numeric values for the pattern the handle was planned for (superlu_defs.h:545-566; Newton steps, time
 * stepping, parameter sweeps).  For handles made by sluamd_[dz]CreateLUHandleFromSymb[Grid]; a view-created handle takes new values in store form through
 * sluamd_[dz]SetValues.  nzval: the values of the SAME CSR (rowptr / colind, rowptr[n] entries, the caller's order) the handle was created from.
 *  1. Pattern and permutations are reused: nothing of the plan, the tables, the tile records, the exchange plans or perm_c is rebuilt.  After the call the
 *     handle is UNFACTORED and holds the new matrix (sluamd_dGetDiagInv refuses until the next factorisation), and a later sluamd_dResetValues restores the
 *     NEW values.
 *  2. An equilibrated handle reuses R, C and equed, as the reference does for this value of Fact (pdgssvx3d.c:672-697: DiagScale, R and C are inputs and A is
 *     scaled with them): the values are stored as (a r[i]) c[j], in exactly the order sluamd_[dz]Equilibrate documents, so the result can be reproduced bit
 *     for bit on the host.  R and C are not recomputed, and sluamd_[dz]Equilibrate keeps refusing a second call; a caller whose new values have drifted far
 *     from the old scalings creates a new handle.  out->equed returns the handle's equed (SLUAMD_EQUED_N on a handle that was never equilibrated).
 *  3. out->anorm: the 1-norm of the matrix the handle now holds (scaled if equilibrated), for thresh = eps_single * anorm of the next sluamd_p[dz]gstrf3d; the
 *     definition and the summation caveat of sluamd_equil_t::anorm (fp64 atomics: relative error <= k 2^-52 for a longest column of k entries; complex16: the
 *     true modulus).  Computed only when out != NULL, and only with an attached matrix: a handle created from the symbolic structure keeps rowptr / colind on
 *     the device only with one, and no second copy of the structure is kept for the norm -- out != NULL without an attached matrix: SLUAMD_EINVAL.
 *  4. A matrix attached by sluamd_[dz]AttachMatrix or sluamd_[dz]Equilibrate receives the new (scaled) values too, in CSR order: sluamd_p[dz]gsrfs3d and
 *     sluamd_p[dz]gssvx3d_solve(..., refine = 1) then refine the NEW system.  It must be the matrix the handle was created from (same number of entries,
 *     else SLUAMD_EINVAL).  If nothing is attached, nothing is attached by this call.
 *  5. Grid handles: every rank passes the complete value array, as at creation, and updates its own entries.  No communication: the call is not collective
 *     and may run on the ranks in any order, but EVERY rank must have made it before the next (collective) factorisation.
 *  6. Ordering: the host-pointer form stages the values through a device buffer the handle keeps (it grows once) and returns when the stream work is queued
 *     and the staging copy is complete (nzval may be reused at once).  The _dev form only queues work on the handle's stream and reads d_nzval in stream
 *     order: the caller keeps it alive and unchanged until the next synchronising call on the handle (a factorisation, a solve, a call with out != NULL);
 *     what produced d_nzval on another stream must be complete before the call.  With out != NULL both forms synchronise once, to return anorm.
 *  7. Errors, all SLUAMD_EINVAL with a message in sluamd_last_error() and the handle untouched: null handle or null values; a handle not created from the
 *     symbolic structure (the message names sluamd_dSetValues); a handle of the other precision; the two cases of 3. and 4.
 * The first update of a handle whose values are scaled also builds, on the device, the (row, column) of every owned entry (8 bytes each) from the attached
 * structure; it is not built at creation, which every handle pays. */
typedef struct sluamd_update {
    double anorm;             /* 1-norm of the matrix the handle now holds (scaled if equilibrated) */
    int32_t equed;            /* the handle's SLUAMD_EQUED_* (unchanged by the call) */
    int32_t reserved;
} sluamd_update_t;
int sluamd_dUpdateValues(sluamd_handle_t h, const double *nzval, sluamd_update_t *out);                   /* host pointer   */
int sluamd_dUpdateValues_dev(sluamd_handle_t h, const double *d_nzval, sluamd_update_t *out);             /* device pointer */
int sluamd_zUpdateValues(sluamd_handle_t h, const sluamd_doublecomplex *nzval, sluamd_update_t *out);
int sluamd_zUpdateValues_dev(sluamd_handle_t h, const sluamd_doublecomplex *d_nzval, sluamd_update_t *out);

/* ---- Fixed-size batches: `count` systems A_k X_k = B_k of order m that share ONE sparsity pattern and differ in values, with info, berr and refinement steps
 * per matrix (the role of the reference's pdgssvx3d_csc_batch, SRC/double/pdgssvx3d_csc_batch.c, reached through pddrive3d -b).  Time stepping and ensembles:
 * hundreds of small systems, each of which would pay its own symbolic factorisation, plan, tables and arena as a handle of its own, with kernels too small
 * to fill the device.  The batch is the block-diagonal matrix diag(A_0 .. A_{count-1}) on ONE ordinary 1 x 1 x 1 handle, planned for the replicated
 * structure (sluamd_symb_replicate): count copies of one elimination tree are count-wide DAG levels of the same kernels.
 *   s: the symbolic structure of ONE matrix (maxsup <= 256), rowptr / colind its CSR pattern, perm_c_final the perm_c_out of its symbolic factorisation;
 *   nzval: matrix k's values at nzval + k stride (stride >= nnz), in the order of the shared CSR;
 *   B, X: matrix k's m x nrhs column-major block at B + k strideB / X + k strideX, leading dimensions ldb, ldx >= m, the caller's ordering.
 * sluamd_dBatchCreate plans once and distributes the values; sluamd_dBatchUpdateValues[_dev] is the same distribution path for new values of the same pattern
 * (Fact = SamePattern_SameRowPerm) and leaves the batch UNFACTORED; the _dev form reads d_nzval in the order of the handle's stream and the caller keeps it
 * unchanged until the next synchronising call (a factorisation or a solve).  The values are gathered through the entry map of one matrix plus the per-copy
 * offset; no count-times-larger map exists.
 * sluamd_dBatchFactor: info[k] = the smallest column of matrix k (1-based, in A_k's numbering after perm_c) whose U diagonal entry is exactly zero, else 0 --
 * what sluamd_pdgstrf3d returns for A_k factored alone under SLUAMD_INFO_FIRST.  A singular A_k disturbs no other matrix: its inf / NaN stay inside its own
 * blocks, and so do its solutions'.
 * sluamd_dBatchSolve[_dev]: pack (xp[k m + perm_c[i], j] = B_k[i, j]), the handle's solve (trans = SLUAMD_NOTRANS / _TRANS / _CONJ), unpack: the only passes over
 * the right-hand sides when refine == 0.  refine != 0: the loop of sluamd_pdgsrfs3d -- of sluamd_pdgsrfs3d_trans for SLUAMD_TRANS / SLUAMD_CONJ: the residual
 * of A_k^T x = b / A_k^H x = b over the transposed index of the attached matrix, the correction by the transposed sweeps -- with the stopping rule
 * per matrix -- berr[k nrhs + j], steps[k] (those of the last right-hand side), SAFE1 / SAFE2 formed from m so that a matrix sees the constants it would see
 * alone; one copy of count doubles to the host per sweep; a column ends when no matrix continues; a matrix that has stopped keeps the X and berr of its
 * stopping sweep while the others go on.  The loop refines against the matrix ATTACHED to the batch's handle, which is the batch's own block-diagonal
 * matrix (order count m, column k m + j for entry (i, j) of matrix k) unless the caller attached another one through sluamd_BatchHandle; such a matrix
 * must be block diagonal too (the residual of matrix k reads X_k only), and sluamd_dBatchUpdateValues refuses while it is attached.
 * berr and steps may be NULL when refine == 0 (steps is then all zero).  nrhs == 0 returns 0.
 * sluamd_BatchHandle: the handle, borrowed (sluamd_get_stats, sluamd_setup_times, sluamd_plan_table; it dies with the batch).
 * Not available on a batch: process grids (no entry point takes one), RowPerm and the single-matrix sluamd_[dz]Equilibrate made through the
 * borrowed handle (every later batch call returns SLUAMD_EINVAL), replace_tiny_pivot (it needs a threshold
 * eps anorm_k per matrix inside the diagonal LU kernels), supernodes wider than 256 columns.  Other errors (SLUAMD_EINVAL): count <= 0, stride < nnz,
 * ldb or ldx < m, strides smaller than a block, a solve of an unfactored batch, refine without berr.
 * sluamd_dBatchEquilibrate: pdgsequ + pdlaqgs PER MATRIX, once per batch, before the factorisation.  out[k] is what sluamd_dEquilibrate returns for A_k alone:
 * equed, rowcnd, colcnd, amax, R and C (sluamd_BatchGetScalings: count m values each, matrix-major, ones where a side is not scaled) bit for bit -- the maxima
 * are exact --, anorm with the summation caveat of sluamd_equil_t::anorm.  A matrix with an exactly zero row or column gets its own out[k].info (i + 1, or
 * m + j + 1, in its own numbering) and stays unscaled with equed = N; the others proceed.  The scaled values replace the attached ones and are distributed
 * into the store: the batch is UNFACTORED afterwards.  sluamd_dBatchUpdateValues[_dev] on an equilibrated batch re-applies the stored R, C and equed of every
 * matrix, (a r[i]) c[j] in that order, as sluamd_dUpdateValues does.  sluamd_dBatchSolve takes B and returns X in the caller's scaling (B scaled by R, X by C;
 * the roles swapped for a transposed system); with refine the scaled system is refined and berr is that of the scaled system, as in the reference.
 * Errors (SLUAMD_EINVAL): a second call; a batch whose handle had another matrix attached, or was equilibrated / row-permuted through sluamd_BatchHandle
 * (every batch call refuses such a handle).
 * complex16 (the role of pzgssvx3d_csc_batch): the sluamd_zBatch* calls are the twins of the sluamd_dBatch* calls with the same contract on a complex16 handle;
 * values, B and X are sluamd_doublecomplex, strides and leading dimensions count values, R, C and berr are real.  SLUAMD_TRANS solves A_k^T x = b, SLUAMD_CONJ
 * A_k^H x = b (on a double batch the two are the same).  sluamd_zBatchFactor: a U diagonal entry is zero when it is exactly 0 + 0i.  sluamd_zBatchEquilibrate:
 * out[k] is what sluamd_zEquilibrate returns for A_k alone (maxima of |re| + |im|, anorm of the moduli).  Refinement: berr from the moduli |re| + |im| of
 * sluamd_pzgsrfs3d.  sluamd_BatchGetScalings, sluamd_BatchHandle and sluamd_BatchDestroy serve both precisions.  A d call on a complex16 batch and a z call on
 * a double batch return SLUAMD_EINVAL with a message that names the other call. */
typedef struct sluamd_batch_s *sluamd_batch_t;
int sluamd_dBatchCreate(sluamd_batch_t *b, sluamd_symb_t s, int32_t count, const sluamd_int_t *rowptr, const sluamd_int_t *colind, const double *nzval,
                        int64_t stride, const sluamd_int_t *perm_c_final, const sluamd_options_t *opt);
int sluamd_dBatchUpdateValues(sluamd_batch_t b, const double *nzval, int64_t stride);
int sluamd_dBatchUpdateValues_dev(sluamd_batch_t b, const double *d_nzval, int64_t stride);
int sluamd_dBatchEquilibrate(sluamd_batch_t b, sluamd_equil_t *out /* [count] */);
int sluamd_BatchGetScalings(sluamd_batch_t b, double *r /* [count m] */, double *c /* [count m] */);
int sluamd_dBatchFactor(sluamd_batch_t b, int32_t *info /* [count] */);
int sluamd_dBatchSolve(sluamd_batch_t b, int trans, const double *B, int64_t ldb, int64_t strideB, double *X, int64_t ldx, int64_t strideX, int32_t nrhs,
                       int refine, double *berr /* [count * nrhs] */, int32_t *steps /* [count] */);
int sluamd_dBatchSolve_dev(sluamd_batch_t b, int trans, const double *d_B, int64_t ldb, int64_t strideB, double *d_X, int64_t ldx, int64_t strideX, int32_t nrhs,
                           int refine, double *berr, int32_t *steps);
int sluamd_zBatchCreate(sluamd_batch_t *b, sluamd_symb_t s, int32_t count, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                        const sluamd_doublecomplex *nzval, int64_t stride, const sluamd_int_t *perm_c_final, const sluamd_options_t *opt);
int sluamd_zBatchUpdateValues(sluamd_batch_t b, const sluamd_doublecomplex *nzval, int64_t stride);
int sluamd_zBatchUpdateValues_dev(sluamd_batch_t b, const sluamd_doublecomplex *d_nzval, int64_t stride);
int sluamd_zBatchEquilibrate(sluamd_batch_t b, sluamd_equil_t *out /* [count] */);
int sluamd_zBatchFactor(sluamd_batch_t b, int32_t *info /* [count] */);
int sluamd_zBatchSolve(sluamd_batch_t b, int trans, const sluamd_doublecomplex *B, int64_t ldb, int64_t strideB, sluamd_doublecomplex *X, int64_t ldx,
                       int64_t strideX, int32_t nrhs, int refine, double *berr /* [count * nrhs] */, int32_t *steps /* [count] */);
int sluamd_zBatchSolve_dev(sluamd_batch_t b, int trans, const sluamd_doublecomplex *d_B, int64_t ldb, int64_t strideB, sluamd_doublecomplex *d_X, int64_t ldx,
                           int64_t strideX, int32_t nrhs, int refine, double *berr, int32_t *steps);
sluamd_handle_t sluamd_BatchHandle(sluamd_batch_t b);
void sluamd_BatchDestroy(sluamd_batch_t b);

/* ---- The adjoint value gradient: sensitivities of a solve with respect to the stored values of A, from the attached pattern (PDE-constrained optimisation,
 * implicit layers, parameter fitting around sluamd_[dz]UpdateValues).  For X = op(A)^-1 B and a real scalar loss with gradient Gbar = d loss / d conj(X) (the
 * convention of PyTorch's complex autograd; for real data simply d loss / d X), the gradient with respect to B is one solve with the adjoint operator, Lam, and the
 * gradient with respect to the stored entry e = (i, j) of A is a sampled outer product of Lam and X:
 *   SLUAMD_NOTRANS (A X = B):    G[e] = - sum_r Lam[i, r] conj(X[j, r]),   Lam = A^-H Gbar              (sluamd_p[dz]gssvx3d_solve with SLUAMD_CONJ)
 *   SLUAMD_TRANS   (A^T X = B):  G[e] = - sum_r conj(X[i, r]) Lam[j, r],   Lam = conj(A)^-1 Gbar = conj(A^-1 conj(Gbar))    (SLUAMD_NOTRANS on conj(Gbar), conjugated)
 *   SLUAMD_CONJ    (A^H X = B):  G[e] = - sum_r X[i, r] conj(Lam[j, r]),   Lam = A^-1 Gbar               (SLUAMD_NOTRANS)
 * Real handles: conjugation is the identity, and SLUAMD_TRANS is SLUAMD_CONJ.  trans names the system that was SOLVED; the caller computes Lam.
 * G[nnz]: in the entry order of the CSR the handle was created from, which is the attached one (sluamd_[dz]AttachMatrix / sluamd_[dz]Equilibrate); a duplicated
 * (i, j) receives the full value in each of its entries (the derivative of a matrix whose duplicates sum).  Lam and X: n x nrhs, column-major, leading dimensions
 * ldl, ldx >= n counted in values, in the caller's ordering and scaling -- what sluamd_p[dz]gssvx3d_solve returns, so an equilibrated handle needs nothing
 * special: the call reads only the PATTERN of the attached matrix, neither its values nor the factors (the handle need not be factored).
 * One thread per stored entry writes G[e], the sum over r ascending in fused multiply-adds, no atomics: two calls return the same bits.  nrhs > 32 runs in panels
 * of 32 right-hand sides, every panel after the first accumulating into G in that order.  nrhs == 0 zero-fills G.
 * The first call builds, on the device, the row of every entry (4 bytes each); the host form stages Lam, X and G through a block the handle keeps (it grows
 * only); both belong to the attached matrix and go with it.  Both forms synchronise the handle's stream before returning; what produced the device blocks on
 * another stream must be complete before the call.
 * Errors, all SLUAMD_EINVAL with a message: null handle or pointers, nrhs < 0, ldl or ldx < n, a trans other than the three, a handle of the other precision
 * (the message names the twin), no attached matrix, a grid handle, a handle that carries a row permutation (sluamd_SetRowPerm: its entries are those of Pr A),
 * the handle of a batch.
 * sluamd_[dz]BatchAdjointValues[_dev]: the same for every matrix of a batch in one launch -- matrix k's Lam, X and G at k strideL, k strideX, k strideG (values;
 * strideL >= ldl (nrhs - 1) + m, strideX likewise, strideG >= nnz of ONE matrix), the shared pattern read once. */
int sluamd_dAdjointValues(sluamd_handle_t h, int trans, const double *Lam, int64_t ldl, const double *X, int64_t ldx, int32_t nrhs, double *G);
int sluamd_dAdjointValues_dev(sluamd_handle_t h, int trans, const double *d_Lam, int64_t ldl, const double *d_X, int64_t ldx, int32_t nrhs, double *d_G);
int sluamd_zAdjointValues(sluamd_handle_t h, int trans, const sluamd_doublecomplex *Lam, int64_t ldl, const sluamd_doublecomplex *X, int64_t ldx, int32_t nrhs,
                          sluamd_doublecomplex *G);
int sluamd_zAdjointValues_dev(sluamd_handle_t h, int trans, const sluamd_doublecomplex *d_Lam, int64_t ldl, const sluamd_doublecomplex *d_X, int64_t ldx,
                              int32_t nrhs, sluamd_doublecomplex *d_G);
int sluamd_dBatchAdjointValues(sluamd_batch_t b, int trans, const double *Lam, int64_t ldl, int64_t strideL, const double *X, int64_t ldx, int64_t strideX,
                               int32_t nrhs, double *G, int64_t strideG);
int sluamd_dBatchAdjointValues_dev(sluamd_batch_t b, int trans, const double *d_Lam, int64_t ldl, int64_t strideL, const double *d_X, int64_t ldx, int64_t strideX,
                                   int32_t nrhs, double *d_G, int64_t strideG);
int sluamd_zBatchAdjointValues(sluamd_batch_t b, int trans, const sluamd_doublecomplex *Lam, int64_t ldl, int64_t strideL, const sluamd_doublecomplex *X,
                               int64_t ldx, int64_t strideX, int32_t nrhs, sluamd_doublecomplex *G, int64_t strideG);
int sluamd_zBatchAdjointValues_dev(sluamd_batch_t b, int trans, const sluamd_doublecomplex *d_Lam, int64_t ldl, int64_t strideL, const sluamd_doublecomplex *d_X,
                                   int64_t ldx, int64_t strideX, int32_t nrhs, sluamd_doublecomplex *d_G, int64_t strideG);

/* ------------------------------------------------------------------------------------------------
 * Process grids: nprow x npcol x npdep ranks, one rank per GPU (gridinfo3d_t, superlu_defs.h:385-420).
 *
 * The reference exchanges panels with MPI inside pdgstrf3d / pdgstrs3d:
 *   - inside a 2-D layer, per supernode k: the factored diagonal block goes down process column k % Pc and along process
 *     row k % Pr (dDiagFactIBCast, dtrfCommWrapper.c:32-118), the L panel along the process rows and the U panel down the
 *     process columns (dIBcastRecvLPanel / dIBcastRecvUPanel, dtrfCommWrapper.c:377-548, dcommunication_aux.c:32-430);
 *   - between layers, after every level of the elimination forest: the pairwise sum of the replicated ancestor panels
 *     (dreduceAllAncestors3d, pd3dcomm.c:1046-1081) and MPI_Allreduce(MIN) of info (pdgstrf3d.c:388-392);
 *   - in the solve: x_k down the process column, lsum along the process row, and the Z exchanges of the ancestor part of
 *     x (pdgstrs3d.c:1405-1535, :7180-7181).
 * Here all of it runs inside the library, in C, over a communicator object: RCCL called directly (ncclSend / ncclRecv
 * groups on the library's HIP streams, so an exchange overlaps the Schur tiles of the previous level), or a transport
 * supplied by the application (MPI in the reference-side binding of INTEGRATION.md), or an in-process world (tests).
 * World rank of grid position (row, col, z) = (z * nprow + row) * npcol + col  (layer-major, superlu_grid3d.c).
 * ------------------------------------------------------------------------------------------------ */
typedef struct sluamd_comm_s *sluamd_comm_t;

#define SLUAMD_UNIQUE_ID_BYTES 128
/* RCCL: rank 0 calls sluamd_comm_rccl_unique_id and ships the 128 bytes to every rank by any means (MPI_Bcast, a file,
 * a torch.distributed store); every rank then calls sluamd_comm_create_rccl (collective: ncclCommInitRank). */
int sluamd_comm_rccl_unique_id(void *id128);
int sluamd_comm_create_rccl(sluamd_comm_t *comm, const void *id128, int nprow, int npcol, int npdep, int myrow, int mycol,
                            int myz, int device);

/* Application-supplied transport on HOST buffers (the library stages device ranges through pinned memory).  isend / irecv
 * start one message to / from world rank `peer` (messages between one pair of ranks match in the order they were
 * started); waitall completes every message started since the last waitall; allreduce_min_i32 runs over the whole grid.
 * All return 0 on success. */
typedef struct sluamd_comm_callbacks {
    void *ctx;
    int (*isend)(void *ctx, const void *buf, int64_t bytes, int peer);
    int (*irecv)(void *ctx, void *buf, int64_t bytes, int peer);
    int (*waitall)(void *ctx);
    int (*allreduce_min_i32)(void *ctx, int32_t *v);
} sluamd_comm_callbacks_t;
int sluamd_comm_create_callbacks(sluamd_comm_t *comm, const sluamd_comm_callbacks_t *cb, int nprow, int npcol, int npdep,
                                 int myrow, int mycol, int myz);

/* In-process world: comms[nprow*npcol*npdep] (indexed by world rank), one per thread; any number of ranks per device. */
int sluamd_comm_create_local(sluamd_comm_t *comms, int nprow, int npcol, int npdep);
/* Transport self-test (collective): ring exchange of `bytes` bytes as one stream-ordered group between device fills, the
 * host-buffer group and the min-all-reduce -- every operation the drivers use of a transport; 0 when all data arrived intact.
 * On a one-rank communicator every message goes to the rank itself. */
int sluamd_comm_selftest(sluamd_comm_t comm, int64_t bytes);
int sluamd_comm_rank(sluamd_comm_t comm);
int sluamd_comm_size(sluamd_comm_t comm);
void sluamd_comm_destroy(sluamd_comm_t comm);

/* sluamd_dCreateLUHandle for one rank of a process grid (collective over `comm`): `lu` is that rank's dLocalLU_t view
 * (pointer arrays of ceil(nsupers/npcol) block columns and ceil(nsupers/nprow) block rows, local index lk = k / npcol,
 * lb = k / nprow; superlu_defs.h:270-279), `forests` its dtrf3Dpartition_t (required when npdep > 1).  The index arrays
 * of the panels a rank will receive are exchanged once here (the reference ships them with every panel message,
 * dIBcast_LPanel, dcommunication_aux.c:32-60).  The handle then works with the single-rank entry points:
 * sluamd_pdgstrf3d / sluamd_pdgstrs3d[_dev] / sluamd_dCopyLU2Host / sluamd_dSetValues become collective calls.
 * `comm` must outlive the handle. */
int sluamd_dCreateLUHandleGrid(sluamd_handle_t *h, const sluamd_dLUview_t *lu, const sluamd_forest_view_t *forests,
                               const sluamd_options_t *opt, sluamd_comm_t comm);
/* complex16 on any nprow x npcol x npdep grid (pzgstrf3d.c: XY panel exchange -- ztrfCommWrapper.c, zcommunication_aux.c --, the 333-392 ancestor
 * reduction; the distributed pzgstrs3d): complex16 values travel as pairs of doubles through the double path's exchange plans; collective like
 * sluamd_dCreateLUHandleGrid */
int sluamd_zCreateLUHandleGrid(sluamd_handle_t *h, const sluamd_zLUview_t *lu, const sluamd_forest_view_t *forests,
                               const sluamd_options_t *opt, sluamd_comm_t comm);
/* Same from the library's own symbolic factorisation (every rank holds the complete structure `s`; no structure exchange):
 * the store of this rank's grid position is built and A's values are distributed on the device (pddistribute3d +
 * dinit3DLUstructForest, pddistribute3d.c:1357, pd3dcomm.c:334-800).  sn_tree (sluamd_symb_partition) may be NULL when
 * npdep == 1. */
int sluamd_dCreateLUHandleFromSymbGrid(sluamd_handle_t *h, sluamd_symb_t s, const sluamd_int_t *rowptr,
                                       const sluamd_int_t *colind, const double *nzval, const sluamd_int_t *perm_c_final,
                                       const sluamd_options_t *opt, const int32_t *sn_tree, sluamd_comm_t comm);
/* complex16 twin */
int sluamd_zCreateLUHandleFromSymbGrid(sluamd_handle_t *h, sluamd_symb_t s, const sluamd_int_t *rowptr, const sluamd_int_t *colind,
                                       const sluamd_doublecomplex *nzval, const sluamd_int_t *perm_c_final,
                                       const sluamd_options_t *opt, const int32_t *sn_tree, sluamd_comm_t comm);
/* Grid solve, replicated form (sluamd_pdgstrs3d[_dev] on a grid handle): every rank passes the COMPLETE permuted right-hand side
 * x = Pc*Pr*b (n x nrhs) and every rank receives the complete solution (direct all-gather of the owners' rows).
 *
 * Grid solve, distributed form = the boundary of the reference's pdgstrs3d[_newsolve] (pdgstrs3d.c:6604, :6935) including
 * pdReDistribute3d_B_to_X (:6265) and pdReDistribute3d_X_to_B (:6404): B is distributed by block rows over the processes of
 * layer 0 -- this rank holds rows [fst_row, fst_row + m_loc) of the ORIGINAL right-hand side, column-major with leading dimension
 * ldb (NRformat_loc); ranks of the other layers pass m_loc = 0 -- and is overwritten by rows of the solved vector y (L U y = x).
 * perm_in[i]  = row of the factored system that row i of B goes to: x[perm_in[i]] = B[i], i.e. ScalePermstruct->perm_c[perm_r[i]];
 * perm_out[i] = row of y returned in row i: B[i] = y[perm_out[i]].  The reference returns the rows of the PERMUTED solution
 *               (perm_out = identity; pdgssvx3d applies Pc^T itself); perm_out = perm_c gives x in the original order.
 * Both are replicated on every rank; NULL = identity.  Every row travels once to the rank that consumes it and every row of the
 * solution once back; nothing is replicated.  Collective on grid handles; works on single-rank handles too (m_loc = n). */
int sluamd_pdgstrs3d_dist(sluamd_handle_t h, double *B, int64_t ldb, int32_t nrhs, int64_t m_loc, int64_t fst_row,
                          const sluamd_int_t *perm_in, const sluamd_int_t *perm_out);
/* complex16 twin: the boundary of pzgstrs3d[_newsolve] (SRC/complex16/pzgstrs3d.c) */
int sluamd_pzgstrs3d_dist(sluamd_handle_t h, sluamd_doublecomplex *B, int64_t ldb, int32_t nrhs, int64_t m_loc, int64_t fst_row,
                          const sluamd_int_t *perm_in, const sluamd_int_t *perm_out);

#ifdef __cplusplus
}
#endif
#endif /* SUPERLU_DIST_AMD_H */
