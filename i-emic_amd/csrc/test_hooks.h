/*
 * test_hooks.h -- entry points that drive the dense solvers of the preconditioner on their
 * own (schur_cr.h, band_lu.hip) for tests/test_gpu_dense.py, and the coupled model's
 * preconditioner (coupled.hip) for tests/test_gpu_coupled_krylov.py, and the DCGS2 update pass
 * (krylov.hip) for tests/test_dcgs_fused_coef.py, and the T/S multigrid's plan, levels and
 * fusion switch (iemic_test_ts_mg_plan, iemic_test_ts_mg_level, iemic_test_ts_mg_nofuse;
 * ts_mg.hip, ts_mg_setup.hip) for tests/test_gpu_ts_mg.py, its entry launch and the packed
 * operand's switch (iemic_test_ts_mg_entry, iemic_test_ts_mg_nopack) for
 * tests/test_gpu_ts_entry_pack.py, and the Ritz-vector and residual
 * kernels of the stability analysis (eigs.hip) for tests/test_gpu_eigs.py, and the active set with its
 * tile descriptors, the compressed SpMV beside the full one and the dynamics defect
 * (iemic_test_active_set, iemic_test_spmv_c, iemic_test_dyn_defect; active_set.hip, spmv.hip) for
 * tests/test_gpu_spmv_tiles.py, and the projected model's block product and Gram product
 * (iemic_test_spmm, iemic_test_spmm_kb, iemic_test_gram, iemic_test_gram_cost,
 * iemic_test_solver_calls; spmv.hip,
 * projected.hip) for tests/test_gpu_projected.py.  They are exported from the
 * device library but are NOT part of its public ABI (include/iemic.h, IEMIC_ABI_VERSION):
 * tests/dense_hooks.py binds them.  All pointers are host pointers; every hook runs on the
 * context's stream, owns its device buffers and returns the usual IEMIC_* codes.
 */
#ifndef IEMIC_TEST_HOOKS_H
#define IEMIC_TEST_HOOKS_H

#include "../../include/iemic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IEMIC_TEST_PLAN_LEN 128

/* Block cyclic reduction of the n m x n m block tridiagonal system
 *     L_i x_{i-1} + D_i x_i + R_i x_{i+1} = b_i      (periodic: indices mod n)
 * D, L, R: n m x m column-major blocks each (cr_factor_blocks); D == NULL: the level-0 blocks
 * come from the 9-point rows S9 (n m x 9) and col_of_ij (m x n) through cr_factor.
 * nsolve right-hand sides b (nsolve x n m) are solved one after another on the same SchurCR
 * into x, and into xT (transposed order, may be NULL).  *info: the device flag cr_check reads;
 * cr_check's error is returned.  plan (IEMIC_TEST_PLAN_LEN ints): nlev, lt, tM, ncomp,
 * nsteps, then for each down step and then each up step rc, nwg, cls.ncls, levels spanned. */
int iemic_test_cr_solve(iemic_ctx* ctx, int n, int m, int periodic, int tail_max, const double* D,
                        const double* L, const double* R, const double* S9, const int* col_of_ij,
                        int nsolve, const double* b, double* x, double* xT, int* info, int* plan);

/* One SchurCR factorised with the blocks (D1, L1, R1) and solved for b, then factorised again
 * with (D2, L2, R2) and solved for b into x: what every Newton step does. */
int iemic_test_cr_refactor(iemic_ctx* ctx, int n, int m, int periodic, int tail_max, const double* D1,
                           const double* L1, const double* R1, const double* D2, const double* L2,
                           const double* R2, const double* b, double* x);

/* The batched Gauss-Jordan inverse as the levels call it: A holds nsrc m x m column-major
 * blocks, block s0 + k sstep is inverted into X block k (k < count).  *info: the device flag. */
int iemic_test_cr_inverse(iemic_ctx* ctx, int m, int count, int s0, int sstep, int nsrc, const double* A,
                          double* X, int* info);

/* band_lu_inverse with cols = 0 .. N-1: ab (N x (2 bl + bu + 1), gbtrf layout by rows) comes
 * back factorised, piv (N) and X (N x N row-major; untouched when *info != 0) are written,
 * *stage_o reports the branch of k_band_lu.  Shapes whose LDS need exceeds the device's are
 * refused with IEMIC_EINVAL before any launch (*stage_o is still set). */
int iemic_test_band_inverse(iemic_ctx* ctx, int N, int bl, int bu, double* ab, int* piv, double* X, int* info,
                            int* stage_o);

/* The coupled model's forward block Gauss-Seidel preconditioner (cpl_prec, coupled.hip) on
 * host vectors [ocean (reference order) | atmosphere]: pack, z_o = M_o^-1 r_o,
 * z_a = M_a^-1 (r_a - C_ao z_o), unpack; use_prec == 0: z = r.  The Jacobians must be current.
 * The atmosphere's preconditioner is computed first when it is not current (prec_valid).
 * The ocean's is computed, in its default kind, only when none was ever computed: a new ocean
 * Jacobian does not mark it stale, so the caller rebuilds it, as iemic_coupled_solve does
 * before every solve.  The device copy of z starts as NaN bit patterns, so an entry that
 * cpl_prec does not write comes back as NaN. */
int iemic_test_coupled_prec(iemic_coupled* cm, const double* r_host, double* z_host, int use_prec);

/* The DCGS2 update pass of one Arnoldi step (dcgs_update, krylov.hip) on host data: nv basis
 * vectors Q (nv x ldq, ldq >= N even), the summed dot rows hb (2 nv + 5; rows 2 nv + 3, 2 nv + 4
 * come back as beta, h_jj), u and w (N even; both overwritten).  fused != 0: the solve's
 * launch, coefficients formed in the update's prologue; fused == 0: k_dcgs_coef and the
 * update from its coefficient array.  hrows (2 nv + 5): what the kernels stored into the
 * solve's pinned slot (NaN bit patterns where they stored nothing).  act != NULL (N a
 * multiple of 6): the new w also goes into the planar rrP (6 planes of ps cells, cell act[a]
 * < ps of compressed cell a; NaN bit patterns elsewhere). */
int iemic_test_dcgs_update(iemic_ctx* ctx, int fused, int nv, int64_t N, int64_t ldq, const double* Q, double* hb,
                           double* u, double* w, double* hrows, const int* act, int64_t ps, double* rrP);

/* The T/S multigrid of the block Gauss-Seidel preconditioner as it was last set up (one rank).
 * plan (IEMIC_TEST_PLAN_LEN ints): nlev, the lane count P, sweeps, hr, the coarsest level's
 * assembly (0 device inverse, 1 cyclic reduction, 2 host), then per level n, m, par, the
 * colour count and 1 where mg_fused holds. */
int iemic_test_ts_mg_plan(iemic_ctx* ctx, int* plan);

/* Level q after the last apply, in the halo-free order (component, jl, i, k): off (16 x ncl), diag
 * (4 x ncl), the right-hand side b and the iterate z (2 x ncl each; z is the one the level
 * hands upward, zu on a fused level), ncl = n m l; cinv ((2 ncl)^2, row-major) when q is the
 * coarsest level (else it may be NULL). */
int iemic_test_ts_mg_level(iemic_ctx* ctx, int q, double* off, double* diag, double* b, double* z, double* cinv);

/* on != 0: no level is visited by the fused launches (k_mg_dn / k_mg_up) until it is cleared */
int iemic_test_ts_mg_nofuse(iemic_ctx* ctx, int on);

/* on != 0: the T/S solve's entry launch reads the slot-major Jacobian (k_mg_entry) instead of
 * the packed operand (k_mg_entry_p) until it is cleared: the pack's reference and A/B switch */
int iemic_test_ts_mg_nopack(iemic_ctx* ctx, int on);

/* The entry launch alone (ts_mg_entry) from host data: rr and zd are component-planar vectors
 * of NE = 6 x ext cells doubles (the planar right-hand side and the dynamics iterate); level
 * 0's right-hand side b and iterate z come back as in iemic_test_ts_mg_level (2 x ncl each;
 * the device copies start as NaN bit patterns).  *pack_doubles (may be NULL): the doubles of
 * the packed operand.  The preconditioner's own planar right-hand side is put back. */
int iemic_test_ts_mg_entry(iemic_ctx* ctx, int64_t NE, const double* rr, const double* zd, double* b, double* z,
                           int64_t* pack_doubles);

/* k_eig_ritz (eigs.hip) on an arbitrary basis: V (j x ldv, ldv >= N), Y (j x p row-major),
 * X (p x N) = the p combinations sum_i Y[i][q] V_i over the first N entries of every row; the
 * device copy of X starts as NaN bit patterns. */
int iemic_test_eig_ritz(iemic_ctx* ctx, int j, int p, int64_t N, int64_t ldv, const double* V, const double* Y,
                        double* X);

/* k_eig_compress (eigs.hip) on an arbitrary basis, in place: V ((j + 1) x ldv, ldv >= N, in-out),
 * Q (j x p row-major), 1 <= p < j <= IEMIC_EIGS_MAX_M, p <= 16.  On return columns 0 .. p - 1 hold
 * sum_i Q[i][q] V_i and column p the old column j over the first N entries of every row; the
 * whole device copy comes back, so the caller sees what else was written. */
int iemic_test_eig_compress(iemic_ctx* ctx, int j, int p, int64_t N, int64_t ldv, double* V, const double* Q);

/* Measurement helper: on a basis of j + 1 vectors of the context's own layout, GPU milliseconds
 * (events) of nrep thick-restart compressions by k_eig_compress (ms[0 .. nrep)) and of what
 * it replaces (ms[nrep .. 2 nrep)): k_eig_ritz into p scratch vectors, p copies back and the
 * copy of column j to column p.  Both sides include their upload of the j x p coefficients. */
int iemic_test_eig_compress_cost(iemic_ctx* ctx, int j, int p, int nrep, double* ms);

/* k_eig_residual and its second stage (eigs.hip) on host data of length N: out2 = sum |a - mu B
 * x|^2, sum |a|^2 with a = ar + i ai, x = xr + i xi, mu = mu_r + i mu_i; ai = xi = NULL: real. */
int iemic_test_eig_residual(iemic_ctx* ctx, int64_t N, const double* ar, const double* ai, const double* xr,
                            const double* xi, const double* B, double mu_r, double mu_i, double* out2);

/* The active set of the block Gauss-Seidel set-up (ActiveSet, one rank): counts = nact, natile,
 * ric; act (nact ints, may be NULL): the active cells as owned cells; atl (8 natile ints, may be
 * NULL): the compressed SpMV's tile records as act_tiles wrote them. */
int iemic_test_active_set(iemic_ctx* ctx, int64_t* counts, int* act, int* atl);

/* The compressed SpMV and the full one on the same device x (one rank).  x (reference order) is
 * staged as iemic_spmv stages it, halo exchange included, after what a solve runs before its
 * first SpMV (gs_refresh: the stream is repacked after a new Jacobian); IEMIC_ESTATE when a solve
 * would not take the compressed basis.  yc (6 nact doubles): spmv_kernel_c's result, written into
 * a device buffer with 64 guard doubles before and after it, all NaN bit patterns first;
 * *guard_changed: 1 when a guard double no longer holds that pattern.  y (reference order):
 * spmv_kernel's result, its device buffer NaN bit patterns first. */
int iemic_test_spmv_c(iemic_ctx* ctx, const double* x, double* yc, double* y, int* guard_changed);

/* The dynamics defect alone (spmv_dyn_defect, one rank): z and rr are component-planar vectors of
 * NE = 6 x ext cells doubles, as iemic_test_ts_mg_entry takes them; d (NE doubles) = rr - A z on
 * the active cells' U/V/W/P rows with the context's own identity flags, from a device buffer of
 * NaN bit patterns (what the kernel does not write comes back as such).  The hook's buffers are
 * its own: none of the preconditioner's work vectors is touched. */
int iemic_test_dyn_defect(iemic_ctx* ctx, int64_t NE, const double* z, const double* rr, double* d);

/* The block product of the projected model (spmm_kernel, spmv.hip) on k host columns V (each
 * in the reference order, staged as iemic_spmv stages its x, halo exchange included; collective
 * on several ranks): W (k columns, reference order) receives this rank's owned rows, from a
 * device buffer of NaN bit patterns.  kbmax: columns per k_spmm7 launch, 1, 2 or 4 (0: default). */
int iemic_test_spmm(iemic_ctx* ctx, int k, int kbmax, const double* V, double* W);

/* columns per k_spmm7 launch in iemic_proj_init_step and iemic_time_spmm until changed (0: default) */
int iemic_test_spmm_kb(iemic_ctx* ctx, int kbmax);

/* G (ka x kb, row-major) = V^T diag(d) W by proj_gram (projected.hip) on host columns in the
 * reference order (d: one column, or NULL); a basis of at least max(ka, kb) columns must be set
 * (its work space is used).  Summed over the ranks. */
int iemic_test_gram(iemic_ctx* ctx, int ka, int kb, const double* V, const double* d, const double* W, double* G);

/* out2 = sum (x - a)^2, sum (x - b)^2 over the owned rows of variable var (-1: all) by
 * score_sqdist2 (score.hip): the two sums iemic_score takes its distances from.  x, a, b: host
 * vectors in the reference order; x NULL: the resident state.  Summed over the ranks. */
int iemic_test_sqdist2(iemic_ctx* ctx, int var, const double* x, const double* a, const double* b, double* out2);

/* Measurement helper (one rank): GPU milliseconds per k x k Gram product of the set basis and its
 * scratch, results fetched, nrep each: by proj_gram (ms[0]), by k multi-dot pairs each fetched on
 * its own (ms[1]) and by the same k launch pairs with one fetch (ms[2]). */
int iemic_test_gram_cost(iemic_ctx* ctx, int k, int nrep, double* ms);

/* out[0], out[1]: the calls of krylov_solve (FGMRES or IDR(s), from any entry point) and of
 * prec_compute since the context was created */
int iemic_test_solver_calls(iemic_ctx* ctx, int64_t* out);

#ifdef __cplusplus
}
#endif

#endif
