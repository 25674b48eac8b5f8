/* gcge_ops.h — the operator table ("plugin ABI") of the GCG hot path.
 *
 * This is OUR declaration of the function-pointer table that GCGE's solver
 * layers are written against.  It must stay bit-identical in layout (member
 * order, types, the five opaque workspace pointers and the two nested table
 * pointers) to the reference's `struct OPS_`  (/root/reference/src/ops.h:43-152)
 * so that
 *   - a back-end written against this header (OPS_HIP_Set) can be handed to the
 *     reference's unmodified solver code (GCG, ModifiedGramSchmidt, BlockPCG), and
 *   - our solver stack can be driven by a back-end compiled against the
 *     reference header (e.g. app_ccs in oracle/_ref).
 * tests/test_abi.py checks sizeof/offsetof of every member against the reference
 * header when /root/reference is present.
 *
 * Argument conventions (reference: src/ops.h:78-103):
 *   - a "multivector" is an opaque handle `void **`; only the back-end that
 *     created it may look inside;
 *   - column ranges are half open: start[0]:end[0] selects columns of the FIRST
 *     multivector argument, start[1]:end[1] of the SECOND;
 *   - small dense results (inner products, Q^T A P, coefficients) live in HOST
 *     memory, column-major, and are complete when the call returns.
 */
#ifndef GCGE_OPS_H
#define GCGE_OPS_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OPS_ {
	/* ---- services -------------------------------------------------------- */
	void   (*Printf) (const char *fmt, ...);
	double (*GetWtime) (void);
	int    (*GetOptionFromCommandLine) (const char *name, char type, void *data,
			int argc, char *argv[], struct OPS_ *ops);
	/* ---- sparse matrix --------------------------------------------------- */
	void (*MatView)  (void *mat, struct OPS_ *ops);
	void (*MatAxpby) (double alpha, void *matX, double beta, void *matY, struct OPS_ *ops);
	/* ---- single vector (unused when the multivector slots are set) -------- */
	void (*VecCreateByMat)    (void **des_vec, void *src_mat, struct OPS_ *ops);
	void (*VecCreateByVec)    (void **des_vec, void *src_vec, struct OPS_ *ops);
	void (*VecDestroy)        (void **des_vec, struct OPS_ *ops);
	void (*VecView)           (void *x, struct OPS_ *ops);
	void (*VecInnerProd)      (void *x, void *y, double *inner_prod, struct OPS_ *ops);
	void (*VecLocalInnerProd) (void *x, void *y, double *inner_prod, struct OPS_ *ops);
	void (*VecSetRandomValue) (void *x, struct OPS_ *ops);
	void (*VecAxpby)          (double alpha, void *x, double beta, void *y, struct OPS_ *ops);
	void (*MatDotVec)         (void *mat, void *x, void *y, struct OPS_ *ops);
	void (*MatTransDotVec)    (void *mat, void *x, void *y, struct OPS_ *ops);
	/* ---- block of vectors ------------------------------------------------- */
	void (*MultiVecCreateByMat)      (void ***multi_vec, int num_vec, void *src_mat, struct OPS_ *ops);
	void (*MultiVecCreateByVec)      (void ***multi_vec, int num_vec, void *src_vec, struct OPS_ *ops);
	void (*MultiVecCreateByMultiVec) (void ***multi_vec, int num_vec, void **src_mv, struct OPS_ *ops);
	void (*MultiVecDestroy)          (void ***multi_vec, int num_vec, struct OPS_ *ops);
	void (*GetVecFromMultiVec)       (void **multi_vec, int col, void **vec, struct OPS_ *ops);
	void (*RestoreVecForMultiVec)    (void **multi_vec, int col, void **vec, struct OPS_ *ops);
	void (*MultiVecView)             (void **x, int start, int end, struct OPS_ *ops);
	/* inner_prod(k x m) = x[:,s0:e0)^T y[:,s1:e1); nsdIP: 'N' full, 'S' symmetric, 'D' diagonal */
	void (*MultiVecLocalInnerProd)   (char nsdIP, void **x, void **y, int is_vec,
			int *start, int *end, double *inner_prod, int ldIP, struct OPS_ *ops);
	void (*MultiVecInnerProd)        (char nsdIP, void **x, void **y, int is_vec,
			int *start, int *end, double *inner_prod, int ldIP, struct OPS_ *ops);
	void (*MultiVecSetRandomValue)   (void **multi_vec, int start, int end, struct OPS_ *ops);
	/* y = alpha x + beta y on column ranges (x == NULL: scale only) */
	void (*MultiVecAxpby)            (double alpha, void **x, double beta, void **y,
			int *start, int *end, struct OPS_ *ops);
	/* y = x coef + y diag(beta) */
	void (*MultiVecLinearComb)       (void **x, void **y, int is_vec, int *start, int *end,
			double *coef, int ldc, double *beta, int incb, struct OPS_ *ops);
	void (*MatDotMultiVec)           (void *mat, void **x, void **y, int *start, int *end, struct OPS_ *ops);
	void (*MatTransDotMultiVec)      (void *mat, void **x, void **y, int *start, int *end, struct OPS_ *ops);
	/* qAp = Q^T A P ; ntsdQAP: 'N','S','D' or 'T' (store the transpose) */
	void (*MultiVecQtAP)             (char ntsA, char ntsdQAP, void **mvQ, void *matA, void **mvP,
			int is_vec, int *start, int *end, double *qAp, int ldQAP, void **mv_ws, struct OPS_ *ops);
	/* ---- small dense (host) ----------------------------------------------- */
	struct OPS_ *lapack_ops;
	void (*DenseMatQtAP) (char ntluA, char nsdC, int nrowsA, int ncolsA, int nrowsC, int ncolsC,
			double alpha, double *matQ, int ldQ, double *matA, int ldA, double *matP, int ldP,
			double beta, double *matC, int ldC, double *dbl_ws);
	void (*DenseMatOrth) (double *mat, int nrows, int ldm, int start, int *end,
			double orth_zero_tol, double *dbl_ws, int length, int *int_ws);
	/* ---- linear solvers ---------------------------------------------------- */
	void (*LinearSolver)      (void *mat, void *b, void *x, struct OPS_ *ops);
	void *linear_solver_workspace;
	void (*MultiLinearSolver) (void *mat, void **b, void **x, int *start, int *end, struct OPS_ *ops);
	void *multi_linear_solver_workspace;
	/* ---- block orthonormalisation ------------------------------------------ */
	void (*MultiVecOrth) (void **x, int start_x, int *end_x, void *B, struct OPS_ *ops);
	void *orth_workspace;
	/* ---- multigrid: hierarchy from the back-end, transfers through P_array (used by BlockAMG) ------ */
	void (*MultiGridCreate)  (void ***A_array, void ***B_array, void ***P_array,
			int *num_levels, void *A, void *B, struct OPS_ *ops);
	void (*MultiGridDestroy) (void ***A_array, void ***B_array, void ***P_array,
			int *num_levels, struct OPS_ *ops);
	void (*VecFromItoJ)      (void **P_array, int level_i, int level_j,
			void *vec_i, void *vec_j, void **vec_ws, struct OPS_ *ops);
	void (*MultiVecFromItoJ) (void **P_array, int level_i, int level_j,
			void **multi_vec_i, void **multi_vec_j, int *startIJ, int *endIJ,
			void ***multi_vec_ws, struct OPS_ *ops);
	/* ---- eigensolver ------------------------------------------------------- */
	void (*EigenSolver) (void *A, void *B, double *eval, void **evec,
			int nevGiven, int *nevConv, struct OPS_ *ops);
	void *eigen_solver_workspace;
	/* ---- composite back-ends (PAS) ----------------------------------------- */
	struct OPS_ *app_ops;
} OPS;

/* life cycle (reference: src/ops.c:26-149) */
void OPS_Create  (OPS **ops);   /* all slots NULL                               */
void OPS_Setup   (OPS  *ops);   /* back-fill NULL slots with the defaults below */
void OPS_Destroy (OPS **ops);

/* defaults installed by OPS_Setup (reference: src/ops_multi_vec.c) */
void   DefaultPrintf (const char *fmt, ...);
double DefaultGetWtime (void);
int    DefaultGetOptionFromCommandLine (const char *name, char type, void *value,
		int argc, char *argv[], struct OPS_ *ops);
void   DefaultMultiVecInnerProd (char nsdIP, void **x, void **y, int is_vec,
		int *start, int *end, double *inner_prod, int ldIP, struct OPS_ *ops);
void   DefaultMultiVecQtAP (char ntsA, char ntsdQAP, void **mvQ, void *matA, void **mvP,
		int is_vec, int *startQP, int *endQP, double *qAp, int ldQAP,
		void **mv_ws, struct OPS_ *ops);

/* multigrid transfers through P_array (reference: src/ops_multi_grid.c:20-117; installed by OPS_Setup, src/ops.c:107-112) */
void   DefaultVecFromItoJ (void **P_array, int level_i, int level_j, void *vec_i, void *vec_j, void **vec_ws, struct OPS_ *ops);
void   DefaultMultiVecFromItoJ (void **P_array, int level_i, int level_j, void **multi_vec_i, void **multi_vec_j,
		int *startIJ, int *endIJ, void ***multi_vec_ws, struct OPS_ *ops);

/* Host dense back-end: column-major blocks in host memory.  Layout-compatible
 * with the reference's LAPACKVEC/LAPACKMAT (app/app_lapack.h:17-20).          */
typedef struct GCGE_DENSE_ {
	double *data; int nrows; int ncols; int ldd;
} GCGE_DENSE;
void OPS_DENSE_Set (struct OPS_ *ops);   /* counterpart of OPS_LAPACK_Set (app_lapack.c) */

/* Communicator hook for row-partitioned back-ends (one process per GPU).
 * The reference reduces partial Gram matrices with MPI_Allreduce
 * (src/ops_multi_vec.c:206-228, src/ops_lin_sol.c:317,365); here the reduction
 * is a callback so the same host code runs over RCCL, gloo or nothing.       */
typedef struct GCGE_COMM_ {
	int rank, size;
	/* in-place sum over ranks of n contiguous doubles in HOST memory */
	void (*allreduce_sum) (double *buf, int n, void *ctx);
	void *ctx;
} GCGE_COMM;
void       GCGE_SetComm (const GCGE_COMM *comm);   /* NULL: single rank */
GCGE_COMM *GCGE_GetComm (void);
/* Opt-in: the back-end's MultiVecLocalInnerProd slot returns the sum over the ranks too.  For solver stacks that reduce their
 * "local" products through MPI only — the reference's BlockPCG (src/ops_lin_sol.c:306-321,355-369: MultiVecLocalInnerProd, then
 * MPI_Allreduce under OPS_USE_MPI) — so that a NON-MPI build of the reference spans the ranks with flag 0 as well.  Honoured by
 * OPS_HIP_Set's slot; libgcge_host.so's own BlockPCG skips its reduction while it is on.  Get: 1 only while a communicator exists. */
void       GCGE_SetLocalInnerProdReduces (int on);
int        GCGE_GetLocalInnerProdReduces (void);
/* What one call of ops->MultiLinearSolver carries beyond the slot's arguments: published by the caller before the call,
 * cleared after it (our GCG driver around its W solves; BlockAMG republishes it without rhs_scale for its smoothing calls).
 *   sigma, matB   shift of the W systems (sigma == 0: none).  The reference calls a user-defined solver (flag 1) with A only
 *                 (ops_eig_sol_gcg.c:584-618); a shift-aware solver (the HIP back-end's fused block CG) applies A + sigma B.
 *   user_scale    n_user_scale column scales of the "user" tolerance type of BlockPCG (src/ops_lin_sol.c:186-192: a column has
 *                 converged below tol * |scale_j|; the reference's GCG leaves lambda_j + sigma in BlockPCG's scalar scratch,
 *                 which a solver behind flag 1 does not have).
 *   rhs_scale     b = x diag(rhs_scale) with x holding the initial guess and b NOT filled in (the solver may use it as scratch):
 *                 the driver's systems A w = (lambda + sigma) x for B == NULL, published only to a solver that takes them
 *                 (GCGE_SolverTakesScaledRhs, gcge_solver.h).  The reference forms b through MatDotMultiVec + MultiVecLinearComb
 *                 (src/ops_eig_sol_gcg.c:560-577).  NULL: b is an ordinary right-hand side.
 *   x_src, x_src_col   the initial guess is NOT in the solver call's x: it is columns [x_src_col, x_src_col + m) of the block x_src,
 *                 which the solver must not write; the result goes to the call's x.  Together with rhs_scale: b = x_src diag(rhs_scale),
 *                 and the solver leaves that b in the call's b.  Published only to a back-end whose record says start_in_place;
 *                 such a back-end accepts ANY call of this kind: where its one-sweep start does not take the operands it makes
 *                 the copy and b itself first and goes on as if it had been handed them.  NULL: x holds the initial guess.
 *   idle_blocks   n_idle blocks the driver does not need during the call (its work blocks): scratch for the solver — the fused
 *                 HIP solver takes those that match its own blocks as further slots of its direction ring.
 *   final_residual_cols   whose residual the caller reads after the call: 0 every column's (a direct call), k > 0 only that of
 *                 the leading k columns, < 0 none.  A solver may then leave out the work of its LAST iteration that only measures
 *                 the residual of the other columns; x, the iteration count and the column statistics stay as they are.  BlockAMG
 *                 sets it for its smoothing calls where the back-end's record says its smoother honours it (amg_final_cols).   */
typedef struct GCGE_LINSOL_ARGS_ {
	double sigma; void *matB;
	const double *user_scale; int n_user_scale;
	const double *rhs_scale;
	void ***idle_blocks; int n_idle;
	void **x_src; int x_src_col;
	int final_residual_cols;
} GCGE_LINSOL_ARGS;
void       GCGE_SetLinearSolverArgs (const GCGE_LINSOL_ARGS *args);   /* copied; NULL clears */
const GCGE_LINSOL_ARGS *GCGE_GetLinearSolverArgs (void);              /* never NULL; all zero when nothing is published */

/* Published by the GCG driver around a W solve whose right-hand sides it moved off an odd column (gcg.c: GCGE_GcgRhsOrigin):
 * the block and the column they now start at; NULL otherwise.  What a solver computes must not depend on where b lies.  A
 * back-end with two routes for one step that round differently, chosen by b's column (the fused CG's start: |r|^2 summed inside
 * the product sweep or by the column-dot kernel), takes for these right-hand sides the sums of the route an odd column led to. */
void       GCGE_SetRealignedRhs (void **b, int b0);                   /* b == NULL clears */
void     **GCGE_GetRealignedRhs (int *b0);

/* What a back-end offers beyond the slots of struct OPS_ (NULL / 0: not offered).  Registered once by the back-end
 * (GCGE_SetBackend; OPS_HIP_Set does it), it applies to every table whose MatDotMultiVec AND MultiVecLinearComb are the ones
 * `ops` held then; GCGE_BackendOf returns a copy — all zero for other tables — minus what the opt-out switches of the
 * environment turn off at the time of the call (listed in ops_table.c).
 *   residual_sq   res_sq[j] = sum over the LOCAL rows of ((A x_j) - lambda_j (B x_j))^2, j = start .. end-1, in one go for
 *                 CheckConvergence (the slots take 11 block streams: src/ops_eig_sol_gcg.c:195-315); 0 declines.
 *   inplace_lincomb_cols   MultiVecLinearComb works ROW BY ROW (every output row written after its input row was read), so a
 *                 panel update y == x with the output columns inside the input range and at most this many of them is safe: the
 *                 orthonormalisation and ComputeP skip the reference's work block + copy back (src/ops_orth.c,
 *                 src/ops_eig_sol_gcg.c:624-640).
 *   symeig        the small dense eigensolver (contract of GCGE_SymEig) on the device, for n >= symeig_min_n (GCGE_SymEigFor).
 *   amg_smoother_setup / _residual   the back-end's block CG as BlockAMG's smoother (both or neither): setup(max_iter, rate,
 *                 tol, tol_type, ops) installs it in ops->MultiLinearSolver, residual(ops) returns what BlockPCGSolver.residual
 *                 would hold after the call.  Default: BlockPCG over the slots (src/ops_lin_sol.c:482-486,626-629).
 *   amg_residual  r[:, r0..) = b[:, b0..) - A x[:, x0..)  and  amg_prolong_add  xf[:, f0..) += P xc[:, c0..)  as one sweep each,
 *                 bit for bit the slot calls they replace (src/ops_lin_sol.c:596-606, :626-640); 0 declines.
 *   amg_form_rhs  b[:, b0..) = x[:, x0..) diag(scale) in one sweep: BlockAMG then takes rhs_scale systems; 0 declines.
 *   scaled_rhs_solver   the back-end's solver that takes rhs_scale systems, as installed in ops->MultiLinearSolver.
 *   pas_border    the bordered product of PAS's composite table in one pass over QX (GCGE_PAS_BORDER_FN, gcge_pas.h).
 *   mat_identity / mat_free   the identity of the size of a (whole, one-rank) matrix through the back-end's normal upload, and its
 *                 release: PAS's hierarchy of a standard problem takes its coarse masses P^T P from it (NULL: not offered).
 *   mat_rows_as_given   1 when the device rows of a matrix are in the order the caller gave them (0: the back-end re-ordered).
 *   amg_final_cols   1 when the smoother of amg_smoother_setup honours GCGE_LINSOL_ARGS.final_residual_cols: BlockAMG then tells each
 *                 smoothing call that no residual is read (-1), except the cycle's last one, whose column 0 it reads (1).
 *   block_moves   the three block moves of an outer iteration of GCG in one sweep over the rows (reference ComputeX + the head of
 *                 ComputeW, src/ops_eig_sol_gcg.c:458-471,:536-577):  V[:, x0..x1) = ritz[:, x0..x1);  for the runs (lo_i, hi_i) of
 *                 runs[] = {count; lo_0, hi_0, ...} (all inside [x0, x1)), packed:  V[:, w0 + blk..) = ritz[:, lo_i..hi_i);  and
 *                 with b != NULL  b[:, b0 + blk..) = ritz[:, lo_i..hi_i) diag(scale[blk..]), every product rounded once.  b may be
 *                 the block ritz itself with target columns over source columns: every row is read whole before any of it is
 *                 written.  0 declines with nothing touched.  With ritz == V and an empty range x0 == x1 no X move is asked for
 *                 and V itself is the source (the Ritz vectors already live there: ritz_in_place): the runs, ascending and ending
 *                 at or before w0, are read and the W start vectors and b (a block other than V) written, nothing else.
 *   ritz_in_place   the Ritz vectors written over X and P moved in behind them, in one launch:  V[:, n0..x1) = V[:, n0..w1) C  in
 *                 place (C column-major, (w1 - n0) x (x1 - n0), leading dimension ldc), and after it  V[:, p0..p0 + np) =
 *                 S[:, 0..np)  for a staging block S (np == 0: none; the target lies outside [n0, x1), inside [n0, w1) or not).
 *                 Every output row is written after the last read of that row.  Same arithmetic as MultiVecLinearComb + MultiVecAxpby:
 *                 the same bits.  0 declines with nothing touched: more than 128 output columns, blocks in different row orders,
 *                 unaligned leading dimensions, shapes whose MultiVecLinearComb does not work row by row from registers.  GCG then
 *                 forms P before the Ritz vectors and drops the reference's ComputeX (src/ops_eig_sol_gcg.c:458-471).
 *   start_in_place   1 when the back-end's solvers (scaled_rhs_solver, the smoother of amg_smoother_setup) honour
 *                 GCGE_LINSOL_ARGS.x_src: GCG then leaves the W start vectors and b to the first smoothing sweep of BlockAMG (gcg.c).
 *   panel_norms_sq   out[j] = sum over the LOCAL rows of y[r, start + j]^2, j < end - start, for the panel y[:, start..end) that the
 *                 LAST call of MultiVecLinearComb wrote, summed by that call from the values it stored (no second pass over the
 *                 panel; a fixed order: the same sums on every run, rounded otherwise than MultiVecInnerProd('D')'s).  0 when that
 *                 call did not collect them, or wrote another panel, or any other call came in between.
 *   multigrid_refresh   the coarse levels of a live hierarchy of ops->MultiGridCreate recomputed in place after level 0 took new
 *                 values for the same structure: 0 done, l >= 1 the first level that declined (those below it are refreshed), -1
 *                 nothing written (GCGE_AMGRefresh, gcge_solver.h; the HIP back-end's gcge_hip_multigrid_refresh, gcge_hip.h).
 *                 Rank-local: it calls nothing collective.
 *   multigrid_refresh_check   what multigrid_refresh decides from the handles alone, before it writes: 0 it would go on, -1 it would
 *                 return -1.  Rank-local and free of side effects; GCGE_AMGRefresh agrees on it over the ranks before any rank
 *                 writes.  NULL: multigrid_refresh is asked alone.
 *   pcg_step      one step of the preconditioned CG of GCGE_PCGSolve (gcge_solver.h) on a window of m columns, in one sweep:
 *                 x[:, x0..) += p[:, p0..) diag(alpha) ;  r[:, r0..) -= w[:, w0..) diag(alpha) ;  rr[j] = sum over the LOCAL rows of
 *                 r_new[r, j]^2 — for the columns with flag[j] != 0 only; a column without a flag keeps the bits of its x and r (its
 *                 rr[j] is 0).  alpha, flag, rr: host arrays of m entries.  The slots take, per flagged column, two MultiVecAxpby,
 *                 then MultiVecLocalInnerProd('D') over the window: 4 reads + 2 writes + 2 reads.  0 declines, nothing touched.
 *   pcg_dots      zr[j] = sum z[r, j] r[r, j] and zw[j] = sum z[r, j] w[r, j] over the LOCAL rows, j < m, from ONE read of z, r and w
 *                 (the slots: two MultiVecLocalInnerProd('D'), 4 reads).  Host arrays.  0 declines.
 *   pcg_direction p[:, p0..) = z[:, z0..) + p diag(beta) for the columns with flag[j] == 1, p = z for those with flag[j] == 2 (p is
 *                 not read: it may hold anything), and a column with flag[j] == 0 keeps its bits (the slots: one MultiVecAxpby per
 *                 flagged column).  beta, flag: host arrays of m entries.  0 declines, nothing touched.
 *   amg_smoother_niter   the iteration count of the last call of the smoother of amg_smoother_setup (what BlockPCGSolver.niter would
 *                 hold): GCGE_PCGSolve without a hierarchy reports it.  NULL: that solve takes BlockPCG over the slots.
 *   pcg_shift     the shift of GCGE_PCGSolveDeflated's operator on a window of m columns, in one sweep: w[:, w0..) -= q[:, q0..)
 *                 diag(shift) ;  pw[j] = sum over the LOCAL rows of p[r, j] w_new[r, j] — for the columns with flag[j] != 0 only; a
 *                 column without a flag keeps the bits of its w (its pw[j] is 0).  q is B p, or p itself (the same block and column:
 *                 the row is read once).  shift, flag, pw: host arrays of m entries.  The slots take one MultiVecAxpby per flagged
 *                 column, then MultiVecLocalInnerProd('D'): 3 reads + 1 write + 2 reads in m + 1 launches.  0 declines, nothing
 *                 touched.
 *   cheb_step     one step of the three-term recurrence of GCGE_ChebFilter (gcge_solver.h) on a window of m columns:
 *                 out[:, o0..) = alpha (A y[:, y0..) - c y[:, y0..)) - beta z[:, z0..), out, y and z three different blocks; beta == 0:
 *                 z is not read and may be NULL (a filter's first step).  Nothing is waited for.  The slots take MatDotMultiVec into
 *                 out and two MultiVecAxpby: 2 + 3 + 3 block streams; the HIP back-end 3 on matrices whose product it can rebuild
 *                 inside the sweep, 6 otherwise.  1 taken, 0 declines with nothing touched.
 *   cheb_accum    the sums of GCGE_ChebBandFilter (gcge_solver.h) on a window of m columns, in one sweep:
 *                 acc[:, a0..) = [acc[:, a0..) +] mu_a ta[:, ta0..) + mu_b tb[:, tb0..), acc, ta and tb three different blocks;
 *                 init != 0: acc is not read and may hold anything; tb == NULL: one term, mu_b is ignored.  Nothing is waited for.
 *                 The slots take two MultiVecAxpby (one for one term): 3 + 3 block streams; the HIP back-end 4 (init: 3).  Rounded
 *                 as s = fma(mu_a, ta, acc) (init: mu_a ta), then fma(mu_b, tb, s): not the bits of the two Axpby.  1 taken, 0
 *                 declines with nothing touched.
 *   cheb_step_dots   cheb_step, and additionally the two LOCAL column sums the kernel polynomial method takes from every step
 *                 (GCGE_ChebMoments, gcge_solver.h):  oo[j] = sum over the LOCAL rows of out[r, o0 + j]^2 ,  oy[j] = the same of
 *                 out[r, o0 + j] y[r, y0 + j],  j < m, of the out it has just written; oo, oy: host arrays of m entries, so the call
 *                 waits for them.  out is bit for bit what cheb_step writes for the same operands.  The slots take cheb_step (or its
 *                 slot sequence) and two MultiVecLocalInnerProd('D'): 3 to 4 more block reads in two launches with two drains; the HIP
 *                 back-end forms the sums inside the step's sweep (6 block streams, as the step alone) or, behind the fused step, from
 *                 one read of out and y (3 + 2).  1 taken, 0 declines with nothing touched. */
typedef int    (*GCGE_RESIDUAL_FN) (void *A, void *B, void **x, int start, int end, const double *lambda, double *res_sq);
typedef int    (*GCGE_SYMEIG_FN) (char uplo, int n, const double *a, int lda, double *w, double *z, int ldz);
typedef void   (*GCGE_SMOOTHER_SETUP_FN) (int max_iter, double rate, double tol, const char *tol_type, struct OPS_ *ops);
typedef double (*GCGE_SMOOTHER_RESIDUAL_FN) (struct OPS_ *ops);
typedef int    (*GCGE_AMG_RESIDUAL_FN) (void *A, void **b, int b0, void **x, int x0, void **r, int r0, int ncols, struct OPS_ *ops);
typedef int    (*GCGE_AMG_PROLONG_ADD_FN) (void *P, void **xc, int c0, void **xf, int f0, int ncols, struct OPS_ *ops);
typedef int    (*GCGE_AMG_FORM_RHS_FN) (void **b, int b0, void **x, int x0, const double *scale, int ncols, struct OPS_ *ops);
typedef void   (*GCGE_LINSOL_FN) (void *mat, void **b, void **x, int *start, int *end, struct OPS_ *ops);
typedef int    (*GCGE_BLOCK_MOVES_FN) (void **ritz, void **V, int x0, int x1, const int *runs, int w0, void **b, int b0,
		const double *scale, struct OPS_ *ops);
typedef int    (*GCGE_RITZ_IN_PLACE_FN) (void **V, int n0, int x1, int w1, const double *coef, int ldc, void **S, int p0, int np,
		struct OPS_ *ops);
typedef int    (*GCGE_PANEL_NORMS_FN) (void **y, int start, int end, double *out, struct OPS_ *ops);
typedef int    (*GCGE_PCG_STEP_FN) (void **p, int p0, void **w, int w0, void **x, int x0, void **r, int r0, int m, const double *alpha,
		const int *flag, double *rr, struct OPS_ *ops);
typedef int    (*GCGE_PCG_DOTS_FN) (void **z, int z0, void **r, int r0, void **w, int w0, int m, double *zr, double *zw, struct OPS_ *ops);
typedef int    (*GCGE_PCG_DIRECTION_FN) (void **z, int z0, void **p, int p0, int m, const double *beta, const int *flag, struct OPS_ *ops);
typedef int    (*GCGE_PCG_SHIFT_FN) (void **p, int p0, void **q, int q0, void **w, int w0, int m, const double *shift, const int *flag,
		double *pw, struct OPS_ *ops);
typedef int    (*GCGE_CHEB_STEP_FN) (void *A, void **y, int y0, void **z, int z0, void **out, int o0, int m, double alpha, double c,
		double beta, struct OPS_ *ops);
typedef int    (*GCGE_CHEB_ACCUM_FN) (void **acc, int a0, void **ta, int ta0, double mu_a, void **tb, int tb0, double mu_b, int m,
		int init, struct OPS_ *ops);
typedef int    (*GCGE_CHEB_STEP_DOTS_FN) (void *A, void **y, int y0, void **z, int z0, void **out, int o0, int m, double alpha, double c,
		double beta, double *oo, double *oy, struct OPS_ *ops);
typedef struct GCGE_BACKEND_ {
	GCGE_RESIDUAL_FN residual_sq;
	int inplace_lincomb_cols;
	GCGE_SYMEIG_FN symeig; int symeig_min_n;
	GCGE_SMOOTHER_SETUP_FN amg_smoother_setup; GCGE_SMOOTHER_RESIDUAL_FN amg_smoother_residual;
	GCGE_AMG_RESIDUAL_FN amg_residual; GCGE_AMG_PROLONG_ADD_FN amg_prolong_add; GCGE_AMG_FORM_RHS_FN amg_form_rhs;
	GCGE_LINSOL_FN scaled_rhs_solver;
	int  (*pas_border) (void **QX, int s, void **q, int q0, void **y, int y0, int m, double beta,
			const double *t, int ldt, double *g, int ldg);
	void *(*mat_identity) (void *like); void (*mat_free) (void *mat);
	int  (*mat_rows_as_given) (void *mat);
	int amg_final_cols;
	GCGE_BLOCK_MOVES_FN block_moves;
	GCGE_RITZ_IN_PLACE_FN ritz_in_place;
	GCGE_PANEL_NORMS_FN panel_norms_sq;
	int start_in_place;
	int  (*multigrid_refresh) (void **A_array, void **B_array, void **P_array, int num_levels);
	int  (*multigrid_refresh_check) (void **A_array, void **B_array, void **P_array, int num_levels);
	GCGE_PCG_STEP_FN pcg_step; GCGE_PCG_DOTS_FN pcg_dots; GCGE_PCG_DIRECTION_FN pcg_direction;
	int  (*amg_smoother_niter) (struct OPS_ *ops);
	GCGE_PCG_SHIFT_FN pcg_shift;
	GCGE_CHEB_STEP_FN cheb_step;
	GCGE_CHEB_ACCUM_FN cheb_accum;
	GCGE_CHEB_STEP_DOTS_FN cheb_step_dots;
} GCGE_BACKEND;
void       GCGE_SetBackend (struct OPS_ *ops, const GCGE_BACKEND *backend);
GCGE_BACKEND GCGE_BackendOf (struct OPS_ *ops);
void       GCGE_SetQuiet (OPS *ops, int quiet);   /* silence ops->Printf (and the dense table's) */

#ifdef __cplusplus
}
#endif
#endif /* GCGE_OPS_H */
