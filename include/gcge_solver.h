/* gcge_solver.h — host-side solver stack of the GCG hot path, written against
 * the operator table of gcge_ops.h only (never looks inside a multivector).
 *
 * Public names, argument order and defaults mirror the reference so that its
 * harness and drivers read the same:
 *   block orthonormalisation   src/ops_orth.h:18-41
 *   block PCG                  src/ops_lin_sol.h:29-45
 *   GCG eigensolver            src/ops_eig_sol_gcg.h:21-83
 *   harness                    test/test_eig_sol_gcg.c:28
 */
#ifndef GCGE_SOLVER_H
#define GCGE_SOLVER_H

#include "gcge_ops.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- small dense symmetric eigensolver (replaces dsyevx / dsyev) ---------- */
int GCGE_SymEig (char uplo, int n, const double *a, int lda, double *w,
		double *z, int ldz, double *work /* >= 2n */);
/*     the host implementation itself (GCGE_SymEig is this; kept under both names) */
int GCGE_SymEigHost (char uplo, int n, const double *a, int lda, double *w,
		double *z, int ldz, double *work /* >= 2n */);
/*     ... or through the back-end of the table (GCGE_BackendOf(ops).symeig, gcge_ops.h) for n >= its symeig_min_n: what the
 *     GCG driver and the orthonormalisation call.  The host solver where the back-end offers none or its solver fails.   */
int GCGE_SymEigFor (struct OPS_ *ops, char uplo, int n, const double *a, int lda, double *w,
		double *z, int ldz, double *work /* >= 2n */);

/* ---- block orthonormalisation (sets ops->MultiVecOrth + orth_workspace) ---- */
typedef struct ModifiedGramSchmidtOrth_ {
	int    block_size;     /* columns orthonormalised among themselves per sweep (<=0: half) */
	int    max_reorth;
	double orth_zero_tol;  /* a column with B-norm below this is dropped                      */
	double reorth_tol;     /* stop re-orthogonalising when max |coef| falls below this        */
	void   **mv_ws;        /* >= block columns of scratch (holds B x)                         */
	double *dbl_ws;
} ModifiedGramSchmidtOrth;
typedef ModifiedGramSchmidtOrth BinaryGramSchmidtOrth;

void MultiVecOrthSetup_ModifiedGramSchmidt (int block_size, int max_reorth,
		double orth_zero_tol, void **mv_ws, double *dbl_ws, struct OPS_ *ops);
void MultiVecOrthSetup_BinaryGramSchmidt (int block_size, int max_reorth,
		double orth_zero_tol, void **mv_ws, double *dbl_ws, struct OPS_ *ops);
/* block Cholesky-QR variant of the MGS scheme (method name "chol"): the same contract with
 * BLOCK operations only — what a GPU back-end wants (block_size <= columns of mv_ws).      */
void MultiVecOrthSetup_CholeskyQR (int block_size, int max_reorth,
		double orth_zero_tol, void **mv_ws, double *dbl_ws, struct OPS_ *ops);

/* ---- block conjugate gradients (sets ops->MultiLinearSolver) --------------- */
typedef struct BlockPCGSolver_ {
	int max_iter; double rate; double tol; char tol_type[8];   /* "abs" | "rel" | "user" */
	void   **mv_ws[3];    /* r, p, w : one column per right-hand side                      */
	double *dbl_ws;       /* 6 * (number of right-hand sides)                              */
	int    *int_ws;       /* 2 * (number of right-hand sides)                              */
	void   *pc;           /* stored, never applied (as in the reference)                   */
	/* optional replacement for y = A x (the A + sigma B product); z[s:...) is scratch     */
	void  (*MatDotMultiVec) (void **x, void **y, int *start, int *end, void **z, int s, struct OPS_ *ops);
	int niter; double residual;
} BlockPCGSolver;

void MultiLinearSolverSetup_BlockPCG (int max_iter, double rate, double tol,
		const char *tol_type, void **mv_ws[3], double *dbl_ws, int *int_ws, void *pc,
		void (*MatDotMultiVec) (void **x, void **y, int *start, int *end, void **z, int s, struct OPS_ *ops),
		struct OPS_ *ops);

/* ---- V-cycle multigrid with block CG smoothing (sets ops->MultiLinearSolver) ------
 * The reference's BlockAMG (src/ops_lin_sol.h:47-60, src/ops_lin_sol.c:466-715): same struct, same argument order.
 * max_iter[0] = V-cycles at most, max_iter[2l + 1] / [2l + 2] = pre- / post-smoothing CG iterations on level l (the
 * coarsest level only pre-smooths: that is its solve); rate[l], tol[l] the CG's stopping parameters on level l, tol[0]
 * also the stopping residual of the cycles.  A_array / P_array: num_levels matrices and num_levels - 1 prolongations of
 * the back-end (ops->MultiGridCreate).  mv_array_ws[i][l]: 0 right-hand side and 1 solution of level l >= 1, 2 / 3 / 4 the
 * CG's r / p / w on level l (2 also holds the residual and the prolongated correction).                                  */
typedef struct BlockAMGSolver_ {
	int    *max_iter; double *rate; double *tol; char tol_type[8];
	void   **A_array; void **P_array; int num_levels;
	void   ***mv_array_ws[5]; double *dbl_ws; int *int_ws;
	void   *pc;
	int    niter; double residual;
} BlockAMGSolver;
void MultiLinearSolverSetup_BlockAMG (int *max_iter, double *rate, double *tol, const char *tol_type,
		void **A_array, void **P_array, int num_levels, void ***mv_array_ws[5], double *dbl_ws, int *int_ws,
		void *pc, struct OPS_ *ops);
/*     1: ops->MultiLinearSolver takes systems published as b = x diag(rhs_scale) (GCGE_LINSOL_ARGS, gcge_ops.h) — it is the
 *     back-end's scaled_rhs_solver, or BlockAMG over a back-end with amg_form_rhs (GCGE_BACKEND).  BlockAMG smooths with the
 *     back-end's amg_smoother_* and takes its amg_residual / amg_prolong_add where the back-end offers them.              */
int GCGE_SolverTakesScaledRhs (struct OPS_ *ops);
/*     1: ... and forms b from the scales itself before it starts (BlockAMG over amg_form_rhs; the back-end's scaled_rhs_solver
 *     never reads b).  The GCG driver then has b written by the sweep that moves X and the start vectors
 *     (GCGE_BACKEND.block_moves) and publishes an ordinary right-hand side.                                                  */
int GCGE_SolverFormsScaledRhs (struct OPS_ *ops);
/*     BlockAMG as the solver of GCG's W systems, the way the reference's SiO2 driver sets it up under OPS_USE_AMG
 *     (test/test_eig_sol_SiO2_MAT.c:96-128,160-170): hierarchy from ops->MultiGridCreate (at most max_levels), work blocks of
 *     block_size columns per level, max_iter = {cycles, smooth0, smooth0, smooth, smooth, ...} (reference: {1, 5, 5, 4, 4, ...}),
 *     rate = {rate0, 1e-16, ...}, tol = {1e-14, 1e-16, ...}, "abs".  Create once (set-up, like the matrix upload), Install
 *     puts BlockAMG into ops->MultiLinearSolver; run the harness with flag 1.  `-gcge_amg_levels L` makes the harness do all
 *     of that itself.  NULL: the back-end has no MultiGridCreate.                                                           */
typedef struct GCGE_AMG_ {
	void **A_array, **B_array, **P_array; int num_levels, block_size, own_smoother;
	void ***mv_ws[5]; int *max_iter; double *rate, *tol; double *dbl_ws; int *int_ws;
} GCGE_AMG;
GCGE_AMG *GCGE_AMGCreate (void *A, void *B, int max_levels, int block_size, int cycles, int smooth0, int smooth, double rate0,
		struct OPS_ *ops);
void GCGE_AMGInstall (GCGE_AMG *amg, struct OPS_ *ops);
void GCGE_AMGDestroy (GCGE_AMG **amg, struct OPS_ *ops);
/*     After A (and B) took new values in place for the same structure: the coarse levels of amg's hierarchy recomputed where they are,
 *     through the back-end's multigrid_refresh (GCGE_BACKEND, gcge_ops.h), whose return value this is — 0: the hierarchy of the new
 *     values; l >= 1: level l declined, the caller destroys the hierarchy and creates it again; -1: nothing was written, also when
 *     the back-end of `ops` offers no refresh.  Work blocks, parameter arrays and the installed solver are not touched.
 *     Over a communicator (GCGE_SetComm: a hierarchy of row slabs) the call is COLLECTIVE and every rank gets the same return: the
 *     back-end's refresh is rank-local, and the ranks agree by two all-reduces every rank reaches unconditionally — one on what the
 *     back-end decides from the handles alone (multigrid_refresh_check), before any rank writes, so a -1 anywhere is a -1 everywhere
 *     with nothing written; one after the level loop, whose result is the smallest level that declined on any rank, or 0.          */
int  GCGE_AMGRefresh (GCGE_AMG *amg, struct OPS_ *ops);

/* ---- linear systems A X = B, converged to a tolerance (csrc/host/block_fpcg.c) -------
 * Flexible preconditioned block CG, every column with its own alpha and beta as in BlockPCG; the preconditioner z = V(r) is one call
 * of BlockAMG over `amg` from z = 0 (installed as GCGE_AMGInstall does and called through ops->MultiLinearSolver with cleared
 * GCGE_LINSOL_ARGS; the slot, its workspace pointer and what was published are put back before GCGE_PCGSolve returns):
 *     alpha_j = (z.r)_j / (p.w)_j ;  x += alpha p ;  r -= alpha w ;  beta_j = -alpha_j (z_new.w)_j / (z_old.r_old)_j ;  p = z + beta p
 * A column stops at |r_j| <= tol |b_j| (|b_j| = 0: x_j = 0, rel_res 0) and is retired with alpha = 0 and no flag: its x, r, p keep their
 * bits; the V-cycle runs over the contiguous window of the columns still active.  m > amg->block_size: chunks of block_size columns,
 * each solved as a call of its own would.  When the recurrence is through with a chunk, b - A x is formed (the back-end's amg_residual,
 * else the slots); a column whose TRUE relative residual is above tol starts again from it, within max_iter.  rel_res[j] is always
 * that true value, col_iters[j] the V-cycles column j saw (at most max_iter).
 * amg == NULL: one call of the block CG that exists — the back-end's amg_smoother_setup(max_iter, 0, tol, "rel") where it is offered,
 * BlockPCG on the solver's blocks otherwise —, then the same true-residual report; col_iters[j] is that call's iteration count.
 * The sweeps go through GCGE_BACKEND.pcg_step / pcg_dots / pcg_direction (gcge_ops.h) where the back-end offers them.
 * GCGE_PCGCreate: four blocks of max_cols columns created by A (r, z, p, w) and the scalar arrays; NULL on bad arguments, among
 * them a hierarchy whose level 0 is not A.  GCGE_PCGSolve: zero_start != 0 starts from x = 0 whatever x holds; returns the number
 * of columns with rel_res <= tol, -1 on bad arguments (m > max_cols among them), -2 while a communicator of more than one rank is
 * set (single rank only) — nothing is written then.
 *
 * GCGE_PCGSolveDeflated: on the same solver, for m columns, the deflated and per-column-shifted systems
 *     Q^T (A - shift_j B) y_j = Q^T b_j ,  y_j in range(Q) ,  Q = I - X X^T B      (B == NULL: the identity)
 * with X = X[:, xc0..xc0+k) B-orthonormal (the computed eigenvectors; the adjoint systems of eigenvector gradients, shift_j their
 * eigenvalues: positive definite on range(Q) while shift_j is below the first eigenvalue NOT in X, conditioned like the inverse of
 * that gap).  The same recurrence — flexible beta, per-column alpha and beta, retired columns keep their bits, chunks of
 * amg->block_size — with the operator  w = A p ; w -= shift_j (B p) ; w -= MX (X^T w)  and the preconditioner  z = V(r) ;
 * z -= X (MX^T z), V the UNCHANGED V-cycle on A; without a hierarchy z = r (the same loop with the identity: the fused block CG
 * cannot take this operator).  MX = B X is formed once per call in a work block the solver creates on first use (B == NULL: X
 * itself), B p in a second one.  The shift and p.w go through GCGE_BACKEND.pcg_shift where it is offered and does not decline, the
 * projections through the table's MultiVecInnerProd / MultiVecLinearComb.  What is checked and reported is the TRUE projected
 * residual |Q^T (b_j - (A - shift_j B) y_j)| relative to |Q^T b_j|; a column whose Q^T b_j is at the rounding level of forming it,
 * |Q^T b_j| <= 2^10 eps |b_j| (b_j inside span(MX)), gets y_j = 0 and rel_res 0.  zero_start == 0: the start is projected into
 * range(Q) first.  shift: m host doubles.  The table and the published GCGE_LINSOL_ARGS are left as found, and GCGE_PCGSolve on the
 * same solver is not affected.  Returns as GCGE_PCGSolve: -2 under a communicator of more than one rank, -1 on bad arguments (k < 0,
 * X the block of b or of y, m > max_cols, ...) with nothing written, else the number of columns with rel_res <= tol.              */
typedef struct GCGE_PCG_ GCGE_PCG;
GCGE_PCG *GCGE_PCGCreate (void *A, GCGE_AMG *amg, int max_cols, struct OPS_ *ops);
int  GCGE_PCGSolve (GCGE_PCG *s, void **b, int b0, void **x, int x0, int m, double tol, int max_iter, int zero_start,
		double *rel_res, int *col_iters, struct OPS_ *ops);
int  GCGE_PCGSolveDeflated (GCGE_PCG *s, void *B, void **X, int xc0, int k, const double *shift, void **b, int b0, void **y, int y0,
		int m, double tol, int max_iter, int zero_start, double *rel_res, int *col_iters, struct OPS_ *ops);
void GCGE_PCGDestroy (GCGE_PCG **s, struct OPS_ *ops);

/* ---- GCG eigensolver (sets ops->EigenSolver) -------------------------------- */
typedef struct GCGSolver_ {
	void   *A; void *B; double sigma;
	double *eval; void **evec;
	int    nevMax; int multiMax; double gapMin;
	int    nevInit; int nevGiven; int nevConv;
	int    block_size; double tol[2]; int numIterMax;   /* tol = {absolute, relative} */
	int    numIter; int sizeV;
	void   **mv_ws[4]; double *dbl_ws; int *int_ws;
	int    length_dbl_ws;
	int    user_defined_multi_linear_solver;   /* 0: BlockPCG, 1: ops->MultiLinearSolver, 2: both */
	int    check_conv_max_num;
	char   initX_orth_method[8]; int initX_orth_block_size; int initX_orth_max_reorth; double initX_orth_zero_tol;
	char   compP_orth_method[8]; int compP_orth_block_size; int compP_orth_max_reorth; double compP_orth_zero_tol;
	char   compW_orth_method[8]; int compW_orth_block_size; int compW_orth_max_reorth; double compW_orth_zero_tol;
	int    compW_cg_max_iter; double compW_cg_rate; double compW_cg_tol; char compW_cg_tol_type[8];
	int    compW_cg_auto_shift; double compW_cg_shift; int compW_cg_order;
	int    compRR_min_num; double compRR_min_gap; double compRR_tol;
} GCGSolver;

void EigenSolverSetup_GCG (int multiMax, double gapMin, int nevInit, int nevMax,
		int block_size, double tol[2], int numIterMax,
		int user_defined_multi_linear_solver,
		void **mv_ws[4], double *dbl_ws, int *int_ws, struct OPS_ *ops);
void EigenSolverCreateWorkspace_GCG (int nevInit, int nevMax, int block_size, void *mat,
		void ***mv_ws, double **dbl_ws, int **int_ws, struct OPS_ *ops);
void EigenSolverDestroyWorkspace_GCG (int nevInit, int nevMax, int block_size, void *mat,
		void ***mv_ws, double **dbl_ws, int **int_ws, struct OPS_ *ops);
void EigenSolverSetParameters_GCG (int check_conv_max_num,
		const char *initX_orth_method, int initX_orth_block_size, int initX_orth_max_reorth, double initX_orth_zero_tol,
		const char *compP_orth_method, int compP_orth_block_size, int compP_orth_max_reorth, double compP_orth_zero_tol,
		const char *compW_orth_method, int compW_orth_block_size, int compW_orth_max_reorth, double compW_orth_zero_tol,
		int compW_cg_max_iter, double compW_cg_rate, double compW_cg_tol, const char *compW_cg_tol_type,
		int compW_cg_auto_shift, int compRR_min_num, double compRR_min_gap, double compRR_tol,
		struct OPS_ *ops);
void EigenSolverSetParametersFromCommandLine_GCG (int argc, char *argv[], struct OPS_ *ops);

/* phase timers of the last solve (same phases as the reference's TIME_GCG table) */
typedef struct GCGE_Timing_ {
	double initX, checkconv, compP, compRR, rr_matW, dsyevx, compRV, compW, linsol, compX, total;
} GCGE_Timing;
const GCGE_Timing *GCGE_LastTiming (void);
/* column at which ComputeW packs the `total` right-hand sides inside the scratch columns [startN, endX) of the eigenvector block
 * when the first unconverged column is `first`: even whenever first, first + 1 or first - 1 fits, else `first` */
int GCGE_GcgRhsOrigin (int first, int total, int startN, int endX);
/* counters since the library was loaded: outer iterations whose first unconverged column was odd, those of them whose b moved to
 * an even column, outer iterations whose X / W / b moves were one sweep (GCGE_BACKEND.block_moves).  NULL: not wanted. */
void GCGE_GcgBlockMoveStats (long *odd_origins, long *realigned, long *fused_moves);
/* counters since the library was loaded: launches that wrote the Ritz vectors over X and moved P in behind them
 * (GCGE_BACKEND.ritz_in_place; 0 over a table that does not offer it: the driver then keeps ComputeRitzVec / ComputeP / ComputeX) */
void GCGE_GcgRitzInPlaceStats (long *fused_launches);
/* ComputeW's test for leaving the W start vectors and b to the solver (GCGE_LINSOL_ARGS.x_src): 1, with the source range
 * [*lo, *lo + *total), when the runs offset[] = {count; lo_0, hi_0, ...} are ONE contiguous range (adjacent runs count as one) and
 * its first column, its length and startW are even; 0 otherwise (no run, a hole between runs, an odd column or length) */
int GCGE_GcgStartInPlaceRange (const int *offset, int startW, int *lo, int *total);
/* counters since the library was loaded: outer iterations whose W solve started from the Ritz vectors where they lie, and outer
 * iterations of a back-end that offers it (in-place Ritz vectors, BlockAMG's scaled right-hand sides) that moved them first */
void GCGE_GcgStartInPlaceStats (long *in_place, long *declined);
/* counters since the library was loaded, of the "twice is enough" test of the Cholesky-QR scheme's projection (orth.c: project_out):
 * times it was made, times it asked for another pass, times the column norms came from the panel update that wrote the columns
 * (GCGE_BACKEND.panel_norms_sq) */
void GCGE_OrthKahanStats (long *tests, long *another_pass, long *norms_from_update);

/* ---- harness ---------------------------------------------------------------- */
/* flag: 0 BlockPCG inside GCG, 1 the back-end's own ops->MultiLinearSolver, 2 both */
int TestEigenSolverGCG (void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops);

/* Same run, but returning the results instead of printing them (used by the python
 * tests and bench.py).  eval must hold nevMax doubles.  Returns 0 on success. */
typedef struct GCGE_RunResult_ {
	int nevConv, numIter, nevMax, block_size, nevInit;
	double seconds;
	GCGE_Timing timing;
} GCGE_RunResult;
int GCGE_RunGCG (void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops,
		double *eval, void ***evec_out /* NULL: destroy */, GCGE_RunResult *res);
/* Warm start: evec is a block of nevMax columns (MultiVecCreateByMat) owned by the caller whose first nevGiven
 * columns are start vectors — the nevGiven argument of ops->EigenSolver (reference src/ops_eig_sol_gcg.c:101-158,
 * 1253); the eigenvectors are returned in the same block. */
int GCGE_RunGCGGiven (void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops,
		double *eval, void **evec, int nevGiven, GCGE_RunResult *res);

/* Residual norms of eigenpairs a solve returned: out[j - start] = || A x_j - eval[j - start] B x_j ||_2 for the columns j = start ..
 * end - 1 of evec (B == NULL: the identity), summed over all ranks.  Through the back-end's residual_sq (GCGE_BackendOf(ops), the
 * routine CheckConvergence uses) where it is offered and accepts; otherwise by CheckConvergence's slot sequence on two blocks of
 * end - start columns created for the call.  Returns 0, -1 on bad arguments.                                                      */
int GCGE_ResidualNorms (void *A, void *B, void **evec, int start, int end, const double *eval, double *out, struct OPS_ *ops);

/* ---- Chebyshev-filtered subspace iteration (csrc/host/chfsi.c): the smallest eigenpairs of a STANDARD problem without a linear
 * solve — no preconditioner, no hierarchy, and A need not be definite.  Single rank.
 * GCGE_ChebFilter: x[:, x0..x0+m) <- p(A) x[:, x0..x0+m) in place, p the Chebyshev polynomial of the given degree scaled to 1 at
 * `lowest` and bounded by 1 on [lower, upper] (so nothing overflows at any degree), by the three-term recurrence with
 *     e = (upper - lower) / 2,  c = (upper + lower) / 2,  sigma_1 = e / (lowest - c),  tau = 2 / sigma_1
 *     step 1:       Y_1 = (sigma_1 / e) (A - c) X
 *     step i >= 2:  sigma' = 1 / (tau - sigma) ;  Y_i = (2 sigma' / e) (A - c) Y_{i-1} - sigma sigma' Y_{i-2} ;  sigma = sigma'
 * over x and the two work blocks (windows [0, m) of work1 and work2, m columns or more each; three different blocks), the result
 * copied back into x when it ends elsewhere.  One step is the back-end's cheb_step (GCGE_BACKEND, gcge_ops.h) where it is offered
 * and accepts, else MatDotMultiVec and two MultiVecAxpby.  Returns 0; -1 on bad arguments (degree < 1, lower >= upper, lowest >=
 * lower, aliased blocks) with nothing written.
 * GCGE_RunChFSI: options in harness style: -nevConv (30), -nevMax (2 nevConv), -gcge_abs_tol / -gcge_rel_tol (1e-1 / 1e-8, tested
 * by the rule of the GCG driver's convergence check), -gcge_max_niter (100), -chfsi_degree (20), -chfsi_lanczos_steps (10),
 * -chfsi_upper_bound (unset: theta_max + |beta_k| of that many Lanczos steps on one random column, the safeguarded bound of Zhou
 * and Li).  evec: the caller's block of nevMax columns whose first nevGiven columns are start vectors (the rest is drawn by
 * MultiVecSetRandomValue); eval: nevMax doubles.  The start block is orthonormalised as GCG's initial block is by default and
 * tested after a Rayleigh-Ritz step, so a converged start returns with numIter == 0.  Per iteration: lower = the block's largest
 * Ritz value, lowest = its smallest; the columns behind the locked ones are filtered, orthonormalised against the locked ones and
 * among themselves, Rayleigh-Ritz, residual norms (GCGE_ResidualNorms), the count of LEADING converged pairs advances.  ops->MultiVecOrth
 * and its workspace are put back before it returns.  Returns 0 for a completed run, converged or not (res->nevConv says);
 * -1 bad arguments and -2 a communicator of more than one rank, both with evec untouched; -3 the block lost rank; -4 the dense
 * eigensolver failed; -5 the upper bound is not above the block's Ritz values.                                                    */
typedef struct GCGE_CHFSI_RESULT_ {
	int nevConv, numIter, degree;
	double seconds, lower, upper;      /* the last filter's lower end; the upper bound used */
} GCGE_CHFSI_RESULT;
int GCGE_ChebFilter (void *A, void **x, int x0, int m, int degree, double lower, double upper, double lowest,
		void **work1, void **work2, struct OPS_ *ops);
int GCGE_RunChFSI (void *A, int argc, char *argv[], struct OPS_ *ops, double *eval, void **evec, int nevGiven,
		GCGE_CHFSI_RESULT *res);

/* ---- Eigenpairs INSIDE an interval [a, b] (csrc/host/chfsi.c): spectrum slicing with a band-pass Chebyshev filter.  For interior
 * pairs (the states round a gap, the modes of a frequency band) and indefinite matrices; NOT for the smallest pairs of a definite
 * matrix, which GCG with a kept hierarchy finds several times faster.  Single rank.  The ends a and b belong in gaps of the
 * spectrum: an eigenvalue AT an end sits at rho = p(end) and may be counted either way.
 * GCGE_ChebBandCoefficients: mu[0..degree] of p(t) = sum_j mu_j T_j(t), t = (lambda - c) / e, c = (lmax + lmin) / 2,
 * e = (lmax - lmin) / 2: with t_a = max(-1, (a - c) / e), t_b = min(1, (b - c) / e), theta = acos t,
 *     gamma_0 = (theta_a - theta_b) / pi,   gamma_j = 2 (sin j theta_a - sin j theta_b) / (j pi),
 *     mu_j = gamma_j g_j,   g_j = ((p + 2 - j) cos(j alpha) + sin(j alpha) cot alpha) / (p + 2),   alpha = pi / (p + 2), p = degree
 * (the Jackson factors: p is then monotone across each end, within [0, 1], about 1/2 at the ends).  -1 unless lmin < lmax, a < b,
 * [a, b] meets [lmin, lmax] and degree >= 2.
 * GCGE_ChebBandFilter: x[:, x0..x0+m) <- sum_j mu_j T_j((A - c) / e) x[:, x0..x0+m).  T_1 is the back-end's cheb_step with alpha = 1 / e,
 * beta = 0, T_{j+1} with alpha = 2 / e, beta = 1, over x and the windows [0, m) of work1 and work2 in a ring of three as in
 * GCGE_ChebFilter; the iterates are added to the window [0, m) of acc (a fourth block) in PAIRS while both are live — init on
 * (T_0, T_1), then (T_2, T_3), ... after each odd step, a last single term at an even degree — by the back-end's cheb_accum
 * (GCGE_BACKEND, gcge_ops.h: one sweep, 4 block streams for a pair) where it is offered and accepts, else by MultiVecAxpby(mu_a, T_a,
 * init ? 0 : 1, acc) and MultiVecAxpby(mu_b, T_b, 1, acc) (6 streams; over a table without the slot the bits are those of these two
 * calls); acc is copied into x at the end and keeps the result.
 * Returns 0; -1 on bad arguments (those of the coefficients, aliased blocks) with nothing written.
 * GCGE_RunChFSIBand: every eigenpair with a <= lambda <= b.  Options in harness style: -chfsi_band_lo, -chfsi_band_hi and -nevMax
 * (the block width) are required; -chfsi_degree (unset: ceil(GCGE_CHFSI_BAND_DEGREE_FACTOR (lmax - lmin) / (b - a)) within
 * [20, 1000]), -gcge_abs_tol / -gcge_rel_tol, -gcge_max_niter (100), -chfsi_lanczos_steps (10), -chfsi_lower_bound /
 * -chfsi_upper_bound (taken as they are; what is unset comes from ONE Lanczos run: theta_min - |beta_k|, theta_max + |beta_k|).
 * The start block is made as in GCGE_RunChFSI.  Per iteration, on all columns (no locking: p >= p(end) inside the interval, so
 * converged vectors stay): residual norms of the Ritz vectors X, Y = p(A) X, rho_i = x_i^T y_i.  A Ritz pair with theta_i in [a, b]
 * is GENUINE when rho_i >= edge = min(p(a), p(b)), else spurious (a mixture of outside eigenvectors: its rho is a convex
 * combination of values of p below the edge value).  The run has converged when at least one pair is genuine and every genuine
 * pair passes GCGE_RunChFSI's residual test; otherwise Y is orthonormalised, Rayleigh-Ritz, and on.  So a run of numIter iterations
 * applies numIter + 1 filters.  On return the genuine pairs stand first in evec / eval, ascending, res->nevConv of them, the
 * other Ritz pairs behind them.  Returns 0 for a completed run (res->converged says whether the test passed; an interval that
 * holds nothing ends after max_niter with 0 pairs); -1 / -2 as GCGE_RunChFSI with evec untouched; -3, -4 as there; -5 bounds that
 * are not bounds for the interval; -6 the block is too small: after two iterations every column held a genuine pair
 * (res->nevConv = the columns), so more pairs may lie inside than the block can hold.
 * Memory: beside evec the run holds FOUR blocks of nevMax columns (the ring's two work blocks, the accumulator, the copy of the
 * Ritz vectors), five in all.
 * GCGE_LanczosBounds: the Lanczos bounds alone, -1 when they fail.  The start column is drawn by MultiVecSetRandomValue from the
 * random stream as it stands: the two drivers seed it (srand(0)) before they draw, a caller who wants the same bounds on every
 * call does the same.                                                                                                            */
#define GCGE_CHFSI_BAND_DEGREE_FACTOR 6.0      /* the fewest matrix products among 2, 3, 4, 6: profiles/chfsi_band/README.md */
typedef struct GCGE_CHFSI_BAND_RESULT_ {
	int nevConv, numIter, degree, spurious, converged;      /* genuine pairs; outer iterations; -; inside pairs rejected at the end; the test passed */
	double seconds, lmin, lmax, edge;                       /* the bounds used; min(p(a), p(b)) */
} GCGE_CHFSI_BAND_RESULT;
int GCGE_LanczosBounds (void *A, int steps, double *lmin, double *lmax, struct OPS_ *ops);
int GCGE_ChebBandCoefficients (int degree, double a, double b, double lmin, double lmax, double *mu);
int GCGE_ChebBandFilter (void *A, void **x, int x0, int m, int degree, double a, double b, double lmin, double lmax,
		void **work1, void **work2, void **acc, struct OPS_ *ops);
int GCGE_RunChFSIBand (void *A, int argc, char *argv[], struct OPS_ *ops, double *eval, void **evec, int nevGiven,
		GCGE_CHFSI_BAND_RESULT *res);

/* ---- Counting before solving (csrc/host/chfsi.c): the kernel polynomial method.  GCGE_RunChFSIBand wants a block wider than the
 * number of eigenvalues inside, ends in gaps of the spectrum and a degree; these two routines estimate all three from the Chebyshev
 * moments of a few probe vectors, for the price of ceil(degree / 2) products with a block of m columns.
 * GCGE_ChebMoments: moments[j * m + col] = v_col^T T_j((A - c) / e) v_col, j = 0 .. degree, for the columns v[:, v0..v0+m), with
 * c = (lmax + lmin) / 2, e = (lmax - lmin) / 2 and [lmin, lmax] bounds of the spectrum (GCGE_LanczosBounds).  With t_k = T_k v:
 *     mu_0 = v . v ,  mu_1 = t_1 . v ,  mu_2k = 2 t_k . t_k - mu_0 ,  mu_{2k-1} = 2 t_k . t_{k-1} - mu_1
 * so the recurrence runs ceil(degree / 2) steps, t_k into the window [0, m) of w1, w2, w3 in turn (three different blocks of m columns
 * or more, none of them v); v is read only.  Each step is ONE call of the back-end's cheb_step_dots (GCGE_BACKEND, gcge_ops.h: the
 * step and both sums) where it is offered and accepts, else cheb_step (or its slot sequence) followed by two
 * MultiVecLocalInnerProd('D').  The local sums are added over the communicator (lin_sol.c's rule), so row slabs work.  moments:
 * (degree + 1) m doubles.  Returns 0; -1 on bad arguments (degree < 1, m < 1, lmin >= lmax, aliased blocks) with nothing written.
 * GCGE_ChebCountFromMoments: per_probe[col] = sum_j mu_j moments[j * m + col] with mu = GCGE_ChebBandCoefficients(degree, a, b, lmin,
 * lmax): the probe's estimate of tr p(A), p the band-pass polynomial of [a, b] — for probes with v^T v = n and independent entries of
 * mean 0 (Rademacher +-1 columns), whose expectation of v^T p(A) v is tr p(A) = sum_i p(lambda_i), about the number of eigenvalues
 * inside when a and b lie in gaps.  *count = the mean over the probes, *stderr_ = the sample standard deviation / sqrt(m) (0 for
 * m == 1); per_probe: m doubles, or NULL.  No matrix: another interval is recounted from the same moments.  -1 on the coefficients'
 * bad arguments (degree < 2 among them), m < 1 or a NULL pointer, with nothing written.                                              */
int GCGE_ChebMoments (void *A, void **v, int v0, int m, int degree, double lmin, double lmax,
		void **w1, void **w2, void **w3, double *moments, struct OPS_ *ops);
int GCGE_ChebCountFromMoments (const double *moments, int m, int degree, double a, double b, double lmin, double lmax,
		double *count, double *stderr_, double *per_probe);

/* ---- PAS eigensolver (sets ops->EigenSolver; reference src/ops_eig_sol_pas.h) -------------------------------------
 * Rayleigh-Ritz on the coarsest level H = num_levels - 1, then per iteration: prolongate X one level (down to level 0),
 * smooth A X = Lambda B X by BlockAMG from that level down, make X B-orthogonal to range(P_H) and B-orthonormal, solve the
 * augmented problem (gcge_pas.h) with our GCG over the composite table, form the Ritz vectors P_H q + X x; on level 0 the
 * residuals are checked (abs AND rel).  A_array / B_array / P_array: the back-end's hierarchy (ops->MultiGridCreate) built
 * with the process-wide scale (gcge_mg_get_defaults: A_{l+1} = scale P^T A_l P); B_array[l] the Galerkin masses, B_array[0]
 * NULL for a standard problem (then every B_array[l], l >= 1, must be P^T P: GCGE_RunPAS builds the hierarchy from the
 * identity).  mv_ws[i][l]: blocks of level l — i = 0 .. 5 nevMax columns, i = 6 nevMax + 2 block_size_rr columns.
 * dbl_ws / int_ws: at least what GCGE_PASWorkspaceSizes returns (the inner GCG's arenas are PAS's own).                 */
typedef struct PASSolver_ {
	void   **A; void **B; void **P;
	double *eval; void **evec; int nevConv;
	int    nevMax; int multiMax; double gapMin;
	int    block_size; double tol[2]; int numIterMax;
	int    num_levels; int level_aux;
	int    numIter;
	int    block_size_rr; double tol_rr[2]; int numIterMax_rr;
	void   ***mv_ws[7]; double *dbl_ws; int *int_ws;
	int    check_conv_max_num;
	int    compN_user_defined_multi_linear_solver;
	int    compN_bamg_max_iter[32]; double compN_bamg_rate[16]; double compN_bamg_tol[16]; char compN_bamg_tol_type[8];
	int    orthX_user_defined_multi_linear_solver;
	int    orthX_ls_max_iter; double orthX_ls_rate; double orthX_ls_tol; char orthX_ls_tol_type[8];
	char   orthX_orth_method[8]; int orthX_orth_block_size; int orthX_orth_max_reorth; double orthX_orth_zero_tol;
	int    compRR_gcg_check_conv_max_num;
	char   compRR_gcg_initX_orth_method[8]; int compRR_gcg_initX_orth_block_size; int compRR_gcg_initX_orth_max_reorth;
	double compRR_gcg_initX_orth_zero_tol;
	char   compRR_gcg_compP_orth_method[8]; int compRR_gcg_compP_orth_block_size; int compRR_gcg_compP_orth_max_reorth;
	double compRR_gcg_compP_orth_zero_tol;
	char   compRR_gcg_compW_orth_method[8]; int compRR_gcg_compW_orth_block_size; int compRR_gcg_compW_orth_max_reorth;
	double compRR_gcg_compW_orth_zero_tol;
	int    compRR_gcg_compW_cg_max_iter; double compRR_gcg_compW_cg_rate; double compRR_gcg_compW_cg_tol;
	char   compRR_gcg_compW_cg_tol_type[8];
	int    compRR_gcg_compRR_min_num; double compRR_gcg_compRR_min_gap; double compRR_gcg_compRR_tol;
	double scale;      /* the hierarchy's scale (A_{l+1} = scale P^T A_l P), read at set-up */
	int    status;     /* 0, or < 0: the last solve stopped (-8: a level the back-end re-ordered) */
} PASSolver;

void EigenSolverSetup_PAS (int multiMax, double gapMin, int nevMax,
		int block_size, double tol[2], int numIterMax,
		int block_size_rr, double tol_rr[2], int numIterMax_rr,
		void **A_array, void **B_array, void **P_array, int num_levels,
		void ***mv_ws[7], double *dbl_ws, int *int_ws, struct OPS_ *ops);
void EigenSolverSetParameters_PAS (int check_conv_max_num,
		int compN_user_defined_multi_linear_solver,
		int *compN_bamg_max_iter, double *compN_bamg_rate, double *compN_bamg_tol, const char *compN_bamg_tol_type,
		int orthX_user_defined_multi_linear_solver,
		int orthX_ls_max_iter, double orthX_ls_rate, double orthX_ls_tol, const char *orthX_ls_tol_type,
		const char *orthX_orth_method, int orthX_orth_block_size, int orthX_orth_max_reorth, double orthX_orth_zero_tol,
		int compRR_gcg_check_conv_max_num,
		const char *compRR_gcg_initX_orth_method, int compRR_gcg_initX_orth_block_size,
		int compRR_gcg_initX_orth_max_reorth, double compRR_gcg_initX_orth_zero_tol,
		const char *compRR_gcg_compP_orth_method, int compRR_gcg_compP_orth_block_size,
		int compRR_gcg_compP_orth_max_reorth, double compRR_gcg_compP_orth_zero_tol,
		const char *compRR_gcg_compW_orth_method, int compRR_gcg_compW_orth_block_size,
		int compRR_gcg_compW_orth_max_reorth, double compRR_gcg_compW_orth_zero_tol,
		int compRR_gcg_compW_cg_max_iter, double compRR_gcg_compW_cg_rate, double compRR_gcg_compW_cg_tol,
		const char *compRR_gcg_compW_cg_tol_type,
		int compRR_gcg_compRR_min_num, double compRR_gcg_compRR_min_gap, double compRR_gcg_compRR_tol,
		struct OPS_ *ops);
void GCGE_PASWorkspaceSizes (int nevMax, int block_size_rr, long *length_dbl_ws, long *length_int_ws);

/* PAS, then (unless -gcge_pas_only 1) GCG warm-started from PAS's nevConv vectors: test/test_eig_sol_pas.c.
 * Options: -gcge_pas_levels (3), -gcge_pas_max_iter (50), -gcge_pas_abs_tol / -gcge_pas_rel_tol (1e-1 / 1e-8),
 * -gcge_pas_rr_max_iter (100), -gcge_pas_only (0), plus GCG's.  eval: nevMax doubles (PAS's values with -gcge_pas_only).
 * Returns 0; -7: the back-end has no MultiGridCreate or the hierarchy has fewer than 2 levels; -8: a level the back-end
 * re-ordered (the prolongations are in the hierarchy's numbering); -9: B == NULL and no matrix upload (gcge_pas.h).     */
typedef struct GCGE_PAS_RESULT_ {
	int nevConv, numIter, num_levels;
	double seconds;
	GCGE_RunResult gcg;   /* the warm-started GCG (zero with -gcge_pas_only 1) */
} GCGE_PAS_RESULT;
int GCGE_RunPAS (void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops,
		double *eval, void ***evec_out /* NULL: destroy */, GCGE_PAS_RESULT *res);
int TestEigenSolverPAS (void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops);

#ifdef __cplusplus
}
#endif
#endif
