/* Block conjugate gradients with per-column scalars — the "inverse power" step
 * of GCG (W ~ A^-1 (lambda B x)).  Semantics of the reference's BlockPCG
 * (src/ops_lin_sol.c:140-437): every right-hand side runs its own CG recurrence
 * (own alpha, beta, rho), columns retire individually once their residual has
 * dropped by `rate` or below tol*||b||, contiguous runs of still-active columns are
 * multiplied by A together, and no preconditioner is applied.
 *
 * Written against the operator table only.  The two per-iteration reductions
 * (p^T w and r^T r) use MultiVecLocalInnerProd + one GCGE_COMM all-reduce each,
 * as the reference does with MPI_Allreduce (:317, :365).
 */
#include <assert.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "gcge_solver.h"

static void reduce_over_ranks(double *v, int n)
{
	GCGE_COMM *c = GCGE_GetComm();
	if (GCGE_GetLocalInnerProdReduces()) return;      /* the back-end's MultiVecLocalInnerProd summed over the ranks already */
	if (c != NULL && n > 0) c->allreduce_sum(v, n, c->ctx);
}

static void BlockPCG(void *mat, void **mv_b, void **mv_x, int *start_bx, int *end_bx, struct OPS_ *ops)
{
	BlockPCGSolver *s = (BlockPCGSolver*)ops->multi_linear_solver_workspace;
	void **mv_r = s->mv_ws[0], **mv_p = s->mv_ws[1], **mv_w = s->mv_ws[2];
	const int nrhs = end_bx[0] - start_bx[0];
	double *norm_b = s->dbl_ws, *rho1 = norm_b + nrhs, *rho2 = rho1 + nrhs, *pTw = rho2 + nrhs;
	double *init_res = pTw + nrhs, *last_res = init_res + nrhs;
	int *active = s->int_ws, *run = active + nrhs;      /* run[]: starts of contiguous runs */
	int nact, nrun, niter, i, c, start[2], end[2];
	assert(nrhs == end_bx[1] - start_bx[1]);
	if (nrhs <= 0) { s->niter = 0; return; }

	if (0 == strcmp(s->tol_type, "rel")) {
		start[0] = start_bx[0]; end[0] = end_bx[0]; start[1] = start_bx[0]; end[1] = end_bx[0];
		ops->MultiVecInnerProd('D', mv_b, mv_b, 0, start, end, norm_b, 1, ops);
		for (i = 0; i < nrhs; ++i) norm_b[i] = sqrt(norm_b[i]);
	} else if (0 == strcmp(s->tol_type, "user")) {
		for (i = 0; i < nrhs; ++i) norm_b[i] = fabs(norm_b[i]);   /* caller stored the scales */
	} else {
		for (i = 0; i < nrhs; ++i) norm_b[i] = 1.0;
	}
	/* r = b - A x ;  rho2 = diag(r^T r) */
	start[0] = start_bx[1]; end[0] = end_bx[1]; start[1] = 0; end[1] = nrhs;
	if (s->MatDotMultiVec != NULL) s->MatDotMultiVec(mv_x, mv_r, start, end, mv_p, 0, ops);
	else ops->MatDotMultiVec(mat, mv_x, mv_r, start, end, ops);
	start[0] = start_bx[0]; end[0] = end_bx[0]; start[1] = 0; end[1] = nrhs;
	ops->MultiVecAxpby(1.0, mv_b, -1.0, mv_r, start, end, ops);
	start[0] = 0; end[0] = nrhs; start[1] = 0; end[1] = nrhs;
	ops->MultiVecInnerProd('D', mv_r, mv_r, 0, start, end, rho2, 1, ops);
	for (i = 0; i < nrhs; ++i) init_res[i] = sqrt(rho2[i]);
	nact = 0;
	for (i = 0; i < nrhs; ++i)
		if (init_res[i] > s->tol * norm_b[i]) { active[nact] = i; rho2[nact] = rho2[i]; ++nact; }

	niter = 0;
	while (niter < s->max_iter && nact > 0) {
		double *out;
		/* split the active list into runs of consecutive column indices */
		nrun = 0; run[nrun++] = 0;
		for (i = 1; i < nact; ++i) if (active[i] - active[i - 1] > 1) run[nrun++] = i;
		run[nrun] = nact;
		/* p = r + beta p ; w = A p ; pTw = diag(p^T w) */
		out = pTw;
		for (i = 0; i < nrun; ++i) {
			for (c = run[i]; c < run[i + 1]; ++c) {
				double beta = (niter == 0) ? 0.0 : rho2[c] / rho1[c];
				start[0] = start[1] = active[c]; end[0] = end[1] = active[c] + 1;
				ops->MultiVecAxpby(1.0, mv_r, beta, mv_p, start, end, ops);
			}
			start[0] = start[1] = active[run[i]]; end[0] = end[1] = active[run[i + 1] - 1] + 1;
			if (s->MatDotMultiVec != NULL) s->MatDotMultiVec(mv_p, mv_w, start, end, mv_b, start_bx[0], ops);
			else ops->MatDotMultiVec(mat, mv_p, mv_w, start, end, ops);
			ops->MultiVecLocalInnerProd('D', mv_p, mv_w, 0, start, end, out, 1, ops);
			out += run[i + 1] - run[i];
		}
		reduce_over_ranks(pTw, nact);
		memcpy(rho1, rho2, nact * sizeof(double));
		/* x += alpha p ; r -= alpha w ; rho2 = diag(r^T r) */
		out = rho2;
		for (i = 0; i < nrun; ++i) {
			for (c = run[i]; c < run[i + 1]; ++c) {
				double alpha = rho2[c] / pTw[c];
				start[0] = active[c]; end[0] = active[c] + 1;
				start[1] = start_bx[1] + active[c]; end[1] = start[1] + 1;
				ops->MultiVecAxpby(alpha, mv_p, 1.0, mv_x, start, end, ops);
				start[0] = start[1] = active[c]; end[0] = end[1] = active[c] + 1;
				ops->MultiVecAxpby(-alpha, mv_w, 1.0, mv_r, start, end, ops);
			}
			start[0] = start[1] = active[run[i]]; end[0] = end[1] = active[run[i + 1] - 1] + 1;
			ops->MultiVecLocalInnerProd('D', mv_r, mv_r, 0, start, end, out, 1, ops);
			out += run[i + 1] - run[i];
		}
		reduce_over_ranks(rho2, nact);
		for (i = 0; i < nact; ++i) last_res[active[i]] = sqrt(rho2[i]);
		/* retire converged columns, compacting rho1/rho2 */
		{
			int keep = 0;
			for (i = 0; i < nact; ++i) {
				c = active[i];
				if (last_res[c] > s->rate * init_res[c] && last_res[c] > s->tol * norm_b[c]) {
					active[keep] = c; rho1[keep] = rho1[i]; rho2[keep] = rho2[i]; ++keep;
				}
			}
			nact = keep;
		}
		++niter;
	}
	s->niter = niter;
	s->residual = (niter > 0) ? last_res[active[0]] : init_res[0];
}

void MultiLinearSolverSetup_BlockPCG(int max_iter, double rate, double tol, const char *tol_type,
		void **mv_ws[3], double *dbl_ws, int *int_ws, void *pc,
		void (*MatDotMultiVec)(void **x, void **y, int *start, int *end, void **z, int s, struct OPS_ *ops),
		struct OPS_ *ops)
{
	static BlockPCGSolver bpcg;
	bpcg.max_iter = max_iter; bpcg.rate = rate; bpcg.tol = tol;
	strncpy(bpcg.tol_type, tol_type, sizeof(bpcg.tol_type) - 1);
	bpcg.tol_type[sizeof(bpcg.tol_type) - 1] = '\0';
	bpcg.mv_ws[0] = mv_ws[0]; bpcg.mv_ws[1] = mv_ws[1]; bpcg.mv_ws[2] = mv_ws[2];
	bpcg.dbl_ws = dbl_ws; bpcg.int_ws = int_ws; bpcg.pc = pc;
	bpcg.MatDotMultiVec = MatDotMultiVec;
	bpcg.niter = 0; bpcg.residual = -1.0;
	ops->multi_linear_solver_workspace = (void*)&bpcg;
	ops->MultiLinearSolver = BlockPCG;
}

/* ---- V-cycle multigrid with block CG as the smoother: the reference's BlockAMG
 * (src/ops_lin_sol.c:466-715; set up as in test/test_eig_sol_SiO2_MAT.c:96-180, test/test_multi_grid.c:97-129).
 * The hierarchy A_array / P_array comes from the back-end's MultiGridCreate slot.  One cycle over L levels:
 *   down, l = 0 .. L-2:  max_iter[2l + 1] CG iterations on A_l x_l = b_l from the current x_l (pre-smoothing),
 *                        r = b_l - A_l x_l, b_{l+1} = P_l^T r, x_{l+1} = 0;
 *   coarsest level:      max_iter[2L - 1] CG iterations (its solve);
 *   up, l = L-2 .. 0:    x_l += P_l x_{l+1}, max_iter[2l + 2] CG iterations (post-smoothing).
 * max_iter[0] cycles at most, stopping once the residual the last smoothing call reports is below tol[0].
 * Level 0 is the caller's b / x and column ranges, level l >= 1 is mv_array_ws[0 / 1][l] over columns [0, m); mv_array_ws[2 / 3 / 4][l]
 * are the CG's r / p / w (2 doubles as the residual / correction block, 4 as the scratch of MultiVecFromItoJ), as the reference.
 *
 * The smoother is installed in ops->MultiLinearSolver and called through it (BlockPCG and a back-end's block CG both find their
 * state in ops->multi_linear_solver_workspace): the back-end's amg_smoother_* where its record offers them (GCGE_BACKEND,
 * gcge_ops.h), the solver stack's BlockPCG otherwise (the reference's choice, :482-486,:626-629); likewise the residual and the
 * correction as one sweep each where the record offers amg_residual / amg_prolong_add.  Where the record says the smoother honours
 * GCGE_LINSOL_ARGS.final_residual_cols (amg_final_cols), every smoothing call is told that its residual goes unread, except the
 * cycle's last one, whose column 0 becomes the cycle's residual: the other calls skip the work of their last iteration that only
 * measures it (x and the iteration counts stay bit for bit what they were). */
struct amg_level { void **b, **x; int start[2], end[2]; };
static struct amg_level amg_level(const BlockAMGSolver *bamg, int l, void **mv_b, void **mv_x, const int *start_bx, const int *end_bx)
{
	const int m = end_bx[1] - start_bx[1];
	struct amg_level v = {mv_b, mv_x, {start_bx[0], start_bx[1]}, {end_bx[0], end_bx[1]}};
	if (l > 0) { v.b = bamg->mv_array_ws[0][l]; v.x = bamg->mv_array_ws[1][l]; v.start[0] = v.start[1] = 0; v.end[0] = v.end[1] = m; }
	return v;
}
/* first != NULL with first->x_src: the call's initial guess lies there and its b is still to be formed from it (this call of the
 * smoother is told so, the later ones see an ordinary b and x) */
static void smooth(const GCGE_BACKEND *be, const BlockAMGSolver *bamg, int l, int max_iter, int last, struct amg_level *v,
		GCGE_LINSOL_ARGS *first, struct OPS_ *ops)
{
	void **mv_ws[3] = {bamg->mv_array_ws[2][l], bamg->mv_array_ws[3][l], bamg->mv_array_ws[4][l]};
	const GCGE_LINSOL_ARGS published = *GCGE_GetLinearSolverArgs();
	const int elsewhere = first != NULL && first->x_src != NULL;
	if (be->amg_final_cols || elsewhere) {      /* last: the cycle's residual is column 0 of this call's (see below) */
		GCGE_LINSOL_ARGS a = published;
		if (be->amg_final_cols) a.final_residual_cols = last ? 1 : -1;
		if (elsewhere) { a.x_src = first->x_src; a.x_src_col = first->x_src_col; a.rhs_scale = first->rhs_scale; first->x_src = NULL; }
		GCGE_SetLinearSolverArgs(&a);
	}
	if (be->amg_smoother_setup != NULL) be->amg_smoother_setup(max_iter, bamg->rate[l], bamg->tol[l], bamg->tol_type, ops);
	else MultiLinearSolverSetup_BlockPCG(max_iter, bamg->rate[l], bamg->tol[l], bamg->tol_type, mv_ws, bamg->dbl_ws, bamg->int_ws,
			NULL, NULL, ops);
	ops->MultiLinearSolver(bamg->A_array[l], v->b, v->x, v->start, v->end, ops);
	if (elsewhere) GCGE_SetLinearSolverArgs(&published);
}

static void BlockAlgebraicMultiGrid(const GCGE_BACKEND *be, BlockAMGSolver *bamg, void **mv_b, void **mv_x, int *start_bx,
		int *end_bx, GCGE_LINSOL_ARGS *first, struct OPS_ *ops)
{
	GCGE_LINSOL_FN solver = ops->MultiLinearSolver;
	void *solver_ws = ops->multi_linear_solver_workspace;
	const int L = bamg->num_levels, m = end_bx[1] - start_bx[1];
	int l, cs[2] = {0, 0}, ce[2] = {m, m};          /* the column range of a coarse level's blocks */
	struct amg_level f, c;
	assert(end_bx[0] - start_bx[0] == m);
	for (l = 0; l < L - 1; ++l) {
		void *A = bamg->A_array[l], **r = bamg->mv_array_ws[2][l];
		f = amg_level(bamg, l, mv_b, mv_x, start_bx, end_bx);
		c = amg_level(bamg, l + 1, mv_b, mv_x, start_bx, end_bx);
		smooth(be, bamg, l, bamg->max_iter[2 * l + 1], 0, &f, first, ops);
		if (!(be->amg_residual != NULL && be->amg_residual(A, f.b, f.start[0], f.x, f.start[1], r, 0, m, ops))) {
			int s[2] = {f.start[1], 0}, e[2] = {f.end[1], m};
			ops->MatDotMultiVec(A, f.x, r, s, e, ops);                 /* r = b - A x */
			s[0] = f.start[0]; e[0] = f.end[0];
			ops->MultiVecAxpby(1.0, f.b, -1.0, r, s, e, ops);
		}
		ops->MultiVecFromItoJ(bamg->P_array, l, l + 1, r, c.b, cs, ce, bamg->mv_array_ws[4], ops);
		ops->MultiVecAxpby(0.0, NULL, 0.0, c.x, cs, ce, ops);
	}
	f = amg_level(bamg, L - 1, mv_b, mv_x, start_bx, end_bx);
	smooth(be, bamg, L - 1, bamg->max_iter[2 * L - 1], L == 1, &f, first, ops);
	for (l = L - 2; l >= 0; --l) {
		void **r = bamg->mv_array_ws[2][l];
		f = amg_level(bamg, l, mv_b, mv_x, start_bx, end_bx);
		c = amg_level(bamg, l + 1, mv_b, mv_x, start_bx, end_bx);
		if (!(be->amg_prolong_add != NULL && be->amg_prolong_add(bamg->P_array[l], c.x, 0, f.x, f.start[1], m, ops))) {
			int s[2] = {0, f.start[1]}, e[2] = {m, f.end[1]};
			ops->MultiVecFromItoJ(bamg->P_array, l + 1, l, c.x, r, cs, ce, bamg->mv_array_ws[4], ops);
			ops->MultiVecAxpby(1.0, r, 1.0, f.x, s, e, ops);
		}
		smooth(be, bamg, l, bamg->max_iter[2 * l + 2], l == 0, &f, first, ops);
	}
	/* residual of the smoothing call that ran last (src/ops_lin_sol.c:643: read from the solver behind the table) */
	bamg->residual = be->amg_smoother_setup != NULL ? be->amg_smoother_residual(ops) :
			((BlockPCGSolver*)ops->multi_linear_solver_workspace)->residual;
	ops->MultiLinearSolver = solver;
	ops->multi_linear_solver_workspace = solver_ws;
}

static void BlockAMG(void *mat, void **mv_b, void **mv_x, int *start_bx, int *end_bx, struct OPS_ *ops)
{
	BlockAMGSolver *bamg = (BlockAMGSolver*)ops->multi_linear_solver_workspace;
	const GCGE_BACKEND be = GCGE_BackendOf(ops);
	const GCGE_LINSOL_ARGS args = *GCGE_GetLinearSolverArgs();
	GCGE_LINSOL_ARGS first = args;      /* what the first smoothing call (always level 0's) is told beyond the others */
	int idx;
	(void)mat;      /* level 0 of the hierarchy IS the matrix (src/ops_lin_sol.c:477) */
	/* the initial guess lies elsewhere (args.x_src: the GCG driver over a back-end with start_in_place): the back-end's smoother
	 * takes it from there in its first call and leaves b = x_src diag(scale) behind; any other smoother gets the copy first */
	first.x_src = NULL;
	if (args.x_src != NULL) {
		if (be.start_in_place && be.amg_smoother_setup != NULL && args.rhs_scale != NULL) first = args;
		else {
			int s[2], e[2];
			s[0] = args.x_src_col; e[0] = s[0] + end_bx[1] - start_bx[1]; s[1] = start_bx[1]; e[1] = end_bx[1];
			ops->MultiVecAxpby(1.0, args.x_src, 0.0, mv_x, s, e, ops);
		}
	}
	/* systems published as b = x diag(scale) (GCGE_SolverTakesScaledRhs): b is formed here, once, from the initial guess;
	 * the smoothing calls then see an ordinary right-hand side */
	if (first.x_src != NULL) {
		GCGE_LINSOL_ARGS formed = args;
		formed.rhs_scale = NULL; formed.x_src = NULL; formed.x_src_col = 0;
		GCGE_SetLinearSolverArgs(&formed);
	} else if (args.rhs_scale != NULL) {
		GCGE_LINSOL_ARGS formed = args;
		const int ncols = end_bx[1] - start_bx[1];
		if (!(be.amg_form_rhs != NULL && be.amg_form_rhs(mv_b, start_bx[0], mv_x, start_bx[1], args.rhs_scale, ncols, ops))) {
			int s[2], e[2];
			s[0] = start_bx[1]; e[0] = end_bx[1]; s[1] = start_bx[0]; e[1] = end_bx[0];
			ops->MultiVecAxpby(1.0, mv_x, 0.0, mv_b, s, e, ops);
			ops->MultiVecLinearComb(NULL, mv_b, 0, s, e, NULL, 0, (double*)args.rhs_scale, 1, ops);
		}
		formed.rhs_scale = NULL; formed.x_src = NULL; formed.x_src_col = 0;
		GCGE_SetLinearSolverArgs(&formed);
	} else if (args.x_src != NULL) {      /* copied above, b was the caller's */
		GCGE_LINSOL_ARGS formed = args;
		formed.x_src = NULL; formed.x_src_col = 0;
		GCGE_SetLinearSolverArgs(&formed);
	}
	for (idx = 0; idx < bamg->max_iter[0]; ++idx) {
		BlockAlgebraicMultiGrid(&be, bamg, mv_b, mv_x, start_bx, end_bx, &first, ops);
		bamg->niter = idx + 1;
		if (bamg->residual < bamg->tol[0]) break;
	}
	if (args.rhs_scale != NULL || args.x_src != NULL || be.amg_final_cols) GCGE_SetLinearSolverArgs(&args);   /* (the caller clears it) */
}

int GCGE_SolverTakesScaledRhs(struct OPS_ *ops)
{
	const GCGE_BACKEND be = GCGE_BackendOf(ops);
	return ops->MultiLinearSolver != NULL &&
			(ops->MultiLinearSolver == be.scaled_rhs_solver || (ops->MultiLinearSolver == BlockAMG && be.amg_form_rhs != NULL));
}

int GCGE_SolverFormsScaledRhs(struct OPS_ *ops)
{
	return ops->MultiLinearSolver == BlockAMG && GCGE_BackendOf(ops).amg_form_rhs != NULL;
}

void MultiLinearSolverSetup_BlockAMG(int *max_iter, double *rate, double *tol, const char *tol_type,
		void **A_array, void **P_array, int num_levels, void ***mv_array_ws[5], double *dbl_ws, int *int_ws,
		void *pc, struct OPS_ *ops)
{
	static BlockAMGSolver bamg;
	int i;
	bamg.max_iter = max_iter; bamg.rate = rate; bamg.tol = tol;
	strncpy(bamg.tol_type, tol_type, sizeof(bamg.tol_type) - 1);
	bamg.tol_type[sizeof(bamg.tol_type) - 1] = '\0';
	bamg.A_array = A_array; bamg.P_array = P_array; bamg.num_levels = num_levels;
	for (i = 0; i < 5; ++i) bamg.mv_array_ws[i] = mv_array_ws[i];
	bamg.dbl_ws = dbl_ws; bamg.int_ws = int_ws; bamg.pc = pc;
	bamg.niter = 0; bamg.residual = -1.0;
	ops->multi_linear_solver_workspace = (void*)&bamg;
	ops->MultiLinearSolver = BlockAMG;
}
