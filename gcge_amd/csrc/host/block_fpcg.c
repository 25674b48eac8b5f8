/* Linear systems A X = B with a few right-hand sides, converged to a tolerance: flexible preconditioned block CG whose
 * preconditioner is one BlockAMG V-cycle (lin_sol.c), or — without a hierarchy — one call of the block CG that exists.
 *
 * Written against the operator table only.  Every column runs its own recurrence (own alpha, beta), as in BlockPCG:
 *     z = V(r)                                   one V-cycle from z = 0 over the window of columns still active
 *     beta_j = -alpha_j (z.w)_j / (z_old.r_old)_j ;  p = z + beta p        (the first step and a restart: p = z)
 *     w = A p ;  alpha_j = (z.r)_j / (p.w)_j
 *     x += alpha p ;  r -= alpha w ;  a column stops at |r_j| <= tol |b_j|
 * beta is the Polak-Ribiere form z_new.(r_new - r_old) / (z_old.r_old) with r_new - r_old = -alpha w put in, so no old residual is
 * stored.  It has to be this one: the V-cycle smooths with CG, which stops by a rate and is no fixed linear operator, and with a
 * preconditioner that changes from step to step only the flexible beta keeps the new direction conjugate to the last one.
 *
 * The three vector sweeps of a step go through the back-end's pcg_step / pcg_dots / pcg_direction where its record offers them
 * (GCGE_BACKEND, gcge_ops.h) and through the slots otherwise.  Retired columns get no flag: their x, r, p keep their bits.
 * The scalars live on the host; every one of them passes reduce_over_ranks, the one place a collective would go.
 *
 * The contract is the TRUE residual: when the recurrence calls a chunk done, b - A x is formed; a column still above tol starts
 * again from it, within max_iter, and what is reported is always the true relative residual.                                    */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "gcge_solver.h"

struct GCGE_PCG_ {
	void *A; GCGE_AMG *amg; int max_cols;
	void **r, **z, **p, **w;
	double *dbl_ws;      /* 10 * max_cols */
	int *int_ws;         /* 6 * max_cols */
};

/* single rank for now (GCGE_PCGSolve refuses a communicator): the sums arrive complete */
static void reduce_over_ranks(double *v, int n) { (void)v; (void)n; }

GCGE_PCG *GCGE_PCGCreate(void *A, GCGE_AMG *amg, int max_cols, struct OPS_ *ops)
{
	GCGE_PCG *s;
	if (A == NULL || ops == NULL || max_cols < 1 || (amg != NULL && (amg->num_levels < 1 || amg->block_size < 1 || amg->A_array[0] != A)))
		return NULL;
	s = (GCGE_PCG*)calloc(1, sizeof(GCGE_PCG));
	s->A = A; s->amg = amg; s->max_cols = max_cols;
	ops->MultiVecCreateByMat(&s->r, max_cols, A, ops);
	ops->MultiVecCreateByMat(&s->z, max_cols, A, ops);
	ops->MultiVecCreateByMat(&s->p, max_cols, A, ops);
	ops->MultiVecCreateByMat(&s->w, max_cols, A, ops);
	s->dbl_ws = (double*)calloc(10 * (size_t)max_cols, sizeof(double));
	s->int_ws = (int*)calloc(6 * (size_t)max_cols, sizeof(int));
	return s;
}

void GCGE_PCGDestroy(GCGE_PCG **ps, struct OPS_ *ops)
{
	GCGE_PCG *s;
	if (ps == NULL || *ps == NULL) return;
	s = *ps;
	ops->MultiVecDestroy(&s->r, s->max_cols, ops);
	ops->MultiVecDestroy(&s->z, s->max_cols, ops);
	ops->MultiVecDestroy(&s->p, s->max_cols, ops);
	ops->MultiVecDestroy(&s->w, s->max_cols, ops);
	free(s->dbl_ws); free(s->int_ws); free(s);
	*ps = NULL;
}

static void col_dots(void **x, int x0, void **y, int y0, int m, double *out, struct OPS_ *ops)
{
	int st[2] = {x0, y0}, en[2] = {x0 + m, y0 + m};
	ops->MultiVecLocalInnerProd('D', x, y, 0, st, en, out, 1, ops);
}

/* r[:, r0..) = b[:, b0..) - A x[:, x0..), rr[j] = |r_j|^2 */
static void true_residual(const GCGE_BACKEND *be, void *A, void **b, int b0, void **x, int x0, void **r, int r0, int m, double *rr,
		struct OPS_ *ops)
{
	if (m <= 0) return;
	if (!(be->amg_residual != NULL && be->amg_residual(A, b, b0, x, x0, r, r0, m, ops))) {
		int st[2] = {x0, r0}, en[2] = {x0 + m, r0 + m};
		ops->MatDotMultiVec(A, x, r, st, en, ops);
		st[0] = b0; en[0] = b0 + m;
		ops->MultiVecAxpby(1.0, b, -1.0, r, st, en, ops);
	}
	col_dots(r, r0, r, r0, m, rr, ops);
	reduce_over_ranks(rr, m);
}

/* x[:, x0..) += alpha p ; r -= alpha w ; rr[j] = |r_j|^2 — flagged columns of the window of m columns (p, w, r from column c0) */
static void sweep_step(const GCGE_BACKEND *be, GCGE_PCG *s, void **x, int x0, int c0, int m, const double *alpha, const int *flag,
		double *rr, struct OPS_ *ops)
{
	int j;
	if (!(be->pcg_step != NULL && be->pcg_step(s->p, c0, s->w, c0, x, x0, s->r, c0, m, alpha, flag, rr, ops))) {
		for (j = 0; j < m; ++j) {
			int st[2] = {c0 + j, x0 + j}, en[2] = {c0 + j + 1, x0 + j + 1};
			if (!flag[j]) continue;
			ops->MultiVecAxpby(alpha[j], s->p, 1.0, x, st, en, ops);
			st[1] = c0 + j; en[1] = c0 + j + 1;
			ops->MultiVecAxpby(-alpha[j], s->w, 1.0, s->r, st, en, ops);
		}
		col_dots(s->r, c0, s->r, c0, m, rr, ops);
	}
	reduce_over_ranks(rr, m);
}

/* zr[j] = z_j . r_j, zw[j] = z_j . w_j over the window */
static void sweep_dots(const GCGE_BACKEND *be, GCGE_PCG *s, int c0, int m, double *zr, double *zw, struct OPS_ *ops)
{
	if (!(be->pcg_dots != NULL && be->pcg_dots(s->z, c0, s->r, c0, s->w, c0, m, zr, zw, ops))) {
		col_dots(s->z, c0, s->r, c0, m, zr, ops);
		col_dots(s->z, c0, s->w, c0, m, zw, ops);
	}
	reduce_over_ranks(zr, m); reduce_over_ranks(zw, m);
}

/* flag 1: p = z + beta p ; flag 2: p = z ; flag 0: p keeps its bits */
static void sweep_direction(const GCGE_BACKEND *be, GCGE_PCG *s, int c0, int m, const double *beta, const int *flag, struct OPS_ *ops)
{
	int j;
	if (be->pcg_direction != NULL && be->pcg_direction(s->z, c0, s->p, c0, m, beta, flag, ops)) return;
	for (j = 0; j < m; ++j) {
		int st[2] = {c0 + j, c0 + j}, en[2] = {c0 + j + 1, c0 + j + 1};
		if (!flag[j]) continue;
		ops->MultiVecAxpby(1.0, s->z, flag[j] == 2 ? 0.0 : beta[j], s->p, st, en, ops);
	}
}

/* z[:, c0..c0+m) = V(r[:, c0..c0+m)): one call of BlockAMG over s->amg from z = 0; the table and what was published stay as found */
static void vcycle(GCGE_PCG *s, int c0, int m, struct OPS_ *ops)
{
	void (*solver) (void*, void**, void**, int*, int*, struct OPS_*) = ops->MultiLinearSolver;
	void *solver_ws = ops->multi_linear_solver_workspace;
	const GCGE_LINSOL_ARGS published = *GCGE_GetLinearSolverArgs();
	int st[2] = {c0, c0}, en[2] = {c0 + m, c0 + m};
	ops->MultiVecAxpby(0.0, NULL, 0.0, s->z, st, en, ops);
	GCGE_AMGInstall(s->amg, ops);
	GCGE_SetLinearSolverArgs(NULL);
	ops->MultiLinearSolver(s->A, s->r, s->z, st, en, ops);
	GCGE_SetLinearSolverArgs(&published);
	ops->MultiLinearSolver = solver;
	ops->multi_linear_solver_workspace = solver_ws;
}

/* one chunk of m columns, b from column b0, x from column x0; the work blocks from column 0 */
static void solve_chunk_amg(const GCGE_BACKEND *be, GCGE_PCG *s, void **b, int b0, void **x, int x0, int m, double tol, int max_iter,
		int zero_start, double *rel_res, int *col_iters, struct OPS_ *ops)
{
	double *norm_b = s->dbl_ws, *rr = norm_b + m, *zr = rr + m, *zr_new = zr + m, *zw = zr_new + m, *pw = zw + m, *alpha = pw + m,
			*beta = alpha + m, *tmp = beta + m;
	int *active = s->int_ws, *fresh = active + m, *dirty = fresh + m, *flag = dirty + m, *done = flag + m;
	int j, nact, lo, hi, st[2], en[2];

	col_dots(b, b0, b, b0, m, norm_b, ops);
	reduce_over_ranks(norm_b, m);
	for (j = 0; j < m; ++j) { norm_b[j] = sqrt(norm_b[j]); col_iters[j] = 0; alpha[j] = beta[j] = 0.0; done[j] = 0; }
	st[0] = st[1] = x0; en[0] = en[1] = x0 + m;
	if (zero_start) ops->MultiVecAxpby(0.0, NULL, 0.0, x, st, en, ops);
	else for (j = 0; j < m; ++j) if (norm_b[j] == 0.0) {      /* the solution of a zero right-hand side is known */
		int s1[2] = {x0 + j, x0 + j}, e1[2] = {x0 + j + 1, x0 + j + 1};
		ops->MultiVecAxpby(0.0, NULL, 0.0, x, s1, e1, ops);
	}
	if (zero_start) {      /* r = b */
		st[0] = b0; en[0] = b0 + m; st[1] = 0; en[1] = m;
		ops->MultiVecAxpby(1.0, b, 0.0, s->r, st, en, ops);
		for (j = 0; j < m; ++j) rr[j] = norm_b[j] * norm_b[j];
	} else true_residual(be, s->A, b, b0, x, x0, s->r, 0, m, rr, ops);
	for (j = 0; j < m; ++j) {
		rel_res[j] = norm_b[j] > 0.0 ? sqrt(rr[j]) / norm_b[j] : 0.0;
		active[j] = norm_b[j] > 0.0 && sqrt(rr[j]) > tol * norm_b[j] && max_iter > 0;
		fresh[j] = 1; dirty[j] = 0;
	}
	for (;;) {
		nact = 0;
		for (j = 0; j < m; ++j) nact += active[j];
		if (nact == 0) {
			/* the recurrence is through with every column: what it moved is measured by its true residual, and a column that
			 * is not there yet starts again from it */
			lo = 0; hi = m;
			while (lo < m && !dirty[lo]) ++lo;
			while (hi > lo && !dirty[hi - 1]) --hi;
			if (hi <= lo) break;
			true_residual(be, s->A, b, b0 + lo, x, x0 + lo, s->r, lo, hi - lo, tmp + lo, ops);
			for (j = lo; j < hi; ++j) {
				if (!dirty[j]) continue;
				dirty[j] = 0; rr[j] = tmp[j];
				rel_res[j] = sqrt(rr[j]) / norm_b[j];
				if (rel_res[j] > tol && !done[j] && col_iters[j] < max_iter) { active[j] = 1; fresh[j] = 1; }
			}
			continue;
		}
		lo = 0; hi = m;
		while (!active[lo]) ++lo;
		while (!active[hi - 1]) --hi;
		/* z = V(r) on the window, then the scalars of the new direction from one read of z, r, w */
		vcycle(s, lo, hi - lo, ops);
		for (j = lo; j < hi; ++j) col_iters[j] += active[j];
		sweep_dots(be, s, lo, hi - lo, zr_new + lo, zw + lo, ops);
		for (j = lo; j < hi; ++j) {
			flag[j] = !active[j] ? 0 : fresh[j] ? 2 : 1;
			beta[j] = flag[j] == 1 ? -alpha[j] * zw[j] / zr[j] : 0.0;
			if (active[j]) { zr[j] = zr_new[j]; fresh[j] = 0; }
		}
		sweep_direction(be, s, lo, hi - lo, beta + lo, flag + lo, ops);
		/* w = A p, alpha */
		st[0] = st[1] = lo; en[0] = en[1] = hi;
		ops->MatDotMultiVec(s->A, s->p, s->w, st, en, ops);
		col_dots(s->p, lo, s->w, lo, hi - lo, pw + lo, ops);
		reduce_over_ranks(pw + lo, hi - lo);
		for (j = lo; j < hi; ++j) {
			flag[j] = active[j];
			alpha[j] = 0.0;
			if (!active[j]) continue;
			if (pw[j] > 0.0 && zr[j] > 0.0) alpha[j] = zr[j] / pw[j];
			else { flag[j] = 0; active[j] = 0; done[j] = 1; }      /* no descent direction left (r = 0, or V(r) lost definiteness) */
		}
		sweep_step(be, s, x, x0 + lo, lo, hi - lo, alpha + lo, flag + lo, tmp + lo, ops);
		for (j = lo; j < hi; ++j) {
			if (!flag[j]) continue;
			rr[j] = tmp[j]; dirty[j] = 1;
			if (!(sqrt(rr[j]) > tol * norm_b[j]) || col_iters[j] >= max_iter) active[j] = 0;
		}
	}
}

/* no hierarchy: one call of the block CG that exists, to "rel" tol; then the same true-residual report */
static void solve_plain(const GCGE_BACKEND *be, GCGE_PCG *s, void **b, int b0, void **x, int x0, int m, double tol, int max_iter,
		int zero_start, double *rel_res, int *col_iters, struct OPS_ *ops)
{
	void (*solver) (void*, void**, void**, int*, int*, struct OPS_*) = ops->MultiLinearSolver;
	void *solver_ws = ops->multi_linear_solver_workspace;
	const GCGE_LINSOL_ARGS published = *GCGE_GetLinearSolverArgs();
	double *norm_b = s->dbl_ws, *rr = norm_b + m, *cg_dbl = rr + m;      /* cg_dbl: 6 m */
	void **mv_ws[3] = {s->r, s->p, s->w};
	int st[2] = {x0, x0}, en[2] = {x0 + m, x0 + m}, niter, j;

	if (zero_start) ops->MultiVecAxpby(0.0, NULL, 0.0, x, st, en, ops);
	if (be->amg_smoother_setup != NULL && be->amg_smoother_niter != NULL) be->amg_smoother_setup(max_iter, 0.0, tol, "rel", ops);
	else MultiLinearSolverSetup_BlockPCG(max_iter, 0.0, tol, "rel", mv_ws, cg_dbl, s->int_ws, NULL, NULL, ops);
	GCGE_SetLinearSolverArgs(NULL);
	st[0] = b0; en[0] = b0 + m;
	ops->MultiLinearSolver(s->A, b, x, st, en, ops);
	niter = be->amg_smoother_setup != NULL && be->amg_smoother_niter != NULL ? be->amg_smoother_niter(ops)
			: ((BlockPCGSolver*)ops->multi_linear_solver_workspace)->niter;
	GCGE_SetLinearSolverArgs(&published);
	ops->MultiLinearSolver = solver;
	ops->multi_linear_solver_workspace = solver_ws;

	col_dots(b, b0, b, b0, m, norm_b, ops);
	reduce_over_ranks(norm_b, m);
	true_residual(be, s->A, b, b0, x, x0, s->r, 0, m, rr, ops);
	for (j = 0; j < m; ++j) {
		if (norm_b[j] == 0.0) {
			int s1[2] = {x0 + j, x0 + j}, e1[2] = {x0 + j + 1, x0 + j + 1};
			ops->MultiVecAxpby(0.0, NULL, 0.0, x, s1, e1, ops);
			rel_res[j] = 0.0;
		} else rel_res[j] = sqrt(rr[j]) / sqrt(norm_b[j]);
		col_iters[j] = niter;
	}
}

int GCGE_PCGSolve(GCGE_PCG *s, void **b, int b0, void **x, int x0, int m, double tol, int max_iter, int zero_start,
		double *rel_res, int *col_iters, struct OPS_ *ops)
{
	GCGE_COMM *comm = GCGE_GetComm();
	GCGE_BACKEND be;
	int c, j, nconv = 0;
	if (comm != NULL && comm->size > 1) return -2;      /* row slabs: not yet */
	if (s == NULL || ops == NULL || b == NULL || x == NULL || b == x || rel_res == NULL || col_iters == NULL) return -1;
	if (m < 1 || m > s->max_cols || b0 < 0 || x0 < 0 || !(tol > 0.0) || max_iter < 0) return -1;
	be = GCGE_BackendOf(ops);
	if (s->amg == NULL) solve_plain(&be, s, b, b0, x, x0, m, tol, max_iter, zero_start, rel_res, col_iters, ops);
	else {
		const int chunk = s->amg->block_size < s->max_cols ? s->amg->block_size : s->max_cols;
		for (c = 0; c < m; c += chunk)
			solve_chunk_amg(&be, s, b, b0 + c, x, x0 + c, m - c < chunk ? m - c : chunk, tol, max_iter, zero_start, rel_res + c,
					col_iters + c, ops);
	}
	for (j = 0; j < m; ++j) nconv += rel_res[j] <= tol;
	return nconv;
}
