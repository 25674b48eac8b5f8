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
 * again from it, within max_iter, and what is reported is always the true relative residual.
 *
 * GCGE_PCGSolveDeflated runs the same loop on the operator Q^T (A - shift_j B) restricted to range(Q), Q = I - X X^T B (the adjoint
 * systems of eigenvector gradients): w = A p, the shift, w -= MX (X^T w); z = V(r) with the UNCHANGED V-cycle on A (the identity
 * without a hierarchy), z -= X (MX^T z).  The shift and p.w are the back-end's pcg_shift where it is offered, the projections the
 * table's MultiVecInnerProd / MultiVecLinearComb.  The residual that is checked and reported is Q^T (b - (A - shift B) y).           */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "gcge_solver.h"

struct GCGE_PCG_ {
	void *A; GCGE_AMG *amg; int max_cols;
	void **r, **z, **p, **w;
	double *dbl_ws;      /* 10 * max_cols */
	int *int_ws;         /* 6 * max_cols */
	void **mx, **bp;     /* GCGE_PCGSolveDeflated with B, created on first use: B X (mx_cols columns) and B p (max_cols) */
	int mx_cols;
};

/* What GCGE_PCGSolveDeflated adds to the loop of a chunk (NULL: GCGE_PCGSolve): the operator Q^T (A - shift_j B) on range(Q),
 * Q = I - X X^T B with X = X[:, x0..x0+k) and MX = B X = MX[:, mx0..mx0+k) (B == NULL: X itself); coef: k doubles for every
 * column of a chunk */
typedef struct { void *B; void **X; int x0, k; void **MX; int mx0; const double *shift; double *coef; } Deflation;

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
	if (s->mx != NULL) ops->MultiVecDestroy(&s->mx, s->mx_cols, ops);
	if (s->bp != NULL) ops->MultiVecDestroy(&s->bp, s->max_cols, ops);
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

/* v[:, v0..v0+m) -= S[:, s0..s0+k) (T[:, t0..t0+k)^T v): Q^T v with S = MX, T = X; Q v with S = X, T = MX */
static void project_out(void **S, int s0, void **T, int t0, int k, void **v, int v0, int m, double *coef, struct OPS_ *ops)
{
	double one = 1.0;
	int st[2] = {t0, v0}, en[2] = {t0 + k, v0 + m}, i;
	if (k <= 0 || m <= 0) return;
	ops->MultiVecInnerProd('N', T, v, 0, st, en, coef, k, ops);
	for (i = 0; i < k * m; ++i) coef[i] = -coef[i];
	st[0] = s0; en[0] = s0 + k;
	ops->MultiVecLinearComb(S, v, 0, st, en, coef, k, &one, 0, ops);
}

/* the B p of the deflated operator for p[:, p0..p0+m): the work block bp from column c0, or p itself without B */
static void **shift_operand(GCGE_PCG *s, const Deflation *d, void **p, int p0, int c0, int m, int *q0, struct OPS_ *ops)
{
	int st[2] = {p0, c0}, en[2] = {p0 + m, c0 + m};
	*q0 = p0;
	if (d->B == NULL) return p;
	ops->MatDotMultiVec(d->B, p, s->bp, st, en, ops);
	*q0 = c0;
	return s->bp;
}

/* w = Q^T (A - shift B) p on the window of m columns from column c0, w = A p being there already; pw[j] = p_j . w_j for the flagged
 * columns, taken before the projection (p in range(Q): p^T Q^T w = p^T w) */
static void sweep_shift(const GCGE_BACKEND *be, GCGE_PCG *s, const Deflation *d, int c0, int m, const int *flag, double *pw,
		struct OPS_ *ops)
{
	int q0, j;
	void **q = shift_operand(s, d, s->p, c0, c0, m, &q0, ops);
	if (!(be->pcg_shift != NULL && be->pcg_shift(s->p, c0, q, q0, s->w, c0, m, d->shift + c0, flag, pw, ops))) {
		for (j = 0; j < m; ++j) {
			int st[2] = {q0 + j, c0 + j}, en[2] = {q0 + j + 1, c0 + j + 1};
			if (flag[j]) ops->MultiVecAxpby(-d->shift[c0 + j], q, 1.0, s->w, st, en, ops);
		}
		col_dots(s->p, c0, s->w, c0, m, pw, ops);
	}
	reduce_over_ranks(pw, m);
	project_out(d->MX, d->mx0, d->X, d->x0, d->k, s->w, c0, m, d->coef, ops);
}

/* r[:, r0..) = Q^T (b[:, b0..) - (A - shift B) x[:, x0..)), rr[j] = |r_j|^2; shift from entry r0 (the work blocks' column) */
static void deflated_residual(const GCGE_BACKEND *be, GCGE_PCG *s, const Deflation *d, void **b, int b0, void **x, int x0, int r0, int m,
		double *rr, struct OPS_ *ops)
{
	int q0, j;
	void **q;
	if (m <= 0) return;
	if (!(be->amg_residual != NULL && be->amg_residual(s->A, b, b0, x, x0, s->r, r0, m, ops))) {
		int st[2] = {x0, r0}, en[2] = {x0 + m, r0 + m};
		ops->MatDotMultiVec(s->A, x, s->r, st, en, ops);
		st[0] = b0; en[0] = b0 + m;
		ops->MultiVecAxpby(1.0, b, -1.0, s->r, st, en, ops);
	}
	q = shift_operand(s, d, x, x0, r0, m, &q0, ops);
	for (j = 0; j < m; ++j) {
		int st[2] = {q0 + j, r0 + j}, en[2] = {q0 + j + 1, r0 + j + 1};
		ops->MultiVecAxpby(d->shift[r0 + j], q, 1.0, s->r, st, en, ops);
	}
	project_out(d->MX, d->mx0, d->X, d->x0, d->k, s->r, r0, m, d->coef, ops);
	col_dots(s->r, r0, s->r, r0, m, rr, ops);
	reduce_over_ranks(rr, m);
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

/* one chunk of m columns, b from column b0, x from column x0; the work blocks from column 0.  d == NULL: A x = b with the V-cycle.
 * d != NULL: the deflated, shifted systems (d->shift from entry 0), b, its norm and every residual projected by Q^T; a column whose
 * Q^T b is at the rounding level of forming it, |Q^T b_j| <= 2^10 eps |b_j|, counts as a zero right-hand side */
static void solve_chunk(const GCGE_BACKEND *be, GCGE_PCG *s, const Deflation *d, void **b, int b0, void **x, int x0, int m, double tol,
		int max_iter, int zero_start, double *rel_res, int *col_iters, struct OPS_ *ops)
{
	double *norm_b = s->dbl_ws, *rr = norm_b + m, *zr = rr + m, *zr_new = zr + m, *zw = zr_new + m, *pw = zw + m, *alpha = pw + m,
			*beta = alpha + m, *tmp = beta + m;
	int *active = s->int_ws, *fresh = active + m, *dirty = fresh + m, *flag = dirty + m, *done = flag + m;
	int j, nact, lo, hi, st[2], en[2];

	col_dots(b, b0, b, b0, m, norm_b, ops);
	reduce_over_ranks(norm_b, m);
	if (d != NULL) {      /* r = Q^T b and its norm */
		st[0] = b0; en[0] = b0 + m; st[1] = 0; en[1] = m;
		ops->MultiVecAxpby(1.0, b, 0.0, s->r, st, en, ops);
		project_out(d->MX, d->mx0, d->X, d->x0, d->k, s->r, 0, m, d->coef, ops);
		col_dots(s->r, 0, s->r, 0, m, tmp, ops);
		reduce_over_ranks(tmp, m);
		for (j = 0; j < m; ++j) norm_b[j] = sqrt(tmp[j]) <= 1024.0 * DBL_EPSILON * sqrt(norm_b[j]) ? 0.0 : tmp[j];
	}
	for (j = 0; j < m; ++j) { norm_b[j] = sqrt(norm_b[j]); col_iters[j] = 0; alpha[j] = beta[j] = 0.0; done[j] = 0; }
	st[0] = st[1] = x0; en[0] = en[1] = x0 + m;
	if (zero_start) ops->MultiVecAxpby(0.0, NULL, 0.0, x, st, en, ops);
	else {
		if (d != NULL) project_out(d->X, d->x0, d->MX, d->mx0, d->k, x, x0, m, d->coef, ops);      /* the start into range(Q) */
		for (j = 0; j < m; ++j) if (norm_b[j] == 0.0) {      /* the solution of a zero right-hand side is known */
			int s1[2] = {x0 + j, x0 + j}, e1[2] = {x0 + j + 1, x0 + j + 1};
			ops->MultiVecAxpby(0.0, NULL, 0.0, x, s1, e1, ops);
		}
	}
	if (zero_start) {      /* r = b */
		st[0] = b0; en[0] = b0 + m; st[1] = 0; en[1] = m;
		if (d == NULL) ops->MultiVecAxpby(1.0, b, 0.0, s->r, st, en, ops);
		for (j = 0; j < m; ++j) rr[j] = norm_b[j] * norm_b[j];
	} else if (d != NULL) deflated_residual(be, s, d, b, b0, x, x0, 0, m, rr, ops);
	else true_residual(be, s->A, b, b0, x, x0, s->r, 0, m, rr, ops);
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
			if (d != NULL) deflated_residual(be, s, d, b, b0 + lo, x, x0 + lo, lo, hi - lo, tmp + lo, ops);
			else true_residual(be, s->A, b, b0 + lo, x, x0 + lo, s->r, lo, hi - lo, tmp + lo, ops);
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
		/* z = V(r) on the window (deflated: projected into range(Q); no hierarchy: z = r), then the scalars of the new direction
		 * from one read of z, r, w */
		if (s->amg != NULL) vcycle(s, lo, hi - lo, ops);
		else {
			st[0] = st[1] = lo; en[0] = en[1] = hi;
			ops->MultiVecAxpby(1.0, s->r, 0.0, s->z, st, en, ops);
		}
		if (d != NULL) project_out(d->X, d->x0, d->MX, d->mx0, d->k, s->z, lo, hi - lo, d->coef, ops);
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
		if (d != NULL) sweep_shift(be, s, d, lo, hi - lo, active + lo, pw + lo, ops);
		else {
			col_dots(s->p, lo, s->w, lo, hi - lo, pw + lo, ops);
			reduce_over_ranks(pw + lo, hi - lo);
		}
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
			solve_chunk(&be, s, NULL, b, b0 + c, x, x0 + c, m - c < chunk ? m - c : chunk, tol, max_iter, zero_start, rel_res + c,
					col_iters + c, ops);
	}
	for (j = 0; j < m; ++j) nconv += rel_res[j] <= tol;
	return nconv;
}

int GCGE_PCGSolveDeflated(GCGE_PCG *s, void *B, void **X, int xc0, int k, const double *shift, void **b, int b0, void **y, int y0, int m,
		double tol, int max_iter, int zero_start, double *rel_res, int *col_iters, struct OPS_ *ops)
{
	GCGE_COMM *comm = GCGE_GetComm();
	GCGE_BACKEND be;
	Deflation d;
	int c, j, chunk, nconv = 0;
	if (comm != NULL && comm->size > 1) return -2;      /* row slabs: not yet */
	if (s == NULL || ops == NULL || b == NULL || y == NULL || b == y || shift == NULL || rel_res == NULL || col_iters == NULL) return -1;
	if (m < 1 || m > s->max_cols || b0 < 0 || y0 < 0 || !(tol > 0.0) || max_iter < 0) return -1;
	if (k < 0 || xc0 < 0 || (k > 0 && (X == NULL || X == b || X == y))) return -1;
	be = GCGE_BackendOf(ops);
	chunk = s->amg != NULL && s->amg->block_size < s->max_cols ? s->amg->block_size : s->max_cols;
	d.B = B; d.X = X; d.x0 = xc0; d.k = k; d.MX = X; d.mx0 = xc0;
	if (B != NULL) {      /* MX = B X, once per call; B p goes to a block of its own */
		if (k > s->mx_cols) {
			if (s->mx != NULL) ops->MultiVecDestroy(&s->mx, s->mx_cols, ops);
			ops->MultiVecCreateByMat(&s->mx, k, s->A, ops);
			s->mx_cols = k;
		}
		if (s->bp == NULL) ops->MultiVecCreateByMat(&s->bp, s->max_cols, s->A, ops);
		if (k > 0) {
			int st[2] = {xc0, 0}, en[2] = {xc0 + k, k};
			ops->MatDotMultiVec(B, X, s->mx, st, en, ops);
		}
		d.MX = s->mx; d.mx0 = 0;
	}
	d.coef = (double*)malloc(sizeof(double) * (size_t)(k > 0 ? k : 1) * (size_t)chunk);
	for (c = 0; c < m; c += chunk) {
		d.shift = shift + c;
		solve_chunk(&be, s, &d, b, b0 + c, y, y0 + c, m - c < chunk ? m - c : chunk, tol, max_iter, zero_start, rel_res + c,
				col_iters + c, ops);
	}
	free(d.coef);
	for (j = 0; j < m; ++j) nconv += rel_res[j] <= tol;
	return nconv;
}
