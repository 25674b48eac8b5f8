/* Chebyshev-filtered subspace iteration (Zhou, Saad, Tiago, Chelikowsky, J. Comput. Phys. 219 (2006) 172-184): the smallest
 * eigenpairs of a symmetric standard problem A x = lambda x without a linear solve — no preconditioner, no hierarchy, no
 * definiteness.  Written against the operator table only, like gcg.c.
 *
 *   GCGE_ChebFilter   X <- p(A) X with the scaled Chebyshev polynomial p of a given degree that is 1 at `lowest` and bounded by 1 in
 *                     modulus on [lower, upper]: components of the eigenvalues in [lower, upper] are damped, those below `lower` grow
 *                     relative to them like a Chebyshev polynomial outside its interval.
 *   GCGE_RunChFSI     upper bound by a few Lanczos steps, then per iteration: filter the unconverged columns, orthonormalise them
 *                     against the locked ones and among themselves, Rayleigh-Ritz, residuals, lock the leading converged pairs.
 *   GCGE_ChebBandFilter, GCGE_RunChFSIBand   (at the end of the file) the eigenpairs INSIDE an interval [a, b]: the filter is the
 *                     Jackson-damped Chebyshev expansion of the interval's indicator, a sum of the recurrence's iterates.
 *   GCGE_ChebMoments, GCGE_ChebCountFromMoments   (behind them) what that solve needs to know in advance — how many eigenvalues lie in
 *                     an interval, where the gaps are — from the Chebyshev moments of a few probe vectors (the kernel polynomial method).
 *
 * The filter is the three-term recurrence  Y_{j+1} = alpha_j (A - c I) Y_j - beta_j Y_{j-1}.  One step goes through the back-end's
 * cheb_step (GCGE_BACKEND, gcge_ops.h) where the table offers it and it accepts, else through the slots: MatDotMultiVec into the
 * output block and two MultiVecAxpby.  The band filter's sums go the same way: the back-end's cheb_accum, else two MultiVecAxpby.
 */
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gcge_solver.h"

/* out[:, o0..) = alpha (A y[:, y0..) - c y[:, y0..)) - beta z[:, z0..)   (beta == 0: z is not read) */
static void cheb_step(void *A, void **y, int y0, void **z, int z0, void **out, int o0, int m, double alpha, double c, double beta,
		const GCGE_BACKEND *be, struct OPS_ *ops)
{
	int s[2], e[2];
	if (be->cheb_step != NULL && be->cheb_step(A, y, y0, z, z0, out, o0, m, alpha, c, beta, ops)) return;
	s[0] = y0; e[0] = y0 + m; s[1] = o0; e[1] = o0 + m;
	ops->MatDotMultiVec(A, y, out, s, e, ops);
	ops->MultiVecAxpby(-alpha * c, y, alpha, out, s, e, ops);                 /* alpha (A y) - alpha c y */
	if (beta != 0.0) {
		s[0] = z0; e[0] = z0 + m;
		ops->MultiVecAxpby(-beta, z, 1.0, out, s, e, ops);
	}
}

/* the filter with the work blocks' windows at column w0 (the driver puts them on x's own column: the back-end's fused step wants
 * the three windows on one column) */
static int cheb_filter(void *A, void **x, int x0, int m, int degree, double lower, double upper, double lowest,
		void **work1, void **work2, int w0, struct OPS_ *ops)
{
	const GCGE_BACKEND be = GCGE_BackendOf(ops);
	void **blk[3]; int col[3], i, s[2], e[2];
	double ee, c, sigma, sigma1, tau;
	if (A == NULL || x == NULL || work1 == NULL || work2 == NULL || ops == NULL || x0 < 0 || w0 < 0 || m < 0 || degree < 1) return -1;
	if (!(lower < upper) || !(lowest < lower)) return -1;
	if (x == work1 || x == work2 || work1 == work2) return -1;
	if (m == 0) return 0;
	ee = 0.5 * (upper - lower); c = 0.5 * (upper + lower);
	sigma1 = ee / (lowest - c); tau = 2.0 / sigma1; sigma = sigma1;
	blk[0] = x; col[0] = x0; blk[1] = work1; col[1] = w0; blk[2] = work2; col[2] = w0;
	/* step i reads block (i - 1) % 3 (and (i - 2) % 3) and writes block i % 3 */
	cheb_step(A, blk[0], col[0], NULL, 0, blk[1], col[1], m, sigma1 / ee, c, 0.0, &be, ops);
	for (i = 2; i <= degree; ++i) {
		const double sigma2 = 1.0 / (tau - sigma);
		const int iy = (i - 1) % 3, iz = (i - 2) % 3, io = i % 3;
		cheb_step(A, blk[iy], col[iy], blk[iz], col[iz], blk[io], col[io], m, 2.0 * sigma2 / ee, c, sigma * sigma2, &be, ops);
		sigma = sigma2;
	}
	if (degree % 3 != 0) {
		const int ir = degree % 3;
		s[0] = col[ir]; e[0] = col[ir] + m; s[1] = x0; e[1] = x0 + m;
		ops->MultiVecAxpby(1.0, blk[ir], 0.0, x, s, e, ops);
	}
	return 0;
}

int GCGE_ChebFilter(void *A, void **x, int x0, int m, int degree, double lower, double upper, double lowest,
		void **work1, void **work2, struct OPS_ *ops)
{
	return cheb_filter(A, x, x0, m, degree, lower, upper, lowest, work1, work2, 0, ops);
}

static double col_dot(void **x, int cx, void **y, int cy, struct OPS_ *ops)
{
	int s[2], e[2]; double v = 0.0;
	s[0] = cx; e[0] = cx + 1; s[1] = cy; e[1] = cy + 1;
	ops->MultiVecInnerProd('D', x, y, 0, s, e, &v, 1, ops);
	return v;
}
static void col_axpby(double a, void **x, int cx, double b, void **y, int cy, struct OPS_ *ops)
{
	int s[2], e[2];
	s[0] = cx; e[0] = cx + 1; s[1] = cy; e[1] = cy + 1;
	ops->MultiVecAxpby(a, x, b, y, s, e, ops);
}

/* theta_max(T_k) + |beta_k| after k Lanczos steps from one random column: the safeguarded upper bound of Zhou and Li (Y. Zhou,
 * R.-C. Li, Linear Algebra Appl. 435 (2011) 480-493), and theta_min(T_k) - |beta_k|, the same at the other end, from the same run
 * (either pointer may be NULL).  Returns 0; -1, with 0 in both, when the start vector vanishes or the dense eigensolver fails. */
static int lanczos_bounds(void *A, int steps, struct OPS_ *ops, double *lower_out, double *upper_out)
{
	void **v; int j, k = 0, ip = 0, iv = 1, iw = 2, s[2], e[2];
	double *al, *be, *T, *w, *z, *work, nrm, last = 0.0, upper = 0.0, lower = 0.0; int rc = -1;
	if (steps < 1) steps = 1;
	al = (double*)calloc(2 * (size_t)steps + 2 * (size_t)steps * steps + 3 * (size_t)steps, sizeof(double));
	be = al + steps; T = be + steps; z = T + (size_t)steps * steps; w = z + (size_t)steps * steps; work = w + steps;
	ops->MultiVecCreateByMat(&v, 3, A, ops);
	ops->MultiVecSetRandomValue(v, iv, iv + 1, ops);
	nrm = sqrt(col_dot(v, iv, v, iv, ops));
	if (nrm > 0.0) {
		col_axpby(0.0, NULL, 0, 1.0 / nrm, v, iv, ops);
		for (j = 0; j < steps; ++j) {
			int t;
			s[0] = iv; e[0] = iv + 1; s[1] = iw; e[1] = iw + 1;
			ops->MatDotMultiVec(A, v, v, s, e, ops);
			al[j] = col_dot(v, iv, v, iw, ops);
			col_axpby(-al[j], v, iv, 1.0, v, iw, ops);
			if (j > 0) col_axpby(-be[j - 1], v, ip, 1.0, v, iw, ops);
			be[j] = sqrt(col_dot(v, iw, v, iw, ops));
			k = j + 1; last = be[j];
			if (!(be[j] > DBL_EPSILON * fabs(al[j])) || j + 1 == steps) break;      /* an invariant subspace: T_k's values are exact */
			col_axpby(0.0, NULL, 0, 1.0 / be[j], v, iw, ops);
			t = ip; ip = iv; iv = iw; iw = t;
		}
		for (j = 0; j < k; ++j) {
			T[(size_t)k * j + j] = al[j];
			if (j + 1 < k) T[(size_t)k * j + j + 1] = T[(size_t)k * (j + 1) + j] = be[j];
		}
		if (GCGE_SymEigHost('U', k, T, k, w, z, k, work) == 0) { upper = w[k - 1] + fabs(last); lower = w[0] - fabs(last); rc = 0; }
	}
	ops->MultiVecDestroy(&v, 3, ops);
	free(al);
	if (lower_out != NULL) *lower_out = lower;
	if (upper_out != NULL) *upper_out = upper;
	return rc;
}

int GCGE_LanczosBounds(void *A, int steps, double *lmin, double *lmax, struct OPS_ *ops)
{
	GCGE_COMM *comm = GCGE_GetComm();
	if (A == NULL || ops == NULL || steps < 1 || (comm != NULL && comm->size > 1)) return -1;
	return lanczos_bounds(A, steps, ops, lmin, lmax);
}

/* Ritz pairs of A on span X[:, c..n): X[:, c..n) <- X[:, c..n) Q, eval[c..n) ascending; `work` a block of n - c columns or more */
static int rayleigh_ritz(void *A, void **x, int c, int n, double *eval, void **work, double *H, double *Q, double *dws, struct OPS_ *ops)
{
	int N = n - c, s[2], e[2];
	if (N <= 0) return 0;
	s[0] = c; e[0] = n; s[1] = c; e[1] = n;
	ops->MultiVecQtAP('S', 'N', x, A, x, 0, s, e, H, N, work, ops);
	if (GCGE_SymEigFor(ops, 'U', N, H, N, eval + c, Q, N, dws) != 0) return -1;
	s[0] = c; e[0] = n; s[1] = 0; e[1] = N;
	ops->MultiVecLinearComb(x, work, 0, s, e, Q, N, NULL, 0, ops);
	s[0] = 0; e[0] = N; s[1] = c; e[1] = n;
	ops->MultiVecAxpby(1.0, work, 0.0, x, s, e, ops);
	return 0;
}

/* the leading converged pairs among [c, upto) by the rule of gcg.c's CheckConvergence: the new count */
static int leading_converged(void *A, void **x, int c, int upto, const double *eval, const double tol[2], double *res, struct OPS_ *ops)
{
	int idx;
	if (upto <= c) return c;
	if (GCGE_ResidualNorms(A, NULL, x, c, upto, eval + c, res, ops) != 0) return c;
	for (idx = 0; idx < upto - c; ++idx) {
		const double ev = fabs(eval[c + idx]);
		const int bad = ev > tol[1] ? (res[idx] > tol[0] || res[idx] > ev * tol[1]) : (res[idx] > tol[0]);
		if (bad) {
			ops->Printf("ChFSI: [%d] %6.14e (%6.4e, %6.4e)\n", c + idx, eval[c + idx], res[idx], res[idx] / ev);
			break;
		}
	}
	return c + idx;
}

int GCGE_RunChFSI(void *A, int argc, char *argv[], struct OPS_ *ops, double *eval, void **evec, int nevGiven, GCGE_CHFSI_RESULT *res)
{
	int nevConv = 30, nevMax, max_niter = 100, degree = 20, lanczos_steps = 10, have_upper, conv = 0, numIter = 0, ncol, given, end, rc = 0, pass;
	double tol[2] = {1e-1, 1e-8}, upper = 0.0, lower = 0.0, lowest = 0.0, t0, *H, *Q, *dws, *rn, *orth_ws;
	void **w1, **w2; GCGE_COMM *comm = GCGE_GetComm();
	void (*orth_before) (void **, int, int *, void *, struct OPS_ *); void *orth_ws_before;

	if (res != NULL) memset(res, 0, sizeof(*res));
	if (A == NULL || ops == NULL || eval == NULL || evec == NULL || nevGiven < 0) return -1;
	if (comm != NULL && comm->size > 1) return -2;      /* row slabs: not yet */
	ops->GetOptionFromCommandLine("-nevConv", 'i', &nevConv, argc, argv, ops);
	nevMax = 2 * nevConv;
	ops->GetOptionFromCommandLine("-nevMax", 'i', &nevMax, argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_abs_tol", 'f', &tol[0], argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_rel_tol", 'f', &tol[1], argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_max_niter", 'i', &max_niter, argc, argv, ops);
	ops->GetOptionFromCommandLine("-chfsi_degree", 'i', &degree, argc, argv, ops);
	ops->GetOptionFromCommandLine("-chfsi_lanczos_steps", 'i', &lanczos_steps, argc, argv, ops);
	have_upper = ops->GetOptionFromCommandLine("-chfsi_upper_bound", 'f', &upper, argc, argv, ops);
	if (nevConv < 1 || nevMax < nevConv || nevGiven > nevMax || degree < 1 || max_niter < 0 || lanczos_steps < 1) return -1;
	if (have_upper && !(upper == upper && fabs(upper) <= DBL_MAX)) return -1;

	t0 = ops->GetWtime();
	ops->Printf("===============================================\n");
	ops->Printf("ChFSI Eigen Solver\n");
	ops->Printf("nevGiven = %d, nevConv = %d, nevMax = %d, degree = %d\n", nevGiven, nevConv, nevMax, degree);
	srand(0);      /* as the harness: the random columns are the rand() stream after srand(0) where the back-end draws from it */
	orth_before = ops->MultiVecOrth; orth_ws_before = ops->orth_workspace;
	ops->MultiVecCreateByMat(&w1, nevMax, A, ops);
	ops->MultiVecCreateByMat(&w2, nevMax, A, ops);
	H = (double*)calloc(2 * (size_t)nevMax * nevMax + 3 * (size_t)nevMax + (size_t)nevMax * nevMax + 2 * (size_t)nevMax, sizeof(double));
	Q = H + (size_t)nevMax * nevMax; dws = Q + (size_t)nevMax * nevMax; rn = dws + 2 * (size_t)nevMax; orth_ws = rn + nevMax;

	ops->MultiVecSetRandomValue(evec, nevGiven, nevMax, ops);      /* (first: the same columns whether a bound is given or not) */

	/* 1. the upper bound */
	if (!have_upper) lanczos_bounds(A, lanczos_steps, ops, NULL, &upper);
	ops->Printf("ChFSI: upper bound %6.14e (%s)\n", upper, have_upper ? "given" : "Lanczos");

	/* 2. the start block: the given columns, the rest random, orthonormalised as GCG's InitializeX does by default */
	MultiVecOrthSetup_ModifiedGramSchmidt(80, 2, 2 * DBL_EPSILON, w2, orth_ws, ops);
	given = nevGiven;
	ops->MultiVecOrth(evec, 0, &given, NULL, ops);
	if (given < nevGiven) ops->MultiVecSetRandomValue(evec, given, nevMax, ops);      /* dependent start vectors were dropped */
	ncol = nevMax;
	ops->MultiVecOrth(evec, given, &ncol, NULL, ops);
	if (ncol < nevConv) rc = -3;      /* the random block has no full rank */
	if (rc == 0 && rayleigh_ritz(A, evec, 0, ncol, eval, w1, H, Q, dws, ops) != 0) rc = -4;
	if (rc == 0) conv = leading_converged(A, evec, 0, nevConv, eval, tol, rn, ops);

	/* 3. filter, orthonormalise, Rayleigh-Ritz, test, lock */
	while (rc == 0 && conv < nevConv && numIter < max_niter) {
		lowest = eval[0]; lower = eval[ncol - 1];
		if (!(lower > lowest)) lower = lowest + 0.5 * fabs(upper - lowest);        /* a block of one column */
		if (!(upper > lower)) {                                                  /* a bound below the block's Ritz values: not a bound */
			ops->Printf("ChFSI: the upper bound %6.14e is not above the largest Ritz value %6.14e\n", upper, lower);
			rc = -5; break;
		}
		if (cheb_filter(A, evec, conv, ncol - conv, degree, lower, upper, lowest, w1, w2, conv, ops) != 0) { rc = -5; break; }
		for (pass = 0, end = conv; pass < 3 && end < ncol; ++pass) {             /* (a dropped column is drawn again) */
			if (pass > 0) ops->MultiVecSetRandomValue(evec, end, ncol, ops);
			given = end; end = ncol;
			ops->MultiVecOrth(evec, given, &end, NULL, ops);
		}
		if (end < nevConv) { rc = -3; break; }
		ncol = end;
		if (rayleigh_ritz(A, evec, conv, ncol, eval, w1, H, Q, dws, ops) != 0) { rc = -4; break; }
		++numIter;
		conv = leading_converged(A, evec, conv, nevConv, eval, tol, rn, ops);
	}

	ops->MultiVecOrth = orth_before; ops->orth_workspace = orth_ws_before;
	ops->MultiVecDestroy(&w1, nevMax, ops);
	ops->MultiVecDestroy(&w2, nevMax, ops);
	free(H);
	if (res != NULL) {
		res->nevConv = conv; res->numIter = numIter; res->degree = degree; res->seconds = ops->GetWtime() - t0;
		res->lower = lower; res->upper = upper;
	}
	ops->Printf("numIter = %d, nevConv = %d\n", numIter, conv);
	ops->Printf("Time is %.3f\n", ops->GetWtime() - t0);
	return rc;
}

/* ---- eigenpairs inside an interval: a band-pass filter, a SUM of Chebyshev terms ------------------------------------------------
 * p(t) = sum_j mu_j T_j(t), t = (lambda - c) / e, the Jackson-damped Chebyshev expansion of the indicator of [a, b] (A. Weisse,
 * G. Wellein, A. Alvermann, H. Fehske, Rev. Mod. Phys. 78 (2006) 275-306; E. Di Napoli, E. Polizzi, Y. Saad, Numer. Linear Algebra
 * Appl. 23 (2016) 674-692): about 1 inside, about 0 outside, 1/2 at the ends, monotone across each end. */
int GCGE_ChebBandCoefficients(int degree, double a, double b, double lmin, double lmax, double *mu)
{
	const double pi = 3.14159265358979323846;
	double c, e, ta, tb, tha, thb, al;
	int j;
	if (mu == NULL || degree < 2 || !(lmin < lmax) || !(a < b) || !(a <= lmax) || !(b >= lmin)) return -1;
	c = 0.5 * (lmax + lmin); e = 0.5 * (lmax - lmin);
	ta = (a - c) / e; if (ta < -1.0) ta = -1.0;
	tb = (b - c) / e; if (tb > 1.0) tb = 1.0;
	tha = acos(ta); thb = acos(tb);
	al = pi / (degree + 2);
	for (j = 0; j <= degree; ++j) {
		const double gamma = j == 0 ? (tha - thb) / pi : 2.0 * (sin(j * tha) - sin(j * thb)) / (j * pi);
		const double g = ((degree + 2 - j) * cos(j * al) + sin(j * al) * (cos(al) / sin(al))) / (degree + 2);
		mu[j] = gamma * g;
	}
	return 0;
}

/* p at lambda by the recurrence, lambda clamped to [lmin, lmax] (an end outside the bounds has no eigenvalue near it) */
static double band_poly(int degree, const double *mu, double c, double e, double lambda)
{
	double t = (lambda - c) / e, t0 = 1.0, t1, p;
	int j;
	if (t < -1.0) t = -1.0;
	if (t > 1.0) t = 1.0;
	t1 = t; p = mu[0] + mu[1] * t;
	for (j = 2; j <= degree; ++j) {
		const double t2 = 2.0 * t * t1 - t0;
		p += mu[j] * t2; t0 = t1; t1 = t2;
	}
	return p;
}

/* acc[:, a0..) = [acc +] mu_a ta[:, ta0..) + mu_b tb[:, tb0..)   (tb == NULL: one term; init: acc is not read): the back-end's
 * cheb_accum (one sweep) where the table offers it and it accepts, else two MultiVecAxpby */
static void cheb_accum(void **acc, int a0, void **ta, int ta0, double mu_a, void **tb, int tb0, double mu_b, int m, int init,
		const GCGE_BACKEND *be, struct OPS_ *ops)
{
	int s[2], e[2];
	if (be->cheb_accum != NULL && be->cheb_accum(acc, a0, ta, ta0, mu_a, tb, tb0, mu_b, m, init, ops)) return;
	s[0] = ta0; e[0] = ta0 + m; s[1] = a0; e[1] = a0 + m;
	ops->MultiVecAxpby(mu_a, ta, init ? 0.0 : 1.0, acc, s, e, ops);
	if (tb != NULL) {
		s[0] = tb0; e[0] = tb0 + m;
		ops->MultiVecAxpby(mu_b, tb, 1.0, acc, s, e, ops);
	}
}

/* x[:, x0..) <- sum_j mu[j] T_j((A - c) / e) x[:, x0..): the ring of three blocks of cheb_filter (block 0 is x itself, the work
 * blocks' windows at column w0), the iterates added to acc[:, w0..) in pairs while both are live (the order a one-pass kernel for
 * two terms would take: init on (T_0, T_1), then (T_2, T_3), ...), acc copied into x at the end (and left holding the result). */
static void cheb_band_filter(void *A, void **x, int x0, int m, int degree, const double *mu, double c, double ee,
		void **work1, void **work2, void **acc, int w0, struct OPS_ *ops)
{
	const GCGE_BACKEND be = GCGE_BackendOf(ops);
	void **blk[3]; int col[3], i, s[2], e[2];
	blk[0] = x; col[0] = x0; blk[1] = work1; col[1] = w0; blk[2] = work2; col[2] = w0;
	/* step i reads block (i - 1) % 3 (and (i - 2) % 3) and writes T_i into block i % 3 */
	cheb_step(A, blk[0], col[0], NULL, 0, blk[1], col[1], m, 1.0 / ee, c, 0.0, &be, ops);
	cheb_accum(acc, w0, blk[0], col[0], mu[0], blk[1], col[1], mu[1], m, 1, &be, ops);
	for (i = 2; i <= degree; ++i) {
		const int iy = (i - 1) % 3, iz = (i - 2) % 3, io = i % 3;
		cheb_step(A, blk[iy], col[iy], blk[iz], col[iz], blk[io], col[io], m, 2.0 / ee, c, 1.0, &be, ops);
		if (i & 1) cheb_accum(acc, w0, blk[iy], col[iy], mu[i - 1], blk[io], col[io], mu[i], m, 0, &be, ops);
		else if (i == degree) cheb_accum(acc, w0, blk[io], col[io], mu[i], NULL, 0, 0.0, m, 0, &be, ops);
	}
	s[0] = w0; e[0] = w0 + m; s[1] = x0; e[1] = x0 + m;
	ops->MultiVecAxpby(1.0, acc, 0.0, x, s, e, ops);
}

int GCGE_ChebBandFilter(void *A, void **x, int x0, int m, int degree, double a, double b, double lmin, double lmax,
		void **work1, void **work2, void **acc, struct OPS_ *ops)
{
	double *mu;
	if (A == NULL || x == NULL || work1 == NULL || work2 == NULL || acc == NULL || ops == NULL || x0 < 0 || m < 0 || degree < 2) return -1;
	if (x == work1 || x == work2 || work1 == work2 || acc == x || acc == work1 || acc == work2) return -1;
	mu = (double*)malloc(((size_t)degree + 1) * sizeof(double));
	if (mu == NULL) return -1;
	if (GCGE_ChebBandCoefficients(degree, a, b, lmin, lmax, mu) != 0) { free(mu); return -1; }
	if (m > 0) cheb_band_filter(A, x, x0, m, degree, mu, 0.5 * (lmax + lmin), 0.5 * (lmax - lmin), work1, work2, acc, 0, ops);
	free(mu);
	return 0;
}

static int pair_passes(double eval, double rn, const double tol[2])
{
	const double ev = fabs(eval);
	return ev > tol[1] ? !(rn > tol[0] || rn > ev * tol[1]) : !(rn > tol[0]);      /* (leading_converged's rule) */
}

int GCGE_RunChFSIBand(void *A, int argc, char *argv[], struct OPS_ *ops, double *eval, void **evec, int nevGiven, GCGE_CHFSI_BAND_RESULT *res)
{
	int nevMax = 0, max_niter = 100, degree = 0, lanczos_steps = 10, have_a, have_b, have_n, have_lo, have_up, have_deg;
	int numIter = 0, ncol = 0, given, end, rc = 0, pass, i, j, ngen = 0, nspur = 0, converged = 0, *kind, s[2], e[2];
	double tol[2] = {1e-1, 1e-8}, a = 0.0, b = 0.0, lmin = 0.0, lmax = 0.0, edge = 0.0, c, ee, t0, *H, *Q, *dws, *rn, *rho, *ev2, *orth_ws, *mu = NULL;
	void **w1, **w2, **acc, **xc; GCGE_COMM *comm = GCGE_GetComm();
	void (*orth_before) (void **, int, int *, void *, struct OPS_ *); void *orth_ws_before;

	if (res != NULL) memset(res, 0, sizeof(*res));
	if (A == NULL || ops == NULL || eval == NULL || evec == NULL || nevGiven < 0) return -1;
	if (comm != NULL && comm->size > 1) return -2;      /* row slabs: not yet */
	have_a = ops->GetOptionFromCommandLine("-chfsi_band_lo", 'f', &a, argc, argv, ops);
	have_b = ops->GetOptionFromCommandLine("-chfsi_band_hi", 'f', &b, argc, argv, ops);
	have_n = ops->GetOptionFromCommandLine("-nevMax", 'i', &nevMax, argc, argv, ops);
	have_deg = ops->GetOptionFromCommandLine("-chfsi_degree", 'i', &degree, argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_abs_tol", 'f', &tol[0], argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_rel_tol", 'f', &tol[1], argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_max_niter", 'i', &max_niter, argc, argv, ops);
	ops->GetOptionFromCommandLine("-chfsi_lanczos_steps", 'i', &lanczos_steps, argc, argv, ops);
	have_lo = ops->GetOptionFromCommandLine("-chfsi_lower_bound", 'f', &lmin, argc, argv, ops);
	have_up = ops->GetOptionFromCommandLine("-chfsi_upper_bound", 'f', &lmax, argc, argv, ops);
	if (!have_a || !have_b || !have_n || !(a < b) || !(fabs(a) <= DBL_MAX) || !(fabs(b) <= DBL_MAX)) return -1;
	if (nevMax < 1 || nevGiven > nevMax || (have_deg && degree < 2) || max_niter < 0 || lanczos_steps < 1) return -1;
	if ((have_lo && !(fabs(lmin) <= DBL_MAX)) || (have_up && !(fabs(lmax) <= DBL_MAX))) return -1;
	if (have_lo && have_up && (!(lmin < lmax) || !(a <= lmax) || !(b >= lmin))) return -1;

	t0 = ops->GetWtime();
	ops->Printf("===============================================\n");
	ops->Printf("ChFSI Eigen Solver, interval [%6.14e, %6.14e]\n", a, b);
	srand(0);      /* as GCGE_RunChFSI */
	orth_before = ops->MultiVecOrth; orth_ws_before = ops->orth_workspace;
	ops->MultiVecCreateByMat(&w1, nevMax, A, ops);
	ops->MultiVecCreateByMat(&w2, nevMax, A, ops);
	ops->MultiVecCreateByMat(&acc, nevMax, A, ops);
	ops->MultiVecCreateByMat(&xc, nevMax, A, ops);
	H = (double*)calloc(2 * (size_t)nevMax * nevMax + 3 * (size_t)nevMax + (size_t)nevMax * nevMax + 2 * (size_t)nevMax + 3 * (size_t)nevMax, sizeof(double));
	Q = H + (size_t)nevMax * nevMax; dws = Q + (size_t)nevMax * nevMax; rn = dws + 2 * (size_t)nevMax; orth_ws = rn + nevMax;
	rho = orth_ws + (size_t)nevMax * nevMax + 2 * (size_t)nevMax; ev2 = rho + nevMax;
	kind = (int*)calloc((size_t)nevMax, sizeof(int));      /* of a pair inside [a, b]: 1 genuine, 2 spurious; 0 outside */

	ops->MultiVecSetRandomValue(evec, nevGiven, nevMax, ops);

	/* 1. the bounds: one Lanczos run gives whichever the caller left out */
	if (!have_lo || !have_up) {
		double lo = 0.0, up = 0.0;
		if (lanczos_bounds(A, lanczos_steps, ops, &lo, &up) != 0) rc = -5;
		if (!have_lo) lmin = lo;
		if (!have_up) lmax = up;
	}
	ops->Printf("ChFSI: bounds %6.14e (%s), %6.14e (%s)\n", lmin, have_lo ? "given" : "Lanczos", lmax, have_up ? "given" : "Lanczos");
	if (rc == 0 && (!(lmin < lmax) || !(a <= lmax) || !(b >= lmin))) rc = -5;      /* the interval misses the bounds */
	c = 0.5 * (lmax + lmin); ee = 0.5 * (lmax - lmin);
	if (rc == 0 && !have_deg) {
		const double d = ceil(GCGE_CHFSI_BAND_DEGREE_FACTOR * (lmax - lmin) / (b - a));
		degree = d < 20.0 ? 20 : d > 1000.0 ? 1000 : (int)d;
	}
	if (rc == 0) {
		mu = (double*)malloc(((size_t)degree + 1) * sizeof(double));
		if (mu == NULL || GCGE_ChebBandCoefficients(degree, a, b, lmin, lmax, mu) != 0) rc = -5;
	}
	if (rc == 0) {
		const double pa = band_poly(degree, mu, c, ee, a), pb = band_poly(degree, mu, c, ee, b);
		edge = pa < pb ? pa : pb;
		ops->Printf("ChFSI: degree %d, p(a) = %6.14e, p(b) = %6.14e\n", degree, pa, pb);
	}

	/* 2. the start block, as GCGE_RunChFSI */
	if (rc == 0) {
		MultiVecOrthSetup_ModifiedGramSchmidt(80, 2, 2 * DBL_EPSILON, w2, orth_ws, ops);
		given = nevGiven;
		ops->MultiVecOrth(evec, 0, &given, NULL, ops);
		if (given < nevGiven) ops->MultiVecSetRandomValue(evec, given, nevMax, ops);
		ncol = nevMax;
		ops->MultiVecOrth(evec, given, &ncol, NULL, ops);
		if (ncol < 1) rc = -3;
	}
	if (rc == 0 && rayleigh_ritz(A, evec, 0, ncol, eval, w1, H, Q, dws, ops) != 0) rc = -4;

	/* 3. residuals of the Ritz vectors, filter (their rho comes out of it), decide on THOSE vectors; else orthonormalise, Rayleigh-Ritz */
	while (rc == 0) {
		int all_pass = 1;
		if (GCGE_ResidualNorms(A, NULL, evec, 0, ncol, eval, rn, ops) != 0) { rc = -4; break; }
		s[0] = 0; e[0] = ncol; s[1] = 0; e[1] = ncol;
		ops->MultiVecAxpby(1.0, evec, 0.0, xc, s, e, ops);                              /* the Ritz vectors, kept */
		cheb_band_filter(A, evec, 0, ncol, degree, mu, c, ee, w1, w2, acc, 0, ops);
		ops->MultiVecInnerProd('D', xc, evec, 0, s, e, rho, 1, ops);                    /* rho_i = x_i^T p(A) x_i */
		ngen = nspur = 0;
		for (i = 0; i < ncol; ++i) {
			kind[i] = 0;
			if (!(eval[i] >= a && eval[i] <= b)) continue;
			if (rho[i] >= edge) {
				kind[i] = 1; ++ngen;
				if (!pair_passes(eval[i], rn[i], tol)) {
					if (all_pass) ops->Printf("ChFSI: [%d] %6.14e (%6.4e, rho %6.4e)\n", i, eval[i], rn[i], rho[i]);
					all_pass = 0;
				}
			} else { kind[i] = 2; ++nspur; }
		}
		if (numIter >= 2 && ngen == ncol) rc = -6;                                    /* every column holds a wanted pair: the block is too small */
		else if (ngen > 0 && all_pass) converged = 1;
		if (converged || rc != 0 || numIter >= max_niter) {
			/* the Ritz vectors back from xc, the genuine pairs first (ascending, as they are), the others behind them: one block
			 * copy when the genuine pairs already lead, column by column otherwise */
			for (i = 0; i < ncol && (kind[i] == 1) == (i < ngen); ++i) ;
			if (i == ncol) {
				s[0] = 0; e[0] = ncol; s[1] = 0; e[1] = ncol;
				ops->MultiVecAxpby(1.0, xc, 0.0, evec, s, e, ops);
				break;
			}
			for (pass = 1, j = 0; pass >= 0; --pass)
				for (i = 0; i < ncol; ++i)
					if ((kind[i] == 1) == pass) { col_axpby(1.0, xc, i, 0.0, evec, j, ops); ev2[j] = eval[i]; ++j; }
			memcpy(eval, ev2, (size_t)ncol * sizeof(double));
			break;
		}
		for (pass = 0, end = 0; pass < 3 && end < ncol; ++pass) {                     /* (a dropped column is drawn again) */
			if (pass > 0) ops->MultiVecSetRandomValue(evec, end, ncol, ops);
			given = end; end = ncol;
			ops->MultiVecOrth(evec, given, &end, NULL, ops);
		}
		if (end < 1) { rc = -3; break; }
		ncol = end;
		if (rayleigh_ritz(A, evec, 0, ncol, eval, w1, H, Q, dws, ops) != 0) { rc = -4; break; }
		++numIter;
	}

	ops->MultiVecOrth = orth_before; ops->orth_workspace = orth_ws_before;
	ops->MultiVecDestroy(&w1, nevMax, ops);
	ops->MultiVecDestroy(&w2, nevMax, ops);
	ops->MultiVecDestroy(&acc, nevMax, ops);
	ops->MultiVecDestroy(&xc, nevMax, ops);
	free(H); free(kind); free(mu);
	if (res != NULL) {
		res->nevConv = ngen; res->numIter = numIter; res->degree = degree; res->spurious = nspur; res->converged = converged;
		res->seconds = ops->GetWtime() - t0; res->lmin = lmin; res->lmax = lmax; res->edge = edge;
	}
	ops->Printf("numIter = %d, inside = %d, spurious = %d\n", numIter, ngen, nspur);
	ops->Printf("Time is %.3f\n", ops->GetWtime() - t0);
	return rc;
}

/* ---- eigenvalue counts and the density of states from Chebyshev moments: the kernel polynomial method (Weisse et al., cited above;
 * L. Lin, Y. Saad, C. Yang, SIAM Rev. 58 (2016) 34-65; E. Di Napoli, E. Polizzi, Y. Saad, cited above, for the counts) ---------------
 * mu_j = v^T T_j(At) v, At = (A - c) / e, for every column v of a block of probes.  With t_k = T_k(At) v and T_2k = 2 T_k^2 - 1,
 * T_{2k+1} = 2 T_{k+1} T_k - T_1 (A symmetric: v^T T_k T_l v = t_k . t_l),
 *     mu_2k = 2 t_k . t_k - mu_0 ,   mu_{2k-1} = 2 t_k . t_{k-1} - mu_1 :
 * two column sums per step of the recurrence, ceil(degree / 2) steps and as many products, no second block of vectors. */

/* the sums every rank holds over its own rows, added over the ranks: lin_sol.c's rule for sums that came out of
 * MultiVecLocalInnerProd (a back-end may have reduced them already); a slot's sums are local whatever that switch says */
static void sum_over_ranks(double *v, int n, int from_slot)
{
	GCGE_COMM *c = GCGE_GetComm();
	if (!from_slot && GCGE_GetLocalInnerProdReduces()) return;
	if (c != NULL && n > 0) c->allreduce_sum(v, n, c->ctx);
}

static void local_col_dots(void **x, int x0, void **y, int y0, int m, double *out, struct OPS_ *ops)
{
	int s[2], e[2];
	s[0] = x0; e[0] = x0 + m; s[1] = y0; e[1] = y0 + m;
	ops->MultiVecLocalInnerProd('D', x, y, 0, s, e, out, 1, ops);
}

/* cheb_step, and dots[j] = out_j . out_j, dots[m + j] = out_j . y_j over all ranks: ONE call of the back-end's cheb_step_dots where
 * the table offers it and it accepts, else the step and two MultiVecLocalInnerProd('D') */
static void cheb_step_dots(void *A, void **y, int y0, void **z, int z0, void **out, int o0, int m, double alpha, double c, double beta,
		double *dots, const GCGE_BACKEND *be, struct OPS_ *ops)
{
	if (be->cheb_step_dots != NULL && be->cheb_step_dots(A, y, y0, z, z0, out, o0, m, alpha, c, beta, dots, dots + m, ops)) {
		sum_over_ranks(dots, 2 * m, 1);
		return;
	}
	cheb_step(A, y, y0, z, z0, out, o0, m, alpha, c, beta, be, ops);
	local_col_dots(out, o0, out, o0, m, dots, ops);
	local_col_dots(out, o0, y, y0, m, dots + m, ops);
	sum_over_ranks(dots, 2 * m, 0);
}

int GCGE_ChebMoments(void *A, void **v, int v0, int m, int degree, double lmin, double lmax, void **w1, void **w2, void **w3,
		double *moments, struct OPS_ *ops)
{
	void **ring[3]; double *dots, c, ee; int k, col, steps;
	if (A == NULL || v == NULL || w1 == NULL || w2 == NULL || w3 == NULL || moments == NULL || ops == NULL) return -1;
	if (v0 < 0 || m < 1 || degree < 1 || !(lmin < lmax)) return -1;
	if (v == w1 || v == w2 || v == w3 || w1 == w2 || w1 == w3 || w2 == w3) return -1;
	dots = (double*)malloc(2 * (size_t)m * sizeof(double));
	if (dots == NULL) return -1;
	{
		const GCGE_BACKEND be = GCGE_BackendOf(ops);
		ring[0] = w1; ring[1] = w2; ring[2] = w3;
		c = 0.5 * (lmax + lmin); ee = 0.5 * (lmax - lmin);
		steps = (degree + 1) / 2;
		local_col_dots(v, v0, v, v0, m, moments, ops);                               /* mu_0 = v . v */
		sum_over_ranks(moments, m, 0);
		/* step k writes t_k into ring[(k - 1) % 3] from t_{k-1} and t_{k-2} (t_0 is v itself, read only) */
		for (k = 1; k <= steps; ++k) {
			void **out = ring[(k - 1) % 3], **y = k == 1 ? v : ring[(k - 2) % 3], **z = k == 1 ? NULL : k == 2 ? v : ring[k % 3];
			cheb_step_dots(A, y, k == 1 ? v0 : 0, z, k == 2 ? v0 : 0, out, 0, m, k == 1 ? 1.0 / ee : 2.0 / ee, c, k == 1 ? 0.0 : 1.0,
					dots, &be, ops);
			for (col = 0; col < m; ++col) {
				moments[(size_t)(2 * k - 1) * m + col] = k == 1 ? dots[m + col] : 2.0 * dots[m + col] - moments[m + col];
				if (2 * k <= degree) moments[(size_t)(2 * k) * m + col] = 2.0 * dots[col] - moments[col];
			}
		}
	}
	free(dots);
	return 0;
}

int GCGE_ChebCountFromMoments(const double *moments, int m, int degree, double a, double b, double lmin, double lmax,
		double *count, double *stderr_, double *per_probe)
{
	double *mu, mean = 0.0, var = 0.0; int j, col;
	if (moments == NULL || count == NULL || stderr_ == NULL || m < 1 || degree < 2) return -1;
	mu = (double*)malloc(((size_t)degree + 1 + (size_t)m) * sizeof(double));
	if (mu == NULL) return -1;
	if (GCGE_ChebBandCoefficients(degree, a, b, lmin, lmax, mu) != 0) { free(mu); return -1; }
	{
		double *pp = mu + degree + 1;
		for (col = 0; col < m; ++col) {
			double s = 0.0;
			for (j = 0; j <= degree; ++j) s += mu[j] * moments[(size_t)j * m + col];
			pp[col] = s; mean += s;
		}
		mean /= m;
		for (col = 0; col < m; ++col) var += (pp[col] - mean) * (pp[col] - mean);
		*count = mean;
		*stderr_ = m > 1 ? sqrt(var / (m - 1)) / sqrt((double)m) : 0.0;
		if (per_probe != NULL) memcpy(per_probe, pp, (size_t)m * sizeof(double));
	}
	free(mu);
	return 0;
}
