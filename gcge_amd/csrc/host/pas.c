/* PAS (parallel augmented subspace) eigensolver and its composite operator table.
 *
 * Algorithm of the reference's src/ops_eig_sol_pas.c (PAS, PromoteX, ComputeN, OrthXtoQ, ComputeRayleighRitz,
 * ComputeRitzVec, CheckConvergence) and of its composite type app/app_pas.c, written from the math:
 *   - the composite table (gcge_pas.h) works through app_ops slots on the coarse part and host dense work on the tail;
 *   - our hierarchies are scaled (A_{l+1} = scale P^T A_l P, gcge_multigrid.h): every level-l quantity that enters the
 *     fine-level Rayleigh-Ritz problem carries the factor scale^-l (a power of two: exact), and the smoothing systems of
 *     level l read A_l v = scale^l lambda B_l v;
 *   - B == NULL: the masses of the coarse levels are P^T P (diagonal: the aggregate sizes), never the identity.
 * Every block lives in app_ops; only the tails (s x ncols) and the projected matrices are host memory.
 */
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gcge_solver.h"
#include "gcge_pas.h"
#include "gcge_multigrid.h"

/* ================================================================ composite table */
#define APP(ops) ((ops)->app_ops)

static GCGE_MAT_IDENTITY_FN g_identity = NULL; static GCGE_MAT_FREE_FN g_free = NULL;
void GCGE_PAS_SetMatIdentity(GCGE_MAT_IDENTITY_FN identity, GCGE_MAT_FREE_FN mat_free) { g_identity = identity; g_free = mat_free; }
GCGE_MAT_IDENTITY_FN GCGE_PAS_MatIdentityOf(struct OPS_ *ops, GCGE_MAT_FREE_FN *mat_free)
{
	GCGE_BACKEND be = GCGE_BackendOf(ops);
	if (be.mat_identity != NULL) { if (mat_free != NULL) *mat_free = be.mat_free; return be.mat_identity; }
	if (mat_free != NULL) *mat_free = g_free;
	return g_identity;
}

static void pv_new(PASVEC **pv, int ncols, int s)
{
	PASVEC *v = (PASVEC*)calloc(1, sizeof(PASVEC));
	v->x.nrows = s; v->x.ncols = ncols; v->x.ldd = s > 0 ? s : 1;
	v->x.data = (double*)calloc((size_t)v->x.ldd * (ncols > 0 ? ncols : 1), sizeof(double));
	v->owned = 1;
	*pv = v;
}
static void PAS_MultiVecCreateByMat(void ***mv, int num_vec, void *mat, struct OPS_ *ops)
{
	PASMAT *M = (PASMAT*)mat; PASVEC *v;
	pv_new(&v, num_vec, M->size);
	APP(ops)->MultiVecCreateByMat(&v->q, num_vec, M->mat_H, APP(ops));
	*mv = (void**)v;
}
static void PAS_MultiVecCreateByMultiVec(void ***mv, int num_vec, void **src, struct OPS_ *ops)
{
	PASVEC *s = (PASVEC*)src, *v;
	pv_new(&v, num_vec, s->x.nrows);
	APP(ops)->MultiVecCreateByMultiVec(&v->q, num_vec, s->q, APP(ops));
	*mv = (void**)v;
}
static void PAS_MultiVecDestroy(void ***mv, int num_vec, struct OPS_ *ops)
{
	PASVEC *v = (PASVEC*)*mv;
	if (v != NULL && v->owned) {
		APP(ops)->MultiVecDestroy(&v->q, num_vec, APP(ops));
		free(v->x.data); free(v);
	}
	*mv = NULL;
}
static void PAS_MultiVecView(void **x, int start, int end, struct OPS_ *ops)
{
	PASVEC *v = (PASVEC*)x;
	APP(ops)->MultiVecView(v->q, start, end, APP(ops));
	ops->lapack_ops->MultiVecView((void**)&v->x, start, end, ops->lapack_ops);
}
/* the tail's share of an inner product, added to ip */
static void tail_ip_add(char nsd, PASVEC *x, PASVEC *y, int *start, int *end, double *ip, int ldIP, struct OPS_ *ops)
{
	int k = end[0] - start[0], m = end[1] - start[1], i, j;
	double *t;
	if (k <= 0 || m <= 0 || x->x.nrows == 0) return;
	t = (double*)calloc((size_t)k * m, sizeof(double));
	ops->lapack_ops->MultiVecLocalInnerProd(nsd, (void**)&x->x, (void**)&y->x, 0, start, end, t, k, ops->lapack_ops);
	if (nsd == 'D') { for (j = 0; j < m; ++j) ip[(size_t)j * ldIP] += t[(size_t)j * k]; }
	else for (j = 0; j < m; ++j) for (i = 0; i < k; ++i) ip[i + (size_t)j * ldIP] += t[i + (size_t)j * k];
	free(t);
}
static void PAS_MultiVecLocalInnerProd(char nsd, void **x, void **y, int is_vec, int *start, int *end, double *ip, int ldIP,
		struct OPS_ *ops)
{
	GCGE_COMM *comm = GCGE_GetComm();
	APP(ops)->MultiVecLocalInnerProd(nsd, ((PASVEC*)x)->q, ((PASVEC*)y)->q, is_vec, start, end, ip, ldIP, APP(ops));
	if (comm == NULL || comm->rank == 0) tail_ip_add(nsd, (PASVEC*)x, (PASVEC*)y, start, end, ip, ldIP, ops);   /* once over the ranks */
}
static void PAS_MultiVecInnerProd(char nsd, void **x, void **y, int is_vec, int *start, int *end, double *ip, int ldIP,
		struct OPS_ *ops)
{
	APP(ops)->MultiVecInnerProd(nsd, ((PASVEC*)x)->q, ((PASVEC*)y)->q, is_vec, start, end, ip, ldIP, APP(ops));
	tail_ip_add(nsd, (PASVEC*)x, (PASVEC*)y, start, end, ip, ldIP, ops);   /* after the reduction: the tail counts once */
}
static void PAS_MultiVecSetRandomValue(void **x, int start, int end, struct OPS_ *ops)
{
	PASVEC *v = (PASVEC*)x;
	APP(ops)->MultiVecSetRandomValue(v->q, start, end, APP(ops));
	ops->lapack_ops->MultiVecSetRandomValue((void**)&v->x, start, end, ops->lapack_ops);
}
static void PAS_MultiVecAxpby(double alpha, void **x, double beta, void **y, int *start, int *end, struct OPS_ *ops)
{
	PASVEC *vx = (PASVEC*)x, *vy = (PASVEC*)y;
	APP(ops)->MultiVecAxpby(alpha, vx ? vx->q : NULL, beta, vy->q, start, end, APP(ops));
	ops->lapack_ops->MultiVecAxpby(alpha, vx ? (void**)&vx->x : NULL, beta, (void**)&vy->x, start, end, ops->lapack_ops);
}
static void PAS_MultiVecLinearComb(void **x, void **y, int is_vec, int *start, int *end, double *coef, int ldc,
		double *beta, int incb, struct OPS_ *ops)
{
	PASVEC *vx = (PASVEC*)x, *vy = (PASVEC*)y;
	APP(ops)->MultiVecLinearComb(vx ? vx->q : NULL, vy->q, is_vec, start, end, coef, ldc, beta, incb, APP(ops));
	ops->lapack_ops->MultiVecLinearComb(vx ? (void**)&vx->x : NULL, (void**)&vy->x, is_vec, start, end, coef, ldc, beta, incb,
			ops->lapack_ops);
}
/* y = M x:  y_q = alpha QQ x_q + QX x_x,   y_x = QX^T x_q + XX x_x   (QX == NULL: y_q = alpha QQ x_q, y_x = x_x) */
static void PAS_MatDotMultiVec(void *mat, void **x, void **y, int *start, int *end, struct OPS_ *ops)
{
	PASMAT *M = (PASMAT*)mat; PASVEC *vx = (PASVEC*)x, *vy = (PASVEC*)y;
	struct OPS_ *app = APP(ops);
	int m = end[0] - start[0], s = M->size, i, j, k;
	const double *t; double *g, *yx;
	int ys[2], ye[2];
	if (m <= 0) return;
	ys[0] = ys[1] = start[1]; ye[0] = ye[1] = end[1];
	app->MatDotMultiVec(M->QQ, vx->q, vy->q, start, end, app);
	t = vx->x.data + (size_t)vx->x.ldd * start[0];
	yx = vy->x.data + (size_t)vy->x.ldd * start[1];
	if (M->QX == NULL) {
		if (M->alpha != 1.0) app->MultiVecAxpby(0.0, NULL, M->alpha, vy->q, ys, ye, app);
		for (j = 0; j < m; ++j) memcpy(yx + (size_t)vy->x.ldd * j, t + (size_t)vx->x.ldd * j, s * sizeof(double));
		return;
	}
	g = (double*)calloc((size_t)s * m, sizeof(double));
	{
		GCGE_BACKEND be = GCGE_BackendOf(app); GCGE_COMM *comm = GCGE_GetComm();
		int fused = be.pas_border != NULL && (comm == NULL || comm->size <= 1) &&
				be.pas_border(M->QX, s, vx->q, start[0], vy->q, start[1], m, M->alpha, t, vx->x.ldd, g, s) == 0;
		if (!fused) {   /* the slots: scale, y_q += QX t (LinearComb), g = QX^T x_q (a Gram, reduced over the ranks) */
			int st[2], en[2]; double *ones = (double*)malloc((size_t)m * sizeof(double));
			for (j = 0; j < m; ++j) ones[j] = 1.0;
			if (M->alpha != 1.0) app->MultiVecAxpby(0.0, NULL, M->alpha, vy->q, ys, ye, app);
			st[0] = 0; en[0] = s; st[1] = start[1]; en[1] = end[1];
			app->MultiVecLinearComb(M->QX, vy->q, 0, st, en, (double*)t, vx->x.ldd, ones, 1, app);
			st[0] = 0; en[0] = s; st[1] = start[0]; en[1] = end[0];
			app->MultiVecInnerProd('N', M->QX, vx->q, 0, st, en, g, s, app);
			free(ones);
		}
	}
	for (j = 0; j < m; ++j) {
		double *yj = yx + (size_t)vy->x.ldd * j; const double *tj = t + (size_t)vx->x.ldd * j, *gj = g + (size_t)s * j;
		for (i = 0; i < s; ++i) yj[i] = gj[i];
		for (k = 0; k < s; ++k) { double c = tj[k]; const double *xk = M->XX + (size_t)s * k; for (i = 0; i < s; ++i) yj[i] += xk[i] * c; }
	}
	free(g);
}

void OPS_PAS_Set(struct OPS_ *pas_ops, struct OPS_ *app_ops)
{
	pas_ops->app_ops = app_ops;
	pas_ops->Printf = app_ops->Printf;
	pas_ops->GetWtime = app_ops->GetWtime;
	pas_ops->GetOptionFromCommandLine = app_ops->GetOptionFromCommandLine;
	pas_ops->MultiVecCreateByMat = PAS_MultiVecCreateByMat;
	pas_ops->MultiVecCreateByMultiVec = PAS_MultiVecCreateByMultiVec;
	pas_ops->MultiVecDestroy = PAS_MultiVecDestroy;
	pas_ops->MultiVecView = PAS_MultiVecView;
	pas_ops->MultiVecLocalInnerProd = PAS_MultiVecLocalInnerProd;
	pas_ops->MultiVecInnerProd = PAS_MultiVecInnerProd;
	pas_ops->MultiVecSetRandomValue = PAS_MultiVecSetRandomValue;
	pas_ops->MultiVecAxpby = PAS_MultiVecAxpby;
	pas_ops->MultiVecLinearComb = PAS_MultiVecLinearComb;
	pas_ops->MatDotMultiVec = PAS_MatDotMultiVec;
	pas_ops->MatTransDotMultiVec = PAS_MatDotMultiVec;     /* symmetric */
	pas_ops->MultiVecQtAP = DefaultMultiVecQtAP;          /* M P through the composite product, then the composite Gram */
	if (pas_ops->lapack_ops == NULL) { OPS_Create(&pas_ops->lapack_ops); OPS_DENSE_Set(pas_ops->lapack_ops); }
	pas_ops->lapack_ops->Printf = app_ops->Printf;
}

/* ================================================================ PAS */
typedef struct {
	struct OPS_ *ops, *pas_ops; PASSolver *p;
	int L, H, level, sizeX, sizeC, startN, endN, sizeN;
	void ***X, ***W[6];         /* X = mv_ws[0]; W[0] = mv_ws[1] (QX), W[1..5] = mv_ws[2..6] */
	double *ss_x, *XX, *dbl;    /* tail of the Ritz vectors, X^T A X (in dbl_ws), scratch of the solvers and orthonormalisation */
	int    *iws;
	double *sfac;               /* sfac[l] = scale^-l */
	double *eval; void **ritz;
} Pas;

static double *pas_res_scratch = NULL;

/* y = B_l x on columns (B_l == NULL: the identity of a standard problem on level 0) */
static void mat_B(Pas *c, int l, void **x, void **y, int *s, int *e)
{
	struct OPS_ *ops = c->ops;
	if (c->p->B[l] != NULL) ops->MatDotMultiVec(c->p->B[l], x, y, s, e, ops);
	else ops->MultiVecAxpby(1.0, x, 0.0, y, s, e, ops);
}
/* level i -> j on columns s0.. of x to columns s1.. of y, intermediate levels staged in W[2] */
static void transfer(Pas *c, int i, int j, void **x, int x0, void **y, int y0, int m)
{
	int st[2], en[2];
	st[0] = x0; en[0] = x0 + m; st[1] = y0; en[1] = y0 + m;
	c->ops->MultiVecFromItoJ(c->p->P, i, j, x, y, st, en, c->W[2], c->ops);
}

static void PromoteX(Pas *c)
{
	transfer(c, c->level, c->level - 1, c->X[c->level], 0, c->X[c->level - 1], 0, c->sizeX);
}

/* smoothing of A_l v = scale^l lambda B_l v by BlockAMG from level l down, columns startN .. endN */
static void ComputeN(Pas *c, void **v)
{
	struct OPS_ *ops = c->ops; PASSolver *p = c->p; int l = c->level, s[2], e[2], j, m = c->endN - c->startN;
	void **b = c->W[1][l], ***amg_ws[5];
	double *lam = (double*)malloc((size_t)(m > 0 ? m : 1) * sizeof(double));
	if (m <= 0) { free(lam); return; }
	s[0] = c->startN; e[0] = c->endN; s[1] = 0; e[1] = m;
	mat_B(c, l, v, b, s, e);
	for (j = 0; j < m; ++j) lam[j] = c->eval[c->startN + j] / c->sfac[l];
	s[0] = 0; e[0] = m;
	ops->MultiVecLinearComb(NULL, b, 0, s, e, NULL, 0, lam, 1, ops);
	for (j = 0; j < 5; ++j) amg_ws[j] = c->W[1 + j] + l;   /* (the cycle's right-hand side block of its top level, b, is unused) */
	MultiLinearSolverSetup_BlockAMG(p->compN_bamg_max_iter, p->compN_bamg_rate, p->compN_bamg_tol, p->compN_bamg_tol_type,
			p->A + l, p->P + l, p->num_levels - l, amg_ws, c->dbl, c->iws, NULL, ops);
	s[0] = 0; e[0] = m; s[1] = c->startN; e[1] = c->endN;
	ops->MultiLinearSolver(p->A[l], b, v, s, e, ops);
	free(lam);
}

/* X_l = orth_B(v - P q), q = B_H^-1 P^T B_l v;  the tail of the start vectors x = X^T B_l (v - P q) (v = P q + X x) */
static void OrthXtoQ(Pas *c, void **v)
{
	struct OPS_ *ops = c->ops; PASSolver *p = c->p; int l = c->level, H = c->H, n = c->sizeX, s[2], e[2], endX;
	void **Y = c->W[1][l], **q = c->X[H], **bH = c->W[1][H], **ws3[3];
	s[0] = 0; e[0] = n; s[1] = 0; e[1] = n;
	mat_B(c, l, v, Y, s, e);
	transfer(c, l, H, Y, 0, bH, 0, n);
	ops->MultiVecAxpby(0.0, NULL, 0.0, q, s, e, ops);
	ws3[0] = c->W[3][H]; ws3[1] = c->W[4][H]; ws3[2] = c->W[5][H];
	MultiLinearSolverSetup_BlockPCG(p->orthX_ls_max_iter, p->orthX_ls_rate, p->orthX_ls_tol, p->orthX_ls_tol_type, ws3,
			c->dbl, c->iws, NULL, NULL, ops);
	ops->MultiLinearSolver(p->B[H], bH, q, s, e, ops);
	transfer(c, H, l, q, 0, Y, 0, n);
	ops->MultiVecAxpby(1.0, v, -1.0, Y, s, e, ops);                 /* Y = v - P q */
	if (v != c->X[l]) ops->MultiVecAxpby(1.0, Y, 0.0, c->X[l], s, e, ops);
	else ops->MultiVecAxpby(1.0, Y, 0.0, v, s, e, ops);
	if (0 == strcmp("bgs", p->orthX_orth_method))
		MultiVecOrthSetup_BinaryGramSchmidt(p->orthX_orth_block_size, p->orthX_orth_max_reorth, p->orthX_orth_zero_tol,
				c->W[4][l], c->dbl, ops);
	else
		MultiVecOrthSetup_ModifiedGramSchmidt(p->orthX_orth_block_size, p->orthX_orth_max_reorth, p->orthX_orth_zero_tol,
				c->W[4][l], c->dbl, ops);
	endX = n;
	ops->MultiVecOrth(c->X[l], 0, &endX, p->B[l], ops);
	if (endX < n) {
		int k = endX; endX = n;
		ops->MultiVecSetRandomValue(c->X[l], k, n, ops);
		ops->MultiVecOrth(c->X[l], k, &endX, p->B[l], ops);
	}
	ops->MultiVecQtAP('S', 'N', c->X[l], p->B[l], Y, 0, s, e, c->ss_x, n, c->W[5][l], ops);
}

/* the augmented problem on level l: XX = scale^-l X^T A_l X, QX = scale^-l P^T(A_l X); GCG over the composite table */
static void ComputeRayleighRitz(Pas *c, PASMAT *ssA, PASMAT *ssB)
{
	struct OPS_ *ops = c->ops, *pops = c->pas_ops; PASSolver *p = c->p;
	int l = c->level, H = c->H, n = c->sizeX, s[2], e[2], i, b = p->block_size_rr, T = n + 2 * b, nevConv;
	void **AX = c->W[0][l];
	double *gdbl; int *gint;
	PASVEC evec, ws[4]; void **gws[4];
	s[0] = 0; e[0] = n; s[1] = 0; e[1] = n;
	ops->MatDotMultiVec(p->A[l], c->X[l], AX, s, e, ops);
	ops->MultiVecInnerProd('S', c->X[l], AX, 0, s, e, c->XX, n, ops);
	for (i = 0; i < n * n; ++i) c->XX[i] *= c->sfac[l];
	for (i = 0; i < n; ++i) { int j; for (j = 0; j < i; ++j) { double a = 0.5 * (c->XX[i + j * n] + c->XX[j + i * n]); c->XX[i + j * n] = c->XX[j + i * n] = a; } }
	transfer(c, l, H, AX, 0, c->W[0][H], 0, n);
	ops->MultiVecAxpby(0.0, NULL, c->sfac[l], c->W[0][H], s, e, ops);
	/* composite blocks around the level-H blocks: the Ritz vectors (q = X[H], x = ss_x) and GCG's four work blocks */
	memset(&evec, 0, sizeof(evec));
	evec.q = c->X[H]; evec.x.data = c->ss_x; evec.x.nrows = n; evec.x.ncols = n; evec.x.ldd = n;
	for (i = 0; i < 4; ++i) {
		int cols = i == 0 ? T : b;
		memset(&ws[i], 0, sizeof(PASVEC));
		ws[i].q = i == 0 ? c->W[5][H] : c->W[1 + i][H];
		ws[i].x.nrows = n; ws[i].x.ncols = cols; ws[i].x.ldd = n;
		ws[i].x.data = (double*)calloc((size_t)n * cols, sizeof(double));
		gws[i] = (void**)&ws[i];
	}
	gdbl = (double*)calloc((size_t)2 * T * T + 10 * (size_t)T + T + (size_t)n * b, sizeof(double));
	gint = (int*)calloc((size_t)6 * T + 2 * (b + 3), sizeof(int));
	EigenSolverSetup_GCG(p->multiMax, p->gapMin, n, n, b, p->tol_rr, p->numIterMax_rr, 0, gws, gdbl, gint, pops);
	EigenSolverSetParameters_GCG(p->compRR_gcg_check_conv_max_num,
			p->compRR_gcg_initX_orth_method, p->compRR_gcg_initX_orth_block_size, p->compRR_gcg_initX_orth_max_reorth,
			p->compRR_gcg_initX_orth_zero_tol,
			p->compRR_gcg_compP_orth_method, p->compRR_gcg_compP_orth_block_size, p->compRR_gcg_compP_orth_max_reorth,
			p->compRR_gcg_compP_orth_zero_tol,
			p->compRR_gcg_compW_orth_method, p->compRR_gcg_compW_orth_block_size, p->compRR_gcg_compW_orth_max_reorth,
			p->compRR_gcg_compW_orth_zero_tol,
			p->compRR_gcg_compW_cg_max_iter, p->compRR_gcg_compW_cg_rate, p->compRR_gcg_compW_cg_tol,
			p->compRR_gcg_compW_cg_tol_type, 0,
			p->compRR_gcg_compRR_min_num, p->compRR_gcg_compRR_min_gap, p->compRR_gcg_compRR_tol, pops);
	nevConv = p->nevConv < n - b ? p->nevConv : n - b;
	pops->EigenSolver(ssA, ssB, c->eval, (void**)&evec, n, &nevConv, pops);
	for (i = 0; i < 4; ++i) free(ws[i].x.data);
	free(gdbl); free(gint);
}

/* Ritz vectors of columns sizeC .. sizeX on level l: dst = P q + X x (dst == X[l] above level 0) */
static void ComputeRitzVec(Pas *c, void **dst)
{
	struct OPS_ *ops = c->ops; int l = c->level, n = c->sizeX, m = n - c->sizeC, s[2], e[2];
	void **T = c->W[1][l];
	if (m <= 0) return;
	s[0] = 0; e[0] = n; s[1] = 0; e[1] = m;
	ops->MultiVecLinearComb(c->X[l], T, 0, s, e, c->ss_x + (size_t)n * c->sizeC, n, NULL, 0, ops);
	transfer(c, c->H, l, c->X[c->H], c->sizeC, dst, c->sizeC, m);
	s[0] = 0; e[0] = m; s[1] = c->sizeC; e[1] = n;
	ops->MultiVecAxpby(1.0, T, 1.0, dst, s, e, ops);
}

/* residuals of numCheck pairs from startN on level 0: abs AND rel, then no cut inside a cluster (gapMin) */
static int CheckConvergence(Pas *c, int numCheck)
{
	struct OPS_ *ops = c->ops; PASSolver *p = c->p; int s[2], e[2], idx;
	void **AX = c->W[1][0], **BX = c->W[2][0];
	double *res = pas_res_scratch, *ev = c->eval + c->startN;
	if (numCheck <= 0) return c->sizeC;
	s[0] = c->startN; e[0] = c->startN + numCheck; s[1] = 0; e[1] = numCheck;
	ops->MatDotMultiVec(p->A[0], c->ritz, AX, s, e, ops);
	mat_B(c, 0, c->ritz, BX, s, e);
	s[0] = 0; e[0] = numCheck;
	ops->MultiVecLinearComb(NULL, BX, 0, s, e, NULL, 0, ev, 1, ops);
	ops->MultiVecAxpby(-1.0, BX, 1.0, AX, s, e, ops);
	ops->MultiVecInnerProd('D', AX, AX, 0, s, e, res, 1, ops);
	for (idx = 0; idx < numCheck; ++idx) {
		res[idx] = sqrt(res[idx]);
		ops->Printf("PAS: [%d] %6.14e (%6.4e, %6.4e)\n", c->startN + idx, ev[idx], res[idx], res[idx] / fabs(ev[idx]));
	}
	for (idx = 0; idx < numCheck; ++idx)
		if (res[idx] > p->tol[0] || res[idx] > fabs(ev[idx]) * p->tol[1]) break;
	for (; idx > 0 && idx < numCheck; --idx)
		if (fabs((ev[idx - 1] - ev[idx]) / ev[idx - 1]) > p->gapMin) break;
	return c->sizeC + idx;
}

/* one row order for every level: the prolongations are built in the hierarchy's numbering */
static int levels_as_given(struct OPS_ *ops, PASSolver *p)
{
	GCGE_BACKEND be = GCGE_BackendOf(ops); int l;
	if (be.mat_rows_as_given == NULL) return 1;
	for (l = 1; l < p->num_levels; ++l) {
		if (!be.mat_rows_as_given(p->A[l])) return 0;
		if (p->B[l] != NULL && !be.mat_rows_as_given(p->B[l])) return 0;
	}
	return 1;
}

static void PAS(void *A, void *B, double *eval, void **evec, int nevGiven, int *nevConv, struct OPS_ *ops)
{
	PASSolver *p = (PASSolver*)ops->eigen_solver_workspace; Pas ctx, *c = &ctx;
	PASMAT ssA, ssB; int i, l, nev, numIter, numCheck, s[2], e[2];
	void (*eig_sol)(void*, void*, double*, void**, int, int*, struct OPS_*); void *eig_ws;
	memset(c, 0, sizeof(*c));
	p->status = 0; p->numIter = 0;
	if (!levels_as_given(ops, p)) {
		ops->Printf("PAS: a level of the hierarchy was re-ordered by the back-end; the prolongations are in the hierarchy's row order\n");
		fprintf(stderr, "PAS: a coarse level does not keep the row order its prolongation was built for\n");
		p->status = -8; *nevConv = 0; return;
	}
	c->ops = ops; c->p = p; c->L = p->num_levels; c->H = p->level_aux; c->level = c->H;
	c->sizeX = p->nevMax; c->sizeC = 0; c->startN = 0; c->sizeN = c->sizeX; c->endN = c->sizeX;
	c->eval = eval; c->ritz = evec;
	c->X = p->mv_ws[0];
	for (i = 0; i < 6; ++i) c->W[i] = p->mv_ws[1 + i];
	c->ss_x = p->dbl_ws; c->XX = c->ss_x + (size_t)c->sizeX * c->sizeX;
	c->dbl = (double*)calloc((size_t)4 * (c->sizeX + 2 * p->block_size_rr) * (c->sizeX + 2 * p->block_size_rr) + 64 * (size_t)c->sizeX + 1024, sizeof(double));
	c->iws = (int*)calloc((size_t)8 * c->sizeX + 64, sizeof(int));
	memset(c->ss_x, 0, (size_t)c->sizeX * c->sizeX * sizeof(double));
	c->sfac = (double*)malloc((size_t)c->L * sizeof(double));
	for (l = 0; l < c->L; ++l) c->sfac[l] = l == 0 ? 1.0 : c->sfac[l - 1] / p->scale;
	pas_res_scratch = (double*)malloc((size_t)c->sizeX * sizeof(double));
	p->nevConv = *nevConv;

	OPS_Create(&c->pas_ops);
	OPS_PAS_Set(c->pas_ops, ops);
	OPS_Setup(c->pas_ops);
	memset(&ssA, 0, sizeof(ssA)); memset(&ssB, 0, sizeof(ssB));
	ssA.QQ = p->A[c->H]; ssA.alpha = c->sfac[c->H]; ssA.QX = c->W[0][c->H]; ssA.XX = c->XX; ssA.size = c->sizeX; ssA.mat_H = p->A[c->H];
	ssB.QQ = p->B[c->H]; ssB.alpha = 1.0; ssB.size = c->sizeX; ssB.mat_H = p->A[c->H];

	/* 1. Rayleigh-Ritz on level H: plain GCG on (A_H, B_H) over app_ops (its eigenvalues times scale^-H are the fine ones) */
	{
		int b = p->block_size_rr, T = c->sizeX + 2 * b, nc;
		void **gws[4]; double *gdbl; int *gint;
		gws[0] = c->W[5][c->H]; gws[1] = c->W[2][c->H]; gws[2] = c->W[3][c->H]; gws[3] = c->W[4][c->H];
		gdbl = (double*)calloc((size_t)2 * T * T + 10 * (size_t)T + T + (size_t)c->sizeX * b, sizeof(double));
		gint = (int*)calloc((size_t)6 * T + 2 * (b + 3), sizeof(int));
		eig_sol = ops->EigenSolver; eig_ws = ops->eigen_solver_workspace;
		EigenSolverSetup_GCG(p->multiMax, p->gapMin, c->sizeX, c->sizeX, b, p->tol_rr, p->numIterMax_rr, 0, gws, gdbl, gint, ops);
		EigenSolverSetParameters_GCG(p->compRR_gcg_check_conv_max_num,
				p->compRR_gcg_initX_orth_method, p->compRR_gcg_initX_orth_block_size, p->compRR_gcg_initX_orth_max_reorth,
				p->compRR_gcg_initX_orth_zero_tol,
				p->compRR_gcg_compP_orth_method, p->compRR_gcg_compP_orth_block_size, p->compRR_gcg_compP_orth_max_reorth,
				p->compRR_gcg_compP_orth_zero_tol,
				p->compRR_gcg_compW_orth_method, p->compRR_gcg_compW_orth_block_size, p->compRR_gcg_compW_orth_max_reorth,
				p->compRR_gcg_compW_orth_zero_tol,
				p->compRR_gcg_compW_cg_max_iter, p->compRR_gcg_compW_cg_rate, p->compRR_gcg_compW_cg_tol,
				p->compRR_gcg_compW_cg_tol_type, 0,
				p->compRR_gcg_compRR_min_num, p->compRR_gcg_compRR_min_gap, p->compRR_gcg_compRR_tol, ops);
		nc = p->nevConv < c->sizeX - b ? p->nevConv : c->sizeX - b;
		ops->EigenSolver(p->A[c->H], p->B[c->H], eval, c->X[c->H], 0, &nc, ops);
		ops->EigenSolver = eig_sol; ops->eigen_solver_workspace = eig_ws;
		for (i = 0; i < c->sizeX; ++i) eval[i] *= c->sfac[c->H];
		free(gdbl); free(gint);
	}

	nev = *nevConv; *nevConv = 0; numIter = 0;
	do {
		ops->Printf("PAS: level = %d, numIter = %d, sizeC = %d, sizeN = %d, sizeX = %d\n", c->level, numIter, c->sizeC, c->sizeN, c->sizeX);
		if (c->level == 0) {
			numCheck = (c->startN + c->sizeN < c->sizeX) ? c->sizeN : (c->sizeX - c->startN);
			numCheck = numCheck < p->check_conv_max_num ? numCheck : p->check_conv_max_num;
			c->sizeC = CheckConvergence(c, numCheck);
			if (c->sizeC >= nev) break;
			c->startN = c->sizeC;
			c->endN = c->startN + p->block_size < c->sizeX ? c->startN + p->block_size : c->sizeX;
			c->sizeN = c->endN - c->startN;
		} else {
			PromoteX(c);
			--c->level;
			if (c->level == 0) {
				s[0] = 0; e[0] = c->sizeX; s[1] = 0; e[1] = c->sizeX;
				ops->MultiVecAxpby(1.0, c->X[0], 0.0, c->ritz, s, e, ops);
			}
		}
		ComputeN(c, c->level == 0 ? c->ritz : c->X[c->level]);
		OrthXtoQ(c, c->level == 0 ? c->ritz : c->X[c->level]);
		ComputeRayleighRitz(c, &ssA, &ssB);
		ComputeRitzVec(c, c->level == 0 ? c->ritz : c->X[c->level]);
		++numIter;
	} while (numIter < p->numIterMax + p->num_levels);
	p->numIter = numIter;
	*nevConv = c->sizeC;
	OPS_Destroy(&c->pas_ops);
	free(c->sfac); free(c->dbl); free(c->iws); free(pas_res_scratch); pas_res_scratch = NULL;
}

void GCGE_PASWorkspaceSizes(int nevMax, int block_size_rr, long *length_dbl_ws, long *length_int_ws)
{
	long n = nevMax;
	if (length_dbl_ws != NULL) *length_dbl_ws = 2 * n * n;
	if (length_int_ws != NULL) *length_int_ws = 1;
}

void EigenSolverSetup_PAS(int multiMax, double gapMin, int nevMax,
		int block_size, double tol[2], int numIterMax,
		int block_size_rr, double tol_rr[2], int numIterMax_rr,
		void **A_array, void **B_array, void **P_array, int num_levels,
		void ***mv_ws[7], double *dbl_ws, int *int_ws, struct OPS_ *ops)
{
	static PASSolver g;
	int i; double theta; int min_rows;
	memset(&g, 0, sizeof(g));
	/* defaults of the reference's set-up (src/ops_eig_sol_pas.c) */
	g.nevMax = 1; g.multiMax = 1; g.gapMin = 0.01; g.block_size = 1; g.tol[0] = g.tol[1] = 1e-6; g.numIterMax = 10;
	g.block_size_rr = 1; g.tol_rr[0] = g.tol_rr[1] = 1e-6; g.numIterMax_rr = 10;
	g.check_conv_max_num = 100;
	g.compN_bamg_max_iter[0] = 1;
	for (i = 1; i < 32; ++i) g.compN_bamg_max_iter[i] = i <= 12 ? 4 : i <= 16 ? 20 : i <= 24 ? 40 : i <= 30 ? 80 : 100;
	for (i = 0; i < 16; ++i) { g.compN_bamg_rate[i] = i < 12 ? 1e-2 : 1e-16; g.compN_bamg_tol[i] = i < 8 ? 1e-14 : 1e-26; }
	strcpy(g.compN_bamg_tol_type, "abs");
	/* the solve with B_H: to the round-off (B-orthogonality of X to range(P_H) is what makes B block diagonal) */
	g.orthX_ls_max_iter = 100; g.orthX_ls_rate = 1e-16; g.orthX_ls_tol = 1e-14; strcpy(g.orthX_ls_tol_type, "rel");
	strcpy(g.orthX_orth_method, "mgs"); g.orthX_orth_block_size = -1; g.orthX_orth_max_reorth = 4; g.orthX_orth_zero_tol = 1e-14;
	g.compRR_gcg_check_conv_max_num = 20;
	strcpy(g.compRR_gcg_initX_orth_method, "mgs"); g.compRR_gcg_initX_orth_block_size = -1; g.compRR_gcg_initX_orth_max_reorth = 4;
	g.compRR_gcg_initX_orth_zero_tol = 1e-14;
	strcpy(g.compRR_gcg_compP_orth_method, "mgs"); g.compRR_gcg_compP_orth_block_size = -1; g.compRR_gcg_compP_orth_max_reorth = 4;
	g.compRR_gcg_compP_orth_zero_tol = 1e-14;
	strcpy(g.compRR_gcg_compW_orth_method, "mgs"); g.compRR_gcg_compW_orth_block_size = -1; g.compRR_gcg_compW_orth_max_reorth = 4;
	g.compRR_gcg_compW_orth_zero_tol = 1e-14;
	g.compRR_gcg_compW_cg_max_iter = 30; g.compRR_gcg_compW_cg_rate = 1e-2; g.compRR_gcg_compW_cg_tol = 1e-14;
	strcpy(g.compRR_gcg_compW_cg_tol_type, "abs");
	g.compRR_gcg_compRR_min_num = -1; g.compRR_gcg_compRR_min_gap = 0.01; g.compRR_gcg_compRR_tol = 1e-14;
	if (nevMax > 0) g.nevMax = nevMax;
	if (multiMax >= 0) g.multiMax = multiMax;
	if (gapMin >= 0) g.gapMin = gapMin;
	if (block_size > 0) g.block_size = block_size;
	if (tol != NULL) { g.tol[0] = tol[0]; g.tol[1] = tol[1]; }
	if (numIterMax > 0) g.numIterMax = numIterMax;
	if (block_size_rr > 0) g.block_size_rr = block_size_rr;
	if (tol_rr != NULL) { g.tol_rr[0] = tol_rr[0]; g.tol_rr[1] = tol_rr[1]; }
	if (numIterMax_rr > 0) g.numIterMax_rr = numIterMax_rr;
	g.A = A_array; g.B = B_array; g.P = P_array; g.num_levels = num_levels; g.level_aux = num_levels - 1;
	for (i = 0; i < 7; ++i) g.mv_ws[i] = mv_ws[i];
	g.dbl_ws = dbl_ws; g.int_ws = int_ws;
	gcge_mg_get_defaults(&g.scale, &min_rows, &theta);
	ops->eigen_solver_workspace = (void*)&g;
	ops->EigenSolver = PAS;
}

void EigenSolverSetParameters_PAS(int check_conv_max_num,
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
		struct OPS_ *ops)
{
	PASSolver *p = (PASSolver*)ops->eigen_solver_workspace; int l, L = p->num_levels;
	/* as in the reference, the smoothers are BlockAMG and the B_H solve is ours: no user-defined solver */
	p->compN_user_defined_multi_linear_solver = 0; p->orthX_user_defined_multi_linear_solver = 0;
	if (check_conv_max_num > 0) p->check_conv_max_num = check_conv_max_num;
	if (compN_bamg_max_iter != NULL) {
		p->compN_bamg_max_iter[0] = compN_bamg_max_iter[0];
		for (l = 0; l < L - 1 && 2 * l + 2 < 32; ++l) {
			p->compN_bamg_max_iter[2 * l + 1] = compN_bamg_max_iter[2 * l + 1];
			p->compN_bamg_max_iter[2 * l + 2] = compN_bamg_max_iter[2 * l + 2];
		}
		if (2 * (L - 1) + 1 < 32) p->compN_bamg_max_iter[2 * (L - 1) + 1] = compN_bamg_max_iter[2 * (L - 1) + 1];
	}
	if (compN_bamg_rate != NULL) for (l = 0; l < L && l < 16; ++l) p->compN_bamg_rate[l] = compN_bamg_rate[l];
	if (compN_bamg_tol != NULL) for (l = 0; l < L && l < 16; ++l) p->compN_bamg_tol[l] = compN_bamg_tol[l];
	if (compN_bamg_tol_type != NULL) strncpy(p->compN_bamg_tol_type, compN_bamg_tol_type, 7);
	if (orthX_ls_max_iter > 0) p->orthX_ls_max_iter = orthX_ls_max_iter;
	if (orthX_ls_rate > 0) p->orthX_ls_rate = orthX_ls_rate;
	if (orthX_ls_tol > 0) p->orthX_ls_tol = orthX_ls_tol;
	if (orthX_ls_tol_type != NULL) strncpy(p->orthX_ls_tol_type, orthX_ls_tol_type, 7);
	if (orthX_orth_method != NULL) strncpy(p->orthX_orth_method, orthX_orth_method, 7);
	if (orthX_orth_block_size > 0) p->orthX_orth_block_size = orthX_orth_block_size;
	if (orthX_orth_max_reorth >= 0) p->orthX_orth_max_reorth = orthX_orth_max_reorth;
	if (orthX_orth_zero_tol > 0) p->orthX_orth_zero_tol = orthX_orth_zero_tol;
	if (compRR_gcg_check_conv_max_num > 0) p->compRR_gcg_check_conv_max_num = compRR_gcg_check_conv_max_num;
	if (compRR_gcg_initX_orth_method != NULL) strncpy(p->compRR_gcg_initX_orth_method, compRR_gcg_initX_orth_method, 7);
	p->compRR_gcg_initX_orth_block_size = compRR_gcg_initX_orth_block_size;
	if (compRR_gcg_initX_orth_max_reorth >= 0) p->compRR_gcg_initX_orth_max_reorth = compRR_gcg_initX_orth_max_reorth;
	if (compRR_gcg_initX_orth_zero_tol > 0) p->compRR_gcg_initX_orth_zero_tol = compRR_gcg_initX_orth_zero_tol;
	if (compRR_gcg_compP_orth_method != NULL) strncpy(p->compRR_gcg_compP_orth_method, compRR_gcg_compP_orth_method, 7);
	p->compRR_gcg_compP_orth_block_size = compRR_gcg_compP_orth_block_size;
	if (compRR_gcg_compP_orth_max_reorth >= 0) p->compRR_gcg_compP_orth_max_reorth = compRR_gcg_compP_orth_max_reorth;
	if (compRR_gcg_compP_orth_zero_tol > 0) p->compRR_gcg_compP_orth_zero_tol = compRR_gcg_compP_orth_zero_tol;
	if (compRR_gcg_compW_orth_method != NULL) strncpy(p->compRR_gcg_compW_orth_method, compRR_gcg_compW_orth_method, 7);
	p->compRR_gcg_compW_orth_block_size = compRR_gcg_compW_orth_block_size;
	if (compRR_gcg_compW_orth_max_reorth >= 0) p->compRR_gcg_compW_orth_max_reorth = compRR_gcg_compW_orth_max_reorth;
	if (compRR_gcg_compW_orth_zero_tol > 0) p->compRR_gcg_compW_orth_zero_tol = compRR_gcg_compW_orth_zero_tol;
	if (compRR_gcg_compW_cg_max_iter > 0) p->compRR_gcg_compW_cg_max_iter = compRR_gcg_compW_cg_max_iter;
	if (compRR_gcg_compW_cg_rate > 0) p->compRR_gcg_compW_cg_rate = compRR_gcg_compW_cg_rate;
	if (compRR_gcg_compW_cg_tol > 0) p->compRR_gcg_compW_cg_tol = compRR_gcg_compW_cg_tol;
	if (compRR_gcg_compW_cg_tol_type != NULL) strncpy(p->compRR_gcg_compW_cg_tol_type, compRR_gcg_compW_cg_tol_type, 7);
	p->compRR_gcg_compRR_min_num = compRR_gcg_compRR_min_num;
	if (compRR_gcg_compRR_min_gap >= 0) p->compRR_gcg_compRR_min_gap = compRR_gcg_compRR_min_gap;
	if (compRR_gcg_compRR_tol > 0) p->compRR_gcg_compRR_tol = compRR_gcg_compRR_tol;
}
