/* Operator-table life cycle and the solver-side default slots.
 *
 * Restates the behaviour of the reference's src/ops.c:26-149 (OPS_Create,
 * OPS_Setup, OPS_Destroy) and of the defaults in src/ops_multi_vec.c
 * (DefaultPrintf :26-44, DefaultGetWtime :45-56, DefaultGetOptionFromCommandLine
 * :58-95, DefaultMultiVecInnerProd :202-230, DefaultMultiVecQtAP :351-411).
 *
 * Differences by design:
 *  - GetWtime is a monotonic WALL clock (the reference falls back to clock(),
 *    i.e. CPU time, in serial builds — SURVEY.md §5.1);
 *  - the cross-rank reduction of Gram results goes through GCGE_COMM (one
 *    process per GPU, RCCL/gloo behind a callback) instead of MPI_Allreduce; a
 *    strided result (ldIP > rows) is packed contiguously before the reduction,
 *    which replaces the reference's MPI_Type_vector + user MPI_Op (src/ops.c:259-318).
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <assert.h>

#include "gcge_ops.h"

/* ---------------------------------------------------------------- comm hook */
static GCGE_COMM  g_comm_storage;
static GCGE_COMM *g_comm = NULL;

void GCGE_SetComm(const GCGE_COMM *comm)
{
	/* a communicator of one rank is dropped (nothing to sum) unless GCGE_COMM_KEEP_SINGLE is set: the single-GPU
	 * loop-back tests route every reduction through the real transport that way */
	if (comm == NULL || (comm->size <= 1 && getenv("GCGE_COMM_KEEP_SINGLE") == NULL)) { g_comm = NULL; return; }
	g_comm_storage = *comm; g_comm = &g_comm_storage;
}
GCGE_COMM *GCGE_GetComm(void) { return g_comm; }
/* Opt-in for solver stacks that sum their "local" inner products through MPI only (the reference's BlockPCG:
 * MultiVecLocalInnerProd + MPI_Allreduce under OPS_USE_MPI, src/ops_lin_sol.c:306-321,355-369): a back-end that honours the
 * switch (OPS_HIP_Set's MultiVecLocalInnerProd) then returns the sum over the ranks from its LOCAL slot as well, so a non-MPI
 * build of such a stack spans the ranks with flag 0.  Our own BlockPCG (lin_sol.c) asks before it reduces a second time. */
static int g_local_ip_reduces = 0;
void GCGE_SetLocalInnerProdReduces(int on) { g_local_ip_reduces = on != 0; }
int  GCGE_GetLocalInnerProdReduces(void) { return g_local_ip_reduces && g_comm != NULL; }

static GCGE_LINSOL_ARGS g_linsol_args;
void GCGE_SetLinearSolverArgs(const GCGE_LINSOL_ARGS *args)
{
	if (args != NULL) g_linsol_args = *args;
	else memset(&g_linsol_args, 0, sizeof(g_linsol_args));
}
const GCGE_LINSOL_ARGS *GCGE_GetLinearSolverArgs(void) { return &g_linsol_args; }

static void **g_realigned_b = NULL; static int g_realigned_b0 = 0;
void GCGE_SetRealignedRhs(void **b, int b0) { g_realigned_b = b; g_realigned_b0 = b0; }
void **GCGE_GetRealignedRhs(int *b0) { if (b0 != NULL) *b0 = g_realigned_b0; return g_realigned_b; }

/* The back-end record and the two slots that identify its table.  The lookup applies the opt-out switches, read at every
 * call (the tests flip them inside a running process); each turns off what it names:
 *   GCGE_NO_RESIDUAL_HOOK    residual_sq                                    (CheckConvergence through the slots)
 *   GCGE_NO_INPLACE_LINCOMB  inplace_lincomb_cols                           (panel updates staged through a work block)
 *   GCGE_EIG_HOST            symeig                                         (projected eigenproblems on the host)
 *   GCGE_AMG_HOST_SMOOTHER   amg_smoother_setup, amg_smoother_residual,     (BlockAMG smooths with BlockPCG over the slots)
 *                            amg_smoother_niter
 *   GCGE_AMG_NO_FUSIONS      amg_residual, amg_prolong_add, amg_form_rhs,   (the V-cycle's slot calls;
 *                            amg_final_cols                                  every smoothing call runs its last pass whole)
 *   GCGE_AMG_FULL_LAST_PASS  amg_final_cols                                 (the same, alone)
 *   GCGE_NO_RHS_SCALE        scaled_rhs_solver, amg_form_rhs                (the GCG driver forms b = (lambda + sigma) x)
 *   GCGE_NO_BLOCK_MOVES      block_moves                                    (X, the W start vectors and b moved one by one)
 *   GCGE_NO_RITZ_IN_PLACE    ritz_in_place                                  (Ritz vectors into the eigenvector block, then ComputeX)
 *   GCGE_NO_PANEL_NORMS      panel_norms_sq                                 (column norms by a sweep of their own)
 *   GCGE_NO_START_IN_PLACE   start_in_place                                 (the W start vectors and b moved before the solve)
 *   GCGE_NO_PCG_SWEEPS       pcg_step, pcg_dots, pcg_direction, pcg_shift   (GCGE_PCGSolve's sweeps through the slots)
 *   GCGE_NO_CHEB_STEP        cheb_step                                      (GCGE_ChebFilter's steps through the slots)
 *   GCGE_NO_CHEB_ACCUM       cheb_accum                                     (GCGE_ChebBandFilter's sums by two MultiVecAxpby)
 *   GCGE_NO_CHEB_STEP_DOTS   cheb_step_dots                                 (GCGE_ChebMoments' steps by cheb_step and two inner products) */
static GCGE_BACKEND g_backend; static void *g_backend_matvec = NULL, *g_backend_lincomb = NULL;
void GCGE_SetBackend(struct OPS_ *ops, const GCGE_BACKEND *backend)
{
	g_backend = *backend;
	g_backend_matvec = (void*)ops->MatDotMultiVec; g_backend_lincomb = (void*)ops->MultiVecLinearComb;
}
GCGE_BACKEND GCGE_BackendOf(struct OPS_ *ops)
{
	GCGE_BACKEND b;
	memset(&b, 0, sizeof(b));
	if (ops == NULL || g_backend_matvec == NULL || (void*)ops->MatDotMultiVec != g_backend_matvec ||
			(void*)ops->MultiVecLinearComb != g_backend_lincomb) return b;
	b = g_backend;
	if (getenv("GCGE_NO_RESIDUAL_HOOK") != NULL) b.residual_sq = NULL;
	if (getenv("GCGE_NO_INPLACE_LINCOMB") != NULL) b.inplace_lincomb_cols = 0;
	if (getenv("GCGE_EIG_HOST") != NULL) b.symeig = NULL;
	if (getenv("GCGE_AMG_HOST_SMOOTHER") != NULL) { b.amg_smoother_setup = NULL; b.amg_smoother_residual = NULL; b.amg_smoother_niter = NULL; b.amg_final_cols = 0; }
	if (getenv("GCGE_AMG_NO_FUSIONS") != NULL) { b.amg_residual = NULL; b.amg_prolong_add = NULL; b.amg_form_rhs = NULL; b.amg_final_cols = 0; }
	if (getenv("GCGE_AMG_FULL_LAST_PASS") != NULL) b.amg_final_cols = 0;
	if (getenv("GCGE_NO_RHS_SCALE") != NULL) { b.scaled_rhs_solver = NULL; b.amg_form_rhs = NULL; }
	if (getenv("GCGE_NO_BLOCK_MOVES") != NULL) b.block_moves = NULL;
	if (getenv("GCGE_NO_RITZ_IN_PLACE") != NULL) b.ritz_in_place = NULL;
	if (getenv("GCGE_NO_PANEL_NORMS") != NULL) b.panel_norms_sq = NULL;
	if (getenv("GCGE_NO_START_IN_PLACE") != NULL) b.start_in_place = 0;
	if (getenv("GCGE_NO_PCG_SWEEPS") != NULL) { b.pcg_step = NULL; b.pcg_dots = NULL; b.pcg_direction = NULL; b.pcg_shift = NULL; }
	if (getenv("GCGE_NO_CHEB_STEP") != NULL) b.cheb_step = NULL;
	if (getenv("GCGE_NO_CHEB_ACCUM") != NULL) b.cheb_accum = NULL;
	if (getenv("GCGE_NO_CHEB_STEP_DOTS") != NULL) b.cheb_step_dots = NULL;
	return b;
}

/* ---------------------------------------------------------------- services */
void DefaultPrintf(const char *fmt, ...)
{
	va_list ap;
	if (g_comm != NULL && g_comm->rank != 0) return;   /* rank 0 prints */
	va_start(ap, fmt);
	vprintf(fmt, ap);
	va_end(ap);
}

double DefaultGetWtime(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* scan argv for `name`; the token after it is parsed as int ('i'), double ('f')
 * or copied as a string ('s').  Returns 1 when a value was read. */
int DefaultGetOptionFromCommandLine(const char *name, char type, void *value,
		int argc, char *argv[], struct OPS_ *ops)
{
	int k;
	for (k = 0; k < argc; ++k) {
		if (argv[k] == NULL || strcmp(argv[k], name) != 0) continue;
		if (ops != NULL && ops->Printf != NULL)
			ops->Printf("argv[%d] = \"%s\", name = \"%s\"\n", k, argv[k], name);
		if (k + 1 >= argc) return 0;
		switch (type) {
			case 'i': *(int*)value    = atoi(argv[k + 1]); break;
			case 'f': *(double*)value = atof(argv[k + 1]); break;
			case 's': strcpy((char*)value, argv[k + 1]);   break;
			default : break;
		}
		return 1;
	}
	return 0;
}

/* ---------------------------------------------------------------- defaults */
void DefaultMultiVecInnerProd(char nsdIP, void **x, void **y, int is_vec,
		int *start, int *end, double *inner_prod, int ldIP, struct OPS_ *ops)
{
	int nrows = end[0] - start[0], ncols = end[1] - start[1];
	ops->MultiVecLocalInnerProd(nsdIP, x, y, is_vec, start, end, inner_prod, ldIP, ops);
	if (g_comm == NULL || nrows <= 0 || ncols <= 0) return;
	if (nsdIP == 'D') nrows = 1;          /* one value per column, stride ldIP */
	if (nrows == ldIP) {
		g_comm->allreduce_sum(inner_prod, nrows * ncols, g_comm->ctx);
	} else {
		double *pack = (double*)malloc((size_t)nrows * ncols * sizeof(double));
		int c;
		for (c = 0; c < ncols; ++c)
			memcpy(pack + (size_t)c * nrows, inner_prod + (size_t)c * ldIP, nrows * sizeof(double));
		g_comm->allreduce_sum(pack, nrows * ncols, g_comm->ctx);
		for (c = 0; c < ncols; ++c)
			memcpy(inner_prod + (size_t)c * ldIP, pack + (size_t)c * nrows, nrows * sizeof(double));
		free(pack);
	}
}

/* qAp = Q[:,s0:e0)^T A P[:,s1:e1).  A != NULL: mv_ws[:,0:m) = A P is a visible side
 * effect the orthogonalisation re-uses; 'T' stores the transpose (m x k). */
void DefaultMultiVecQtAP(char ntsA, char ntsdQAP, void **mvQ, void *matA, void **mvP,
		int is_vec, int *startQP, int *endQP, double *qAp, int ldQAP,
		void **mv_ws, struct OPS_ *ops)
{
	int s[2], e[2];
	int k = endQP[0] - startQP[0], m = endQP[1] - startQP[1];
	if (k <= 0 || m <= 0) return;
	if (matA == NULL) {
		if (ntsdQAP == 'T') {
			s[0] = startQP[1]; e[0] = endQP[1]; s[1] = startQP[0]; e[1] = endQP[0];
			ops->MultiVecInnerProd('N', mvP, mvQ, is_vec, s, e, qAp, ldQAP, ops);
		} else {
			ops->MultiVecInnerProd(ntsdQAP, mvQ, mvP, is_vec, startQP, endQP, qAp, ldQAP, ops);
		}
		return;
	}
	s[0] = startQP[1]; e[0] = endQP[1]; s[1] = 0; e[1] = m;
	if (ntsA == 'T') ops->MatTransDotMultiVec(matA, mvP, mv_ws, s, e, ops);
	else             ops->MatDotMultiVec     (matA, mvP, mv_ws, s, e, ops);
	if (ntsdQAP == 'T') {
		s[0] = 0; e[0] = m; s[1] = startQP[0]; e[1] = endQP[0];
		ops->MultiVecInnerProd('N', mv_ws, mvQ, is_vec, s, e, qAp, ldQAP, ops);
	} else {
		s[0] = startQP[0]; e[0] = endQP[0]; s[1] = 0; e[1] = m;
		ops->MultiVecInnerProd(ntsdQAP, mvQ, mv_ws, is_vec, s, e, qAp, ldQAP, ops);
	}
}

/* ---------------------------------------------------------------- multigrid transfers
 * src/ops_multi_grid.c:20-117.  P_array[k] maps level k + 1 to level k.  From a coarse level i to a finer level j the vector is
 * multiplied by P_{i-1}, ..., P_j in turn (MatDot*), from a fine level i to a coarser level j by P_i^T, ..., P_{j-1}^T
 * (MatTransDot*); the levels in between are staged in the caller's per-level work vectors; i == j copies. */
void DefaultVecFromItoJ(void **P_array, int level_i, int level_j, void *vec_i, void *vec_j, void **vec_ws, struct OPS_ *ops)
{
	void *from, *to; int k;
	if (level_i > level_j) {
		for (k = level_i; k > level_j; --k) {
			from = (k == level_i) ? vec_i : vec_ws[k];
			to = (k == level_j + 1) ? vec_j : vec_ws[k - 1];
			ops->MatDotVec(P_array[k - 1], from, to, ops);
		}
	} else if (level_i < level_j) {
		for (k = level_i; k < level_j; ++k) {
			from = (k == level_i) ? vec_i : vec_ws[k];
			to = (k == level_j - 1) ? vec_j : vec_ws[k + 1];
			ops->MatTransDotVec(P_array[k], from, to, ops);
		}
	} else {
		ops->VecAxpby(1.0, vec_i, 0.0, vec_j, ops);
	}
}
void DefaultMultiVecFromItoJ(void **P_array, int level_i, int level_j, void **multi_vec_i, void **multi_vec_j,
		int *startIJ, int *endIJ, void ***multi_vec_ws, struct OPS_ *ops)
{
	void **from, **to; int k, start[2], end[2];
	const int m = endIJ[0] - startIJ[0];
	if (level_i > level_j) {
		for (k = level_i; k > level_j; --k) {
			if (k == level_i) { from = multi_vec_i; start[0] = startIJ[0]; end[0] = endIJ[0]; }
			else              { from = multi_vec_ws[k]; start[0] = 0; end[0] = m; }
			if (k == level_j + 1) { to = multi_vec_j; start[1] = startIJ[1]; end[1] = endIJ[1]; }
			else                  { to = multi_vec_ws[k - 1]; start[1] = 0; end[1] = m; }
			ops->MatDotMultiVec(P_array[k - 1], from, to, start, end, ops);
		}
	} else if (level_i < level_j) {
		for (k = level_i; k < level_j; ++k) {
			if (k == level_i) { from = multi_vec_i; start[0] = startIJ[0]; end[0] = endIJ[0]; }
			else              { from = multi_vec_ws[k]; start[0] = 0; end[0] = m; }
			if (k == level_j - 1) { to = multi_vec_j; start[1] = startIJ[1]; end[1] = endIJ[1]; }
			else                  { to = multi_vec_ws[k + 1]; start[1] = 0; end[1] = m; }
			ops->MatTransDotMultiVec(P_array[k], from, to, start, end, ops);
		}
	} else {
		ops->MultiVecAxpby(1.0, multi_vec_i, 0.0, multi_vec_j, startIJ, endIJ, ops);
	}
}

/* ---------------------------------------------------------------- life cycle */
void OPS_Create(OPS **ops)
{
	*ops = (OPS*)calloc(1, sizeof(OPS));   /* every slot and workspace NULL */
}

void OPS_Setup(OPS *ops)
{
	if (ops->Printf == NULL)                   ops->Printf = DefaultPrintf;
	if (ops->GetWtime == NULL)                 ops->GetWtime = DefaultGetWtime;
	if (ops->GetOptionFromCommandLine == NULL) ops->GetOptionFromCommandLine = DefaultGetOptionFromCommandLine;
	if (ops->lapack_ops == NULL) {
		OPS_Create(&ops->lapack_ops);
		OPS_DENSE_Set(ops->lapack_ops);
	}
	if (ops->DenseMatQtAP == NULL)      ops->DenseMatQtAP = ops->lapack_ops->DenseMatQtAP;
	if (ops->DenseMatOrth == NULL)      ops->DenseMatOrth = ops->lapack_ops->DenseMatOrth;
	if (ops->MultiVecInnerProd == NULL) ops->MultiVecInnerProd = DefaultMultiVecInnerProd;
	if (ops->MultiVecQtAP == NULL)      ops->MultiVecQtAP = DefaultMultiVecQtAP;
	if (ops->VecFromItoJ == NULL)       ops->VecFromItoJ = DefaultVecFromItoJ;               /* src/ops.c:107-112 */
	if (ops->MultiVecFromItoJ == NULL)  ops->MultiVecFromItoJ = DefaultMultiVecFromItoJ;
}

void OPS_Destroy(OPS **ops)
{
	if (ops == NULL || *ops == NULL) return;
	if ((*ops)->lapack_ops != NULL) OPS_Destroy(&(*ops)->lapack_ops);
	free(*ops); *ops = NULL;
}

/* convenience for drivers that want the numbers, not the log */
static void QuietPrintf(const char *fmt, ...) { (void)fmt; }
void GCGE_SetQuiet(OPS *ops, int quiet)
{
	ops->Printf = quiet ? QuietPrintf : DefaultPrintf;
	if (ops->lapack_ops != NULL) ops->lapack_ops->Printf = ops->Printf;
}
