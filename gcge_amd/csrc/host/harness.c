/* Eigensolver harness: allocates the workspace, sets the parameters, seeds the
 * generator, runs ops->EigenSolver and reports.  Same parameter flow and
 * defaults as the reference's test/test_eig_sol_gcg.c:28-169 so that runs are
 * comparable flag for flag (-nevConv -nevMax -blockSize -nevInit + -gcge_*).
 */
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gcge_solver.h"
#include "gcge_pas.h"
#include "gcge_multigrid.h"

/* ---- BlockAMG as the solver of the W systems: what the reference's SiO2 driver does under OPS_USE_AMG
 * (test/test_eig_sol_SiO2_MAT.c:96-128,160-170): hierarchy from ops->MultiGridCreate, per-level work blocks, parameter arrays
 * {cycles, pre_0, post_0, pre_1, post_1, ...}, MultiLinearSolverSetup_BlockAMG, then GCG with a user-defined linear solver. */
GCGE_AMG *GCGE_AMGCreate(void *A, void *B, int max_levels, int block_size, int cycles, int smooth0, int smooth, double rate0,
		struct OPS_ *ops)
{
	GCGE_AMG *amg; int l, i, L = max_levels;
	if (ops->MultiGridCreate == NULL || max_levels < 2 || block_size < 1) return NULL;
	amg = (GCGE_AMG*)calloc(1, sizeof(GCGE_AMG));
	ops->MultiGridCreate(&amg->A_array, &amg->B_array, &amg->P_array, &L, A, B, ops);
	amg->num_levels = L; amg->block_size = block_size;
	amg->max_iter = (int*)calloc(2 * (size_t)L + 1, sizeof(int));
	amg->rate = (double*)calloc(L, sizeof(double)); amg->tol = (double*)calloc(L, sizeof(double));
	amg->max_iter[0] = cycles > 0 ? cycles : 1;
	for (l = 0; l < L; ++l) {
		amg->max_iter[2 * l + 1] = amg->max_iter[2 * l + 2] = l == 0 ? (smooth0 > 0 ? smooth0 : 5) : (smooth > 0 ? smooth : 4);
		amg->rate[l] = l == 0 ? (rate0 > 0.0 ? rate0 : 1e-2) : 1e-16;      /* test_eig_sol_SiO2_MAT.c:104-105 */
		amg->tol[l] = l == 0 ? 1e-14 : 1e-16;                                /* (level 0: the harness's compW_cg_tol, test_eig_sol_gcg.c:112; the SiO2 file has 1e-8) */
	}
	if (2 * (L - 1) + 2 > 2 * L) abort();
	amg->dbl_ws = (double*)calloc(6 * (size_t)block_size, sizeof(double));
	amg->int_ws = (int*)calloc(2 * (size_t)block_size, sizeof(int));
	/* blocks: right-hand side and solution of every coarse level, the residual block of every level; the CG's p and w blocks
	 * only where the smoother is the solver stack's own BlockPCG (a back-end's smoother brings its blocks) */
	amg->own_smoother = GCGE_BackendOf(ops).amg_smoother_setup != NULL;
	for (i = 0; i < 5; ++i) amg->mv_ws[i] = (void***)calloc(L, sizeof(void**));
	for (l = 0; l < L; ++l) {
		for (i = 0; i < 5; ++i) {
			if (i < 2 && l == 0) continue;
			if (i > 2 && amg->own_smoother) { amg->mv_ws[i][l] = amg->mv_ws[2][l]; continue; }
			ops->MultiVecCreateByMat(&amg->mv_ws[i][l], block_size, amg->A_array[l], ops);
		}
	}
	return amg;
}
void GCGE_AMGInstall(GCGE_AMG *amg, struct OPS_ *ops)
{
	MultiLinearSolverSetup_BlockAMG(amg->max_iter, amg->rate, amg->tol, "abs", amg->A_array, amg->P_array, amg->num_levels,
			amg->mv_ws, amg->dbl_ws, amg->int_ws, NULL, ops);
}
void GCGE_AMGDestroy(GCGE_AMG **pamg, struct OPS_ *ops)
{
	GCGE_AMG *amg = *pamg; int l, i;
	if (amg == NULL) return;
	for (l = 0; l < amg->num_levels; ++l)
		for (i = 0; i < 5; ++i) {
			if (amg->mv_ws[i][l] == NULL || (i > 2 && amg->own_smoother)) continue;
			ops->MultiVecDestroy(&amg->mv_ws[i][l], amg->block_size, ops);
		}
	for (i = 0; i < 5; ++i) free(amg->mv_ws[i]);
	l = amg->num_levels;
	ops->MultiGridDestroy(&amg->A_array, &amg->B_array, &amg->P_array, &l, ops);
	free(amg->max_iter); free(amg->rate); free(amg->tol); free(amg->dbl_ws); free(amg->int_ws);
	free(amg); *pamg = NULL;
}

int GCGE_AMGRefresh(GCGE_AMG *amg, struct OPS_ *ops)
{
	const GCGE_BACKEND be = GCGE_BackendOf(ops);
	GCGE_COMM *comm = GCGE_GetComm();
	enum { MAXL = 64 };
	double votes[MAXL + 1];
	int rc, l;
	if (be.multigrid_refresh == NULL) return -1;       /* (the table's, so the same answer on every rank) */
	/* The back-end's refresh is rank-local.  Over a communicator the ranks agree on its outcome by two all-reduces that EVERY rank
	 * reaches, whatever it found itself: the first on what can be decided from the handles, before anything is written — a -1
	 * anywhere is a -1 everywhere with every hierarchy untouched —, the second after the level loop, on the smallest level that
	 * declined on any rank.  No collective sits behind a predicate only one rank evaluates. */
	rc = amg == NULL || amg->num_levels > MAXL ? -1
	     : be.multigrid_refresh_check != NULL ? be.multigrid_refresh_check(amg->A_array, amg->B_array, amg->P_array, amg->num_levels) : 0;
	if (comm != NULL) {
		votes[0] = rc != 0 ? 1.0 : 0.0;
		comm->allreduce_sum(votes, 1, comm->ctx);
		if (votes[0] != 0.0) rc = -1;
	}
	if (rc == 0) rc = be.multigrid_refresh(amg->A_array, amg->B_array, amg->P_array, amg->num_levels);
	else rc = -1;
	if (comm == NULL) return rc;
	/* votes[0]: ranks that wrote nothing; votes[l]: ranks whose level l was the first to decline */
	for (l = 0; l <= MAXL; ++l) votes[l] = 0.0;
	if (rc < 0 || rc > MAXL) votes[0] = 1.0; else if (rc > 0) votes[rc] = 1.0;
	comm->allreduce_sum(votes, MAXL + 1, comm->ctx);
	if (votes[0] != 0.0) return -1;
	for (l = 1; l <= MAXL; ++l) if (votes[l] != 0.0) return l;
	return 0;
}

/* evec_in != NULL: a block of nevMax columns owned by the caller whose first nevGiven columns are start vectors
 * (the `nevGiven` argument of ops->EigenSolver, reference src/ops_eig_sol_gcg.c:101-158) */
static int run_gcg(void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops,
		double *eval_out, void ***evec_out, GCGE_RunResult *res, void **evec_in, int nevGiven)
{
	int nevConv = 30, multiMax = 1, block_size, nevMax, nevInit, i;
	double gapMin = 1e-5, tol_gcg[2] = {1e-1, 1e-8}, *eval, *dbl_ws, t0;
	int max_iter_gcg = 500, *int_ws, sizeV, length_dbl_ws, length_int_ws;
	int amg_levels = 0, amg_cycles = 1, amg_smooth0 = 5, amg_smooth = 4; double amg_rate = 1e-2;
	GCGE_AMG *amg = NULL;
	void **evec, **ws[4];

	ops->GetOptionFromCommandLine("-nevConv", 'i', &nevConv, argc, argv, ops);
	nevMax = 2 * nevConv;
	ops->GetOptionFromCommandLine("-nevMax", 'i', &nevMax, argc, argv, ops);
	block_size = nevConv < 30 ? (nevMax - nevConv) : nevConv / 5;
	ops->GetOptionFromCommandLine("-blockSize", 'i', &block_size, argc, argv, ops);
	nevInit = nevMax;
	ops->GetOptionFromCommandLine("-nevInit", 'i', &nevInit, argc, argv, ops);
	if (nevInit > nevMax) nevInit = nevMax;

	/* -gcge_amg_levels L (>= 2): the W systems are solved by BlockAMG over the back-end's hierarchy instead of BlockPCG —
	 * OPS_USE_AMG of test/test_eig_sol_SiO2_MAT.c:27,96-128,160-170; a hierarchy the caller installed beforehand
	 * (GCGE_AMGCreate + GCGE_AMGInstall, flag 1) is used as it is */
	ops->GetOptionFromCommandLine("-gcge_amg_levels", 'i', &amg_levels, argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_amg_cycles", 'i', &amg_cycles, argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_amg_smooth0", 'i', &amg_smooth0, argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_amg_smooth", 'i', &amg_smooth, argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_amg_rate", 'f', &amg_rate, argc, argv, ops);
	if (amg_levels >= 2) {
		/* -gcge_amg_graph <0|1>: how a matrix without a grid is aggregated (gcge_mg_set_graph_method), for this hierarchy only */
		const int graph_before = gcge_mg_get_graph_method(); int amg_graph = graph_before;
		ops->GetOptionFromCommandLine("-gcge_amg_graph", 'i', &amg_graph, argc, argv, ops);
		gcge_mg_set_graph_method(amg_graph);
		amg = GCGE_AMGCreate(A, B, amg_levels, block_size, amg_cycles, amg_smooth0, amg_smooth, amg_rate, ops);
		gcge_mg_set_graph_method(graph_before);
		if (amg == NULL) { ops->Printf("-gcge_amg_levels: the back-end has no MultiGridCreate\n"); return -7; }
		GCGE_AMGInstall(amg, ops);
		flag = 1;
	}

	eval = (double*)calloc(nevMax, sizeof(double));
	if (evec_in != NULL) evec = evec_in;
	else {
		ops->MultiVecCreateByMat(&evec, nevMax, A, ops);
		ops->MultiVecSetRandomValue(evec, 0, nevMax, ops);
	}
	ops->MultiVecCreateByMat(&ws[0], nevMax + 2 * block_size, A, ops);
	ops->MultiVecSetRandomValue(ws[0], 0, nevMax + 2 * block_size, ops);
	for (i = 1; i < 4; ++i) {
		ops->MultiVecCreateByMat(&ws[i], block_size, A, ops);
		ops->MultiVecSetRandomValue(ws[i], 0, block_size, ops);
	}
	sizeV = nevInit + 2 * block_size;
	length_dbl_ws = 2 * sizeV * sizeV + 10 * sizeV + (nevMax + 2 * block_size) + nevMax * block_size;
	length_int_ws = 6 * sizeV + 2 * (block_size + 3);
	ops->Printf("length_dbl_ws = %d\n", length_dbl_ws);
	ops->Printf("length_int_ws = %d\n", length_int_ws);
	dbl_ws = (double*)calloc(length_dbl_ws, sizeof(double));
	int_ws = (int*)calloc(length_int_ws, sizeof(int));

	srand(0);   /* the initial block is the glibc rand() stream after srand(0) */
	t0 = ops->GetWtime();
	ops->Printf("===============================================\n");
	ops->Printf("GCG Eigen Solver\n");
	EigenSolverSetup_GCG(multiMax, gapMin, nevInit, nevMax, block_size, tol_gcg, max_iter_gcg,
			flag, ws, dbl_ws, int_ws, ops);
	EigenSolverSetParameters_GCG(50,
			"mgs", 80, 2, 2 * DBL_EPSILON,      /* initial X   */
			"mgs", -1, 2, 2 * DBL_EPSILON,      /* P (host)    */
			"mgs", 80, 2, 2 * DBL_EPSILON,      /* W           */
			30, 1e-2, 1e-14, "abs", 0,          /* block CG    */
			-1, gapMin, 2 * DBL_EPSILON, ops);
	EigenSolverSetParametersFromCommandLine_GCG(argc, argv, ops);
	ops->Printf("nevGiven = %d, nevConv = %d, nevMax = %d, block_size = %d, nevInit = %d\n",
			nevGiven, nevConv, nevMax, block_size, nevInit);
	ops->EigenSolver(A, B, eval, evec, nevGiven, &nevConv, ops);
	if (res != NULL) {
		res->seconds = ops->GetWtime() - t0;
		res->nevConv = nevConv; res->numIter = ((GCGSolver*)ops->eigen_solver_workspace)->numIter;
		res->nevMax = nevMax; res->block_size = block_size; res->nevInit = nevInit;
		res->timing = *GCGE_LastTiming();
	}
	ops->Printf("numIter = %d, nevConv = %d\n", ((GCGSolver*)ops->eigen_solver_workspace)->numIter, nevConv);
	ops->Printf("++++++++++++++++++++++++++++++++++++++++++++++\n");
	ops->Printf("Time is %.3f\n", ops->GetWtime() - t0);

	ops->MultiVecDestroy(&ws[0], nevMax + 2 * block_size, ops);
	for (i = 1; i < 4; ++i) ops->MultiVecDestroy(&ws[i], block_size, ops);
	if (amg != NULL) GCGE_AMGDestroy(&amg, ops);
	free(dbl_ws); free(int_ws);
	if (eval_out != NULL) memcpy(eval_out, eval, nevMax * sizeof(double));
	ops->Printf("eigenvalues\n");
	for (i = 0; i < nevConv; ++i) ops->Printf("%d: %6.14e\n", i + 1, eval[i]);
	if (evec_out != NULL) *evec_out = evec;
	else if (evec_in == NULL) ops->MultiVecDestroy(&evec, nevMax, ops);
	free(eval);
	return 0;
}

int GCGE_RunGCG(void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops,
		double *eval_out, void ***evec_out, GCGE_RunResult *res)
{
	return run_gcg(A, B, flag, argc, argv, ops, eval_out, evec_out, res, NULL, 0);
}

int GCGE_RunGCGGiven(void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops,
		double *eval_out, void **evec, int nevGiven, GCGE_RunResult *res)
{
	if (evec == NULL || nevGiven < 0) return -1;
	return run_gcg(A, B, flag, argc, argv, ops, eval_out, NULL, res, evec, nevGiven);
}

int GCGE_ResidualNorms(void *A, void *B, void **evec, int start, int end, const double *eval, double *out, struct OPS_ *ops)
{
	int m = end - start, s[2], e[2], idx; void **w0, **w1;
	GCGE_RESIDUAL_FN hook;
	if (A == NULL || evec == NULL || ops == NULL || start < 0 || m < 0 || (m > 0 && (eval == NULL || out == NULL))) return -1;
	if (m == 0) return 0;
	hook = GCGE_BackendOf(ops).residual_sq;
	if (hook != NULL && hook(A, B, evec, start, end, eval, out)) {
		GCGE_COMM *comm = GCGE_GetComm();          /* the back-end summed over its own rows */
		if (comm != NULL) comm->allreduce_sum(out, m, comm->ctx);
		for (idx = 0; idx < m; ++idx) out[idx] = sqrt(out[idx]);
		return 0;
	}
	/* the slot sequence of CheckConvergence (gcg.c) */
	ops->MultiVecCreateByMat(&w0, m, A, ops);
	ops->MultiVecCreateByMat(&w1, m, A, ops);
	s[0] = start; e[0] = end; s[1] = 0; e[1] = m;
	ops->MatDotMultiVec(A, evec, w0, s, e, ops);
	ops->MatDotMultiVec(B, evec, w1, s, e, ops);
	ops->MultiVecLinearComb(NULL, w1, 0, s, e, NULL, 0, (double*)eval, 1, ops);   /* lambda B x */
	s[0] = 0; e[0] = m;
	ops->MultiVecAxpby(-1.0, w1, 1.0, w0, s, e, ops);                             /* A x - lambda B x */
	ops->MultiVecInnerProd('D', w0, w0, 0, s, e, out, 1, ops);
	for (idx = 0; idx < m; ++idx) out[idx] = sqrt(out[idx]);
	ops->MultiVecDestroy(&w0, m, ops);
	ops->MultiVecDestroy(&w1, m, ops);
	return 0;
}

int TestEigenSolverGCG(void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops)
{
	return GCGE_RunGCG(A, B, flag, argc, argv, ops, NULL, NULL, NULL);
}

/* ---- PAS, then GCG warm-started from its converged vectors: the flow of the reference's test/test_eig_sol_pas.c ------
 * The hierarchy comes from ops->MultiGridCreate (levels 0 .. L-1, level_aux = L-1).  For a standard problem it is built from
 * the back-end's identity (GCGE_PAS_MatIdentityOf): its Galerkin levels are the coarse masses P^T P that PAS needs; level 0
 * stays B == NULL. */
int GCGE_RunPAS(void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops,
		double *eval_out, void ***evec_out, GCGE_PAS_RESULT *res)
{
	int nevConv = 30, multiMax = 1, block_size, nevMax, nevInit, L, l, i, rc = 0, pas_conv;
	double gapMin = 1e-5, tol_pas[2] = {1e-1, 1e-8}, tol_rr[2] = {1e-1, 1e-8}, t0;
	int pas_levels = 3, pas_max_iter = 50, pas_rr_max_iter = 100, pas_only = 0, sizeV, graph_before, amg_graph;
	void **A_array = NULL, **B_array = NULL, **P_array = NULL, ***mv_ws[7], **evec, *I0 = NULL;
	GCGE_MAT_FREE_FN mat_free = NULL;
	double *eval, *dbl_ws; int *int_ws; long ldbl, lint;
	PASSolver *pas;

	if (res != NULL) memset(res, 0, sizeof(*res));
	ops->GetOptionFromCommandLine("-nevConv", 'i', &nevConv, argc, argv, ops);
	nevMax = 2 * nevConv;
	ops->GetOptionFromCommandLine("-nevMax", 'i', &nevMax, argc, argv, ops);
	block_size = nevConv < 30 ? (nevMax - nevConv) : nevConv / 5;
	ops->GetOptionFromCommandLine("-blockSize", 'i', &block_size, argc, argv, ops);
	nevInit = nevMax;
	ops->GetOptionFromCommandLine("-nevInit", 'i', &nevInit, argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_pas_levels", 'i', &pas_levels, argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_pas_max_iter", 'i', &pas_max_iter, argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_pas_abs_tol", 'f', &tol_pas[0], argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_pas_rel_tol", 'f', &tol_pas[1], argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_pas_rr_max_iter", 'i', &pas_rr_max_iter, argc, argv, ops);
	ops->GetOptionFromCommandLine("-gcge_pas_only", 'i', &pas_only, argc, argv, ops);
	if (ops->MultiGridCreate == NULL || pas_levels < 2) {
		ops->Printf("-gcge_pas_levels: PAS needs the back-end's MultiGridCreate and at least 2 levels\n");
		return -7;
	}
	if (B == NULL) {
		GCGE_MAT_IDENTITY_FN identity = GCGE_PAS_MatIdentityOf(ops, &mat_free);
		if (identity == NULL || (I0 = identity(A)) == NULL) {
			ops->Printf("PAS: a standard problem needs the back-end's identity upload (GCGE_BACKEND.mat_identity)\n");
			return -9;
		}
	}
	L = pas_levels;
	graph_before = amg_graph = gcge_mg_get_graph_method();       /* -gcge_amg_graph: as in GCGE_RunGCG */
	ops->GetOptionFromCommandLine("-gcge_amg_graph", 'i', &amg_graph, argc, argv, ops);
	gcge_mg_set_graph_method(amg_graph);
	ops->MultiGridCreate(&A_array, &B_array, &P_array, &L, A, B != NULL ? B : I0, ops);
	gcge_mg_set_graph_method(graph_before);
	if (L < 2) {
		ops->Printf("PAS: the hierarchy has %d level(s); PAS needs 2 or more\n", L);
		ops->MultiGridDestroy(&A_array, &B_array, &P_array, &L, ops);
		if (I0 != NULL && mat_free != NULL) mat_free(I0);
		return -7;
	}
	if (B == NULL) B_array[0] = NULL;   /* level 0 of a standard problem: the identity is not applied */

	sizeV = nevMax + 2 * block_size;
	for (i = 0; i < 7; ++i) {
		mv_ws[i] = (void***)calloc(L, sizeof(void**));
		for (l = 0; l < L; ++l) {
			int cols = i < 6 ? nevMax : sizeV;
			ops->MultiVecCreateByMat(&mv_ws[i][l], cols, A_array[l], ops);
			ops->MultiVecSetRandomValue(mv_ws[i][l], 0, cols, ops);
		}
	}
	GCGE_PASWorkspaceSizes(nevMax, block_size, &ldbl, &lint);
	dbl_ws = (double*)calloc(ldbl, sizeof(double)); int_ws = (int*)calloc(lint, sizeof(int));
	if (nevMax < 1) nevMax = 1;
	eval = (double*)calloc((size_t)nevMax, sizeof(double));
	ops->MultiVecCreateByMat(&evec, nevMax, A, ops);

	srand(0);
	t0 = ops->GetWtime();
	ops->Printf("===============================================\n");
	ops->Printf("PAS Eigen Solver\n");
	EigenSolverSetup_PAS(multiMax, gapMin, nevMax, block_size, tol_pas, pas_max_iter, block_size, tol_rr, pas_rr_max_iter,
			A_array, B_array, P_array, L, mv_ws, dbl_ws, int_ws, ops);
	pas = (PASSolver*)ops->eigen_solver_workspace;
	pas_conv = nevConv;
	ops->EigenSolver(A, B, eval, evec, 0, &pas_conv, ops);
	if (pas->status != 0) rc = pas->status;
	if (res != NULL) {
		res->nevConv = pas_conv; res->numIter = pas->numIter; res->num_levels = L;
		res->seconds = ops->GetWtime() - t0;
	}
	ops->Printf("PAS: numIter = %d, nevConv = %d, time %.3f\n", pas->numIter, pas_conv, ops->GetWtime() - t0);

	for (i = 0; i < 7; ++i) {
		for (l = 0; l < L; ++l) ops->MultiVecDestroy(&mv_ws[i][l], i < 6 ? nevMax : sizeV, ops);
		free(mv_ws[i]);
	}
	if (B == NULL) B_array[0] = I0;
	ops->MultiGridDestroy(&A_array, &B_array, &P_array, &L, ops);
	if (I0 != NULL && mat_free != NULL) mat_free(I0);
	free(dbl_ws); free(int_ws);

	if (rc == 0 && !pas_only) {
		int given = pas_conv < nevInit ? pas_conv : nevInit;
		rc = GCGE_RunGCGGiven(A, B, flag, argc, argv, ops, eval, evec, given, res != NULL ? &res->gcg : NULL);
	}
	if (eval_out != NULL) memcpy(eval_out, eval, nevMax * sizeof(double));
	if (evec_out != NULL) *evec_out = evec;
	else ops->MultiVecDestroy(&evec, nevMax, ops);
	free(eval);
	return rc;
}

int TestEigenSolverPAS(void *A, void *B, int flag, int argc, char *argv[], struct OPS_ *ops)
{
	GCGE_PAS_RESULT r; int rc = GCGE_RunPAS(A, B, flag, argc, argv, ops, NULL, NULL, &r);
	ops->Printf("PAS: nevConv = %d, numIter = %d, levels = %d, %.3f s; GCG: nevConv = %d, numIter = %d, %.3f s (rc %d)\n",
			r.nevConv, r.numIter, r.num_levels, r.seconds, r.gcg.nevConv, r.gcg.numIter, r.gcg.seconds, rc);
	return rc;
}
