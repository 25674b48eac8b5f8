/* GCGE_ChebFilter and GCGE_RunChFSI (csrc/host/chfsi.c) over the CPU oracle's table on a small Laplacian, as a program of its own
 * for the host sanitizers: `make -C gcge_amd/csrc check-chfsi` compiles this file, the host sources and oracle/cpu_backend.c with
 * -fsanitize=address,undefined and runs it.  Checks the eigenvalues against the closed form, a warm start, and the refusals. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gcge_problems.h"
#include "gcge_solver.h"
#include "oracle.h"

static int cmp_double(const void *a, const void *b) { double x = *(const double*)a, y = *(const double*)b; return (x > y) - (x < y); }

int main(void)
{
	enum { N = 8, NEV = 4, NEVMAX = 8 };
	GCGE_CSR A; ORACLE_CCS M; OPS *ops; void **evec, **w1, **w2;
	double eval[NEVMAX], exact[N * N * N]; GCGE_CHFSI_RESULT res; int rc, i, j, k, bad = 0;
	char *argv[] = {"chfsi_check", "-nevConv", "4", "-nevMax", "8", "-chfsi_degree", "15", "-gcge_rel_tol", "1e-9", "-gcge_max_niter", "40",
	                "-chfsi_lanczos_steps", "6"};
	char *argv_bad[] = {"chfsi_check", "-nevConv", "4", "-nevMax", "2"};
	const int argc = (int)(sizeof(argv) / sizeof(argv[0]));

	if (gcge_problem_lap3d(N, 0, -1, &A) != 0) return 2;
	M.data = A.val; M.i_row = A.colidx; M.j_col = A.rowptr; M.nrows = A.nrows; M.ncols = A.ncols;      /* symmetric: CSR is CCS */
	OPS_Create(&ops); OPS_ORACLE_Set(ops); OPS_Setup(ops); GCGE_SetQuiet(ops, 1);
	for (i = 0; i < N; ++i) for (j = 0; j < N; ++j) for (k = 0; k < N; ++k)
		exact[(i * N + j) * N + k] = 6.0 - 2.0 * (cos((i + 1) * M_PI / (N + 1)) + cos((j + 1) * M_PI / (N + 1)) + cos((k + 1) * M_PI / (N + 1)));
	qsort(exact, N * N * N, sizeof(double), cmp_double);

	ops->MultiVecCreateByMat(&evec, NEVMAX, &M, ops);
	rc = GCGE_RunChFSI(&M, argc, argv, ops, eval, evec, 0, &res);
	printf("cold: rc %d, nevConv %d, numIter %d, upper %.6f (lambda_max %.6f)\n", rc, res.nevConv, res.numIter, res.upper, exact[N * N * N - 1]);
	if (rc != 0 || res.nevConv != NEV || res.upper < exact[N * N * N - 1]) ++bad;
	for (i = 0; i < NEV; ++i) if (fabs(eval[i] - exact[i]) > 1e-8 * exact[i]) { printf("eigenvalue %d: %.15e, exact %.15e\n", i, eval[i], exact[i]); ++bad; }
	rc = GCGE_RunChFSI(&M, argc, argv, ops, eval, evec, NEVMAX, &res);                     /* warm: every column given */
	printf("warm: rc %d, nevConv %d, numIter %d\n", rc, res.nevConv, res.numIter);
	if (rc != 0 || res.nevConv != NEV || res.numIter > 1) ++bad;
	if (GCGE_RunChFSI(&M, 5, argv_bad, ops, eval, evec, 0, &res) != -1) ++bad;             /* nevMax < nevConv */
	if (GCGE_RunChFSI(&M, argc, argv, ops, eval, evec, NEVMAX + 1, &res) != -1) ++bad;

	ops->MultiVecCreateByMat(&w1, 3, &M, ops); ops->MultiVecCreateByMat(&w2, 3, &M, ops);
	for (i = 1; i <= 7; ++i) if (GCGE_ChebFilter(&M, evec, 5, 3, i, 6.0, 12.0, 0.1, w1, w2, ops) != 0) ++bad;      /* the last window, every rotation */
	if (GCGE_ChebFilter(&M, evec, 0, 3, 0, 6.0, 12.0, 0.1, w1, w2, ops) != -1) ++bad;
	if (GCGE_ChebFilter(&M, evec, 0, 3, 4, 6.0, 12.0, 0.1, w1, w1, ops) != -1) ++bad;
	ops->MultiVecDestroy(&w1, 3, ops); ops->MultiVecDestroy(&w2, 3, ops);
	ops->MultiVecDestroy(&evec, NEVMAX, ops);
	OPS_Destroy(&ops);
	gcge_csr_free(&A);
	printf(bad ? "chfsi_check: %d FAILED\n" : "chfsi_check: ok\n", bad);
	return bad != 0;
}
