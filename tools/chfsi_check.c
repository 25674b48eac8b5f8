/* GCGE_ChebFilter and GCGE_RunChFSI (csrc/host/chfsi.c) over the CPU oracle's table on a small Laplacian, as a program of its own
 * for the host sanitizers: `make -C gcge_amd/csrc check-chfsi` compiles this file, the host sources and oracle/cpu_backend.c with
 * -fsanitize=address,undefined and runs it.  Checks the eigenvalues against the closed form, a warm start, and the refusals; then
 * the band coefficients, the band filter (odd and even degrees, every rotation) and one GCGE_RunChFSIBand on [0.9, 1.5], which
 * holds 7 of the closed form's eigenvalues (3 + 3 + 1) between neighbours at 0.709 and 1.589. */
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
	{
		enum { BAND = 16, DEG = 60 };
		void **acc, **bvec; double mu[DEG + 1], sum = 0.0, beval[BAND]; GCGE_CHFSI_BAND_RESULT bres; int inside = 0, first = 0;
		char *bargv[] = {"chfsi_check", "-chfsi_band_lo", "0.9", "-chfsi_band_hi", "1.5", "-nevMax", "16", "-chfsi_degree", "60", "-gcge_rel_tol", "1e-9",
		                 "-gcge_max_niter", "60", "-chfsi_lanczos_steps", "8"};
		const int bargc = (int)(sizeof(bargv) / sizeof(bargv[0]));
		if (GCGE_ChebBandCoefficients(DEG, 0.9, 1.5, -0.5, 12.5, mu) != 0) ++bad;
		if (fabs(mu[0] - (acos((0.9 - 6.0) / 6.5) - acos((1.5 - 6.0) / 6.5)) / M_PI) > 1e-15) ++bad;      /* g_0 = 1 */
		for (i = 0; i <= DEG; ++i) sum += fabs(mu[i]);
		if (!(sum < 1.0 + (2.0 / M_PI) * 5.0)) ++bad;                                                       /* (H_60 < 5) */
		if (GCGE_ChebBandCoefficients(1, 0.9, 1.5, -0.5, 12.5, mu) != -1 || GCGE_ChebBandCoefficients(4, 1.5, 0.9, -0.5, 12.5, mu) != -1 ||
		    GCGE_ChebBandCoefficients(4, 13.0, 14.0, -0.5, 12.5, mu) != -1 || GCGE_ChebBandCoefficients(4, 0.9, 1.5, 12.5, -0.5, mu) != -1) ++bad;
		ops->MultiVecCreateByMat(&acc, 3, &M, ops);
		for (i = 2; i <= 8; ++i) if (GCGE_ChebBandFilter(&M, evec, 5, 3, i, 0.9, 1.5, -0.5, 12.5, w1, w2, acc, ops) != 0) ++bad;
		if (GCGE_ChebBandFilter(&M, evec, 0, 3, 1, 0.9, 1.5, -0.5, 12.5, w1, w2, acc, ops) != -1) ++bad;
		if (GCGE_ChebBandFilter(&M, evec, 0, 3, 4, 0.9, 1.5, -0.5, 12.5, w1, w2, w1, ops) != -1) ++bad;
		if (GCGE_ChebBandFilter(&M, evec, 0, 3, 4, 0.9, 1.5, -0.5, 12.5, w1, w2, evec, ops) != -1) ++bad;
		ops->MultiVecDestroy(&acc, 3, ops);

		for (i = 0; i < N * N * N; ++i) if (exact[i] >= 0.9 && exact[i] <= 1.5) { if (inside == 0) first = i; ++inside; }
		ops->MultiVecCreateByMat(&bvec, BAND, &M, ops);
		rc = GCGE_RunChFSIBand(&M, bargc, bargv, ops, beval, bvec, 0, &bres);
		printf("band: rc %d, pairs %d of %d, converged %d, numIter %d, spurious %d, bounds [%.4f, %.4f], edge %.6f\n", rc, bres.nevConv, inside,
		       bres.converged, bres.numIter, bres.spurious, bres.lmin, bres.lmax, bres.edge);
		if (rc != 0 || inside != 7 || bres.nevConv != inside || bres.converged != 1 || bres.lmin > exact[0] || bres.lmax < exact[N * N * N - 1]) ++bad;
		for (i = 0; i < inside && i < bres.nevConv; ++i)
			if (fabs(beval[i] - exact[first + i]) > 1e-8 * exact[first + i]) { printf("band eigenvalue %d: %.15e, exact %.15e\n", i, beval[i], exact[first + i]); ++bad; }
		rc = GCGE_RunChFSIBand(&M, bargc, bargv, ops, beval, bvec, BAND, &bres);                /* warm: every column given */
		printf("band, warm: rc %d, pairs %d, numIter %d\n", rc, bres.nevConv, bres.numIter);
		if (rc != 0 || bres.nevConv != inside || bres.numIter > 1) ++bad;
		if (GCGE_RunChFSIBand(&M, 5, bargv, ops, beval, bvec, 0, &bres) != -1) ++bad;            /* no -nevMax */
		if (GCGE_RunChFSIBand(&M, bargc, bargv, ops, beval, bvec, BAND + 1, &bres) != -1) ++bad;
		ops->MultiVecDestroy(&bvec, BAND, ops);
	}
	ops->MultiVecDestroy(&w1, 3, ops); ops->MultiVecDestroy(&w2, 3, ops);
	ops->MultiVecDestroy(&evec, NEVMAX, ops);
	OPS_Destroy(&ops);
	gcge_csr_free(&A);
	printf(bad ? "chfsi_check: %d FAILED\n" : "chfsi_check: ok\n", bad);
	return bad != 0;
}
