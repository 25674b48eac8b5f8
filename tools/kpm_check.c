/* GCGE_ChebMoments and GCGE_ChebCountFromMoments (csrc/host/chfsi.c) over the CPU oracle's table on a small Laplacian, as a program of
 * its own for the host sanitizers: `make -C gcge_amd/csrc check-kpm` compiles this file, the host sources and oracle/cpu_backend.c with
 * -fsanitize=address,undefined and runs it.  The table offers neither cheb_step_dots nor cheb_step, so every step is the slot sequence
 * and two MultiVecLocalInnerProd('D').
 * Checks: for a column that IS an eigenvector (a tensor sine mode) mu_j = |v|^2 T_j((lambda - c) / e) at every j, odd and even degrees
 * and every rotation of the ring; a window behind column 0; v untouched; with +-1 probes mu_0 = n and the count of [0.9, 1.5] — 7
 * eigenvalues between neighbours at 0.709 and 1.589 — within 4 standard errors of the trace of p over the closed form's spectrum;
 * the refusals. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gcge_problems.h"
#include "gcge_solver.h"
#include "oracle.h"

enum { N = 8, NN = N * N * N, M = 3, MAXDEG = 40, PROBES = 48, CDEG = 60 };

static double cheb_t(int j, double t) { return cos(j * acos(t)); }

int main(void)
{
	GCGE_CSR A; ORACLE_CCS Mat; OPS *ops; void **v, **w1, **w2, **w3, **pv;
	ORACLE_VEC *vv; double lam[M], *mom, *keep, c, e; const double lmin = -0.5, lmax = 12.5;
	static const int mode[M][3] = {{1, 1, 1}, {2, 1, 1}, {3, 2, 1}};
	int i, j, k, col, degree, bad = 0;

	if (gcge_problem_lap3d(N, 0, -1, &A) != 0) return 2;
	Mat.data = A.val; Mat.i_row = A.colidx; Mat.j_col = A.rowptr; Mat.nrows = A.nrows; Mat.ncols = A.ncols;      /* symmetric: CSR is CCS */
	OPS_Create(&ops); OPS_ORACLE_Set(ops); OPS_Setup(ops); GCGE_SetQuiet(ops, 1);
	c = 0.5 * (lmax + lmin); e = 0.5 * (lmax - lmin);

	/* a block of M + 2 columns: guard, M sine modes, guard */
	ops->MultiVecCreateByMat(&v, M + 2, &Mat, ops);
	ops->MultiVecCreateByMat(&w1, M, &Mat, ops); ops->MultiVecCreateByMat(&w2, M + 1, &Mat, ops); ops->MultiVecCreateByMat(&w3, M, &Mat, ops);
	vv = (ORACLE_VEC*)v;
	for (i = 0; i < NN; ++i) { vv->data[i] = 3.0; vv->data[(size_t)(M + 1) * vv->ldd + i] = 5.0; }
	for (col = 0; col < M; ++col) {
		lam[col] = 0.0;
		for (k = 0; k < 3; ++k) lam[col] += 2.0 - 2.0 * cos(mode[col][k] * M_PI / (N + 1));
		for (i = 0; i < N; ++i) for (j = 0; j < N; ++j) for (k = 0; k < N; ++k)
			vv->data[(size_t)(col + 1) * vv->ldd + (i * N + j) * N + k] = sin(mode[col][0] * (k + 1) * M_PI / (N + 1)) *
				sin(mode[col][1] * (j + 1) * M_PI / (N + 1)) * sin(mode[col][2] * (i + 1) * M_PI / (N + 1));
	}
	keep = (double*)malloc((size_t)(M + 2) * vv->ldd * sizeof(double));
	memcpy(keep, vv->data, (size_t)(M + 2) * vv->ldd * sizeof(double));
	mom = (double*)malloc((size_t)(CDEG + 1) * PROBES * sizeof(double));

	for (degree = 1; degree <= MAXDEG; degree += (degree < 8 ? 1 : 16)) {
		double worst = 0.0;
		if (GCGE_ChebMoments(&Mat, v, 1, M, degree, lmin, lmax, w1, w2, w3, mom, ops) != 0) { ++bad; continue; }
		for (col = 0; col < M; ++col)
			for (j = 0; j <= degree; ++j) {
				const double want = mom[col] * cheb_t(j, (lam[col] - c) / e), err = fabs(mom[(size_t)j * M + col] - want) / mom[col];
				if (err > worst) worst = err;
			}
		printf("degree %2d: max |mu_j - |v|^2 T_j(t)| / |v|^2 = %.3e\n", degree, worst);
		if (!(worst <= 1e-10)) ++bad;
	}
	if (memcmp(keep, vv->data, (size_t)(M + 2) * vv->ldd * sizeof(double)) != 0) { printf("v was written\n"); ++bad; }

	/* the refusals: nothing is written */
	mom[0] = -7.0;
	if (GCGE_ChebMoments(&Mat, v, 1, M, 0, lmin, lmax, w1, w2, w3, mom, ops) != -1) ++bad;
	if (GCGE_ChebMoments(&Mat, v, 1, 0, 4, lmin, lmax, w1, w2, w3, mom, ops) != -1) ++bad;
	if (GCGE_ChebMoments(&Mat, v, 1, M, 4, lmax, lmin, w1, w2, w3, mom, ops) != -1) ++bad;
	if (GCGE_ChebMoments(&Mat, v, 1, M, 4, lmin, lmax, w1, w1, w3, mom, ops) != -1) ++bad;
	if (GCGE_ChebMoments(&Mat, v, 1, M, 4, lmin, lmax, w1, w2, v, mom, ops) != -1) ++bad;
	if (GCGE_ChebMoments(&Mat, v, 1, M, 4, lmin, lmax, w1, w2, w3, NULL, ops) != -1) ++bad;
	if (mom[0] != -7.0) ++bad;

	/* +-1 probes: mu_0 = n, and the count of [0.9, 1.5] against the trace of p over the closed form's spectrum */
	{
		double *mu = (double*)malloc((CDEG + 1) * sizeof(double)), trace = 0.0, count = 0.0, se = 0.0, per[PROBES], mean = 0.0;
		unsigned long long s = 88172645463325252ULL;
		ORACLE_VEC *pp;
		ops->MultiVecCreateByMat(&pv, PROBES, &Mat, ops);
		pp = (ORACLE_VEC*)pv;
		for (col = 0; col < PROBES; ++col)
			for (i = 0; i < NN; ++i) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; pp->data[(size_t)col * pp->ldd + i] = (s >> 33) & 1 ? 1.0 : -1.0; }
		ops->MultiVecDestroy(&w1, M, ops); ops->MultiVecDestroy(&w2, M + 1, ops); ops->MultiVecDestroy(&w3, M, ops);
		ops->MultiVecCreateByMat(&w1, PROBES, &Mat, ops); ops->MultiVecCreateByMat(&w2, PROBES, &Mat, ops); ops->MultiVecCreateByMat(&w3, PROBES, &Mat, ops);
		if (GCGE_ChebMoments(&Mat, pv, 0, PROBES, CDEG, lmin, lmax, w1, w2, w3, mom, ops) != 0) ++bad;
		for (col = 0; col < PROBES; ++col) if (mom[col] != (double)NN) ++bad;
		if (GCGE_ChebBandCoefficients(CDEG, 0.9, 1.5, lmin, lmax, mu) != 0) ++bad;
		for (i = 0; i < N; ++i) for (j = 0; j < N; ++j) for (k = 0; k < N; ++k) {
			const double l = 6.0 - 2.0 * (cos((i + 1) * M_PI / (N + 1)) + cos((j + 1) * M_PI / (N + 1)) + cos((k + 1) * M_PI / (N + 1)));
			int q;
			for (q = 0; q <= CDEG; ++q) trace += mu[q] * cheb_t(q, (l - c) / e);
		}
		if (GCGE_ChebCountFromMoments(mom, PROBES, CDEG, 0.9, 1.5, lmin, lmax, &count, &se, per) != 0) ++bad;
		for (col = 0; col < PROBES; ++col) mean += per[col] / PROBES;
		printf("count %.4f, stderr %.4f, trace of p %.4f (7 eigenvalues inside)\n", count, se, trace);
		if (!(fabs(count - trace) <= 4.0 * se) || !(se > 0.0 && se <= 1.5) || fabs(mean - count) > 1e-12 * NN) ++bad;
		if (GCGE_ChebCountFromMoments(mom, 1, CDEG, 0.9, 1.5, lmin, lmax, &count, &se, NULL) != 0 || se != 0.0) ++bad;      /* one probe, no per_probe */
		count = -7.0;
		if (GCGE_ChebCountFromMoments(mom, PROBES, 1, 0.9, 1.5, lmin, lmax, &count, &se, per) != -1) ++bad;
		if (GCGE_ChebCountFromMoments(mom, 0, CDEG, 0.9, 1.5, lmin, lmax, &count, &se, per) != -1) ++bad;
		if (GCGE_ChebCountFromMoments(mom, PROBES, CDEG, 1.5, 0.9, lmin, lmax, &count, &se, per) != -1) ++bad;
		if (GCGE_ChebCountFromMoments(mom, PROBES, CDEG, 13.0, 14.0, lmin, lmax, &count, &se, per) != -1) ++bad;
		if (GCGE_ChebCountFromMoments(NULL, PROBES, CDEG, 0.9, 1.5, lmin, lmax, &count, &se, per) != -1) ++bad;
		if (GCGE_ChebCountFromMoments(mom, PROBES, CDEG, 0.9, 1.5, lmin, lmax, NULL, &se, per) != -1) ++bad;
		if (count != -7.0) ++bad;
		ops->MultiVecDestroy(&pv, PROBES, ops);
		ops->MultiVecDestroy(&w1, PROBES, ops); ops->MultiVecDestroy(&w2, PROBES, ops); ops->MultiVecDestroy(&w3, PROBES, ops);
		free(mu);
	}
	ops->MultiVecDestroy(&v, M + 2, ops);
	free(mom); free(keep);
	OPS_Destroy(&ops);
	gcge_csr_free(&A);
	printf(bad ? "kpm_check: %d FAILED\n" : "kpm_check: ok\n", bad);
	return bad != 0;
}
