/* Stand-alone check of the run and parity test ComputeW makes before it leaves the W start vectors and b to the solver
 * (GCGE_GcgStartInPlaceRange, csrc/host/gcg.c), over synthetic offset[] lists, for a build with the host sanitizers:
 *     make -C gcge_amd/csrc check-start-range
 * compiles this file with the host sources under -fsanitize=address,undefined and runs it.  Every list is a heap block of exactly
 * its own length, so a read past the last run is an error the sanitizer reports.  Exit status 0: every case as expected. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gcge_solver.h"

static int failures = 0;

/* runs: n pairs (lo, hi); expect: 1 / 0; elo, etotal: the range expected with 1 */
static void one(const char *name, int n, const int *runs, int startW, int expect, int elo, int etotal)
{
	int *offset = (int*)malloc((size_t)(2 * n + 1) * sizeof(int));
	int lo = -7, total = -7, got;
	offset[0] = n;
	if (n > 0) memcpy(offset + 1, runs, (size_t)(2 * n) * sizeof(int));
	got = GCGE_GcgStartInPlaceRange(offset, startW, &lo, &total);
	if (got != expect || (expect && (lo != elo || total != etotal)) || (!expect && (lo != -7 || total != -7))) {
		printf("FAIL %s: got %d (lo %d, total %d), expected %d (lo %d, total %d)\n", name, got, lo, total, expect, elo, etotal);
		++failures;
	}
	if (expect && GCGE_GcgStartInPlaceRange(offset, startW, NULL, NULL) != 1) { printf("FAIL %s: NULL outputs\n", name); ++failures; }
	free(offset);
}

int main(void)
{
	int lo, hi, gap, w, n2;
	{ const int r[] = {4, 12};             one("one run", 1, r, 24, 1, 4, 8); }
	{ const int r[] = {4, 10, 10, 12};     one("adjacent runs (tail + padding)", 2, r, 24, 1, 4, 8); }
	{ const int r[] = {4, 9, 9, 10, 10, 16}; one("three adjacent runs, odd inner ends", 3, r, 24, 1, 4, 12); }
	{ const int r[] = {4, 8, 10, 14};      one("a hole", 2, r, 24, 0, 0, 0); }
	{ const int r[] = {5, 13};             one("odd lo", 1, r, 24, 0, 0, 0); }
	{ const int r[] = {4, 11};             one("odd length", 1, r, 24, 0, 0, 0); }
	{ const int r[] = {4, 12};             one("odd W origin", 1, r, 25, 0, 0, 0); }
	{ const int r[] = {4, 4};              one("an empty run", 1, r, 24, 0, 0, 0); }
	{ const int r[] = {10, 14, 4, 8};      one("runs out of order", 2, r, 24, 0, 0, 0); }
	one("zero unconverged columns", 0, NULL, 24, 0, 0, 0);
	if (GCGE_GcgStartInPlaceRange(NULL, 24, &lo, &hi) != 0) { printf("FAIL NULL list\n"); ++failures; }
	/* every two-run list of a small block: 1 exactly for gap 0 and an even origin, length and W origin */
	for (lo = 0; lo < 6; ++lo) for (hi = lo + 1; hi < 9; ++hi) for (gap = 0; gap < 3; ++gap) for (n2 = 1; n2 < 4; ++n2) for (w = 12; w < 14; ++w) {
		const int r[] = {lo, hi, hi + gap, hi + gap + n2};
		const int len = hi + n2 - lo, want = gap == 0 && !((lo | len | w) & 1);
		one("sweep", 2, r, w, want, lo, len);
	}
	/* where b goes stays inside the scratch columns for the origins such ranges have */
	for (lo = 0; lo < 8; ++lo) for (n2 = 1; n2 <= 8 - lo; ++n2) {
		const int b0 = GCGE_GcgRhsOrigin(lo, n2, 0, 8);
		if (b0 < 0 || b0 + n2 > 8 || (!(lo & 1) && b0 != lo)) { printf("FAIL rhs origin %d %d -> %d\n", lo, n2, b0); ++failures; }
	}
	printf(failures ? "start range check: %d failures\n" : "start range check: ok\n", failures);
	return failures != 0;
}
