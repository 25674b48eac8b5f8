/* gcge_multigrid.h — host side of the multigrid hierarchy behind ops->MultiGridCreate.
 *
 * The reference's multigrid solver (BlockAlgebraicMultiGrid, src/ops_lin_sol.c:466-715) takes its hierarchy
 *     A_0 = A,  A_{l+1} ~ P_l^T A_l P_l,   P_l : level l+1 -> level l
 * from the back-end through the MultiGridCreate slot (src/ops.h:134-139; app/app_slepc.c:648-728 asks PETSc GAMG,
 * app/app_hypre.c BoomerAMG, app/app_lapack.c:863-929 builds a fixed 1-D toy).  This header is what OUR back-ends build
 * it from: plain aggregation on the host CSR arrays —
 *   - a lexicographic nx x ny x nz grid read off the rows' column offsets is coarsened 2 x 2 x 2 (cell-centred);
 *   - any other symmetric matrix by greedy aggregation over its strong couplings (Vanek / Mandel / Brezina), or, when
 *     gcge_mg_set_graph_method (1) asks for it, by MIS-2 aggregation (roots two strong edges apart; Bell / Dalton / Olson 2012);
 *   - P is the piecewise-constant prolongation of the aggregates (one 1.0 per row), A_{l+1} = scale * P^T A_l P.
 * scale = 1 is the Galerkin operator.  Piecewise-constant P over-estimates the energy of a smooth coarse function by 2
 * for second-order operators whatever the dimension (only the jumps across aggregate faces count), so the correction a
 * Galerkin coarse problem returns is half of what it should be; scale = 0.5 (the default of the back-ends) is the
 * classical over-correction (Braess 1995) folded into the coarse operator — BlockAMG itself adds the correction with
 * factor 1 (src/ops_lin_sol.c:626-640), so the hierarchy is the only place for it.
 * Everything here is host C; the back-ends wrap the levels into their own matrix handles.
 */
#ifndef GCGE_MULTIGRID_H
#define GCGE_MULTIGRID_H

#include "gcge_problems.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nx, ny, nz of a lexicographic grid (index x + nx (y + ny z)) whose neighbour couplings the rows of A show: +-1 ... +-arm
 * along a line, multiples of nx between lines, of nx ny between planes (1-D and 2-D grids: ny and / or nz = 1).
 * Returns 1 and fills dims[3] (and *arm, may be NULL), 0 when the rows show no such grid.                          */
int gcge_mg_detect_grid (const GCGE_CSR *A, int dims[3], int *arm);     /* also: a slab of rows with GLOBAL columns (ncols = global size) */

/* 2 x 2 x 2 aggregates of an nx x ny x nz grid (the last aggregate of an odd direction holds one layer):
 * agg[r] = coarse index of row r, cdims = coarse grid.  Returns the number of aggregates.                          */
int gcge_mg_aggregate_grid (const int dims[3], int *agg, int cdims[3]);

/* the same cells on a MASKED grid: row r is box point box_of_row[r] = x + nx (y + ny z) of the box `dims` (strictly ascending: the
 * points inside a sphere in scan order, the PARSEC matrices), its cell is (x / 2, y / 2, z / 2) of the box cdims = ceil(dims / 2).
 * A cell is a coarse row when it holds at least one fine row (1 to 8 of them); the occupied cells are numbered in ascending coarse
 * box index, so the coarse rows are a masked grid in scan order again: agg[r] = that number, cbox_out[I] (room for nrows ints) =
 * the coarse box index of coarse row I.  Returns the number of aggregates — gcge_mg_aggregate_grid's result, bit for bit, when every
 * box point is a row; -2: box_of_row is not strictly ascending or leaves the box, -3: out of memory.                          */
int gcge_mg_aggregate_masked (const int dims[3], const int *box_of_row, int nrows, int *agg, int cdims[3], int *cbox_out);

/* greedy aggregation over the strong couplings |a_ij| >= theta * max_k |a_ik| (k != i): pass 1 forms an aggregate from
 * every node whose strong neighbours are all still free, pass 2 attaches the rest to the neighbouring aggregate they are
 * coupled to most strongly, pass 3 turns what is left (isolated rows) into aggregates of their own.
 * Returns the number of aggregates.                                                                                */
int gcge_mg_aggregate_graph (const GCGE_CSR *A, double theta, int *agg);

/* MIS-2 aggregation over the strong couplings, defined so that this sequential routine and the kernels of the HIP back-end
 * (csrc/hip/mg_aggregate.hip) give the same aggregates byte for byte on a symmetric matrix with ascending columns:
 *   strength   thr[r] = theta * max |a_rc| over c != r, c < n (0 without such an entry); entry (r, c) is a strong edge when c != r,
 *              c < n, a_rc != 0 and |a_rc| >= min (thr[r], thr[c]) - read from row r and thr alone, symmetric whenever A is;
 *   priority   rows are compared by (gcge_mg_mis2_key (r), r), the larger wins; the mixer is a bijection, so no two keys tie;
 *   roots      the maximal independent set of the distance-2 graph of the strong edges taken greedily in descending priority: a
 *              row is a root exactly when no root of higher priority lies within two strong edges of it (a row without a strong
 *              edge is a root); the roots in ascending ROW order are aggregates 0 .. nc - 1, so coarse rows follow the fine order;
 *   join 1     every other row with a root among its strong neighbours joins the one it is coupled to by the largest |a_rc|
 *              (ties: the smaller root row);
 *   join 2     every row still free has a strong neighbour placed in join 1 and joins the aggregate of the one with the largest
 *              |a_rc| (ties: the smaller aggregate); rows placed here attract nobody.
 * On a structurally unsymmetric matrix a row the two joins leave free becomes a root itself (renumbered, joins repeated): the
 * result is a partition whatever the input.  Returns the number of aggregates, -3: out of memory.                          */
#define GCGE_MG_MIS2_SEED 0x4D49533247434745ULL
#if defined(__HIPCC__)
#define GCGE_MG_HD __host__ __device__
#else
#define GCGE_MG_HD
#endif
/* the 64-bit mixer of gcge_uniform (csrc/host/problems.c) applied to GCGE_MG_MIS2_SEED + r; never 0 for a row index */
GCGE_MG_HD static inline uint64_t gcge_mg_mis2_key (int r)
{
	uint64_t z = GCGE_MG_MIS2_SEED + (uint64_t)r;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	return z ^ (z >> 31);
}
int gcge_mg_aggregate_mis2 (const GCGE_CSR *A, double theta, int *agg);
/* which of the two a matrix without a grid is aggregated by, process-wide like gcge_mg_set_defaults: 0 the greedy routine (default),
 * 1 MIS-2.  gcge_mg_build and the back-ends' MultiGridCreate slots read it; any other value is ignored.                       */
void gcge_mg_set_graph_method (int method);
int  gcge_mg_get_graph_method (void);

/* Ac = scale * P^T A P for the piecewise-constant P of `agg` (nc aggregates): nc x nc CSR, ascending columns.
 * Rows of the sum are accumulated in ascending fine-row order, entries of a row in storage order (deterministic).   */
int gcge_mg_galerkin (const GCGE_CSR *A, const int *agg, int nc, double scale, GCGE_CSR *Ac);

/* P (nf x nc, one entry 1.0 per row) and its transpose (nc x nf, ascending columns) as CSR                         */
int gcge_mg_prolongation (const int *agg, int nf, int nc, GCGE_CSR *P, GCGE_CSR *PT);

/* the whole hierarchy: level 0 is A itself (not copied: A[0] aliases the caller's arrays and is never freed here)   */
typedef struct GCGE_MG_ {
	int      num_levels;
	int      box_levels;  /* > 0: a hierarchy of gcge_mg_build_masked, gcge_mg_level_box names the rows of its levels   */
	GCGE_CSR *A;          /* [num_levels]      A[0] = the caller's matrix                                  */
	GCGE_CSR *B;          /* [num_levels] or NULL (B == NULL): Galerkin P^T B P, never rescaled            */
	GCGE_CSR *P;          /* [num_levels - 1]  P[l]: rows(A[l]) x rows(A[l+1])                              */
	GCGE_CSR *PT;         /* [num_levels - 1]  the transposes                                               */
	int      (*dims)[3];  /* [num_levels] grid of the level, {0,0,0}: aggregated over the graph             */
} GCGE_MG;
/* Builds at most max_levels levels and stops early when a level has no more than min_rows rows or coarsening stalls
 * (fewer than 1.5 x fewer rows).  Returns 0 and fills mg (mg->num_levels >= 1), -3 out of memory.                  */
int  gcge_mg_build (const GCGE_CSR *A, const GCGE_CSR *B, int max_levels, int min_rows, double scale, GCGE_MG *mg);
void gcge_mg_free (GCGE_MG *mg);

/* gcge_mg_build on a masked grid: the cells of gcge_mg_aggregate_masked at EVERY level (same stopping rules, same scale), level
 * l on the box mg->dims[l] with its rows named by gcge_mg_level_box (mg, l) (mg->A[l].nrows ascending box indices, owned by mg;
 * level 0: a copy of box_of_row).  Returns 0, -2: the geometry does not fit A (see gcge_mg_aggregate_masked), -3: out of memory.
 * The box arrays hang off the block mg->dims points into and box_levels (which sits where the structure had padding) finds them:
 * GCGE_MG keeps its size and the offsets of its members, callers built against the earlier header still match.              */
int  gcge_mg_build_masked (const GCGE_CSR *A, const GCGE_CSR *B, const int dims[3], const int *box_of_row, int max_levels, int min_rows,
		double scale, GCGE_MG *mg);
const int *gcge_mg_level_box (const GCGE_MG *mg, int level);     /* NULL: the level has none (any other hierarchy)            */

/* The hierarchy of ONE row slab (one rank per GPU): A holds rows [part[rank], part[rank + 1]) with GLOBAL columns of a matrix on the
 * lexicographic grid `dims`; every slab is whole planes.  Every rank pairs ITS OWN planes from its first one (an odd count ends in a
 * thinner cell), columns in a neighbour's planes follow the neighbour's pairing through the shared partition: with cuts on even planes
 * the levels are the whole-matrix hierarchy's rows, with a cut on an odd plane the cells next to it are the rank's own — Galerkin
 * either way.  A level is coarsened while every slab holds a plane and some slab two — every rank evaluates that from the shared
 * partition, so all ranks build the same number of levels; level l + 1 has sum_r ceil(planes_r / 2) planes.  mg->A[l] (l >= 1): the coarse slab with GLOBAL coarse columns, row_begin =
 * part_levels[l * (world + 1) + rank]; mg->P[l] / PT[l]: local (owned fine rows x owned coarse rows: the cells of a slab lie inside
 * it).  part_levels (free with free()): the row partition of every level.  Returns 0; -2: the slab is not whole planes of `dims`. */
int gcge_mg_build_slab (const GCGE_CSR *A, const int dims[3], const long *part, int rank, int world, int max_levels, double scale,
		GCGE_MG *mg, long **part_levels_out);

/* Where every LOCAL column of one level of that hierarchy goes (what a refresh of the coarse slab's values in place needs, and all it
 * needs of the neighbours): dims / part are those of level l (part = part_levels + l * (world + 1)), ghost[nghost] the ascending global
 * rows behind level l's halo columns, ghost_c[nghost_c] those of level l + 1.  colagg[c], c < nrows_l + nghost: the LOCAL column of
 * level l + 1 that fine column c aggregates into — an own row through the rank's own pairing (P_l's column), a halo row through its
 * owner's pairing and its place in ghost_c (nrows_{l+1} + index).  *nlo_c (may be NULL): how many of ghost_c lie below the coarse slab
 * (a localized row lists them after its own columns although they come first in global order).  Returns 0; -2: the level is not
 * coarsened (gcge_mg_build_slab would stop here), or a halo row's aggregate is not among ghost_c.                                  */
int gcge_mg_slab_colagg (const int dims[3], const long *part, int rank, int world, const int *ghost, int nghost, const int *ghost_c,
		int nghost_c, int *colagg, int *nlo_c);

/* process-wide defaults the back-ends' MultiGridCreate slots use (the slot's signature has no room for them,
 * src/ops.h:134): scale as above (default 0.5), min_rows (default 64), theta of the graph aggregation (default 0.25) */
void gcge_mg_set_defaults (double scale, int min_rows, double theta);
void gcge_mg_get_defaults (double *scale, int *min_rows, double *theta);

#ifdef __cplusplus
}
#endif
#endif
