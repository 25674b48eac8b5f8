/* gcge_hip.h — C ABI of the MI355X (gfx950) back-end, libgcge_hip.so.
 *
 * Drop-in boundary: `OPS_HIP_Set` fills the operator table of gcge_ops.h exactly as
 * the reference's built-in back-ends do (pattern: app/app_ccs.c:213-249 OPS_CCS_Set,
 * app/app_slepc.c:610-634 OPS_SLEPC_Set), so GCGE's solver layers — the
 * reference's or ours — run with every O(n) operand resident in HBM.
 * Everything below is plain C: pointers and sizes only, no C++/torch types.
 *
 * Device layout of a block of vectors: ROW-major, element (r,c) at d[r*ld + c],
 * ld a multiple of 8 doubles; rows [nrows, nrows+nghost) are halo rows used only
 * while a row-partitioned SpMM runs.  Handles are opaque to the solver
 * (the reference never dereferences them: SURVEY.md §8b "Layout opacity").
 */
#ifndef GCGE_HIP_H
#define GCGE_HIP_H

#include <stddef.h>
#include "gcge_ops.h"
#include "gcge_problems.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime ---------------------------------------------------------------- */
int  gcge_hip_init (int device);              /* hipSetDevice + workspace; 0 on success   */
void gcge_hip_finalize (void);
int  gcge_hip_device_count (void);
void gcge_hip_sync (void);
void *gcge_hip_stream (void);                 /* hipStream_t all kernels are launched on  */

/* ---- back-end registration (replaces OPS_CCS_Set, app/app_ccs.c:213-249) ------ */
void OPS_HIP_Set (struct OPS_ *ops);

/* ---- the driver a maintainer calls from test/main.c:40-49 (counterpart of TestAppCCS, test/test_app_ccs.c:86-140):
 * table + OPS_HIP_Set + OPS_Setup, matrices from a generator or a file, TestEigenSolverGCG(A, B, flag, argc, argv, ops).
 * Options: csrc/host/test_app_hip.c (-hip_problem, -hip_size, -hip_petsc_A/B, -hip_mtx_A/B, -hip_flag, -hip_device).  */
int TestAppHIP (int argc, char *argv[]);

/* ---- sparse matrix handle (replaces CCSMAT, app/app_ccs.h:20-24) -------------- */
typedef struct GCGE_HIP_MAT_ GCGE_HIP_MAT;
/* rows [row_begin,row_begin+nrows) of a symmetric matrix, GLOBAL column indices, host CSR
 * (== the CCS triple j_col/i_row/data).  Single rank: row_begin = 0, nrows = nglobal. */
GCGE_HIP_MAT *gcge_hip_mat_create (int nrows, int nglobal, int row_begin,
		const int *rowptr, const int *colidx, const double *val);
GCGE_HIP_MAT *gcge_hip_mat_create_csr (const GCGE_CSR *A);
/* the same for a matrix on a MASKED grid (one rank): row r is grid point box_of_row[r] = x + nx (y + ny z) of an nx x ny x nz box,
 * rows in scan order (ascending box index) — the grid points inside a sphere of the PARSEC matrices the reference's
 * test/submit.sh:9-15 lists.  Naming the geometry lets the star-stencil rows take the plane sweep (spmm_star.hip, through a row
 * map); results are those of gcge_hip_mat_create on the same arrays.                                                          */
GCGE_HIP_MAT *gcge_hip_mat_create_grid (int nrows, const int *rowptr, const int *colidx, const double *val,
		int nx, int ny, int nz, const int *box_of_row);
/* a whole matrix (one rank) whose rows stay as given: the row order search of gcge_hip_mat_create is not run and the order of another
 * live matrix of the same size is not adopted; gcge_hip_mat_row_order reports "as given".  What MultiGridCreate uploads the coarse
 * levels of a MIS-2 hierarchy with (below).                                                                                     */
GCGE_HIP_MAT *gcge_hip_mat_create_as_given (int nrows, const int *rowptr, const int *colidx, const double *val);
/* A whole square matrix (one rank) from DEVICE-resident CSR arrays (csrc/hip/mat_device.hip): nrows + 1, nnz and nnz entries, columns
 * ascending within a row, complete when the call is made (the caller synchronises its producer).  The call runs on gcge_hip_stream()
 * and synchronises itself; the handle owns copies, so the arrays may be freed afterwards.  Malformed input returns NULL with one
 * line on stderr — checked on the device in this order: rowptr[0] == 0, rowptr non-decreasing, rowptr[nrows] == nnz (reads rowptr
 * only), then every column in [0, nrows) (reads colidx[0 .. nnz) by position); nothing is addressed through an unchecked value.
 * The CSR and pad-8 copies are made on the device, and so is the search for a pattern table: a 64-bit hash per row, the classes of
 * equal hashes in a small table (only a row whose hash differs from its predecessor's touches it), every row verified entry by
 * entry, as bits, against the first row of its class, ids by first occurrence; the table itself is then built by the host code
 * gcge_hip_mat_create uses (csrc/hip/pattern_table.h) from the class representatives, so pid / table / spans are those of the host
 * path bit for bit.  The handle is then what gcge_hip_mat_create_as_given returns for the same arrays: rows as given, the identity
 * order of its size.  The matrix is downloaded once and handed to gcge_hip_mat_create (whose result this then is: by-offset
 * patterns, star / dense / tile forms, the row order search) when a re-ordered matrix of this size is live or when the device
 * search gives up: rows longer than 16, more classes than a table holds, a hash collision, tile mode 2.
 * One difference from the host search: rows are equal here when their lengths and all their entries agree as bits; the host's
 * comparison with the previous row's pattern also merges an EMPTY row with a preceding row whose only entries are explicitly
 * stored (offset 0, +-0.0).  Matrices without explicitly stored zeros on the diagonal are not affected.
 * gcge_hip_mat_device_stats: since load, out[0] matrices analysed on the device, out[1] fall-backs to the host path, out[2] those
 * caused by a hash collision, out[3] bytes copied device to host by these constructors.                                          */
GCGE_HIP_MAT *gcge_hip_mat_create_device (int nrows, long nnz, const int *d_rowptr, const int *d_colidx, const double *d_val);
void gcge_hip_mat_device_stats (long out[4]);
/* New values for a LIVE handle, in place (csrc/hip/mat_values.hip): d_val holds nnz new values for the entries of the CSR arrays the
 * handle was created from, in the caller's order — a DEVICE array, complete when the call is made (the caller synchronises its
 * producer).  For a sequence of nearby operators on one sparsity structure (an SCF loop, a parameter sweep): rowptr, colidx, the pad-8
 * index arrays, pid, the table's offsets, spans and the chain layout stay; only what holds values is re-derived, on the device.  The
 * call runs on gcge_hip_stream() and synchronises it before it returns; the array may be freed afterwards.
 *   0    updated: every product, CG pass and residual through the handle is now that of (rowptr, colidx, d_val).
 *   1    declined: NOTHING of the handle was written (all checks run before the first store); the caller re-creates the matrix.
 *   < 0  bad arguments (NULL handle or array, nnz != gcge_hip_mat_nnz (A)); nothing written.
 * A whole square matrix on one rank, or a ROW SLAB (halo columns, row_begin != 0, a halo plan of any kind: its own bullet below).  The
 * rows of a whole matrix may be as given or re-ordered inside the handle (gcge_hip_spmm_reorder_mode; its own bullet below);
 * d_val is in the CALLER's entry order either way.  What becomes of the handle:
 *   CSR + pad-8 only (no pattern, star, dense or tile form): d_val and the pad-8 values are rewritten, any values; form unchanged.
 *   offsets-only table + per-row values (the "+values" forms of gcge_hip_mat_spmm_form): the same, and the per-row values are
 *     re-scattered by the slot rule of the upload (gcge_pat_value_slot, csrc/hip/pattern_table.h); form unchanged.
 *   value table, classes still uniform (all rows of a class agree, as bits, on the new value of every present slot, none of them
 *     +-0.0): d_val, the pad-8 values and the values of the table's present slots are rewritten; pid, offsets and spans are
 *     untouched, so chain, chain2 and the ring sweep are kept.
 *   value table of at most 8 slots, anything else: d_val and the pad-8 values are rewritten and the handle BECOMES the "+values" form
 *     of the table it has (per-row values allocated and filled by the slot rule; gcge_hip_mat_spmm_form then reports
 *     spmm_pattern+values / spmm_pattern_chain2+values).  There is no way back: a later uniform update re-scatters the per-row values.
 *   star + blocks, or blocks alone (spmm_star+spmm_dense+spmm_pad8, spmm_dense+spmm_pad8), created while gcge_hip_mat_keep_value_maps
 *     was on: the handle kept, on the device, where each stored value came from (csrc/hip/value_maps.h), and the update replays that
 *     (csrc/hip/mat_values_forms.hip): d_val and the pad-8 copy as above, the star's diagonal gathered, the star's remainder formed in a
 *     scratch as "entry minus coefficient" with the rounding of the upload, the block values of every layer and the pad-8 remainder
 *     gathered from it (without a star: from d_val), pads +0.0.  Form, split, blocks, layers and lists are unchanged.  The star's
 *     coefficients are fixed for the life of the handle: an entry that sits at a star position and equalled the coefficient at
 *     creation (it has no slot of its own) must keep those bits.  Every other entry is free, the diagonal any value but NaN.
 *   a handle that re-ordered its rows (gcge_hip_mat_row_order is not "as given"), created while gcge_hip_mat_keep_value_maps was on: it
 *     kept, on the device, which entry of the caller's arrays sits at each position of its own CSR (gcge_hip_mat_entry_map bytes, 4 per
 *     entry).  The update gathers d_val through that map into a block of nnz doubles from the back-end's pool — a TRANSIENT 8 bytes per
 *     entry, for the duration of the call — and then proceeds by the bullet above that fits the handle's form, on that block; the gather
 *     writes the block only, so a decline still leaves the handle untouched.  The block returns to the pool after the call's last
 *     synchronisation.
 *   a row slab: d_val holds one value per entry of the LOCAL arrays the slab was created from, in their order (gcge_dist_localize only
 *     renames columns, a slab never re-orders its rows), and the update proceeds by the bullet above that fits the handle's form: every
 *     stored copy of a value on a slab derives from the rank's own rows.  A star or dense slab needs its value maps like a whole matrix
 *     (gcge_hip_mat_keep_value_maps on when the slab was created, by whichever constructor).  The call is RANK-LOCAL and
 *     COLLECTIVE-FREE: no exchange, no all-reduce, and its return value is this rank's alone.  The rule for callers: reduce the return
 *     codes over the ranks, and if ANY rank declined, EVERY rank frees its slab and creates it again (creation is collective; a rank
 *     that accepted holds the new values, one that declined the old ones).  A halo exchange moves X, not matrix values, but an update
 *     must not overlap a split product: the back-end's stream and, under a native (RCCL) halo plan, its transfer stream are
 *     synchronised before the first store.
 *   declined (1): a value table of 16 slots whose classes do not stay uniform; a row whose count of present table slots (table value
 *     != 0.0) differs from its length, i.e. an explicitly stored +-0.0; under a star, a pinned entry whose new value differs in bits
 *     from its coefficient (a rescaled Laplacian, say) or a NaN on the diagonal; and, decided from the handle alone before d_val is
 *     read, a star or dense handle WITHOUT value maps (the switch was off at creation: the default), a dense form whose remainder is
 *     tiled, any handle with a tile form, a rectangular handle, a re-ordered handle WITHOUT an entry map (the switch was off at
 *     creation).  Every check runs before the first store: a decline has written nothing on that rank.
 * A conversion changes the K1 form between two solves.  Nothing in the back-end keeps a record of a handle's form across calls: the
 * fused CG plans every call from the handle (cg_plan, block_pcg.hip), its parked blocks are keyed by row count and row order, and
 * mat_product.hip reads the handle at every product.  A multigrid hierarchy built from the handle BEFORE an update belongs to the old
 * operator until gcge_hip_multigrid_refresh (below) has given its coarse levels the new Galerkin products; the harness creates and
 * destroys its hierarchy inside every solve.
 * gcge_hip_mat_update_stats: since load, out[0] updates that kept the form, out[1] of those value-table rewrites, out[2] conversions
 * to "+values", out[3] declines, out[4] bad-argument returns, out[5] bytes copied device to host by updates — one flag word per
 * update that has a table or a star, whatever the size of the matrix.  gcge_hip_mat_device_stats is not touched.  An accepted update
 * of a star or dense handle counts in out[0], a decline in out[3]; gcge_hip_mat_update_form_stats adds out[0] star handles updated,
 * out[1] dense handles updated, out[2] declines by a pinned entry, out[3] declines by a NaN diagonal (an update that shows both counts
 * in both).                                                                                                                          */
int  gcge_hip_mat_update_values_device (GCGE_HIP_MAT *A, long nnz, const double *d_val);
void gcge_hip_mat_update_stats (long out[6]);
void gcge_hip_mat_update_form_stats (long out[4]);
/* Value maps, kept on request only.  gcge_hip_mat_keep_value_maps (on): process-wide, read when a matrix is created (like
 * gcge_hip_spmm_reorder_mode), default 0; returns the setting it replaces.  With 0 nothing is kept and a star or dense handle
 * declines every update.  With 1 a handle
 * that takes the star or the dense form also keeps the provenance of its stored values on the device; forms, split, blocks, layers,
 * lists and every stored value array are bit-identical to those of the switch off.  Row slabs keep them like whole matrices (the maps
 * index the entries of the local arrays; halo columns and the box of a masked grid only decide WHERE a value is stored).  gcge_hip_mat_value_maps: the bytes of maps a handle holds (0: none) — 4 per block slot and
 * pad-8 remainder slot; under a star also 1 per CSR entry, 4 per row and 5 per entry of the star's remainder.  The first update of a
 * star handle also allocates, and keeps, a scratch of 8 bytes per entry of the star's remainder.
 * gcge_hip_value_maps_selfcheck (host only, no device; tests): the forms and maps built from val0 (dense_mode: gcge_hip_spmm_dense_mode
 * for the duration of the call), the maps replayed on val1 through value_maps.h, star + diagonal + blocks + remainder expanded back into
 * per-row sums per column and compared with the CSR rows of val1.  Returns the number of differing entries, (row, column) pairs
 * (0: equal), -1: neither a star nor a dense form, -2: an update to val1 would be declined.  out[0] forms found (1 star, 2 blocks, 3 both), out[1] layers of blocks,
 * out[2] pinned entries, out[3] bytes of maps.  _grid: with the masked grid of gcge_hip_mat_create_grid named.
 * _slab: a row slab with LOCAL columns (the arguments of gcge_hip_star_selfcheck_slab; box_of_local_col != NULL: a slab of a masked grid,
 * the box index of every local column, own rows then halo rows), asked of the stored values themselves: everything the maps built from
 * val0 give on val1 — diagonal, the star's remainder, every block and pad-8 slot — against the split and block form built directly
 * from val1, as bits.  Returns the number of differing stored values; -1 / -2 as above; out[3] = entries of the star's remainder that
 * sit in halo columns.
 * The same switch makes a handle that RE-ORDERS its rows (gcge_hip_mat_create under gcge_hip_spmm_reorder_mode, a later matrix of the
 * same size that adopts the live order, the host path gcge_hip_mat_create_device falls back to) keep its entry map on the device:
 * 4 bytes per entry (1.4 GB at 350 M entries), freed with the handle.  gcge_hip_mat_entry_map: the bytes of entry map a handle holds
 * (0: none); gcge_hip_mat_value_maps does not count them.  With the switch off such a handle is what it is without this record.
 * gcge_hip_reorder_entry_map (host only, no device; tests): the routine the upload re-orders with, on the caller's arrays: perm[new]
 * = old (n ints); rowptr_new (n + 1 ints) / colidx_new (rowptr[n] ints): P A P^T with ascending columns; emap[q] (rowptr[n] ints):
 * the index in colidx of the entry at position q of colidx_new.  0: done (n = 0: rowptr_new[0] = 0); -1: perm is no permutation.    */
int  gcge_hip_mat_keep_value_maps (int on);
long gcge_hip_mat_value_maps (const GCGE_HIP_MAT *A);
long gcge_hip_mat_entry_map (const GCGE_HIP_MAT *A);
int  gcge_hip_reorder_entry_map (int n, const int *rowptr, const int *colidx, const int *perm, int *rowptr_new, int *colidx_new, int *emap);
long gcge_hip_value_maps_selfcheck (int nrows, const int *rowptr, const int *colidx, const double *val0, const double *val1, int dense_mode,
                                    long out[4]);
long gcge_hip_value_maps_selfcheck_grid (int nrows, const int *rowptr, const int *colidx, const double *val0, const double *val1, int dense_mode,
                                         int nx, int ny, int nz, const int *box_of_row, long out[4]);
long gcge_hip_value_maps_selfcheck_slab (int nrows, int ncols_local, long row_begin, long nglobal, const int *ghost, const int *rowptr,
                                         const int *colidx, const double *val0, const double *val1, int dense_mode, int nx, int ny, int nz,
                                         const int *box_of_local_col, long out[4]);
/* A matrix of that kind that names NO geometry (read from a file: gcge_load_matrix_market, gcge_load_petsc_binary) gets it
 * recovered at upload by gcge_hip_mat_create itself: x lines from the (r, r + 1) couplings, planes and the shifts between
 * lines / planes from the votes of the star rows' + y / + z neighbours.  A wrong guess costs speed, never the result (the
 * remainder takes every difference); on = 0 switches the recovery off (measurements).                                         */
void gcge_hip_spmm_star_infer (int on);
/* The geometry a one-rank handle carries, whatever K1 form its matrix took: 0 none, 1 named by the caller
 * (gcge_hip_mat_create_grid), 2 recovered at upload (and the grid form built on it).  dims[3] and box_of_row[nrows] (may be
 * NULL) are filled when there is one.  MultiGridCreate coarsens such a matrix by the 2 x 2 x 2 cells of its box (below).     */
int  gcge_hip_mat_geometry (const GCGE_HIP_MAT *A, int *dims, int *box_of_row);
/* Row-partitioned use (one process per GPU): localize the slab with gcge_dist_localize
 * (include/gcge_problems.h), create it with ncols_local = nrows + nghost, then install the halo
 * plan.  exchange(sendbuf, recvbuf, ncols, ctx) must deliver, for every peer, rows
 * [send_off[p], +send_cnt[p]) x ncols of sendbuf into the peer's recvbuf at its ghost offset for
 * this rank (both buffers row-major with ncols columns; device memory for this back-end).    */
typedef void (*gcge_halo_exchange_fn) (double *sendbuf, double *recvbuf, int ncols, void *ctx);
GCGE_HIP_MAT *gcge_hip_mat_create_local (int nrows, int ncols_local, int nglobal, int row_begin,
		const int *rowptr, const int *colidx, const double *val);
/*     the same with the global rows behind the halo columns (ascending, as gcge_dist_ghosts lists them) and the global size:
 *     a slab of a grid matrix cut on plane boundaries then keeps the plane sweep of spmm_star.hip — the planes below and
 *     above the slab are found among its halo rows (gcge_hip_mat_create_slab passes them by itself)                      */
GCGE_HIP_MAT *gcge_hip_mat_create_local_ghosts (int nrows, int ncols_local, int nglobal, int row_begin,
		const int *rowptr, const int *colidx, const double *val, const int *ghost_global);
void gcge_hip_mat_set_halo (GCGE_HIP_MAT *A, int nglobal, int nsend, const int *send_rows,
		double *sendbuf, double *recvbuf, int buf_cols, gcge_halo_exchange_fn fn, void *ctx);
/*     optional split form of the exchange: begin posts the transfers of the packed rows and returns, end returns
 *     when recvbuf is complete; the back-end then multiplies the rows that touch no halo column in between      */
void gcge_hip_mat_set_halo_async (GCGE_HIP_MAT *A, gcge_halo_exchange_fn begin, void (*end) (void *ctx));
void gcge_hip_set_halo_overlap (int on);
void gcge_hip_mat_destroy (GCGE_HIP_MAT *A);
/* ---- multigrid (csrc/hip/multigrid.hip): OPS_HIP_Set fills ops->MultiGridCreate / MultiGridDestroy (reference slots
 * src/ops.h:134-139; what app/app_slepc.c:648-728 gets from PETSc GAMG): the aggregation hierarchy of include/gcge_multigrid.h,
 * built on the device by default (gcge_hip_multigrid_mode below; 2 x 2 x 2 cells of a detected grid, greedy aggregates
 * otherwise, A_{l+1} = scale P^T A_l P; gcge_mg_set_defaults), every level is uploaded like any other matrix, and the fused
 * block CG is the smoother of BlockAMG for this table (GCGE_BACKEND.amg_smoother_setup, include/gcge_ops.h).
 * One rank only.  A prolongation is a RECTANGULAR matrix handle: MatDotMultiVec applies P (rows of level l x rows of level
 * l + 1), MatTransDotMultiVec its transpose (the restriction of src/ops_multi_grid.c:95-113); MultiVecCreateByMat of it gives
 * blocks with its COLUMN count of rows (app_ccs.c:43).                                                                      */
GCGE_HIP_MAT *gcge_hip_mat_create_rect (int nrows, int ncols, const int *rowptr, const int *colidx, const double *val,
		const int *t_rowptr, const int *t_colidx, const double *t_val);      /* CSR of P and CSR of P^T */
GCGE_HIP_MAT *gcge_hip_mat_create_rect_csr (const GCGE_CSR *P);              /* the transpose is formed here */
double gcge_hip_multigrid_seconds (void);    /* host + upload time of the last MultiGridCreate */
/*     Where the hierarchy is built (whole matrices, one rank; row slabs always coarsen as below).  mode 0 (default): on the device
 *     (csrc/hip/mg_device.hip) from the handle's device CSR — grid detection from the sampled rows only, grid aggregates, members and
 *     the Galerkin products A_{l+1} = scale P^T A_l P on the device, P / P^T built there; graph levels download their CSR for the
 *     host aggregation (graph method 0, below); every coarse level is downloaded for gcge_hip_mat_create.  Bit-identical to mode 1, the host build
 *     (gcge_mg_build on the downloaded CSR), which mode 0 also falls back to when a level is out of the kernels' reach.         */
void gcge_hip_multigrid_mode (int mode);
int  gcge_hip_multigrid_get_mode (void);
/*     Masked grids (a handle with a geometry whose box holds more points than the matrix has rows: gcge_hip_mat_geometry): every
 *     level is coarsened by the 2 x 2 x 2 cells of its bounding box (gcge_mg_aggregate_masked / gcge_mg_build_masked,
 *     include/gcge_multigrid.h); the occupied cells in scan order are the next level, uploaded through gcge_hip_mat_create_grid
 *     with its own geometry, so its rows stay as given.  Mode 0 counts, numbers and lists the cells on the device from the
 *     device-resident box array (no part of the fine level comes back), mode 1 runs the host routine; identical hierarchies.
 *     on = 0: such a matrix is treated as one without a grid (greedy aggregates: the graph branch).  Default 1.
 *     Row slabs of a masked grid are not coarsened this way.                                                                   */
void gcge_hip_multigrid_masked_cells (int on);
int  gcge_hip_multigrid_get_masked_cells (void);
/*     Coarse levels without the host (grid and MIS-2 hierarchies of mode 0): on = 1 (default) hands every coarse A_l / B_l to
 *     gcge_hip_mat_create_device straight from the Galerkin output (MIS-2: its as-given variant); a level comes back only when that
 *     constructor falls back.  on = 0: every coarse level is downloaded and uploaded through the host constructors.  Identical
 *     hierarchies either way.  Masked and greedy-graph levels always take the host constructors.                                */
void gcge_hip_multigrid_device_levels (int on);
int  gcge_hip_multigrid_get_device_levels (void);
/*     the device aggregation of a masked grid for a host box array (tests, tools): agg, mem [nrows], ptr [nrows + 1], cbox [nrows]
 *     as gcge_mg_aggregate_masked and the members of every cell in ascending row order; returns the number of aggregates, < 0 for
 *     a geometry the host routine refuses                                                                                     */
int  gcge_hip_mg_aggregate_masked (const int dims[3], const int *box_of_row, int nrows, int *agg, int *ptr, int *mem, int *cbox, int cdims[3]);
/*     Matrices without a grid (FE matrices on tetrahedra, a matrix in an order the upload cannot undo, a masked grid with
 *     gcge_hip_multigrid_masked_cells (0)): gcge_mg_set_graph_method (include/gcge_multigrid.h) selects how they are aggregated.
 *     0 (default): the greedy host routine on the level's downloaded CSR, coarse levels through gcge_hip_mat_create.
 *     1: MIS-2 aggregation (gcge_mg_aggregate_mis2) by the kernels of csrc/hip/mg_aggregate.hip on the level's device CSR, inside the
 *     same level loop — the fine level never comes back, one int per round does; at most 64 rounds, after which the level is
 *     aggregated by the host routine on a downloaded CSR (GCGE_MG_TRACE says so).  Every coarse A_l and B_l of such a hierarchy, in
 *     mode 0 and in mode 1, goes up through gcge_hip_mat_create_as_given: P / P^T, the blocks of MultiVecCreateByMat (A_l) and the
 *     level's rows agree whatever gcge_hip_spmm_reorder_mode says; level 0 keeps the order of its handle.  Host routine, kernels and
 *     gcge_mg_build give the same hierarchy byte for byte.  The harness option is -gcge_amg_graph <0|1>.
 *     gcge_hip_mg_aggregate_graph runs the device routine on a handle's device CSR (tests, tools): agg, mem [nrows], ptr [nrows + 1]
 *     (the members of every aggregate in ascending row order); returns the number of aggregates, -1 when the rounds reached their
 *     cap, -2 bad arguments.  _csr: the same for host arrays.  gcge_hip_mg_graph_rounds: the rounds of the last device aggregation;
 *     gcge_hip_mg_graph_round_cap: the cap, 1 .. 64 (tests of the fall-back).                                                    */
int  gcge_hip_mg_aggregate_graph (const GCGE_HIP_MAT *A, double theta, int *agg, int *ptr, int *mem);
int  gcge_hip_mg_aggregate_graph_csr (int n, const int *rowptr, const int *colidx, const double *val, double theta, int *agg, int *ptr, int *mem);
int  gcge_hip_mg_graph_rounds (void);
void gcge_hip_mg_graph_round_cap (int cap);
/*     the last MultiGridCreate: seconds of its phases (detect, aggregate, Galerkin, transfers, coarse upload / analysis, other)
 *     and the bytes copied device to host; GCGE_MG_TRACE prints them                                                           */
void gcge_hip_multigrid_stats (double *seconds6, long *d2h_bytes);
/*     the device Galerkin product scale P^T A P on A's device CSR for a host aggregate map agg[nrows] (0 <= agg < nc): a host CSR
 *     (gcge_csr_free); 0 on success, 1 when it is out of the kernels' reach, < 0 bad arguments                                     */
int  gcge_hip_mg_galerkin (const GCGE_HIP_MAT *A, const int *agg_host, int nc, double scale, GCGE_CSR *Ac_out);
/*     The numeric half alone, for a coarse structure that exists: the values of scale P^T A P into d_va_c_out, entry by entry where
 *     d_rp_c / d_ci_c (nc rows, ascending columns) name them — the doubles gcge_hip_mg_galerkin_device and the host's gcge_mg_galerkin
 *     give for these values (one wave per coarse row, its columns staged in LDS and searched, the sums in walk order; no float atomics).
 *     A (nf rows) as device CSR, d_agg / d_ptr / d_mem the aggregate of every row and the members of every aggregate, device arrays.
 *     0: written.  1: an entry's coarse column is not in its coarse row — the structure does not belong to this matrix — or a coarse
 *     row holds more than 512 columns; d_va_c_out is then as it was.  One flag word comes back.
 *     gcge_hip_mg_galerkin_values: the same on A's device CSR for a host aggregate map and a host structure; va_c goes up as it is and
 *     comes back as the device function left it (< 0: bad arguments) — tests and tools.                                            */
int  gcge_hip_mg_galerkin_values_device (int nf, const int *d_rowptr, const int *d_colidx, const double *d_val, const int *d_agg, int nc,
		const int *d_ptr, const int *d_mem, double scale, const int *d_rp_c, const int *d_ci_c, double *d_va_c_out);
int  gcge_hip_mg_galerkin_values (const GCGE_HIP_MAT *A, const int *agg_host, int nc, double scale, const int *rp_c, const int *ci_c,
		double *va_c);
/*     A live hierarchy of MultiGridCreate after its level 0 took new values in place (gcge_hip_mat_update_values_device on A_array[0],
 *     and on B_array[0]): for l = 0 .. num_levels - 2 the values of level l + 1 are computed from level l's present values, P_l's
 *     aggregates and level l + 1's own structure (gcge_hip_mg_galerkin_values_device, with the scale the build used) and handed to
 *     gcge_hip_mat_update_values_device (A_{l+1}); the same for B with scale 1.0 when B_array is not NULL and holds a level 0.
 *     Nothing else of the hierarchy changes: P, P^T, structures, forms (but a value table that becomes "+values"), row orders.
 *       0     every level holds the Galerkin product of the level above it over the aggregates the hierarchy has.  On a grid or a
 *             masked grid, whose cells do not depend on the values, that is the hierarchy a fresh MultiGridCreate gives, bit for bit;
 *             aggregation over the graph (greedy or MIS-2) reads the off-diagonal values, so there a fresh build is the same
 *             hierarchy only while the off-diagonals are (a new diagonal) and may otherwise choose other aggregates.
 *       l>=1  level l was the first to decline — its in-place update (a star or dense level built without
 *             gcge_hip_mat_keep_value_maps (1) in force, a pinned star coefficient that moved, an explicit zero in a table row ...)
 *             or the structure check.  The levels below l are refreshed, those from l on keep their old values: still a usable
 *             preconditioner of a nearby operator, no longer the Galerkin hierarchy (with a B, A of level l may have been written
 *             when it is B that declines).  The caller destroys it and creates it again.
 *       -1    nothing was written: A_array is not a hierarchy of this back-end, num_levels is not its level count, a COARSE level whose
 *             handle re-ordered its rows (level 0 may: the hierarchy was built from its CSR in its own order and P_0's rows are numbered
 *             like it; it takes its new values as gcge_hip_mat_update_values_device states), a hierarchy of row slabs one of whose
 *             levels was created without the global rows behind its halo columns (gcge_hip_mat_create_local without _ghosts).
 *             gcge_hip_multigrid_refresh_check answers this much alone, 0 or -1, and writes nothing.
 *     A hierarchy of ROW SLABS is refreshed the same way, every rank its own levels: each coarse row of a slab level is scale x the sum
 *     over fine rows the rank owns (aggregates never cross a cut), so nothing is exchanged; MultiGridCreate keeps, per level, where every
 *     local column — halo columns through their owners' pairing — lands among the next level's local columns (gcge_mg_slab_colagg,
 *     include/gcge_multigrid.h: 4 bytes per local column on the device, freed with the hierarchy), and the numeric product uses the
 *     build's summation order: bit for bit the coarse slabs of a fresh build.  Coarse slabs with a star or dense form need their value
 *     maps (the switch on around MultiGridCreate).  No B below level 0 on slabs: A's levels only.  The call is RANK-LOCAL and
 *     COLLECTIVE-FREE and its return is this rank's; GCGE_AMGRefresh (include/gcge_solver.h) is the collective form: it agrees on the
 *     check before any rank writes and on the smallest declining level afterwards, so every rank sees the same return.
 *     Nothing outside the handles holds values derived from a level's matrix (the smoother's parked blocks are work space keyed by row
 *     count and row order), so a refreshed hierarchy needs no other reset.  gcge_hip_multigrid_refresh_stats: since load, out[0]
 *     refreshes that returned 0, out[1] calls that ended in a decline (l >= 1), out[2] levels written (A and B count separately),
 *     out[3] bytes copied device to host (one flag word per product, plus those of the in-place updates).                          */
int  gcge_hip_multigrid_refresh (void **A_array, void **B_array, void **P_array, int num_levels);
int  gcge_hip_multigrid_refresh_check (void **A_array, void **B_array, void **P_array, int num_levels);
void gcge_hip_multigrid_refresh_stats (long out[4]);
/*     a handle's device CSR (square, or P of a rectangular one) / the P^T triple of a rectangular one as a host copy (gcge_csr_free) */
int  gcge_hip_mat_to_csr (const GCGE_HIP_MAT *A, GCGE_CSR *out);
int  gcge_hip_mat_to_csr_t (const GCGE_HIP_MAT *A, GCGE_CSR *out);
/*     Row slabs (one rank per GPU): a slab that is whole planes of a detected grid (cut on any plane boundary) coarsens by itself
 *     (gcge_mg_build_slab, include/gcge_multigrid.h: local prolongations, coarse slabs with global columns); every coarse slab goes
 *     through the slab constructor — gcge_hip_mat_create_slab over RCCL by default, or the function registered here (a transport of
 *     the caller's: the torch.distributed callbacks of the tests).  MultiGridCreate needs the partition of all ranks:
 *     gcge_hip_mat_create_slab records it, other constructors call gcge_hip_mat_set_partition.  Collective.                     */
typedef GCGE_HIP_MAT *(*gcge_hip_slab_factory_fn) (const long *part, int world, int rank, const int *rowptr, const int *colidx_global,
		const double *val, int buf_cols, void *ctx);
void gcge_hip_set_slab_factory (gcge_hip_slab_factory_fn fn, void *ctx);     /* NULL: gcge_hip_mat_create_slab */
void gcge_hip_mat_set_partition (GCGE_HIP_MAT *A, const long *part, int world);
int  gcge_hip_mat_nrows (const GCGE_HIP_MAT *A);
long gcge_hip_mat_nnz (const GCGE_HIP_MAT *A);

/* ---- multi-GPU from C: RCCL inside the back-end (csrc/hip/rccl_comm.hip) ------------------------------------
 * One process per GPU.  Replaces what the reference does with MPI in its solver layers — MPI_Allreduce of every
 * Gram / dot result (src/ops_multi_vec.c:206-228, src/ops_lin_sol.c:313-321,361-369) — and in its distributed
 * back-ends (off-process part of X inside MatDotMultiVec, app/app_phg.c:292-359).
 *   rank 0:  gcge_hip_comm_unique_id(id);  hand the 128 bytes to every rank (MPI_Bcast, a file, torch.distributed ...)
 *   all:     gcge_hip_init(local_device); gcge_hip_comm_init(rank, world, id);   // also installs GCGE_COMM (gcge_ops.h)
 *            A = gcge_hip_mat_create_slab(part, rowptr, colidx_global, val, block_columns);   // collective
 *            OPS_HIP_Set(ops); ... the solver as on one GPU ...; gcge_hip_comm_finalize();                        */
#define GCGE_HIP_COMM_ID_BYTES 128
int  gcge_hip_comm_unique_id (void *id128);
int  gcge_hip_comm_init (int rank, int world, const void *id128);
void gcge_hip_comm_finalize (void);
int  gcge_hip_comm_rank (void);
int  gcge_hip_comm_size (void);
void gcge_hip_comm_stats (long *n_allreduce, long *n_exchange);
/*     in-place sum over the ranks of n doubles in DEVICE memory on the back-end's stream, nothing waited for      */
int  gcge_hip_comm_allreduce_device (double *d_buf, int n);
/*     1 if `comm` (GCGE_GetComm()) is the one gcge_hip_comm_init installed, i.e. device-side all-reduces are possible  */
int  gcge_hip_comm_is_native (const GCGE_COMM *comm);
/*     rows [part[rank], part[rank+1]) of a symmetric matrix, GLOBAL column indices (host CSR); part has world + 1
 *     entries.  Collective: builds the ghost list, the local numbering and the halo plan (who needs which rows) over
 *     RCCL; products then move buf_cols columns of halo rows per grouped ncclSend/ncclRecv, event-ordered            */
GCGE_HIP_MAT *gcge_hip_mat_create_slab (const long *part, const int *rowptr, const int *colidx_global,
		const double *val, int buf_cols);
/*     ... of a matrix on a MASKED grid (the real-space DFT matrices behind BASELINE config 5 on more than one device; reference
 *     test/submit.sh:9-15): box_of_global_row[r] = x + nx (y + ny z) of GLOBAL row r (rows in scan order), the partition cut between
 *     grid lines (gcge_amd.dist.partition_lines).  The slab keeps the plane sweep: own and halo rows are found through one line table.
 *     gcge_hip_mat_create_local_ghosts_grid: the same for callers that build the slab themselves (gcge_hip_mat_create_local_ghosts
 *     with four more arguments): the box index of every LOCAL column (own rows, then halo rows); NULL: no geometry               */
GCGE_HIP_MAT *gcge_hip_mat_create_slab_grid (const long *part, const int *rowptr, const int *colidx_global, const double *val,
		int buf_cols, int nx, int ny, int nz, const int *box_of_global_row);
GCGE_HIP_MAT *gcge_hip_mat_create_local_ghosts_grid (int nrows, int ncols_local, int nglobal, int row_begin, const int *rowptr,
		const int *colidx, const double *val, const int *ghost_global, int nx, int ny, int nz, const int *box_of_local_col);
/*     the same for a slab matrix that already has LOCAL column indices (gcge_hip_mat_create_local) and a plan computed
 *     elsewhere: npeer slabs, peer[q] = communicator rank owning slab q, rows shipped to / received from it, the
 *     local rows to ship grouped by destination slab                                                               */
int  gcge_hip_mat_set_halo_rccl (GCGE_HIP_MAT *A, int nglobal, int npeer, const int *peer, const int *send_cnt,
		const int *recv_cnt, const int *send_rows, int buf_cols);

/* ---- block-of-vectors transfers (tests, final eigenvectors) ------------------- */
/* columns [c0,c1) <-> host column-major array with leading dimension ldh (>= nrows) */
void gcge_hip_mv_to_host   (void **mv, int c0, int c1, double *host, long ldh);
void gcge_hip_mv_from_host (void **mv, int c0, int c1, const double *host, long ldh);
/* columns [c0,c1) -> DEVICE row-major array: d_out[r * ldo + (j - c0)] (ldo >= c1 - c0), rows in the caller's order whatever order the
 * block lives in; one gather kernel on gcge_hip_stream(), which the call synchronises                                              */
void gcge_hip_mv_to_device (void **mv, int c0, int c1, double *d_out, long ldo);
/* columns [c0,c1) <- DEVICE array with element strides: column j of the caller's row r is d_in[r * row_stride + (j - c0) * col_stride].
 * Rows are in the caller's order whatever order the block lives in (device row i takes the caller's row perm[i], as
 * gcge_hip_mv_from_host); only the block's own nrows rows and the columns of the range are written.  A held-back column scaling is
 * applied first, then overwritten.  Runs on gcge_hip_stream(), which the call synchronises; the caller synchronises its producer.
 * Required (the call aborts otherwise): 0 <= c0 <= c1 <= ncols; with work to do, d_in != NULL, both strides >= 1, no two (r, j)
 * alias — col_stride == 1 && row_stride >= m, row_stride == 1 && col_stride >= nrows, row_stride >= m * col_stride or
 * col_stride >= nrows * row_stride (m = c1 - c0) — and the source's address range lies outside the block's allocation.
 * Rows contiguous (col_stride == 1) is the block-stream form; columns contiguous (row_stride == 1) of a block in the caller's order
 * goes through an LDS transpose; every other shape takes an element kernel.                                  */
void gcge_hip_mv_from_device (void **mv, int c0, int c1, const double *d_in, long row_stride, long col_stride);
int  gcge_hip_mv_nrows (void **mv);
int  gcge_hip_mv_ncols (void **mv);
double *gcge_hip_mv_device_ptr (void **mv, long *ld);

/* 0: MultiVecSetRandomValue draws glibc rand() on the host in the reference's order
 *    (app/app_lapack.c:322-333) and uploads — bit-identical start vectors;
 * 1: counter-based generator on the device (for n ~ 1e7, where 2e9 rand() calls
 *    would dominate the run).                                                      */
void gcge_hip_set_random_mode (int mode, unsigned long long seed);

/* ---- fused block CG behind ops->MultiLinearSolver ------------------------------
 * Same recurrence/stopping rules as BlockPCG (src/ops_lin_sol.c:140-437) with the vector
 * work of an iteration fused into four launches.  GCG uses it through the reference's
 * user_defined_multi_linear_solver = 1 hook (ops_eig_sol_gcg.c:584-618, test_app_ccs.c:109-120):
 * call this once, then run the harness with flag = 1.                                  */
void gcge_hip_bpcg_setup (struct OPS_ *ops, int max_iter, double rate, double tol, const char *tol_type);
void gcge_hip_bpcg_stats (long *spmm_calls, long *spmm_cols, int *last_niter);
/* optional, after gcge_hip_bpcg_setup: create the solver's own blocks (r, p, w and the ring of direction slots) for systems with the
 * rows of mv_like and up to ncols right-hand sides now rather than inside the first solve — the reference hands BlockPCG its blocks
 * from EigenSolverCreateWorkspace_GCG, before the harness starts its timer (test/test_eig_sol_gcg.c:89-143).  Returns the ring
 * length (>= 1), -1 when ops->MultiLinearSolver is not this solver.  Collective when a communicator exists.                    */
int  gcge_hip_bpcg_prepare (struct OPS_ *ops, void *mat, void **mv_like, int ncols);
/*     tol_type: "abs", "rel" or "user" (src/ops_lin_sol.c:175-197; "user": scales from GCGE_LINSOL_ARGS.user_scale).
 *     Residual of the recompute form: 0 automatic (not stored where rate >= 1e-4 and max_iter <= 100), 1 never stored
 *     (r_k = p_k - beta_{k-1} p_{k-1} rebuilt from the ring), 2 always stored                                         */
void gcge_hip_bpcg_residual_form (int form);
long gcge_hip_bpcg_surplus_iters (void);   /* iterations enqueued after the last column retired (device-scalar loop) */
/* iterations the fused solver ran in its recompute form (pattern matrices: the product A p is formed twice per
 * iteration and never stored, gcge_hip_cg_pass1_mv / gcge_hip_cg_pass2_mv); GCGE_CG_NO_RECOMPUTE=1 switches it off */
long gcge_hip_bpcg_recompute_iters (void);
/* of those, iterations whose scalars (alpha, beta, stopping test) were computed on the device, without a host round trip
 * inside the iteration (single rank or RCCL inside the back-end; GCGE_CG_HOST_SCALARS=1 switches it off)            */
long gcge_hip_bpcg_device_scalar_iters (void);
/* iterations of that device-scalar loop with the product STORED (matrices without a pattern form, no shift: product + column sums
 * left on the device by gcge_hip_spmm_dot2_dev, then one sweep over w and the directions); GCGE_CG_STORED_HOST=1: host scalars */
long gcge_hip_bpcg_stored_dev_iters (void);
/* solves with right-hand sides b = x diag(scale) (GCGE_LINSOL_ARGS.rhs_scale) on such a matrix that started as product + ONE sweep
 * (r = x diag(scale) - A x, p0 = r, r.r) instead of forming b; GCGE_CG_NO_FUSED_START=1 switches it off */
long gcge_hip_bpcg_fused_starts (void);
/*     y[:, cy : cy + m) = A x[:, cx : cx + m) with d_out[0, m) = x.y and d_out[m, 2m) = y.y (local rows) left on the device, nothing
 *     waited for; -1 (nothing touched): odd widths / offsets or unaligned blocks                                                */
int gcge_hip_spmm_dot2_dev (void *mat, void **x, void **y, int cx, int cy, int m, double *d_out);
int gcge_hip_spmm_dot2_dev_ok (void *mat, void **x, void **y, int cx, int cy, int m);   /* 1: it takes these operands */
/* columns the fused solver streamed, summed over its iterations, and how many of them were still active */
void gcge_hip_bpcg_column_stats (long *col_iters, long *active_col_iters);
/* CG iterations and host wall time spent inside the fused solver since the last reset (ms per CG iteration) */
void gcge_hip_bpcg_time_stats (long *iters, double *seconds, int reset);
void gcge_hip_bpcg_release (struct OPS_ *ops);

/* ---- live measurement of the K1 launches (HIP events on the launch stream) ---------- */
void gcge_hip_profile_enable (int on);        /* also clears what was recorded            */
long gcge_hip_profile_spmm (int ncols, double *total_ms, double *total_alg_bytes);
/*     by kind: 0 = MatDotMultiVec products (what gcge_hip_profile_spmm returns), 2 / 3 = first / second pass of a
 *     block-CG iteration in its recompute form (below); ncols == 0: all widths                                    */
long gcge_hip_profile_kind (int kind, int ncols, double *total_ms, double *total_alg_bytes);
/*     ... restricted to launches on matrices of nrows local rows (0: all): with BlockAMG the same kernels run on every level of the
 *     hierarchy, and a roofline figure belongs to one problem size                                                              */
long gcge_hip_profile_kind_rows (int kind, int ncols, long nrows, double *total_ms, double *total_alg_bytes);

/* ---- K7: small dense symmetric eigensolver on the device (replaces dsyevx, src/ops_eig_sol_gcg.c:1201-1203) ------
 * all eigenpairs of the symmetric n x n matrix a (HOST, column-major, ld lda; triangle `uplo` is read): w ascending,
 * z (HOST, ld ldz) orthonormal eigenvectors.  Householder tridiagonalisation and the accumulation of Q on the device,
 * implicit QL on the host with recorded rotations, replayed on the device (csrc/hip/eig_device.hip).  0 on success.  */
int gcge_hip_symeig (char uplo, int n, const double *a, int lda, double *w, double *z, int ldz);
long gcge_hip_symeig_calls (void);   /* calls so far: offered by the HIP table's back-end record only: the CPU oracle never gets here */

/* ---- raw kernels (what the slots launch; exposed for micro-benchmarks) --------- */
/* K1  Y[:,0:m) = A X[:,0:m);  x/y point at (row 0, first column); see csrc/hip/spmm*.hip */
int gcge_hip_csr_spmm  (int nrows, const int *d_rowptr, const int *d_colidx, const double *d_val,
		const double *d_x, long ldx, double *d_y, long ldy, int ncols, void *stream);
int gcge_hip_pad8_spmm (int nrows, const int *d_orp, const int *d_pcol, const double *d_pval,
		const double *d_x, long ldx, double *d_y, long ldy, int ncols, void *stream);
/*     the sampled outer product on a CSR pattern (csrc/hip/sample_outer.hip): for every stored entry e of row i with column
 *     j = d_colidx[e]:  d_out[e] = alpha * sum_{c < k} w[c] U[i, c] V[j, c] — what the gradients of eigenvalues and of a solve
 *     with respect to the matrix values are (gcge_amd/grad.py).  U (nrows rows) and V (a row for every column index) are
 *     row-major device blocks, ldu, ldv >= k; d_u == d_v is legal; d_w: k doubles on the device, or NULL for all ones; d_out
 *     in the entry order of the arrays given.  Any k >= 1 and any row lengths; no atomics, and the order of summation is
 *     fixed by k and by whether 16-byte loads apply (even ldu and ldv, d_u and d_v on 16 bytes), so two runs give the same
 *     bits.  -1, before anything touches the device, for nrows < 0, k < 1, ldu < k, ldv < k or (nrows > 0) a NULL array other
 *     than d_w; 0 without a launch for nrows == 0 (rows that are all empty: the launch writes nothing); else a hipError_t.  */
int gcge_hip_csr_sample_outer (int nrows, const int *d_rowptr, const int *d_colidx,
		const double *d_u, long ldu, const double *d_v, long ldv, int k,
		const double *d_w, double alpha, double *d_out, void *stream);
/* K2  G(k x m, row-major on device, ld m) = Q[:,0:k)^T P[:,0:m)  over nrows rows (MFMA f64) */
int gcge_hip_gram (int nrows, const double *d_q, long ldq, int k, const double *d_p, long ldp, int m,
		double *d_g, void *stream);
/*     blocks of vectors freed through MultiVecDestroy are kept by size and reused (hipMalloc/hipFree of multi-GB
 *     blocks cost ~0.3 s each); release returns them to the driver, enable(0) switches the cache off            */
void gcge_hip_pool_release (void);
void gcge_hip_pool_enable (int on);
size_t gcge_hip_pool_cached_bytes (void);
/*     row orders (csrc/hip/mat_upload.hip, reorder.hip): a whole matrix (gcge_hip_mat_create, one rank) that shows neither a pattern
 *     form nor a grid in the order it arrives in is re-ordered inside the handle — grid coordinates recovered from the graph of a
 *     star stencil (scan order: the plane sweep applies again) or reverse Cuthill-McKee.  Blocks of vectors created for it live in
 *     the same order; gcge_hip_mv_to_host / from_host translate; a later matrix of the same size (B) adopts the order.
 *     mode: 0 automatic (>= 65 536 rows), 1 every matrix without a fast form (tests), -1 never                                   */
void gcge_hip_spmm_reorder_mode (int mode);
const char *gcge_hip_mat_row_order (const GCGE_HIP_MAT *A);      /* "as given" or what the upload did */
long gcge_hip_reorder_star_grid (int n, const int *rowptr, const int *colidx, const double *val, int *dims, int *box_of_row);   /* host only */
int  gcge_hip_reorder_rcm (int n, const int *rowptr, const int *colidx, int *perm);                                            /* host only: perm[new] = old */
void gcge_hip_set_spmm_path (int path);   /* 0 automatic (pattern > star rows + block form of the rest > dense blocks + remainder > pad-8 > CSR), 2 no pattern kernels (nor the star sweep), 3 pad-8 / CSR only, 4 no dense blocks */
/*     tile path (csrc/hip/spmm_tile.hip): matrices without a pattern form whose rows are long enough (>= 12 entries on
 *     average; automatic rule: see mode) are additionally kept as row tiles (bricks of a detected grid, or runs of rows) with 16-bit positions into
 *     the tile's list of X rows, which the kernel stages in LDS once per 8-column pass.  mode: 0 automatic (the remainder
 *     of a matrix whose long rows went into dense blocks, when it has short rows on a detected grid), 1 every matrix
 *     without a pattern form, 2 every matrix, -1 never (takes effect at the next gcge_hip_mat_create*)                  */
void gcge_hip_spmm_tile_mode (int mode);
/*     supernode path (csrc/hip/spmm_dense.hip): row sets that share a column set (the dense blocks real-space DFT
 *     Hamiltonians keep per atom) are found at upload and multiplied as dense blocks on FP64 MFMA, the rest of the
 *     matrix through the generic kernels.  mode: 0 automatic (seeds: rows of >= 96 entries, blocks must hold >= 10 % of
 *     the non-zeros), 1 rows of >= 24 entries may seed (tests), -1 never                                                */
void gcge_hip_spmm_dense_mode (int mode);
long gcge_hip_dense_selfcheck (int nrows, int ncols_local, const int *rowptr, const int *colidx, const double *val,
		int min_len, long *nblocks, double *share, double *fill);   /* host-only: blocks + remainder == CSR, bit for bit */
/*     grid path (csrc/hip/spmm_star.hip): matrices without a pattern form on a lexicographic 3-D grid whose rows are mostly
 *     ONE star stencil of arm length <= 6 with a diagonal of their own (the finite-difference Laplacian + local potential of
 *     real-space DFT Hamiltonians): those rows leave the CSR arrays and are multiplied by a plane sweep (z-neighbours in
 *     registers, x / y arms from LDS, 2.5 X rows fetched per row, no matrix stream), the other rows keep all their entries
 *     and take the block form where they hold blocks, a listed remainder otherwise; a matrix whose rows are ALL such stars keeps
 *     the form with an empty remainder (at least half of the rows must be).  Row slabs (one process per GPU) keep the form when
 *     they are whole grid planes: the planes below / above come from the halo rows, and with a split exchange the planes that
 *     need none are swept while the halo is in flight (reference: app/app_phg.c:307-357).  mode: 0 automatic, -1 never   */
void gcge_hip_spmm_star_mode (int mode);
long gcge_hip_star_selfcheck (int nrows, int ncols_local, const int *rowptr, const int *colidx, const double *val,
		long *out /* nx, ny, nz, arm length, star rows */);   /* host-only: star rows + remainder == CSR, bit for bit; -1: no such form */
/*     the same for a row slab with LOCAL columns (halo column nrows + i = global row ghost[i]): additionally checks that the
 *     sweep's own addressing of the planes below / above lands on the halo rows the CSR arrays name.  out[5..10] = first /
 *     last + 1 plane of the slab, of the planes the sweep may load, first halo row of the planes below / above (-1: none) */
long gcge_hip_star_selfcheck_slab (int nrows, int ncols_local, long row_begin, long nglobal, const int *ghost,
		const int *rowptr, const int *colidx, const double *val, long *out);
/*     the same for a matrix on a masked grid (gcge_hip_mat_create_grid)                                                  */
long gcge_hip_star_selfcheck_grid (int nrows, const int *rowptr, const int *colidx, const double *val, int nx, int ny, int nz,
		const int *box_of_row, long *out);
/*     the geometry gcge_hip_mat_create recovers for a matrix on a masked grid that names none (host only): dims[0..2] = nx, ny,
 *     nz of the bounding box, box_of_row[r] = x + nx (y + ny z); 1 found, 0: the rows are no such domain in scan order    */
int  gcge_hip_star_infer_grid (int nrows, const int *rowptr, const int *colidx, int *dims, int *box_of_row);
/*     grid of a matrix whose rows are mostly one star stencil, from a slab of its rows with GLOBAL columns (host only;
 *     what a partitioner needs to cut on plane boundaries).  out[0..3] = nx, ny, nz, arm length; 1 found, 0 none         */
int  gcge_hip_star_grid (int nrows, long row_begin, long nglobal, const int *rowptr, const int *colidx_global,
		const double *val, long *out);
int  gcge_hip_mat_star_stats (const GCGE_HIP_MAT *A, long *out /* nx, ny, nz, arm length, star rows, rows, first / last + 1 plane of the slab */);   /* 0: the matrix has no grid form */
/* masked grids (gcge_hip_mat_create_grid, or a geometry recovered at upload): 3 = swept by the third form through a LINE table (every
 * grid line one run of rows), 2 = by the second form through a point-wise row map, 0 = every grid point is a row / no grid form.
 * gcge_hip_spmm_star_masked_third(0) keeps the second form (measurements).                                            */
int  gcge_hip_mat_star_masked_form (const GCGE_HIP_MAT *A);
void gcge_hip_spmm_star_masked_third (int on);
/* K1 block form: rows of at least `len` entries seed a dense block (default 96); at most `layers` launches of the block kernel (rows
 * inside overlapping blocks get the later ones), later layers seeded by rows of at least `seed_len` entries (defaults 4, 32)       */
void gcge_hip_spmm_dense_min_len (int len);
void gcge_hip_spmm_dense_layers (int layers, int seed_len);
void gcge_hip_spmm_pad8_acc_early (int on);      /* adding row lists request their Y rows when a wave starts (default) */
void gcge_hip_star_product_stats (long *products, long *split);   /* products through the grid form so far, and how many swept their interior planes while the halo travelled */
/*     stencils whose coefficients differ from row to row: the pattern table is then built from the rows' column OFFSETS
 *     only and the values are streamed per row (8 doubles per row), so such matrices keep the pattern kernels (tables of
 *     at most 8 slots); 0 switches that off (takes effect at the next gcge_hip_mat_create*)                             */
void gcge_hip_set_offset_patterns (int on);
/*     column-wise Gram-Schmidt over the slots (the reference's OrthSelf, src/ops_orth.c:45-118): the scaling of x_k is held
 *     back and folded, with the k x 1 Gram of the NEXT column, into the rank-1 update that follows it — one sweep per column
 *     instead of three, same operands and products (1 default, 0: every slot call launches its own kernel)               */
void gcge_hip_set_mgs_fusion (int on);
void gcge_hip_mgs_fusion_stats (long *fused_steps, long *served_grams);
/*     host-only structural self-check of that upload (no device needed): expands the tiles back into (row, column,
 *     value) triples and compares with the CSR arrays bit for bit; returns the number of differences (0 = identical),
 *     the X rows staged per matrix row, the ELL entries per non-zero and the grid strides it detected (0: none)       */
long gcge_hip_tile_selfcheck (int nrows, int ncols_local, const int *rowptr, const int *colidx, const double *val,
		double *xrows_per_row, double *ell_per_nnz, long *strides);
/*     pattern path (csrc/hip/spmm_pattern.hip): matrices whose rows repeat a few stencils {(col - row, value)} are
 *     additionally kept as 16-bit pattern ids + a table of npat * lt {double value; long offset} entries (span, span2 =
 *     longest and second longest |offset| of the interior stencil: launch geometry only); d_dots may be NULL.  gcge_hip_mat_patterns() tells whether a matrix qualified (0: served by the generic kernels).       */
int gcge_hip_pattern_spmm (int nrows, const unsigned short *d_pid, const void *d_tab, int npat, int lt, long span, long span2,
		const double *d_x, long ldx, double *d_y, long ldy, int ncols, double *d_dots, double *d_dots_yy, void *stream);
/*     the two passes of a block-CG iteration on a pattern matrix (reference recurrences: src/ops_lin_sol.c:296-380;
 *     here w = A p is formed twice and never stored).  mode 2: d_dots[j] = sum_r x[r,j] (A x)[r,j], d_dots_yy[j] =
 *     sum_r (A x)[r,j]^2, nothing written.  mode 3: r -= (A x) diag(alpha), pnew = r diag(cr) + x diag(cb),
 *     d_dots[j] = sum_r cr_j r[r,j]^2, with (alpha, cb, cr)_j = flag_j ? (alpha_j, beta_j, 1) : (0, 1, 0); pnew != x.
 *     -1: operands do not qualify (the caller keeps the stored-w form)                                              */
int gcge_hip_pattern_cg (int mode, int nrows, const unsigned short *d_pid, const void *d_tab, int npat, int lt,
		long span, long span2, const double *d_x, long ldx, double *d_r, long ldr, double *d_pnew, long ldp, int ncols,
		const double *d_alpha, const double *d_beta, const int *d_flag, double *d_dots, double *d_dots_yy, void *stream,
		const double *d_b, long ldb);
/*     mode 4: d_dots[j] = sum_r ((A x)[r,j] - alpha_j x[r,j])^2 (residual norms of Ritz pairs);  mode 5: r = b - A x,
 *     pnew = r, d_dots[j] = sum_r r[r,j]^2 (start of the CG; d_b / ldb only used here)                              */
/*     near > 0: the caller knows the table's slots are [-S, 0, +S, -L, +L, -1, +1] (7-point stencil) and passes the
 *     largest |offset| in the table; the passes that
 *     store nothing (modes 2, 4) then run the LDS-ring sweep of csrc/hip/spmm_ring.hip (X rows several grid planes
 *     ahead by LDS-DMA); gcge_hip_spmm_ring_tune(on, planes_ahead) switches it off / picks 2 or 3 planes            */
int gcge_hip_pattern_cg_near (int mode, int nrows, const unsigned short *d_pid, const void *d_tab, int npat, int lt,
		long span, long span2, const double *d_x, long ldx, double *d_r, long ldr, double *d_pnew, long ldp, int ncols,
		const double *d_alpha, const double *d_beta, const int *d_flag, double *d_dots, double *d_dots_yy, void *stream,
		const double *d_b, long ldb, long near);
int gcge_hip_pattern_spmm_near (int nrows, const unsigned short *d_pid, const void *d_tab, int npat, int lt, long span, long span2,
		const double *d_x, long ldx, double *d_y, long ldy, int ncols, double *d_dots, double *d_dots_yy, void *stream, long near);
void gcge_hip_spmm_ring_tune (int on, int planes_ahead);
void gcge_hip_spmm_ring_product (int on);    /* 1: Y = A X through the ring as well (default 0: measured no faster, the product is bound by its read + write traffic) */
void gcge_hip_spmm_ring_wide (int on);      /* 1: 64-bit lane addresses even where 32-bit lane offsets would do (tests) */
void gcge_hip_spmm_ring_xcd (int on);       /* 1: contiguous tile runs per XCD (fabric reads 12.0 -> 9.9 GB per 64 columns at 256^3, same time) */
long gcge_hip_spmm_ring_launches (void);   /* 16-column launches the ring sweep has taken so far */
/*     the same on operator-table objects (halo rows of p fetched by pass 1 and reused by pass 2; sums are the LOCAL
 *     parts, on the host); gcge_hip_cg_fusable: 1 if (mat, p, ncols) qualify                                        */
int gcge_hip_cg_fusable (void *mat, void **p, int ncols);
int gcge_hip_cg_recompute_pays (void *mat);   /* 1: chain + line-exchange layout (HBM-bound product) */
/*     the GCGE_RESIDUAL_FN (include/gcge_ops.h) OPS_HIP_Set registers: squared residual norms of Ritz pairs of a
 *     standard problem in one read of x (kernel MODE 4); returned as void* for test harnesses                    */
void *gcge_hip_residual_hook (void);
int gcge_hip_cg_pass1_mv (void *mat, void **p, int c0, int m, double *host_pw, double *host_ww);
int gcge_hip_cg_start_mv (void *mat, void **x, int xc0, void **b, int bc0, void **r, void **p0, int rc0, int m,
		double *host_rho);   /* r = b - A x, p0 = r, rho = column sums of r^2 (local rows) in one sweep */
/*     the same start for b = x diag(host_scale), never read (kernel MODE 6); with b != NULL the sweep also stores the right-hand
 *     sides it formed into b[:, bc0..) (MODE 8): x may then be columns of any block but r, p0 and b, and is only read        */
int gcge_hip_cg_start_scaled_b_mv (void *mat, void **x, int xc0, const double *host_scale, void **r, void **p0, int rc0, int m,
		void **b, int bc0, double *host_rho);
/*     x[:, xc0..xc0+m) = src[:, sc0..) + sum_{q < cnt} ring_q[:, 0..m) diag(coef[q m ..]): the fused CG's x flush with its read
 *     operand apart from the one it writes (cnt <= 16, 16-byte column pairs; host_coef: cnt * m factors); -1 declines          */
int gcge_hip_cg_accum_x_mv (void **src, int sc0, void **x, int xc0, int m, void ***ring, int cnt, const double *host_coef);
long gcge_hip_bpcg_start_in_place_stats (long *declined);   /* calls with an initial guess elsewhere started in one sweep / materialised first */
int gcge_hip_cg_pass2_mv (void *mat, void **p, void **r, void **pnew, int c0, int m, const double *d_alpha,
		const double *d_beta, const int *d_flag, double *host_rho);
/*     the same two passes with the column sums left on the DEVICE and nothing waited for (the fused CG computes its
 *     scalars there): pass 1: d_out[0,m) = p.(A p), d_out[m,2m) = |A p|^2 (d_out: >= 6 m doubles); pass 2: d_rho[0,m) */
int gcge_hip_cg_pass1_dev (void *mat, void **p, int c0, int m, double *d_out);
/*     second pass without a stored residual (kernel MODE 7): r_k = p_k - beta_{k-1} p_{k-1} rebuilt from the previous
 *     direction pprev (d_betaprev: zeros in the first iteration, where pprev may be p); reads p, pprev, writes pnew */
int gcge_hip_cg_pass2i_dev (void *mat, void **p, void **pprev, void **pnew, int c0, int m, const double *d_alpha,
		const double *d_beta, const int *d_flag, const double *d_betaprev, double *d_rho);
int gcge_hip_cg_pass2i_mv (void *mat, void **p, void **pprev, void **pnew, int c0, int m, const double *d_alpha,
		const double *d_beta, const int *d_flag, const double *d_betaprev, double *host_rho);
long gcge_hip_bpcg_implicit_r_iters (void);   /* CG iterations that ran without a stored residual */
int gcge_hip_cg_pass2_dev (void *mat, void **p, void **r, void **pnew, int c0, int m, const double *d_alpha,
		const double *d_beta, const int *d_flag, double *d_rho);
int gcge_hip_pattern_width (int max_row_len);
int gcge_hip_mat_patterns (const GCGE_HIP_MAT *A);
const char *gcge_hip_mat_spmm_form (const GCGE_HIP_MAT *A);   /* name of the K1 kernel family MatDotMultiVec takes for this matrix */
int gcge_hip_mat_pattern_chain (const GCGE_HIP_MAT *A);   /* 0 none, 1 chain layout (span2 == -1), 2 chain + line exchange (span2 == -L) */
/*     d_out[j] = sum_r x[r,j] y[r,j] */
int gcge_hip_coldots (int nrows, const double *d_x, long ldx, const double *d_y, long ldy, int m,
		double *d_out, void *stream);
/*     d_out[j] = x_j . y_j, d_out[m + j] = y_j . y_j in one sweep (bitwise what two gcge_hip_coldots calls return) */
int gcge_hip_coldots2 (int nrows, const double *d_x, long ldx, const double *d_y, long ldy, int m,
		double *d_out, void *stream);
/*     in-solve rate of K2 / K3 per shape: bracket every Gram and panel update the slots launch with HIP events (no
 *     synchronisation added); the report lists, per (kernel, k, m), calls, average time and 2 n k m flop / time            */
void gcge_hip_dense_profile (int on);
int  gcge_hip_dense_profile_report (char *buf, int len);
/*     the same as numbers: rows of 7 doubles (0 Gram / 1 panel update, k, m, calls, ms in all, flop in all, bytes in all — what each
 *     launch had to move: a panel with beta == NULL or updated in place is not read), largest total time first, at most max_rows;
 *     returns the number of shapes seen (bench.py: roofline_gram / roofline_panel_update)                                       */
int  gcge_hip_dense_profile_shapes (double *out, int max_rows);
/* K3  Y[:,0:m) = X[:,0:k) C + Y diag(beta);  d_c row-major k x m; d_beta NULL => overwrite */
int gcge_hip_lincomb (int nrows, const double *d_x, long ldx, int k, const double *d_c, int m,
		const double *d_beta, double *d_y, long ldy, void *stream);
void gcge_hip_lincomb_tune (int row_fragments);   /* 0 automatic (2 for m > 64 on large blocks), 1, 2: 16-row fragments per wave */
void gcge_hip_gram_tune (int ms);                 /* K2: 4-row steps per macro-step, 1, 2 (the default) or 4; any other value is ignored */
/*     K2 with d_q == d_p, ldq == ldp and k == m <= 64 (the Gram of a block with itself, one tile) takes a symmetric variant: one
 *     fragment load per row, the fragments below the diagonal mirrored instead of accumulated — the same bits.  GCGE_GRAM_NO_SYM=1
 *     in the environment (read per call) keeps the general kernel; the counter is the number of symmetric launches so far        */
long gcge_hip_gram_sym_launches (void);
/* K4  Y[:,0:m) = alpha X[:,0:m) + beta Y   (d_x NULL: scale only; beta == 0: no read of Y) */
int gcge_hip_axpby (int nrows, double alpha, const double *d_x, long ldx, double beta,
		double *d_y, long ldy, int m, void *stream);
/*     The three sweeps of one step of GCGE_PCGSolve and the shift of GCGE_PCGSolveDeflated's operator (gcge_solver.h; GCGE_BACKEND.pcg_step
 *     / pcg_dots / pcg_direction / pcg_shift of OPS_HIP_Set, csrc/hip/pcg_sweeps.hip) on raw device pointers, m columns from each pointer; alpha, beta, flag and the sums are HOST arrays of
 *     m entries, the sums complete when the call returns (the stream is synchronised).  16-byte lanes when m, the origins and the
 *     leading dimensions are even, scalar lanes otherwise: the same results.  Return 0, or the launch's error.
 *       step       x += p diag(alpha) ; r -= w diag(alpha) ; rr[j] = sum_r r_new[r,j]^2 for flag[j] != 0; other columns keep their
 *                  bits (rr[j] = 0)
 *       dots       zr[j] = sum_r z[r,j] r[r,j] ; zw[j] = sum_r z[r,j] w[r,j] from one read of the three blocks
 *       direction  flag[j] == 1: p = z + p diag(beta) ; == 2: p = z (p is not used) ; == 0: the column keeps its bits
 *       shift      w -= q diag(shift) ; pw[j] = sum_r p[r,j] w_new[r,j] for flag[j] != 0; other columns keep the bits of w (pw[j] = 0);
 *                  with d_q == d_p and ldq == ldp the row of p is read once                                                        */
int gcge_hip_pcg_step (int nrows, const double *d_p, long ldp, const double *d_w, long ldw, double *d_x, long ldx, double *d_r, long ldr,
		int m, const double *alpha, const int *flag, double *rr, void *stream);
int gcge_hip_pcg_dots (int nrows, const double *d_z, long ldz, const double *d_r, long ldr, const double *d_w, long ldw, int m,
		double *zr, double *zw, void *stream);
int gcge_hip_pcg_direction (int nrows, const double *d_z, long ldz, double *d_p, long ldp, int m, const double *beta, const int *flag,
		void *stream);
int gcge_hip_pcg_shift (int nrows, const double *d_p, long ldp, const double *d_q, long ldq, double *d_w, long ldw, int m,
		const double *shift, const int *flag, double *pw, void *stream);
/*     GCGE_BACKEND.block_moves of OPS_HIP_Set (include/gcge_ops.h) on blocks of this back-end, for tests: V[:, x0..x1) = ritz[:, x0..x1),
 *     V[:, w0 + ..) = the runs of ritz packed, b[:, b0 + ..) = the same times scale (b NULL: none) in one sweep; 0: declined        */
int gcge_hip_block_moves_mv (void **ritz, void **V, int x0, int x1, const int *runs, int w0, void **b, int b0, const double *scale);
/*     GCGE_BACKEND.ritz_in_place and .panel_norms_sq of OPS_HIP_Set (include/gcge_ops.h) on blocks of this back-end, for tests             */
int gcge_hip_ritz_in_place_mv (void **V, int n0, int x1, int w1, const double *coef, int ldc, void **S, int p0, int np);
int gcge_hip_panel_norms_sq_mv (void **y, int start, int end, double *out);
/*     counters since the library was loaded: out[0] one-sweep starts of the fused block CG taken, out[1] declined ONLY because b starts
 *     on an odd column (matrix in pattern form, even width, x and r on even columns), out[2] / out[3] the same for the V-cycle's
 *     fused residual                                                                                                              */
void gcge_hip_sweep_stats (long out[4]);
/*     One step of a Chebyshev filter (GCGE_ChebFilter, gcge_solver.h; csrc/hip/cheb_sweeps.hip), the sweep on raw device pointers:
 *         out[r, j] <- alpha (out[r, j] - c y[r, j]) - beta z[r, j]        0 <= r < n, 0 <= j < m
 *     in place on out, which holds A y on entry; row-major blocks with their leading dimensions, out apart from y and z.
 *     beta == 0: z is not read (NULL, or any contents).  Rounded as u = fma(-c, y, out), then fma(alpha, u, -(beta z)) (beta == 0:
 *     alpha u): the same bits on every run and in both kernels (16-byte lanes when m, the origins and the leading dimensions are
 *     even, scalar lanes otherwise).  Nothing is waited for.  Return 0, the launch's error, or -1 on bad arguments.                */
int gcge_hip_cheb_sweep (long n, double *out, long ldo, const double *y, long ldy, const double *z, long ldz, int m,
		double alpha, double c, double beta, void *stream);
/*     The step on a matrix handle and blocks of this back-end:  out[:, o0..o0+m) = alpha (A y[:, y0..) - c y[:, y0..)) - beta z[:, z0..),
 *     out, y and z three different blocks (beta == 0: z is not read and may be NULL).  Two paths:
 *       fused            matrices with a pattern table whose product is bound by HBM (gcge_hip_cg_fusable, gcge_hip_cg_recompute_pays),
 *                        beta != 0, one rank, an even width and y0 == z0 == o0 even: ONE call of gcge_hip_cg_pass2i_dev (kernel MODE 7)
 *                        with every column flagged and d_alpha = -alpha, d_betaprev = beta, d_beta = -alpha c - 1 — the product is
 *                        rebuilt in registers: y and z read, out written, 3 block streams and the matrix;
 *       product + sweep  everything else: the handle's ordinary product into out (any K1 form), then gcge_hip_cheb_sweep in place:
 *                        6 block streams and the matrix.  GCGE_CHEB_NO_FUSE=1 in the environment (read per call) forces this path.
 *     Nothing is waited for.  Returns 0; -1 with nothing written for operands no path takes (aliased blocks, a rectangular handle,
 *     column ranges outside a block, blocks of another row count or row order).  gcge_hip_cheb_stats: steps taken fused, steps by
 *     product + sweep, calls that returned -1, since the library was loaded.                                                       */
int gcge_hip_cheb_step_mv (void *mat, void **y, int y0, void **z, int z0, void **out, int o0, int m,
		double alpha, double c, double beta);
void gcge_hip_cheb_stats (long out[3]);
/*     The sums of a band-pass filter (GCGE_ChebBandFilter, gcge_solver.h; csrc/hip/cheb_sweeps.hip) on raw device pointers, in ONE pass:
 *         acc[r, j] <- [acc[r, j] +] mu_a ta[r, j] + mu_b tb[r, j]        0 <= r < n, 0 <= j < m
 *     row-major blocks with their leading dimensions, acc apart from ta and tb: 3 reads + 1 write.  init != 0: acc is NOT read and
 *     may hold anything (2 reads + 1 write).  tb == NULL: one term, mu_b is ignored and nothing of tb is read.  Rounded as
 *     s = fma(mu_a, ta, acc) (init: mu_a ta), then fma(mu_b, tb, s) (one term: s): the same bits on every run and in both kernels
 *     (16-byte lanes when m, the origins and the leading dimensions are even, scalar lanes otherwise).  Nothing is waited for.
 *     Return 0 (also for n == 0 or m == 0), the launch's error, or -1 with nothing written on bad arguments (n < 0, m < 0, NULL acc
 *     or ta, acc == ta or acc == tb).                                                                                              */
int gcge_hip_cheb_accum (long n, double *acc, long lda, const double *ta, long ldta, double mu_a,
		const double *tb, long ldtb, double mu_b, int m, int init, void *stream);
/*     The same on blocks of this back-end (GCGE_BACKEND.cheb_accum of OPS_HIP_Set):  acc[:, a0..a0+m) = [acc[:, a0..) +]
 *     mu_a ta[:, ta0..) + mu_b tb[:, tb0..), acc, ta and tb three different blocks (tb == NULL: one term), on the back-end's stream;
 *     nothing is waited for.  Returns 0; -1 with nothing written for aliased blocks, column ranges outside a block, blocks of
 *     different row counts or row orders, m <= 0.  gcge_hip_cheb_accum_stats: two-term calls, one-term calls, calls that returned
 *     -1, since the library was loaded.                                                                                            */
int gcge_hip_cheb_accum_mv (void **acc, int a0, void **ta, int ta0, double mu_a, void **tb, int tb0, double mu_b, int m, int init);
void gcge_hip_cheb_accum_stats (long out[3]);
/*     The step's sweep with the two column sums of the kernel polynomial method (GCGE_ChebMoments, gcge_solver.h; csrc/hip/cheb_sweeps.hip):
 *     gcge_hip_cheb_sweep with the same operation order — out gets the bits gcge_hip_cheb_sweep writes — and, from the values it stores,
 *         oo[j] = sum_r out_new[r, j]^2 ,   oy[j] = sum_r out_new[r, j] y[r, j]        0 <= j < m
 *     in the same pass: 3 reads + 1 write (beta == 0: 2 + 1), nothing more than the sweep alone.  oo, oy: HOST arrays of m doubles;
 *     the call waits for the stream, as gcge_hip_pcg_dots does.  Every thread adds its rows in ascending order by fma, a workgroup
 *     its row lanes in a fixed order, and the workgroups' partial sums are added in a fixed order: no atomics, the same bits on
 *     every run.  Return 0 (also for n == 0 or m == 0: the sums are 0), the launch's error, or -1 with nothing written on
 *     gcge_hip_cheb_sweep's bad arguments or a NULL oo or oy.
 *     gcge_hip_cheb_dots: the same two sums of a block t that is in memory, tt[j] = sum_r t[r, j]^2, ty[j] = sum_r t[r, j] y[r, j], from
 *     ONE read of t and y (2 reads; t and y may be the same block); -1 on n < 0, m < 0 or a NULL pointer.                          */
int gcge_hip_cheb_sweep_dots (long n, double *out, long ldo, const double *y, long ldy, const double *z, long ldz, int m,
		double alpha, double c, double beta, double *oo, double *oy, void *stream);
int gcge_hip_cheb_dots (long n, const double *t, long ldt, const double *y, long ldy, int m, double *tt, double *ty, void *stream);
/*     The step on a matrix handle with the sums (GCGE_BACKEND.cheb_step_dots of OPS_HIP_Set): gcge_hip_cheb_step_mv's operands, checks
 *     and decisions, out bit for bit what it writes, and oo[j] = sum out[r, o0 + j]^2, oy[j] = sum out[r, o0 + j] y[r, y0 + j] over
 *     the LOCAL rows in host arrays of m doubles (the call waits for them):
 *       fused            the MODE-7 pass, then gcge_hip_cheb_dots on what it wrote: 3 + 2 block streams and the matrix;
 *       product + sweep  the product into out, then gcge_hip_cheb_sweep_dots in place: 6 block streams and the matrix.
 *     Returns 0; -1 with nothing written for the operands gcge_hip_cheb_step_mv refuses and for a NULL oo or oy.
 *     gcge_hip_cheb_step_dots_stats: steps taken fused, steps by product + sweep, calls that returned -1, since the library was
 *     loaded (gcge_hip_cheb_stats does not count these calls).                                                                      */
int gcge_hip_cheb_step_dots_mv (void *mat, void **y, int y0, void **z, int z0, void **out, int o0, int m,
		double alpha, double c, double beta, double *oo, double *oy);
void gcge_hip_cheb_step_dots_stats (long out[3]);

#ifdef __cplusplus
}
#endif
#endif
