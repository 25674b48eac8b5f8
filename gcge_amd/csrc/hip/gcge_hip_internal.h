// Internal helpers shared by the HIP translation units of libgcge_hip.so.
#ifndef GCGE_HIP_INTERNAL_H
#define GCGE_HIP_INTERNAL_H
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#define GCGE_HIP_CHECK(expr)                                                          \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      fprintf(stderr, "gcge_hip: %s failed at %s:%d: %s\n", #expr, __FILE__, __LINE__, \
              hipGetErrorString(e_));                                                 \
      abort();                                                                        \
    }                                                                                 \
  } while (0)

// Shape contract of every slot is checked on the HOST before a kernel is launched: a
// mismatch must abort here, never turn into an out-of-bounds access on the device.
#define GCGE_REQUIRE(cond, what)                                                        \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      fprintf(stderr, "gcge_hip: %s violated (%s) at %s:%d\n", what, #cond, __FILE__, __LINE__); \
      abort();                                                                          \
    }                                                                                   \
  } while (0)

#ifdef __cplusplus
#include <thread>
#include <vector>
#include "gcge_hip.h"
// host-side analysis of a matrix at upload: fn(chunk, first, last) over [0, n) cut into contiguous chunks, one thread each
// (GCGE_UPLOAD_THREADS, default: the cores the process may use, at most 16)
static inline int gcge_upload_threads() {
  const char* e = getenv("GCGE_UPLOAD_THREADS");
  int t = e ? atoi(e) : (int)std::thread::hardware_concurrency();
  if (t < 1) t = 1;
  if (t > 16) t = 16;
  return t;
}
template <class F>
static inline void gcge_parallel_chunks(long n, int nchunks, F fn) {
  if (nchunks <= 1 || n < 65536) { for (int c = 0; c < nchunks; ++c) fn(c, n * c / nchunks, n * (c + 1) / nchunks); return; }
  std::vector<std::thread> th;
  for (int c = 1; c < nchunks; ++c) th.emplace_back([=]() { fn(c, n * c / nchunks, n * (c + 1) / nchunks); });
  fn(0, 0L, n / nchunks);
  for (auto& t : th) t.join();
}
// sparse matrix handle (CCSMAT counterpart): built by mat_upload.hip, multiplied by mat_product.hip, halo plan by rccl_comm.hip
struct GCGE_HIP_MAT_ {
  int nrows;      // local rows
  int nglobal;    // global dimension
  int row_begin;  // first global row
  int nghost;     // halo rows appended to every block of vectors
  long nnz;
  int *d_rowptr, *d_colidx; double* d_val;    // CSR, LOCAL column indices (ghosts >= nrows)
  int *d_orp, *d_pcol; double* d_pval;        // pad-8 copy for the 16-byte-lane kernel
  long noct;
  unsigned short* d_pid; void* d_tab; int npat, pat_lt; long pat_span, pat_span2;   // pattern format (spmm_pattern.hip); d_pid == NULL: not applicable
  double* d_rowval;   // patterns by OFFSETS only: the rows' values, 8 doubles per row in table-slot order (NULL: values in the table)
  long pat_near;  // > 0: chain + line table with slots [-S, 0, +S, -L, +L, -1, +1], the largest |offset| in it (spmm_ring.hip)
  // halo plan of a row-partitioned matrix (one process per GPU); nghost == 0 on a single rank
  int nsend; int* d_send_rows;                 // local rows other ranks need, grouped by destination rank
  double *sendbuf, *recvbuf; int buf_cols;     // exchange buffers (owned by the caller: torch tensors)
  gcge_halo_exchange_fn exchange; void* exchange_ctx;
  // optional split exchange (begin posts the transfers and returns, end completes them) and the rows that do not
  // touch a halo column, [ov_lo, ov_hi): lets the interior product run while the halo is in flight
  gcge_halo_exchange_fn exchange_begin; void (*exchange_end)(void*); int ov_lo, ov_hi;
  void* dense;         // supernode form (spmm_dense.hip): dense row blocks on MFMA + remainder CSR; NULL: no blocks found
  void* tile;          // LDS-staged X-tile form (spmm_tile.hip) of a matrix without a pattern form; NULL: generic kernels
  void* star;          // grid form (spmm_star.hip): rows that are exactly a star stencil, swept plane by plane; NULL: none
  void* star_rem;      // block form (spmm_dense.hip) of the rows the grid form leaves (multiplied first, writes every row)
  void* native_halo;   // RCCL plan of gcge_hip_mat_set_halo_rccl (rccl_comm.hip); it then owns sendbuf / recvbuf
  // rectangular matrices (the prolongations P_l of a multigrid hierarchy, multigrid.hip): nrows x rect_ncols in d_rowptr / d_colidx /
  // d_val, the transpose as a second CSR triple; rect_ncols == 0: an ordinary (symmetric) matrix
  int rect_ncols; int *d_t_rowptr, *d_t_colidx; double* d_t_val;
  int rect_one_per_row;   // 1: every row of a rectangular matrix holds exactly one entry (aggregation prolongations: the fused x += P e)
  // row slabs: the global rows behind the halo columns (host copy, nghost ints; NULL: not named) and the row partition of all ranks
  // (host, part_world + 1 entries; NULL: unknown) — what MultiGridCreate needs to coarsen a slab (multigrid.hip)
  int* h_ghost_global; long* h_part; int part_world;
  // round 5: the row order the back-end chose for itself (mat_upload.hip "row orders"): the device arrays hold P A P^T, every block of
  // vectors created for this matrix lives in the same order; NULL: the caller's order
  struct GcgePerm* perm;
  // one rank, whole matrix: the masked grid its rows live on (mat_upload.hip "geometry"), whatever K1 form the matrix took — what
  // MultiGridCreate coarsens by 2 x 2 x 2 cells.  geom_kind 0: none, 1: named by the caller (gcge_hip_mat_create_grid), 2: recovered
  // at upload (the grid form of spmm_star.hip was built on it); row r is box point h_box[r] = x + nx (y + ny z) of geom_dims, strictly ascending
  int geom_kind; int geom_dims[3]; int* h_box; int* d_box;
  // value maps of the star split (mat_values_forms.hip; NULL: none kept — gcge_hip_mat_keep_value_maps was off at creation, or no grid
  // form); those of the block form live behind star_rem / dense
  struct GcgeStarMaps* star_maps;
  // entry map of a re-ordered handle (mat_upload.hip "row orders"; NULL: none kept — the rows are as given, or
  // gcge_hip_mat_keep_value_maps was off at creation): d_val[q] holds the caller's entry d_emap[q]; nnz ints
  int* d_emap;
};
// mat_values_forms.hip: the device copy of a split's maps (H->keep_maps), and the two halves of an update of a star / dense handle
extern "C" struct GcgeStarMaps* gcge_hip_star_maps_create(const void* star_host, long nnz);
extern "C" void gcge_hip_star_maps_free(struct GcgeStarMaps* M);
extern "C" long gcge_hip_star_maps_bytes(const struct GcgeStarMaps* M);
extern "C" int gcge_hip_mat_has_value_form(const struct GCGE_HIP_MAT_* A);
extern "C" int gcge_hip_mat_holds_value_maps(const struct GCGE_HIP_MAT_* A);                            // by their presence, whatever their size
extern "C" int gcge_hip_mat_forms_check(struct GCGE_HIP_MAT_* A, const double* d_val, long* d2h);      // 0: go on and write, 1: declined
extern "C" void gcge_hip_mat_forms_write(struct GCGE_HIP_MAT_* A, const double* d_val);
// The masked grid a matrix lives on, as the upload hands it to the split of spmm_star.hip (NULL: none): box[i] = x + nx (y + ny z) in an nx x ny x nz
// box.  cols false: box[r] for the nbox = nrows rows of a whole matrix; cols true: box[c] for the nbox local columns of a row slab, own rows, then halo rows.
struct GcgeGridGeom { int nx, ny, nz; const int* box; int nbox; bool cols; };
// One row order per problem size and process: every matrix of n rows (A, then B of a generalised problem) and every block of vectors
// created for them share it.  perm[new] = old, iperm[old] = new; identity: a matrix of this size was uploaded in the caller's order and
// later ones of the same size must follow it.  Reference-counted by matrices and blocks.
struct GcgePerm { int n; int* perm; int* iperm; int identity; long refs; unsigned id; };
extern "C" struct GcgePerm* gcge_hip_perm_acquire(struct GcgePerm* p);      // ++refs (NULL passes through)
extern "C" void gcge_hip_perm_release(struct GcgePerm* p);
extern "C" struct GcgePerm* gcge_hip_perm_live(int n);          // mat_upload.hip: the live order of size n (NULL: none); no reference taken
extern "C" struct GcgePerm* gcge_hip_perm_identity(int n);      // ... the identity order of size n, registered if none is live (NULL: a re-ordered one is)
extern "C" void gcge_hip_halo_native_free(struct GCGE_HIP_MAT_* A);
extern "C" void gcge_hip_comm_transfer_sync(void);              // rccl_comm.hip: the split exchange's transfer stream has drained
// mat_device.hip: gcge_hip_mat_create_device whose fall-back is gcge_hip_mat_create_as_given and which runs beside a re-ordered matrix of
// its size (the coarse levels of a MIS-2 hierarchy, multigrid.hip)
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_device_as_given(int nrows, long nnz, const int* d_rowptr, const int* d_colidx, const double* d_val);
// tests only: a download of d_pid (nrows) / d_tab (npat * pat_lt entries of 16 bytes), returns npat * pat_lt (0: no pattern form; NULL
// outputs are skipped); and the row hash of the device search cut to its low bits (64: all of it, the default; small values force
// collisions for the verify pass to find)
extern "C" long gcge_hip_mat_pattern_table(const GCGE_HIP_MAT* A, unsigned short* pid_out, void* tab_out);
extern "C" void gcge_hip_mat_device_hash_bits(int bits);
// multigrid.hip: the MultiGridCreate / MultiGridDestroy slots of OPS_HIP_Set
extern "C" void gcge_hip_multigrid_create(void*** A_array, void*** B_array, void*** P_array, int* num_levels, void* A, void* B, struct OPS_* ops);
extern "C" void gcge_hip_multigrid_destroy(void*** A_array, void*** B_array, void*** P_array, int* num_levels, struct OPS_* ops);
// mg_device.hip: the device side of MultiGridCreate's hierarchy (d2h: bytes copied device to host are added there; may be NULL)
extern "C" int gcge_hip_mg_detect_grid_device(int n, const int* d_rowptr, const int* d_colidx, int dims[3], long* d2h);
extern "C" void gcge_hip_mg_agg_grid_device(const int dims[3], int* d_agg, int* d_ptr, int* d_mem, int cdims[3]);
extern "C" int gcge_hip_mg_galerkin_device(int nf, const int* d_rowptr, const int* d_colidx, const double* d_val, const int* d_agg, int nc,
                                           const int* d_ptr, const int* d_mem, double scale, int** d_rp_out, int** d_ci_out, double** d_va_out,
                                           long* nnz_out, long* d2h);
extern "C" int gcge_hip_mg_galerkin_values_into(int nf, const int* d_rowptr, const int* d_colidx, const double* d_val, const int* d_agg, int nc,
                                                const int* d_ptr, const int* d_mem, double scale, const int* d_rp_c, const int* d_ci_c,
                                                double* d_va_c, long* d2h);     // (rows that fit are written even when it returns 1)
extern "C" int gcge_hip_mg_galerkin_values_slab_into(int ncols_f, const int* d_rowptr, const int* d_colidx, const double* d_val, const int* d_colagg,
                                                     int nc, const int* d_ptr, const int* d_mem, double scale, const int* d_rp_c, const int* d_ci_c,
                                                     double* d_va_c, int nlo, long* d2h);     // a level of a row-slab hierarchy
extern "C" int gcge_hip_mg_agg_masked_device(const int dims[3], const int* d_box, int nf, int* d_agg, int* d_mem, int** d_ptr_out, int** d_cbox_out,
                                             int cdims[3], long* d2h);
// mg_aggregate.hip: MIS-2 aggregation (gcge_mg_aggregate_mis2) of an n-row device CSR; agg / mem: the caller's, *d_ptr_out allocated
// there; returns the number of aggregates, -1: the rounds reached their cap, nothing allocated (the caller aggregates on the host)
extern "C" int gcge_hip_mg_agg_graph_device(int n, const int* d_rowptr, const int* d_colidx, const double* d_val, double theta, int* d_agg,
                                            int* d_mem, int** d_ptr_out, long* d2h);
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_rect_device(int nf, int nc, const int* d_agg, const int* d_ptr, const int* d_mem);
extern "C" int gcge_hip_mg_download_csr(int nrows, int ncols, long nnz, const int* d_rp, const int* d_ci, const double* d_va, GCGE_CSR* out, long* d2h);
void gcge_hip_mg_members_host(const int* agg, int nf, int nc, std::vector<int>& ptr, std::vector<int>& mem);
// block_pcg.hip: the fused CG's part of the back-end record OPS_HIP_Set registers (the BlockAMG smoother, the scaled-rhs solver)
extern "C" void gcge_hip_bpcg_backend(GCGE_BACKEND* be);
// pcg_sweeps.hip: the three sweeps of GCGE_PCGSolve's step (pcg_step / pcg_dots / pcg_direction) and the fused CG's iteration count
extern "C" void gcge_hip_pcg_backend(GCGE_BACKEND* be);
// cheb_sweeps.hip: the scalars of one fused Chebyshev step (gcge_hip_cheb_step_mv) written to a device staging area by a kernel on
// `stream`; the four pointers (m entries each) stay valid until the next call
extern "C" void gcge_hip_cheb_scalars(int m, double alpha, double c, double beta, void* stream, const double** d_alpha, const double** d_beta,
                                      const double** d_betaprev, const int** d_flag);
// What the block sweeps of block_pcg.hip and pcg_sweeps.hip share.  16-byte lanes (column pairs) need an even width, 16-byte aligned
// column origins and even leading dimensions; cg_tpr: threads per row of such a sweep (m <= 512)
#include <initializer_list>
#include <stdint.h>
static inline bool cg_vec_ok(int m, std::initializer_list<const double*> ptrs, std::initializer_list<long> lds) {
  if (m & 1) return false;
  for (const double* q : ptrs) if ((uintptr_t)q & 15) return false;
  for (long l : lds) if (l & 1) return false;
  return true;
}
static inline int cg_tpr(int m) { int t = 1; while (t < m / 2) t *= 2; return t; }
// the row split of every sweep that leaves partial sums: nb workgroups of rpb rows each (a multiple of 4)
struct CgGrid { long nb, rpb; };
static inline CgGrid cg_grid(long n) {
  long nb = (n + 255) / 256; if (nb > 2048) nb = 2048;
  const long rpb = ((n + nb - 1) / nb + 3) / 4 * 4;
  return {(n + rpb - 1) / rpb, rpb};
}
// A column scaling the slots hold back (column-wise Gram-Schmidt, app_hip.hip) is applied now.  First statement of every EXPORTED
// raw kernel that takes device pointers: the caller may have fetched its pointer before the scaling was held back.
extern "C" void gcge_hip_apply_pending(void);

// ---- app_hip.hip (runtime state, pool, multivector slots) and mat_product.hip (everything that multiplies a matrix handle) ----------
#include <chrono>
struct GcgeHipMV {
  double* d;      // 16-byte aligned: a hipMalloc'd block of the pool (mv_new), never an offset into one
  size_t bytes;   // size of the allocation behind d
  long ld;
  int nrows, nrows_alloc, ncols;
  const GCGE_HIP_MAT_* mat;   // shape donor (row partition)
  GcgePerm* perm;             // the row order of the matrix this block was created for (NULL / identity: the caller's order); see mat_upload.hip
  // column-wise Gram-Schmidt over the slots (app_hip.hip "one sweep per column"): the state lives in the block it belongs to
  int pend_col; double pend_fac;                       // a scaling of column pend_col held back (pend_col < 0: none)
  int spec_c0, spec_c1; unsigned long spec_epoch;      // Gram column of [spec_c0, spec_c1) computed on the way by the call of epoch spec_epoch
  std::vector<double>* spec_dots;                      // (NULL: none)
};
static inline const GcgePerm* real_perm(const GcgePerm* p) { return (p != nullptr && !p->identity) ? p : nullptr; }
// per-slot wall time (gcge_hip_slot_timing, app_hip.hip): one flag test when it is off
struct SlotTimer {
  const char* name; int cols; std::chrono::steady_clock::time_point t0; bool on;
  SlotTimer(const char* n, int c);
  ~SlotTimer();
};
extern "C" {
void gcge_hip_enter(void);                      // top of every entry point that touches block data: counts the call, applies a held-back scaling
double* gcge_hip_stage_d(size_t len);           // device / second device / pinned host staging of at least len doubles
double* gcge_hip_stage_d2(size_t len);
double* gcge_hip_stage_h(size_t len);
void* gcge_hip_pool_alloc(size_t bytes);
void gcge_hip_pool_free(void* q, size_t bytes);
int gcge_hip_spmm_path_get(void);
int gcge_hip_offset_patterns_get(void);
unsigned gcge_hip_mv_row_order_id(void** mv);
void gcge_hip_local_inner_prod(char nsd, void** x, void** y, int* start, int* end, double* ip, int ldIP, struct OPS_* ops);
// mat_product.hip: its slots and hooks of the table OPS_HIP_Set fills, and the fused CG's entry points gcge_hip.h does not name
void gcge_hip_product_slots(struct OPS_* ops, GCGE_BACKEND* be);
void gcge_hip_spmm_dot_mv(void* mat, void** x, void** y, int* start, int* end, double* host_dots, struct OPS_* ops);
void gcge_hip_spmm_dot2_mv(void* mat, void** x, void** y, int* start, int* end, double* host_dots, double* host_yy, struct OPS_* ops);
int gcge_hip_cg_start_scaled_mv(void* mat, void** x, int xc0, const double* host_scale, void** r, void** p0, int rc0, int m, double* host_rho);
int gcge_hip_cg_start_scaled_b_mv(void* mat, void** x, int xc0, const double* host_scale, void** r, void** p0, int rc0, int m, void** b, int bc0,
                                  double* host_rho);
// pas_border.hip
int gcge_hip_pas_border(void** QX, int s, void** q, int q0, void** y, int y0, int m, double beta, const double* t, int ldt, double* g, int ldg);

// ---- kernel files: what other translation units launch or build through them and gcge_hip.h does not name --------------------------
// lincomb_mfma.hip: the panel update by its register form with a row copy / the column norms in its epilogue (1: not taken)
int gcge_hip_lincomb_copy(int nrows, const double* d_x, long ldx, int k, const double* d_c, int m, const double* d_beta, double* d_y, long ldy,
                          const double* d_src, long lds, double* d_dst, long ldd, int ncopy, void* stream);
int gcge_hip_lincomb_norms(int nrows, const double* d_x, long ldx, int k, const double* d_c, int m, const double* d_beta, double* d_y, long ldy,
                           double* d_norms, void* stream);
// vec_kernels.hip
double* gcge_hip_partial_ws(size_t len);
void gcge_hip_reduce_partials(const double* d_partial, int nblocks, int len, double* d_out, void* stream);
void gcge_hip_reduce_partials_head(const double* d_partial, int nblocks, int len, int nout, double* d_out, void* stream);
void gcge_hip_reduce_partials16(const double* d_partial, int nblocks, long slab_stride, int ncols, double* d_out, void* stream);
void gcge_hip_reduce_partials_slabs(const double* d_partial, int nblocks, long slab_stride, int cpp, int ncols, double* d_out, void* stream);
int gcge_hip_resid_sq(int nrows, const double* d_w, long ldw, const double* d_x, long ldx, int m, const double* d_lambda, double* d_out, void* stream);
int gcge_hip_colscale(int nrows, double* d_y, long ldy, int m, const double* d_s, void* stream);
int gcge_hip_block_moves(int nrows, const double* d_src, long lds, double* d_v, long ldv, double* d_b, long ldb, int c0, int npairs, int x0, int x1,
                         const int* d_map, const double* d_scale, int w0, int b0, void* stream);
int gcge_hip_panel_dot1(int nrows, const double* d_x, long ldx, int k, const double* d_y, long ldy, double* d_out, void* stream);
int gcge_hip_rank1_update(int nrows, const double* d_x, long ldx, const double* d_c, const double* d_beta, double* d_y, long ldy, int m, void* stream);
int gcge_hip_colscale1(int nrows, double* d_y, long ldy, double s, void* stream);
int gcge_hip_mgs_step(int nrows, double* d_xk, long ld, double s, const double* d_c, int w, double* d_dots, void* stream);
int gcge_hip_fill_uniform(int nrows, long row_begin, long nglobal, double* d_y, long ldy, int c0, int m, unsigned long long seed, void* stream);
int gcge_hip_colmajor_to_rowmajor(int nrows, int m, const double* d_src, long lds, double* d_dst, long ldd, void* stream);
int gcge_hip_rowmajor_to_colmajor(int nrows, int m, const double* d_src, long lds, double* d_dst, long ldd, void* stream);
// spmm_pad8.hip
int gcge_hip_pad8_spmm_dot(int nrows, const int* d_orp, const int* d_pcol, const double* d_pval, const double* d_x, long ldx, double* d_y, long ldy,
                           int ncols, double* d_dots, void* stream, long x_own_row0);
void gcge_hip_spmm_pad8_auto(double avg_octets_per_row);
void gcge_hip_spmm_pad8_row_map(const int* d_map);
void gcge_hip_spmm_pad8_row_map_add(const int* d_map);
void gcge_hip_spmm_pad8_tune(int rows_per_wave, int batch, int store_policy, int col_pass);   // rows_per_wave 0: back to automatic
void gcge_hip_spmm_pad8_gridcap(int cap);
void gcge_hip_spmm_pad8_schedule(const int* d_sched, int len, int rows_per_wave, int grid);
// spmm.hip: process-wide tuning of the CSR kernels (defaults: 16 rows per wave, XCD group 1, plain stores; the stream kernel, batch 16; no map)
void gcge_hip_spmm_tune(int rows_per_wave, int xcd_group, int nt_store);
void gcge_hip_spmm_variant(int variant, int batch);
void gcge_hip_spmm_set_chunk_map(const int* d_map, unsigned len);
// spmm_pattern.hip, spmm_ring.hip
int gcge_hip_pattern_spmm_vals(int nrows, const unsigned short* d_pid, const void* d_tab, int npat, int lt, long span, long span2, const double* d_x,
                               long ldx, double* d_y, long ldy, int ncols, double* d_dots, double* d_dots_yy, void* stream, long near,
                               const double* d_rowval);
int gcge_hip_pattern_cg_vals(int mode, int nrows, const unsigned short* d_pid, const void* d_tab, int npat, int lt, long span, long span2,
                             const double* d_x, long ldx, double* d_r, long ldr, double* d_pnew, long ldp, int ncols, const double* d_alpha,
                             const double* d_beta, const int* d_flag, double* d_dots, double* d_dots_yy, void* stream, const double* d_b, long ldb,
                             long near, const double* d_rowval);
int gcge_hip_ring_pass(int mode, int nrows, const unsigned short* d_pid, const void* d_tab, int npat, long L, int nw, long nb, const double* d_x,
                       long ldx, int m, double* part, long yyo, const double* d_lambda, void* stream, long maxoff, double* d_y, long ldy, int gy);
// spmm_tile.hip
void* gcge_hip_tile_build(int nrows, int ncols_local, const int* rowptr, const int* colidx, const double* val);
void* gcge_hip_tile_build_for(int nrows, int ncols_local, const int* rowptr, const int* colidx, const double* val, int remainder);
void gcge_hip_tile_free(void* tm);
int gcge_hip_spmm_tile_mode_get(void);
void gcge_hip_tile_stats(const void* tm, long* ntiles, long* ov_nnz, double* xrows_per_row, double* ell_per_nnz, int* brick, long* strides);
int gcge_hip_tile_spmm(const void* tm, const double* d_x, long ldx, double* d_y, long ldy, int ncols, void* stream);
// spmm_dense.hip
void* gcge_hip_dense_build(int nrows, int ncols_local, const int* rowptr, const int* colidx, const double* val, int keep_maps);
void* gcge_hip_dense_build_rows(int nrows, int ncols_local, const int* rowptr, const int* colidx, const double* val, const unsigned char* not_listed,
                                int keep_maps);
void gcge_hip_dense_free(void* dm);
// value maps of a block form (value_maps.h; 0: it holds none): bytes of maps; one map entry per slot of the block values and of the pad-8
// remainder, indices into the nsrc values the form was built from
long gcge_hip_dense_value_maps(const void* dm, const int** d_vmap, double** d_vals, long* nvals, const int** d_pmap, double** d_pval, long* npval,
                               long* nsrc);
int gcge_hip_dense_remainder_is_tiled(const void* dm);
const void* gcge_hip_dense_remainder_tile(const void* dm);
void gcge_hip_dense_stats(const void* dm, long* nblocks, long* items, long* dense_nnz, long* dense_entries, long* rem_nnz);
int gcge_hip_dense_spmm(const void* dm, const double* d_x, long ldx, double* d_y, long ldy, int ncols, void* stream, int which);
const int* gcge_hip_dense_row_list(const void* dm, int* nlisted);
// spmm_star.hip (gcge_hip_star_build: star_split.h)
void gcge_hip_star_free(void* sm);
double* gcge_hip_star_diag(void* sm);
void gcge_hip_star_stats(const void* sm, long* out);
int gcge_hip_star_masked_form(const void* sm);
int gcge_hip_star_interior(const void* sm, int* ilo, int* ihi);
int gcge_hip_star_spmm(const void* sm, const double* d_x, long ldx, double* d_y, long ldy, int ncols, void* stream);
int gcge_hip_star_spmm_part(const void* sm, const double* d_x, long ldx, double* d_y, long ldy, int ncols, double* d_dots, void* stream, int part);
int gcge_hip_star_coldots2_rows(int nlist, const int* d_list, const double* d_x, long ldx, const double* d_y, long ldy, int m, double* d_out, void* stream);
// reorder.hip
double gcge_hip_mean_bandwidth(int n, const int* rowptr, const int* colidx, const int* iperm);
}

#endif

#endif
