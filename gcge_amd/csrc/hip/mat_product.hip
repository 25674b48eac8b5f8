// mat_product — everything that multiplies a matrix handle of the HIP back-end: the layer between the operator table's slots / the
// fused block CG (block_pcg.hip) and the K1 kernels (spmm*.hip).
//   halo_fetch / halo_send / halo_recv   the halo rows of a row slab, blocking or split around the interior product
//   spmm_rows, star_product, spmm_halo   which K1 form a product (or a fused CG pass: CgPass) takes, whole or in row strips
//   HIP_MatDotMultiVec, HIP_MatTransDotMultiVec, gcge_hip_spmm_dot*   the product, alone or with the column sums x.y / y.y
//   gcge_hip_cg_*                        the passes of the fused block CG on a pattern matrix (product formed twice, never stored)
//   gcge_hip_cheb_step_mv                one step of a Chebyshev filter: the second CG pass with prescribed scalars, or product + sweep
//   gcge_hip_cheb_accum_mv               the sums of a band-pass filter on blocks (no matrix: it sits beside the step it follows)
//   gcge_hip_cheb_step_dots_mv           the step with the two column sums of the kernel polynomial method
//   HIP_Amg*, HIP_ResidualSq       the fused sweeps of a V-cycle and the residual norms of Ritz pairs (GCGE_BACKEND)
//   gcge_hip_profile_*                   HIP events around every K1 launch
// Runtime state, staging, pool and the multivector slots live in app_hip.hip (shared names: gcge_hip_internal.h); the handle itself
// is built by mat_upload.hip.  These wrappers run several times per CG iteration on levels bound by launch latency: helpers are
// file-local, take plain pointers and allocate nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "gcge_hip.h"
#include "gcge_solver.h"
#include "gcge_hip_internal.h"

#define g_stream ((hipStream_t)gcge_hip_stream())
#define g_spmm_path (gcge_hip_spmm_path_get())


__global__ __launch_bounds__(256) void halo_pack(int nsend, const int* __restrict__ rows, const double* __restrict__ x,
    long ldx, int m, double* __restrict__ buf) {
  const long total = (long)nsend * m;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long i = idx / m; const int j = (int)(idx - i * m);
    buf[idx] = x[(long)rows[i] * ldx + j];
  }
}
__global__ __launch_bounds__(256) void halo_unpack(int nghost, const double* __restrict__ buf, int m, double* __restrict__ xg,
    long ldx) {
  const long total = (long)nghost * m;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long g = idx / m; const int j = (int)(idx - g * m);
    xg[g * ldx + j] = buf[idx];
  }
}

// ------------------------------------------------------------------ SpMM launch profiling
// HIP events around every K1 launch on the launch stream (bench.py: roofline.achieved =
// algorithmic bytes / average launch duration, measured live inside the timed region).
struct SpmmEvent { hipEvent_t e0, e1; int m; double bytes; int kind; long rows; };   // rows: local rows of the matrix (a solver may run the same kernels on several: the levels of a multigrid cycle)   // kind 0: product (plain or with the column sums), 2 / 3: CG passes
static std::vector<SpmmEvent> g_prof;
static int g_prof_on = 0;
extern "C" void gcge_hip_profile_enable(int on) {
  for (auto& e : g_prof) { hipEventDestroy(e.e0); hipEventDestroy(e.e1); }
  g_prof.clear();
  g_prof_on = on;
}
// sums over the recorded launches with exactly `ncols` columns (0: all); returns the count
// kind 0: MatDotMultiVec products (plain or with the column sums); 2 / 3: first / second pass of the fused CG
extern "C" long gcge_hip_profile_spmm(int ncols, double* total_ms, double* total_alg_bytes) {
  return gcge_hip_profile_kind(0, ncols, total_ms, total_alg_bytes);
}
extern "C" long gcge_hip_profile_kind(int kind, int ncols, double* total_ms, double* total_alg_bytes) {
  return gcge_hip_profile_kind_rows(kind, ncols, 0, total_ms, total_alg_bytes);
}
// ... restricted to the launches on matrices of `nrows` local rows (0: all).  With BlockAMG as the solver the fused CG runs the same
// kernels on every level of the hierarchy; a roofline figure belongs to ONE problem size (bench.py: the finest level).
extern "C" long gcge_hip_profile_kind_rows(int kind, int ncols, long nrows, double* total_ms, double* total_alg_bytes) {
  long cnt = 0; double ms = 0.0, by = 0.0;
  GCGE_HIP_CHECK(hipDeviceSynchronize());
  for (auto& e : g_prof) {
    if (e.kind != kind || (ncols > 0 && e.m != ncols) || (nrows > 0 && e.rows != nrows)) continue;
    float t = 0.f;
    GCGE_HIP_CHECK(hipEventElapsedTime(&t, e.e0, e.e1));
    ms += t; by += e.bytes; ++cnt;
  }
  if (total_ms) *total_ms = ms;
  if (total_alg_bytes) *total_alg_bytes = by;
  return cnt;
}

// The bracket around one K1 launch (on a row slab the interval also holds the halo exchange).  Algorithmic bytes: values
// + indices once, row pointers once, and `streams` block streams of nrows x m doubles — 2 for a product (X read, Y written; the column
// sums add no HBM traffic), 1 / 4 / 3 for the CG passes (p | p, r read, r, p_new written | p, p_prev read, p_new written).
namespace {
struct ProfScope {
  SpmmEvent ev; bool on;
  ProfScope(int kind, const GCGE_HIP_MAT_* A, int m, int streams) : on(g_prof_on != 0) {
    if (!on) return;
    GCGE_HIP_CHECK(hipEventCreate(&ev.e0)); GCGE_HIP_CHECK(hipEventCreate(&ev.e1));
    ev.kind = kind; ev.m = m; ev.rows = A->nrows;
    ev.bytes = 12.0 * (double)A->nnz + 4.0 * ((double)A->nrows + 1.0) + 8.0 * streams * (double)A->nrows * m;
    GCGE_HIP_CHECK(hipEventRecord(ev.e0, g_stream));
  }
  void done() { if (on) { GCGE_HIP_CHECK(hipEventRecord(ev.e1, g_stream)); g_prof.push_back(ev); on = false; } }
  void cancel() { if (on) { hipEventDestroy(ev.e0); hipEventDestroy(ev.e1); on = false; } }   // nothing was launched
  ~ProfScope() { done(); }
};
}

// row-partitioned matrices: the rows other ranks need of X (dx: row 0 of its first column), packed for the exchange, and the halo rows
// of X[:, c_begin : c_begin + m) unpacked behind the local ones
static void halo_send(GCGE_HIP_MAT_* A, const double* dx, long ldx, int m) {
  if (A->nsend <= 0) return;
  long tot = (long)A->nsend * m, g = (tot + 255) / 256; if (g > 4096) g = 4096;
  hipLaunchKernelGGL(halo_pack, dim3((unsigned)g), dim3(256), 0, g_stream, A->nsend, A->d_send_rows, dx, ldx, m, A->sendbuf);
}
static void halo_recv(GCGE_HIP_MAT_* A, GcgeHipMV* vx, int c_begin, int m) {
  long tot = (long)A->nghost * m, g = (tot + 255) / 256; if (g > 4096) g = 4096;
  hipLaunchKernelGGL(halo_unpack, dim3((unsigned)g), dim3(256), 0, g_stream, A->nghost, A->recvbuf, m,
                     vx->d + (long)A->nrows * vx->ld + c_begin, vx->ld);
}
// ... fetched from their owners, in chunks of the exchange buffers' width
static void halo_fetch(GCGE_HIP_MAT_* A, GcgeHipMV* vx, int c_begin, int m) {
  if (A->nghost <= 0) return;
  GCGE_REQUIRE(A->exchange != nullptr && A->buf_cols > 0, "MatDotMultiVec: halo plan installed (gcge_hip_mat_set_halo)");
  for (int c0 = 0; c0 < m; c0 += A->buf_cols) {
    const int mc = (m - c0 < A->buf_cols) ? m - c0 : A->buf_cols;
    halo_send(A, vx->d + c_begin + c0, vx->ld, mc);
    A->exchange(A->sendbuf, A->recvbuf, mc, A->exchange_ctx);
    halo_recv(A, vx, c_begin + c0, mc);
  }
}

// n column sums device -> pinned staging, complete on return (one stream synchronisation); the pinned copy is returned
static double* sums_to_host(const double* d_src, size_t n) {
  double* hd = gcge_hip_stage_h(n);
  GCGE_HIP_CHECK(hipMemcpyAsync(hd, d_src, n * sizeof(double), hipMemcpyDeviceToHost, g_stream));
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
  return hd;
}
// The fused kernels walk a block in 16-byte pairs of columns: ld even, first column even, base 16-byte aligned (every GcgeHipMV::d is —
// gcge_hip_internal.h — so this is also "the pointer to the first column is aligned")
static inline bool pair_ok(const GcgeHipMV* v, int c0) { return !((c0 & 1) || (v->ld & 1) || ((uintptr_t)v->d & 15)); }


__global__ void add3_kernel(double* __restrict__ dst, const double* __restrict__ a, const double* __restrict__ b,
                            const double* __restrict__ c, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (a[i] + b[i]) + c[i];
}

// rows [r0, r1) of Y = A X, optionally with the column sums x.y (and y.y) over those rows (d_dots, d_yy: device, m each).
// want_fused: the caller asked for dots and the matrix/operands qualify for a fused kernel.
// cg != NULL: one of the two passes of a block-CG iteration instead of the product (pattern matrices only,
// gcge_hip_pattern_cg): mode 2 = the sums without storing Y, mode 3 = R / P update with the product recomputed.
struct CgPass { int mode; double* r; long ldr; double* pnew; long ldp; const double *alpha, *beta; const int* flag; const double* b; long ldb; };
static int spmm_rows(GCGE_HIP_MAT_* A, long r0, long r1, const double* dx, long ldx, double* dy, long ldy, int m,
                     double* d_dots, double* d_yy, const CgPass* cg = nullptr) {
  const int nr = (int)(r1 - r0);
  if (nr <= 0) {
    if (d_dots) GCGE_HIP_CHECK(hipMemsetAsync(d_dots, 0, m * sizeof(double), g_stream));
    if (d_yy) GCGE_HIP_CHECK(hipMemsetAsync(d_yy, 0, m * sizeof(double), g_stream));
    return 0;
  }
  if (cg != nullptr) {
    if (A->d_pid == nullptr || g_spmm_path != 0) return -1;
    return gcge_hip_pattern_cg_vals(cg->mode, nr, A->d_pid + r0, A->d_tab, A->npat, A->pat_lt, A->pat_span, A->pat_span2,
                               dx + r0 * ldx, ldx, cg->r ? cg->r + r0 * cg->ldr : nullptr, cg->ldr,
                               cg->pnew ? cg->pnew + r0 * cg->ldp : nullptr, cg->ldp, m, cg->alpha, cg->beta, cg->flag,
                               d_dots, d_yy, g_stream, cg->b ? cg->b + r0 * cg->ldb : nullptr, cg->ldb, A->pat_near,
                               A->d_rowval ? A->d_rowval + 8 * r0 : nullptr);
  }
  double* y = dy + r0 * ldy;
  int rc = -1;
  if (A->d_pid != nullptr && g_spmm_path == 0)
    rc = gcge_hip_pattern_spmm_vals(nr, A->d_pid + r0, A->d_tab, A->npat, A->pat_lt, A->pat_span, A->pat_span2, dx + r0 * ldx, ldx,
                                    y, ldy, m, d_dots, d_yy, g_stream, A->pat_near, A->d_rowval ? A->d_rowval + 8 * r0 : nullptr);
  if (rc != -1) return rc;
  // whole-matrix products only from here: neither the rows of a block nor those of a tile are a row range
  if (A->star != nullptr && d_dots == nullptr && r0 == 0 && r1 == A->nrows && g_spmm_path == 0) {
    rc = gcge_hip_star_spmm(A->star, dx, ldx, dy, ldy, m, g_stream);              // star + diagonal of EVERY row ...
    if (rc == 0) rc = gcge_hip_dense_spmm(A->star_rem, dx, ldx, dy, ldy, m, g_stream, 4);   // ... + what the other rows hold beyond it
  }
  if (rc != -1) return rc;
  if (A->dense != nullptr && d_dots == nullptr && r0 == 0 && r1 == A->nrows && g_spmm_path != 1 && g_spmm_path != 3 && g_spmm_path != 4)
    rc = gcge_hip_dense_spmm(A->dense, dx, ldx, dy, ldy, m, g_stream, 0);
  if (rc != -1) return rc;
  if (A->tile != nullptr && d_dots == nullptr && r0 == 0 && r1 == A->nrows && g_spmm_path != 1 && g_spmm_path != 3)
    rc = gcge_hip_tile_spmm(A->tile, dx, ldx, dy, ldy, m, g_stream);   // whole-matrix products only: a tile's rows are not a row range
  if (rc != -1) return rc;
  if (d_dots) {   // generic fused kernel (the caller checked its contract), y.y by a second pass over y
    rc = gcge_hip_pad8_spmm_dot(nr, A->d_orp + r0, A->d_pcol, A->d_pval, dx, ldx, y, ldy, m, d_dots, g_stream, r0);   // (x.y over the strip's OWN rows of x)
    if (rc == 0 && d_yy) rc = gcge_hip_coldots(nr, y, ldy, y, ldy, m, d_yy, g_stream);
    return rc;
  }
  if (m >= 16) {
    gcge_hip_spmm_pad8_auto(A->nrows > 0 ? (double)A->noct / A->nrows : 1.0);
    rc = gcge_hip_pad8_spmm(nr, A->d_orp + r0, A->d_pcol, A->d_pval, dx, ldx, y, ldy, m, g_stream);
  }
  if (rc == -1) rc = gcge_hip_csr_spmm(nr, A->d_rowptr + r0, A->d_colidx, A->d_val, dx, ldx, y, ldy, m, g_stream);
  return rc;
}

static int g_halo_overlap = 1;
extern "C" void gcge_hip_set_halo_overlap(int on) { g_halo_overlap = on; }

// Y[:, 0:m) = A X[:, c_begin : c_begin + m) for a matrix in grid form (spmm_star.hip), whole or a row slab cut on plane
// boundaries.  On a slab with a split exchange the planes that need no halo row are swept while the halo is in flight (the
// reference's distributed product does the same with its diagonal block: app/app_phg.c:307-357), the first and last STAR_R
// planes and the rows outside the grid form (blocks + listed rows, which may reference any halo row) follow its arrival.
// dd != NULL (4 m doubles, device): the column sums x.y and y.y over the star rows (dd[0:2m)) and over the other rows (dd[2m:4m)).
// -1 before anything was launched or sent: operands the sweep does not take.
static long g_star_products = 0, g_star_split_products = 0;
extern "C" void gcge_hip_star_product_stats(long* products, long* split) { if (products) *products = g_star_products; if (split) *split = g_star_split_products; }
static int star_product(GCGE_HIP_MAT_* A, GcgeHipMV* vx, int c_begin, double* dy, long ldy, int m, double* dd) {
  const double* dx = vx->d + c_begin;
  const long ldx = vx->ld;
  if ((m & 1) || (ldx & 1) || (ldy & 1) || ((uintptr_t)dx & 15) || ((uintptr_t)dy & 15) || dx == dy) return -1;
  const bool split = A->nghost > 0 && g_halo_overlap && A->exchange_begin != nullptr && A->exchange_end != nullptr && m <= A->buf_cols &&
                     gcge_hip_star_interior(A->star, nullptr, nullptr);
  int rc;
  ++g_star_products;
  if (split) {
    ++g_star_split_products;
    halo_send(A, dx, ldx, m);
    A->exchange_begin(A->sendbuf, A->recvbuf, m, A->exchange_ctx);
    rc = gcge_hip_star_spmm_part(A->star, dx, ldx, dy, ldy, m, dd, g_stream, 1);        // overlaps the transfers
    A->exchange_end(A->exchange_ctx);
    halo_recv(A, vx, c_begin, m);
    if (rc == 0) rc = gcge_hip_star_spmm_part(A->star, dx, ldx, dy, ldy, m, dd, g_stream, 2);
  } else {
    halo_fetch(A, vx, c_begin, m);
    rc = gcge_hip_star_spmm_part(A->star, dx, ldx, dy, ldy, m, dd, g_stream, 0);
  }
  GCGE_REQUIRE(rc == 0, "star product: sweep");
  rc = gcge_hip_dense_spmm(A->star_rem, dx, ldx, dy, ldy, m, g_stream, 4);               // += what the rows with more than the star hold beyond it
  GCGE_REQUIRE(rc == 0, "star product: blocks and listed rows");
  if (dd != nullptr) {
    int nlist = 0; const int* list = gcge_hip_dense_row_list(A->star_rem, &nlist);
    GCGE_REQUIRE(gcge_hip_star_coldots2_rows(nlist, list, dx, ldx, dy, ldy, m, dd + 2 * (size_t)m, g_stream) == 0, "star product: sums over the listed rows");
  }
  return 0;
}

// Y[:, 0:m) = A X[:, c_begin : c_begin+m) on a row slab, halo included; d_dots / d_yy as in spmm_rows (3 m doubles of
// scratch behind each when the product is split).  With a split exchange the interior rows are multiplied while the
// halo rows travel, the two boundary strips follow.
static int spmm_halo(GCGE_HIP_MAT_* A, GcgeHipMV* vx, int c_begin, double* dy, long ldy, int m, double* d_dots, double* d_yy,
                     const CgPass* cg = nullptr) {
  const double* dx = vx->d + c_begin;
  if (A->star != nullptr && g_spmm_path == 0 && cg == nullptr && d_dots == nullptr && d_yy == nullptr) {
    const int rc = star_product(A, vx, c_begin, dy, ldy, m, nullptr);
    if (rc != -1) return rc;
  }
  const bool split = g_halo_overlap && A->nghost > 0 && A->exchange_begin != nullptr && A->exchange_end != nullptr &&
                     m <= A->buf_cols && A->ov_hi - A->ov_lo >= A->nrows / 2 &&
                     A->tile == nullptr && A->dense == nullptr;   // (the block and tile forms multiply whole matrices, not row strips)
  if (!split) {
    halo_fetch(A, vx, c_begin, m);
    return spmm_rows(A, 0, A->nrows, dx, vx->ld, dy, ldy, m, d_dots, d_yy, cg);
  }
  GCGE_REQUIRE(A->buf_cols > 0, "MatDotMultiVec: halo plan installed (gcge_hip_mat_set_halo)");
  halo_send(A, dx, vx->ld, m);
  A->exchange_begin(A->sendbuf, A->recvbuf, m, A->exchange_ctx);
  double* d1 = d_dots ? d_dots + m : nullptr; double* d2 = d_dots ? d_dots + 2 * m : nullptr;
  double* y1 = d_yy ? d_yy + m : nullptr;     double* y2 = d_yy ? d_yy + 2 * m : nullptr;
  int rc = spmm_rows(A, A->ov_lo, A->ov_hi, dx, vx->ld, dy, ldy, m, d1, y1, cg);      // interior, overlaps the transfers
  A->exchange_end(A->exchange_ctx);
  halo_recv(A, vx, c_begin, m);
  if (rc == 0) rc = spmm_rows(A, 0, A->ov_lo, dx, vx->ld, dy, ldy, m, d2, y2, cg);     // leading boundary strip
  double* d3 = d_dots ? gcge_hip_stage_d2(2 * (size_t)m) : nullptr;
  if (rc == 0) rc = spmm_rows(A, A->ov_hi, A->nrows, dx, vx->ld, dy, ldy, m, d3, d_yy ? d3 + m : nullptr, cg);   // trailing strip
  if (d_dots) hipLaunchKernelGGL(add3_kernel, dim3((m + 63) / 64), dim3(64), 0, g_stream, d_dots, d1, d2, d3, m);
  if (d_yy) hipLaunchKernelGGL(add3_kernel, dim3((m + 63) / 64), dim3(64), 0, g_stream, d_yy, y1, y2, d3 + m, m);
  return rc;
}

// app_ccs.c:50-139;  mat == NULL copies (identity B)
static void HIP_MatDotMultiVec(void* mat, void** x, void** y, int* start, int* end, struct OPS_* ops) {
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  GcgeHipMV *vx = (GcgeHipMV*)x, *vy = (GcgeHipMV*)y;
  const int m = end[0] - start[0];
  gcge_hip_enter();
  SlotTimer tm_(mat ? "MatDotMultiVec" : "MatDotMultiVec (copy)", m);
  GCGE_REQUIRE(m == end[1] - start[1], "MatDotMultiVec: equal column counts");
  if (m <= 0) return;
  GCGE_REQUIRE(vx != vy || end[0] <= start[1] || end[1] <= start[0], "MatDotMultiVec: x and y ranges must not overlap");
  GCGE_REQUIRE(start[0] >= 0 && end[0] <= vx->ncols && start[1] >= 0 && end[1] <= vy->ncols, "MatDotMultiVec: column ranges");
  if (A != nullptr && A->rect_ncols > 0) {   // a prolongation of the multigrid hierarchy (multigrid.hip): rows of level l x rows of level l + 1
    GCGE_REQUIRE(vx->nrows == A->rect_ncols && vy->nrows == A->nrows, "MatDotMultiVec: shapes of a rectangular matrix");
    GCGE_REQUIRE(gcge_hip_csr_spmm(A->nrows, A->d_rowptr, A->d_colidx, A->d_val, vx->d + start[0], vx->ld, vy->d + start[1], vy->ld, m, g_stream) == 0,
                 "MatDotMultiVec: kernel launch (rectangular matrix)");
    return;
  }
  GCGE_REQUIRE(vx->nrows == vy->nrows, "MatDotMultiVec: equal row counts");
  if (A != nullptr) GCGE_REQUIRE(A->nrows == vy->nrows && A->nrows + A->nghost <= vx->nrows_alloc, "MatDotMultiVec: matrix/vector shapes");
  // blocks and matrix must live in ONE row order (the back-end re-orders matrices without a grid: mat_upload.hip "row orders")
  if (A != nullptr) GCGE_REQUIRE(real_perm(vx->perm) == real_perm(A->perm) && real_perm(vy->perm) == real_perm(A->perm), "MatDotMultiVec: the blocks were created for a matrix in another row order");
  if (A == nullptr) {
    gcge_hip_axpby(vy->nrows, 1.0, vx->d + start[0], vx->ld, 0.0, vy->d + start[1], vy->ld, m, g_stream);
    return;
  }
  double* dy = vy->d + start[1];
  int rc = -1;
  ProfScope prof(0, A, m, 2);
  // Column ranges that are not 16-byte pairs (an odd first column or count: the residual check of a solve with an odd number
  // of locked pairs) would send a matrix WITHOUT a pattern form to the scalar CSR kernel — 23.6 ms instead of 3.7 on BASELINE
  // config 5's matrix.  The whole-matrix forms multiply the enclosing even range of X into a scratch block instead (columns of
  // the padding are allocated and zero), the requested columns are copied out.
  const int xs = start[0] & ~1, xe = (end[0] + 1) & ~1;
  if (A->d_pid == nullptr && (A->star != nullptr || A->dense != nullptr || A->tile != nullptr) && g_spmm_path == 0 &&
      m >= 8 && ((start[0] | start[1] | m) & 1) && xe <= vx->ld) {
    const int mw = xe - xs;
    const long ldt = ((long)mw + 7) / 8 * 8;
    const size_t bytes = (size_t)A->nrows * ldt * sizeof(double);
    double* t = (double*)gcge_hip_pool_alloc(bytes);
    halo_fetch(A, vx, xs, mw);                                             // (row slabs: the halo rows of the widened range)
    rc = spmm_rows(A, 0, A->nrows, vx->d + xs, vx->ld, t, ldt, mw, nullptr, nullptr);
    if (rc == 0) rc = gcge_hip_axpby(vy->nrows, 1.0, t + (start[0] - xs), ldt, 0.0, dy, vy->ld, m, g_stream);
    gcge_hip_pool_free(t, bytes);   // (one stream: whoever takes the block next is ordered behind the copy)
  } else
  if (A->nghost > 0 && m > A->buf_cols) {   // wider than the exchange buffers: column chunks, one after the other
    rc = 0;
    for (int c0 = 0; c0 < m && rc == 0; c0 += A->buf_cols) {
      const int mc = (m - c0 < A->buf_cols) ? m - c0 : A->buf_cols;
      rc = spmm_halo(A, vx, start[0] + c0, dy + c0, vy->ld, mc, nullptr, nullptr);
    }
  } else {
    rc = spmm_halo(A, vx, start[0], dy, vy->ld, m, nullptr, nullptr);
  }
  prof.done();
  GCGE_REQUIRE(rc == 0, "MatDotMultiVec: kernel launch");
}
// How y = A x delivers the column sums x.y and y.y.  pairs: the operands meet the fused kernels' contract.
enum SumsForm {
  SUMS_FUSED,   // by the product's own kernel: pattern matrices, and the fused pad-8 kernel on 16 .. 128 columns of short rows
  SUMS_SWEEP,   // grid form: the plane sweep sums its rows on the way (registers), a short pass over the LIST of the other rows adds theirs
  SUMS_AFTER    // the product, then one sweep over the two blocks
};
static SumsForm sums_form(const GCGE_HIP_MAT_* A, int m, bool pairs) {
  if (A == nullptr) return SUMS_AFTER;
  const bool use_pat = A->d_pid != nullptr && g_spmm_path == 0;
  // generic matrices with long rows (>= 2.5 octets on average): the plain pad-8 kernel with one or two rows per wave
  // plus separate column dots beats the fused kernel (SiO2-like, 36 nnz/row: 6.8 + 1.5 ms against 11 ms)
  const bool long_rows = A->nrows > 0 && (double)A->noct / A->nrows >= 2.5;
  if (pairs && (use_pat || (m >= 16 && m <= 128 && !long_rows))) return SUMS_FUSED;
  return (A->star != nullptr && g_spmm_path == 0) ? SUMS_SWEEP : SUMS_AFTER;
}

// Fused  y = A x  and  dots[j] = sum_r x[r,j] y[r,j]  (the p.w of a CG step) — LOCAL part only; the
// caller reduces over ranks.  Falls back to SpMM + column dots when the fast kernel's alignment
// contract is not met.  Internal entry point of the fused block CG (block_pcg.hip).
extern "C" void gcge_hip_spmm_dot_mv(void* mat, void** x, void** y, int* start, int* end, double* host_dots,
                                     struct OPS_* ops) {
  gcge_hip_spmm_dot2_mv(mat, x, y, start, end, host_dots, nullptr, ops);
}
// host_yy != NULL: additionally yy[j] = sum_r y[r,j]^2 (local part) — free on the pattern path
extern "C" void gcge_hip_spmm_dot2_mv(void* mat, void** x, void** y, int* start, int* end, double* host_dots,
                                      double* host_yy, struct OPS_* ops) {
  gcge_hip_enter();
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  GcgeHipMV *vx = (GcgeHipMV*)x, *vy = (GcgeHipMV*)y;
  const int m = end[0] - start[0];
  if (m <= 0) return;
  const bool aligned = A != nullptr && (m % 2 == 0) && pair_ok(vx, start[0]) && pair_ok(vy, start[1]);
  const SumsForm form = sums_form(A, m, aligned && (A->nghost == 0 || m <= A->buf_cols));
  if (form == SUMS_SWEEP && host_yy != nullptr && vx != vy &&
      vx->nrows == vy->nrows && A->nrows == vy->nrows && A->nrows + A->nghost <= vx->nrows_alloc) {
    ProfScope prof(0, A, m, 2);
    double* dd = gcge_hip_stage_d(4 * (size_t)m);
    const int rc = star_product(A, vx, start[0], vy->d + start[1], vy->ld, m, dd);
    if (rc == 0) {
      prof.done();
      const double* hd = sums_to_host(dd, 4 * (size_t)m);
      for (int j = 0; j < m; ++j) { host_dots[j] = hd[j] + hd[2 * m + j]; host_yy[j] = hd[m + j] + hd[3 * m + j]; }
      return;
    }
    prof.cancel();   // (operands the sweep does not take: the generic route below)
  }
  if (form != SUMS_FUSED) {
    HIP_MatDotMultiVec(mat, x, y, start, end, ops);
    if (host_yy && vx->nrows == vy->nrows) {   // x.y and y.y in one sweep over the two blocks
      double* dd = gcge_hip_stage_d(2 * (size_t)m);
      GCGE_REQUIRE(gcge_hip_coldots2(vx->nrows, vx->d + start[0], vx->ld, vy->d + start[1], vy->ld, m, dd, g_stream) == 0, "spmm_dot: column sums");
      const double* hd = sums_to_host(dd, 2 * (size_t)m);
      memcpy(host_dots, hd, m * sizeof(double));
      memcpy(host_yy, hd + m, m * sizeof(double));
      return;
    }
    gcge_hip_local_inner_prod('D', x, y, start, end, host_dots, 1, ops);       // (LOCAL parts whatever GCGE_SetLocalInnerProdReduces says: the caller reduces)
    if (host_yy) {
      int s2[2] = {start[1], start[1]}, e2[2] = {end[1], end[1]};
      gcge_hip_local_inner_prod('D', y, y, s2, e2, host_yy, 1, ops);
    }
    return;
  }
  GCGE_REQUIRE(vx != vy && vx->nrows == vy->nrows && A->nrows == vy->nrows, "spmm_dot: shapes");
  GCGE_REQUIRE(start[0] >= 0 && end[0] <= vx->ncols && start[1] >= 0 && end[1] <= vy->ncols, "spmm_dot: column ranges");
  GCGE_REQUIRE(A->nrows + A->nghost <= vx->nrows_alloc, "spmm_dot: halo rows allocated");
  GCGE_REQUIRE(A->nghost == 0 || m <= A->buf_cols, "spmm_dot: block wider than the halo buffers");
  double* dd = gcge_hip_stage_d(6 * (size_t)m);            // x.y sums (3 m: total + the strips of a split product), then y.y sums
  double* dyy = host_yy ? dd + 3 * (size_t)m : nullptr;
  ProfScope prof(0, A, m, 2);   // the fused kernel IS the K1 launch of a CG step (same algorithmic bytes: the dots add no HBM traffic)
  int rc = spmm_halo(A, vx, start[0], vy->d + start[1], vy->ld, m, dd, dyy);
  prof.done();
  GCGE_REQUIRE(rc == 0, "spmm_dot: kernel launch");
  double* hd = gcge_hip_stage_h(2 * (size_t)m);   // (the two sums are 3 m apart on the device: two copies, one wait)
  GCGE_HIP_CHECK(hipMemcpyAsync(hd, dd, m * sizeof(double), hipMemcpyDeviceToHost, g_stream));
  if (dyy) GCGE_HIP_CHECK(hipMemcpyAsync(hd + m, dyy, m * sizeof(double), hipMemcpyDeviceToHost, g_stream));
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
  memcpy(host_dots, hd, m * sizeof(double));
  if (host_yy) memcpy(host_yy, hd + m, m * sizeof(double));
}

// The same with the sums LEFT ON THE DEVICE and nothing waited for (the device-scalar loop of block_pcg.hip on matrices whose
// product is stored): y[:, cy : cy + m) = A x[:, cx : cx + m), d_out[0, m) = x.y, d_out[m, 2m) = y.y over the local rows (d_out: 2 m
// doubles).  -1, nothing touched: operands the fused kernels do not take (odd widths or offsets, unaligned blocks).
__global__ void dot2_sum_kernel(int m, const double* __restrict__ a0, const double* __restrict__ a1, const double* __restrict__ b0,
                                const double* __restrict__ b1, double* __restrict__ out) {   // out = [a0 + b0 | a1 + b1] (b: NULL = none)
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) { out[j] = a0[j] + (b0 != nullptr ? b0[j] : 0.0); out[m + j] = a1[j] + (b1 != nullptr ? b1[j] : 0.0); }
}
// 1: gcge_hip_spmm_dot2_dev takes these operands (its contract, for callers that must decide BEFORE touching anything)
extern "C" int gcge_hip_spmm_dot2_dev_ok(void* mat, void** x, void** y, int cx, int cy, int m) {
  const GCGE_HIP_MAT_* A = (const GCGE_HIP_MAT_*)mat;
  const GcgeHipMV *vx = (const GcgeHipMV*)x, *vy = (const GcgeHipMV*)y;
  if (A == nullptr || A->rect_ncols > 0 || vx == nullptr || vy == nullptr) return 0;
  if (m <= 0 || (m & 1) || !pair_ok(vx, cx) || !pair_ok(vy, cy) || vx == vy) return 0;
  if (vx->nrows != vy->nrows || A->nrows != vy->nrows || A->nrows + A->nghost > vx->nrows_alloc) return 0;
  if (A->nghost > 0 && m > A->buf_cols) return 0;
  return 1;
}
extern "C" int gcge_hip_spmm_dot2_dev(void* mat, void** x, void** y, int cx, int cy, int m, double* d_out) {
  gcge_hip_enter();
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  GcgeHipMV *vx = (GcgeHipMV*)x, *vy = (GcgeHipMV*)y;
  if (!gcge_hip_spmm_dot2_dev_ok(mat, x, y, cx, cy, m)) return -1;
  GCGE_REQUIRE(cx >= 0 && cx + m <= vx->ncols && cy >= 0 && cy + m <= vy->ncols, "spmm_dot2_dev: column ranges");
  ProfScope prof(0, A, m, 2);
  const SumsForm form = sums_form(A, m, true);
  int rc = -1;
  if (form == SUMS_SWEEP) {
    double* dd = gcge_hip_stage_d(4 * (size_t)m);                               // sweep: x.y | y.y, listed rows: x.y | y.y
    rc = star_product(A, vx, cx, vy->d + cy, vy->ld, m, dd);
    if (rc == 0) hipLaunchKernelGGL(dot2_sum_kernel, dim3((m + 127) / 128), dim3(128), 0, g_stream, m, (const double*)dd, (const double*)(dd + m),
                                    (const double*)(dd + 2 * (size_t)m), (const double*)(dd + 3 * (size_t)m), d_out);
  }
  if (rc != 0 && form == SUMS_FUSED) {
    double* dd = gcge_hip_stage_d(6 * (size_t)m);                               // x.y (3 m: total + the strips of a split product), then y.y
    rc = spmm_halo(A, vx, cx, vy->d + cy, vy->ld, m, dd, dd + 3 * (size_t)m);
    GCGE_REQUIRE(rc == 0, "spmm_dot2_dev: kernel launch");
    hipLaunchKernelGGL(dot2_sum_kernel, dim3((m + 127) / 128), dim3(128), 0, g_stream, m, (const double*)dd, (const double*)(dd + 3 * (size_t)m),
                       (const double*)nullptr, (const double*)nullptr, d_out);
  } else if (rc != 0) {
    rc = spmm_halo(A, vx, cx, vy->d + cy, vy->ld, m, nullptr, nullptr);
    GCGE_REQUIRE(rc == 0, "spmm_dot2_dev: kernel launch");
    GCGE_REQUIRE(gcge_hip_coldots2(vx->nrows, vx->d + cx, vx->ld, vy->d + cy, vy->ld, m, d_out, g_stream) == 0, "spmm_dot2_dev: column sums");
  }
  prof.done();
  return 0;
}

// ---- the two passes of a fused block-CG iteration (block_pcg.hip) on a pattern matrix -----------------------------
// The product w = A p is formed twice and never stored: pass 1 reads p and returns p.w and w.w (that fixes alpha and
// beta), pass 2 reads p again, rebuilds w in registers and applies  r -= alpha w ; p_new = r + beta p  on the spot.
// 1 + 4 block streams per iteration instead of 2 (product) + 5 (update sweep).  Both return -1 without touching
// anything when the matrix or the operands do not qualify (no pattern form, odd widths, halo wider than the buffers).
extern "C" int gcge_hip_cg_fusable(void* mat, void** p, int ncols) {
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat; GcgeHipMV* vp = (GcgeHipMV*)p;
  if (A == nullptr || A->d_pid == nullptr || g_spmm_path != 0 || getenv("GCGE_CG_NO_RECOMPUTE") != nullptr) return 0;
  if ((ncols & 1) || !pair_ok(vp, 0)) return 0;
  if (A->nghost > 0 && ncols > A->buf_cols) return 0;
  return 1;
}
// Does forming the product twice pay?  Only where the product kernel is bound by HBM: the chain kernel with line exchange
// (about 3 loads per row).  The plain pattern kernel issues 7+ cache-served loads per row and is bound by those, so a
// second product costs more than the two block streams it saves (FE pair n = 10^6: 2.3 against 1.9 ms per iteration).
extern "C" int gcge_hip_cg_recompute_pays(void* mat) {
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  if (A == nullptr || A->d_pid == nullptr) return 0;
  return gcge_hip_mat_pattern_chain(A) == 2;
}
// d_out[0, m) = sum_r p[r,j] (A p)[r,j], d_out[m, 2m) = sum_r (A p)[r,j]^2 over the LOCAL rows, left on the DEVICE (d_out holds
// >= 6 m doubles, the rest is scratch of the split product); fetches the halo rows of p; nothing is waited for
extern "C" int gcge_hip_cg_pass1_dev(void* mat, void** p, int c0, int m, double* d_out) {
  gcge_hip_enter();
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat; GcgeHipMV* vp = (GcgeHipMV*)p;
  if (!gcge_hip_cg_fusable(mat, p, m) || (c0 & 1)) return -1;
  GCGE_REQUIRE(c0 >= 0 && c0 + m <= vp->ncols && A->nrows == vp->nrows && A->nrows + A->nghost <= vp->nrows_alloc, "cg_pass1: shapes");
  double* dd = d_out;
  double* dyy = dd + 3 * (size_t)m;
  ProfScope prof(2, A, m, 1);   // p read
  const CgPass cg = {2, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0};
  const int rc = spmm_halo(A, vp, c0, nullptr, 0, m, dd, dyy, &cg);
  prof.done();
  GCGE_REQUIRE(rc == 0, "cg_pass1: kernel launch");
  GCGE_HIP_CHECK(hipMemcpyAsync(dd + m, dyy, m * sizeof(double), hipMemcpyDeviceToDevice, g_stream));   // both sums side by side
  return 0;
}
// the same with the sums returned to the host (one stream synchronisation)
extern "C" int gcge_hip_cg_pass1_mv(void* mat, void** p, int c0, int m, double* host_pw, double* host_ww) {
  double* dd = gcge_hip_stage_d(6 * (size_t)m);
  if (gcge_hip_cg_pass1_dev(mat, p, c0, m, dd) != 0) return -1;
  const double* hd = sums_to_host(dd, 2 * (size_t)m);
  memcpy(host_pw, hd, m * sizeof(double));
  memcpy(host_ww, hd + m, m * sizeof(double));
  return 0;
}
// r[:, c0:c0+m) -= (A p) diag(alpha); pnew[:, c0:c0+m) = r diag(cr) + p diag(cb); d_rho[j] = sum_r cr_j r[r,j]^2 (local), left on
// the DEVICE.  The halo rows of p must be the ones pass 1 fetched (p unchanged since).  d_alpha / d_beta / d_flag: device, m each.
extern "C" int gcge_hip_cg_pass2_dev(void* mat, void** p, void** r, void** pnew, int c0, int m, const double* d_alpha,
                                     const double* d_beta, const int* d_flag, double* d_rho) {
  gcge_hip_enter();
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  GcgeHipMV *vp = (GcgeHipMV*)p, *vr = (GcgeHipMV*)r, *vn = (GcgeHipMV*)pnew;
  if (!gcge_hip_cg_fusable(mat, p, m) || !pair_ok(vr, c0) || !pair_ok(vn, c0) || vn == vp) return -1;
  GCGE_REQUIRE(c0 >= 0 && c0 + m <= vp->ncols && c0 + m <= vr->ncols && c0 + m <= vn->ncols, "cg_pass2: column ranges");
  GCGE_REQUIRE(A->nrows == vp->nrows && A->nrows == vr->nrows && A->nrows == vn->nrows, "cg_pass2: row counts");
  ProfScope prof(3, A, m, 4);   // p and r read, r and p_new written
  const CgPass cg = {3, vr->d + c0, vr->ld, vn->d + c0, vn->ld, d_alpha, d_beta, d_flag, nullptr, 0};
  const int rc = spmm_rows(A, 0, A->nrows, vp->d + c0, vp->ld, nullptr, 0, m, d_rho, nullptr, &cg);
  prof.done();
  GCGE_REQUIRE(rc == 0, "cg_pass2: kernel launch");
  return 0;
}
extern "C" int gcge_hip_cg_pass2_mv(void* mat, void** p, void** r, void** pnew, int c0, int m, const double* d_alpha,
                                    const double* d_beta, const int* d_flag, double* host_rho) {
  double* dd = gcge_hip_stage_d(6 * (size_t)m);
  if (gcge_hip_cg_pass2_dev(mat, p, r, pnew, c0, m, d_alpha, d_beta, d_flag, dd) != 0) return -1;
  memcpy(host_rho, sums_to_host(dd, (size_t)m), m * sizeof(double));
  return 0;
}

// The same second pass WITHOUT a stored residual (kernel MODE 7): r_k = p_k - beta_{k-1} p_{k-1} is rebuilt from the previous
// direction (pprev, read only; d_betaprev: the beta that formed p_k — zeros in the first iteration, where pprev may be p
// itself), pnew[:, c0:c0+m) = r' diag(cr) + p diag(cb) with r' = r_k - (A p) diag(alpha), d_rho[j] = sum_r cr_j r'[r,j]^2.
// Reads p, pprev, writes pnew: 3 block streams instead of 4.
extern "C" int gcge_hip_cg_pass2i_dev(void* mat, void** p, void** pprev, void** pnew, int c0, int m, const double* d_alpha,
                                      const double* d_beta, const int* d_flag, const double* d_betaprev, double* d_rho) {
  gcge_hip_enter();
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  GcgeHipMV *vp = (GcgeHipMV*)p, *vq = (GcgeHipMV*)pprev, *vn = (GcgeHipMV*)pnew;
  if (!gcge_hip_cg_fusable(mat, p, m) || !pair_ok(vq, c0) || !pair_ok(vn, c0) || vn == vp || vn == vq || d_betaprev == nullptr) return -1;
  GCGE_REQUIRE(c0 >= 0 && c0 + m <= vp->ncols && c0 + m <= vq->ncols && c0 + m <= vn->ncols, "cg_pass2i: column ranges");
  GCGE_REQUIRE(A->nrows == vp->nrows && A->nrows == vq->nrows && A->nrows == vn->nrows, "cg_pass2i: row counts");
  ProfScope prof(3, A, m, 3);   // p and p_prev read, p_new written
  const CgPass cg = {7, vq->d + c0, vq->ld, vn->d + c0, vn->ld, d_alpha, d_beta, d_flag, d_betaprev, 0};
  const int rc = spmm_rows(A, 0, A->nrows, vp->d + c0, vp->ld, nullptr, 0, m, d_rho, nullptr, &cg);
  prof.done();
  GCGE_REQUIRE(rc == 0, "cg_pass2i: kernel launch");
  return 0;
}
extern "C" int gcge_hip_cg_pass2i_mv(void* mat, void** p, void** pprev, void** pnew, int c0, int m, const double* d_alpha,
                                     const double* d_beta, const int* d_flag, const double* d_betaprev, double* host_rho) {
  double* dd = gcge_hip_stage_d(6 * (size_t)m);
  if (gcge_hip_cg_pass2i_dev(mat, p, pprev, pnew, c0, m, d_alpha, d_beta, d_flag, d_betaprev, dd) != 0) return -1;
  memcpy(host_rho, sums_to_host(dd, (size_t)m), m * sizeof(double));
  return 0;
}

// ---- one step of a Chebyshev filter (GCGE_ChebFilter, csrc/host/chfsi.c; GCGE_BACKEND.cheb_step) --------------------------------
//   out[:, o0..o0+m) = alpha (A y[:, y0..) - c y[:, y0..)) - beta z[:, z0..)          out, y, z: three different blocks
// Fused: kernel MODE 7 computes pnew = (p - bp pprev - al (A p)) + cb p from per-column device scalars; with p = y, pprev = z,
// pnew = out and  al = -alpha, bp = beta, cb = -alpha c - 1  that is  y - beta z + alpha A y - alpha c y - y, the step itself: one call
// of gcge_hip_cg_pass2i_dev with every column flagged, 3 block streams and the matrix, its d_rho ignored.  Only where forming the
// product inside the sweep pays (gcge_hip_cg_recompute_pays: the reason is written there), on one rank, with beta != 0 (MODE 7 reads
// pprev) and the three windows on the same even column.  Everything else, and GCGE_CHEB_NO_FUSE=1 (read per call): the ordinary
// product into out, whatever K1 form the handle has, then gcge_hip_cheb_sweep in place on out — 6 block streams and the matrix.
static long g_cheb_stats[3] = {0, 0, 0};      // fused, product + sweep, declined
extern "C" void gcge_hip_cheb_stats(long out[3]) { for (int i = 0; i < 3; ++i) out[i] = g_cheb_stats[i]; }
// one step, with the two sums of GCGE_BACKEND.cheb_step_dots when oo != NULL (then oy != NULL as well): the same checks and the same
// choice of path either way; `stats` counts it
static int cheb_step_any(void* mat, void** y, int y0, void** z, int z0, void** out, int o0, int m, double alpha, double c, double beta,
                         double* oo, double* oy, long* stats) {
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  GcgeHipMV *vy = (GcgeHipMV*)y, *vz = (GcgeHipMV*)z, *vo = (GcgeHipMV*)out;
  const bool hasz = beta != 0.0;
  bool ok = A != nullptr && A->rect_ncols == 0 && vy != nullptr && vo != nullptr && m > 0 && vo != vy && (!hasz || (vz != nullptr && vz != vo && vz != vy));
  ok = ok && y0 >= 0 && y0 + m <= vy->ncols && o0 >= 0 && o0 + m <= vo->ncols && (!hasz || (z0 >= 0 && z0 + m <= vz->ncols));
  ok = ok && A->nrows == vy->nrows && A->nrows == vo->nrows && A->nrows + A->nghost <= vy->nrows_alloc && (!hasz || A->nrows == vz->nrows);
  ok = ok && real_perm(vy->perm) == real_perm(A->perm) && real_perm(vo->perm) == real_perm(A->perm) && (!hasz || real_perm(vz->perm) == real_perm(A->perm));
  if (!ok) { ++stats[2]; return -1; }
  gcge_hip_enter();
  if (hasz && A->nghost == 0 && y0 == z0 && y0 == o0 && !(y0 & 1) && getenv("GCGE_CHEB_NO_FUSE") == nullptr &&
      gcge_hip_cg_fusable(mat, y, m) && gcge_hip_cg_recompute_pays(mat) && pair_ok(vz, z0) && pair_ok(vo, o0)) {
    SlotTimer tm_("Chebyshev step (fused)", m);
    const double *d_al, *d_cb, *d_bp; const int* d_flag;
    gcge_hip_cheb_scalars(m, alpha, c, beta, g_stream, &d_al, &d_cb, &d_bp, &d_flag);
    GCGE_REQUIRE(gcge_hip_cg_pass2i_dev(mat, y, z, out, y0, m, d_al, d_cb, d_flag, d_bp, gcge_hip_stage_d(6 * (size_t)m)) == 0, "Chebyshev step: fused pass");
    if (oo != nullptr)      // the sums from one read of what the pass wrote and of y: 2 more block streams
      GCGE_REQUIRE(gcge_hip_cheb_dots(A->nrows, vo->d + o0, vo->ld, vy->d + y0, vy->ld, m, oo, oy, g_stream) == 0, "Chebyshev step: sums");
    ++stats[0];
    return 0;
  }
  int start[2] = {y0, o0}, end[2] = {y0 + m, o0 + m};
  HIP_MatDotMultiVec(mat, y, out, start, end, nullptr);
  SlotTimer tm_("Chebyshev step (sweep)", m);
  if (oo != nullptr)
    GCGE_REQUIRE(gcge_hip_cheb_sweep_dots(A->nrows, vo->d + o0, vo->ld, vy->d + y0, vy->ld, hasz ? vz->d + z0 : nullptr, hasz ? vz->ld : 0, m, alpha, c,
                                          beta, oo, oy, g_stream) == 0, "Chebyshev step: sweep with sums");
  else
    GCGE_REQUIRE(gcge_hip_cheb_sweep(A->nrows, vo->d + o0, vo->ld, vy->d + y0, vy->ld, hasz ? vz->d + z0 : nullptr, hasz ? vz->ld : 0, m, alpha, c, beta,
                                     g_stream) == 0, "Chebyshev step: sweep");
  ++stats[1];
  return 0;
}
extern "C" int gcge_hip_cheb_step_mv(void* mat, void** y, int y0, void** z, int z0, void** out, int o0, int m, double alpha, double c,
                                     double beta) {
  return cheb_step_any(mat, y, y0, z, z0, out, o0, m, alpha, c, beta, nullptr, nullptr, g_cheb_stats);
}
// The step with the sums of the kernel polynomial method (GCGE_ChebMoments, csrc/host/chfsi.c; GCGE_BACKEND.cheb_step_dots):
// gcge_hip_cheb_step_mv's decisions, and oo[j] = sum out[r, j]^2, oy[j] = sum out[r, j] y[r, j] over the local rows on the host.  Fused:
// the MODE-7 pass, then gcge_hip_cheb_dots (3 + 2 block streams); otherwise the product, then gcge_hip_cheb_sweep_dots (6 streams, as
// the step without sums).  The slots would add two MultiVecLocalInnerProd('D') to either: 3 to 4 more reads, two launches, two drains.
static long g_cheb_step_dots_stats[3] = {0, 0, 0};      // fused, product + sweep, declined
extern "C" void gcge_hip_cheb_step_dots_stats(long out[3]) { for (int i = 0; i < 3; ++i) out[i] = g_cheb_step_dots_stats[i]; }
extern "C" int gcge_hip_cheb_step_dots_mv(void* mat, void** y, int y0, void** z, int z0, void** out, int o0, int m, double alpha, double c,
                                          double beta, double* oo, double* oy) {
  if (oo == nullptr || oy == nullptr) { ++g_cheb_step_dots_stats[2]; return -1; }
  return cheb_step_any(mat, y, y0, z, z0, out, o0, m, alpha, c, beta, oo, oy, g_cheb_step_dots_stats);
}
static int HIP_ChebStepDots(void* mat, void** y, int y0, void** z, int z0, void** out, int o0, int m, double alpha, double c, double beta,
                            double* oo, double* oy, struct OPS_* ops) {
  (void)ops;
  return gcge_hip_cheb_step_dots_mv(mat, y, y0, z, z0, out, o0, m, alpha, c, beta, oo, oy) == 0 ? 1 : 0;
}
static int HIP_ChebStep(void* mat, void** y, int y0, void** z, int z0, void** out, int o0, int m, double alpha, double c, double beta,
                        struct OPS_* ops) {
  (void)ops;
  return gcge_hip_cheb_step_mv(mat, y, y0, z, z0, out, o0, m, alpha, c, beta) == 0 ? 1 : 0;
}

// ---- the sums of a band-pass filter (GCGE_ChebBandFilter, csrc/host/chfsi.c; GCGE_BACKEND.cheb_accum) ----------------------------
//   acc[:, a0..a0+m) = [acc[:, a0..) +] mu_a ta[:, ta0..) + mu_b tb[:, tb0..)         acc, ta, tb: three different blocks
// one call of gcge_hip_cheb_accum (cheb_sweeps.hip) on g_stream: 4 block streams for two terms where two MultiVecAxpby take 6.
// tb == NULL: one term; init: acc is not read.
static long g_cheb_accum_stats[3] = {0, 0, 0};      // two-term calls, one-term calls, declined
extern "C" void gcge_hip_cheb_accum_stats(long out[3]) { for (int i = 0; i < 3; ++i) out[i] = g_cheb_accum_stats[i]; }
extern "C" int gcge_hip_cheb_accum_mv(void** acc, int a0, void** ta, int ta0, double mu_a, void** tb, int tb0, double mu_b, int m, int init) {
  GcgeHipMV *vc = (GcgeHipMV*)acc, *va = (GcgeHipMV*)ta, *vb = (GcgeHipMV*)tb;
  const bool hasb = vb != nullptr;
  bool ok = vc != nullptr && va != nullptr && m > 0 && vc != va && (!hasb || (vb != vc && vb != va));
  ok = ok && a0 >= 0 && a0 + m <= vc->ncols && ta0 >= 0 && ta0 + m <= va->ncols && (!hasb || (tb0 >= 0 && tb0 + m <= vb->ncols));
  ok = ok && vc->nrows == va->nrows && (!hasb || vc->nrows == vb->nrows);
  ok = ok && real_perm(va->perm) == real_perm(vc->perm) && (!hasb || real_perm(vb->perm) == real_perm(vc->perm));
  if (!ok) { ++g_cheb_accum_stats[2]; return -1; }
  gcge_hip_enter();
  SlotTimer tm_("Chebyshev sum", m);
  GCGE_REQUIRE(gcge_hip_cheb_accum(vc->nrows, vc->d + a0, vc->ld, va->d + ta0, va->ld, mu_a, hasb ? vb->d + tb0 : nullptr, hasb ? vb->ld : 0, mu_b, m,
                                   init, g_stream) == 0, "Chebyshev sum: sweep");
  ++g_cheb_accum_stats[hasb ? 0 : 1];
  return 0;
}
static int HIP_ChebAccum(void** acc, int a0, void** ta, int ta0, double mu_a, void** tb, int tb0, double mu_b, int m, int init, struct OPS_* ops) {
  (void)ops;
  return gcge_hip_cheb_accum_mv(acc, a0, ta, ta0, mu_a, tb, tb0, mu_b, m, init) == 0 ? 1 : 0;
}

// ---- the start sweep (kernel MODES 5 / 6): r[:, rc0:rc0+m) = b[:, bc0:bc0+m) - A x[:, xc0:xc0+m), pnew[:, rc0:rc0+m) = r, and the
// column sums of r^2 over the LOCAL rows into dd (6 m doubles: 3 m of scratch behind the sums when the product is split); fetches the
// halo rows of x.  vb == NULL: b_j = d_scale[j] x_j is never formed (MODE 6).  Behind gcge_hip_cg_start_mv, gcge_hip_cg_start_scaled_mv
// and the V-cycle's residual, each with its own answer to operands the sweep does not take.
// 1: matrix and operands qualify (pattern form, 16-byte pairs, r and pnew apart from x, halo buffers wide enough)
static int start_sweep_takes(const GCGE_HIP_MAT_* A, const GcgeHipMV* vx, int xc0, const GcgeHipMV* vb, int bc0, const GcgeHipMV* vr,
                             const GcgeHipMV* vn, int rc0, int m) {
  if (A == nullptr || A->d_pid == nullptr || g_spmm_path != 0) return 0;
  if ((m & 1) || !pair_ok(vx, xc0) || (vb != nullptr && !pair_ok(vb, bc0)) || !pair_ok(vr, rc0) || !pair_ok(vn, rc0)) return 0;
  if (vr == vx || vn == vx || (A->nghost > 0 && m > A->buf_cols)) return 0;
  return 1;
}
// taken / declined for the odd first column of b alone (everything else qualifies, x and r included): gcge_hip_sweep_stats
static long g_sweep_stats[4] = {0, 0, 0, 0};
extern "C" void gcge_hip_sweep_stats(long out[4]) { for (int i = 0; i < 4; ++i) out[i] = g_sweep_stats[i]; }
static int start_sweep_odd_b_only(const GCGE_HIP_MAT_* A, const GcgeHipMV* vx, int xc0, const GcgeHipMV* vb, int bc0, const GcgeHipMV* vr,
                                  const GcgeHipMV* vn, int rc0, int m) {
  if (vb == nullptr || !(bc0 & 1)) return 0;
  return start_sweep_takes(A, vx, xc0, vb, bc0 & ~1, vr, vn, rc0, m);
}
// (d_scale with vb: MODE 8, b is the store target of the right-hand sides the sweep forms)
static int start_sweep(GCGE_HIP_MAT_* A, GcgeHipMV* vx, int xc0, GcgeHipMV* vb, int bc0, const double* d_scale, GcgeHipMV* vr, GcgeHipMV* vn,
                       int rc0, int m, double* dd) {
  const CgPass cg = {vb == nullptr ? 6 : (d_scale != nullptr ? 8 : 5), vr->d + rc0, vr->ld, vn->d + rc0, vn->ld, d_scale, nullptr, nullptr,
                     vb != nullptr ? vb->d + bc0 : nullptr, vb != nullptr ? vb->ld : 0};
  return spmm_halo(A, vx, xc0, nullptr, 0, m, dd, nullptr, &cg);
}

// Start of the block CG in one sweep: r = b - A x, p0 = r (same columns rc0.. of the block p0), host_rho[j] = sum over the LOCAL
// rows of r[r,j]^2.  -1 without touching anything when matrix or operands do not qualify.
extern "C" int gcge_hip_cg_start_mv(void* mat, void** x, int xc0, void** b, int bc0, void** r, void** p0, int rc0, int m,
                                    double* host_rho) {
  gcge_hip_enter();
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  GcgeHipMV *vx = (GcgeHipMV*)x, *vb = (GcgeHipMV*)b, *vr = (GcgeHipMV*)r, *vp = (GcgeHipMV*)p0;
  if (getenv("GCGE_CG_NO_RECOMPUTE") != nullptr) return -1;
  if (!start_sweep_takes(A, vx, xc0, vb, bc0, vr, vp, rc0, m)) { g_sweep_stats[1] += start_sweep_odd_b_only(A, vx, xc0, vb, bc0, vr, vp, rc0, m); return -1; }
  ++g_sweep_stats[0];
  GCGE_REQUIRE(xc0 >= 0 && xc0 + m <= vx->ncols && bc0 >= 0 && bc0 + m <= vb->ncols && rc0 >= 0 && rc0 + m <= vr->ncols &&
               rc0 + m <= vp->ncols, "cg_start: column ranges");
  GCGE_REQUIRE(A->nrows == vx->nrows && A->nrows == vb->nrows && A->nrows == vr->nrows && A->nrows == vp->nrows &&
               A->nrows + A->nghost <= vx->nrows_alloc, "cg_start: shapes");
  double* dd = gcge_hip_stage_d(6 * (size_t)m);
  const int rc = start_sweep(A, vx, xc0, vb, bc0, nullptr, vr, vp, rc0, m, dd);
  GCGE_REQUIRE(rc == 0, "cg_start: kernel launch");
  memcpy(host_rho, sums_to_host(dd, (size_t)m), m * sizeof(double));
  return 0;
}

// The same start for right-hand sides b_j = scale_j x_j (x = the initial guess): the GCG driver's systems
// A w = (lambda + sigma) x start from w = x, so b is never formed and never read.  host_scale: m factors.
// b != NULL (kernel MODE 8): the right-hand sides the sweep forms, b[:, bc0:bc0+m) = x[:, xc0:xc0+m) diag(scale) rounded once, are
// stored as well — for a solver that reads b later (BlockAMG) while x is an initial guess that lies in another block and is only
// read (GCGE_LINSOL_ARGS.x_src).  b must be a block other than x, r and p0; one rank (no halo rows).
extern "C" int gcge_hip_cg_start_scaled_b_mv(void* mat, void** x, int xc0, const double* host_scale, void** r, void** p0, int rc0,
                                             int m, void** b, int bc0, double* host_rho) {
  gcge_hip_enter();
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  GcgeHipMV *vx = (GcgeHipMV*)x, *vr = (GcgeHipMV*)r, *vp = (GcgeHipMV*)p0, *vb = (GcgeHipMV*)b;
  if (getenv("GCGE_CG_NO_RECOMPUTE") != nullptr || !start_sweep_takes(A, vx, xc0, vb, bc0, vr, vp, rc0, m)) return -1;
  if (vb != nullptr && (vb == vx || vb == vr || vb == vp || A->nghost > 0 || bc0 < 0 || bc0 + m > vb->ncols || vb->nrows != A->nrows)) return -1;
  GCGE_REQUIRE(xc0 >= 0 && xc0 + m <= vx->ncols && rc0 >= 0 && rc0 + m <= vr->ncols && rc0 + m <= vp->ncols, "cg_start: column ranges");
  GCGE_REQUIRE(A->nrows == vx->nrows && A->nrows == vr->nrows && A->nrows == vp->nrows &&
               A->nrows + A->nghost <= vx->nrows_alloc, "cg_start: shapes");
  double* dd = gcge_hip_stage_d(7 * (size_t)m);           // [0, 6 m): the sweep's, [6 m, 7 m): scale
  double* hs = gcge_hip_stage_h(2 * (size_t)m);
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));   // the staging buffers are reused
  memcpy(hs, host_scale, m * sizeof(double));
  GCGE_HIP_CHECK(hipMemcpyAsync(dd + 6 * (size_t)m, hs, m * sizeof(double), hipMemcpyHostToDevice, g_stream));
  if (start_sweep(A, vx, xc0, vb, bc0, dd + 6 * (size_t)m, vr, vp, rc0, m, dd) != 0) return -1;
  memcpy(host_rho, sums_to_host(dd, (size_t)m), m * sizeof(double));   // (behind the upload from the same pinned block in stream order)
  return 0;
}
extern "C" int gcge_hip_cg_start_scaled_mv(void* mat, void** x, int xc0, const double* host_scale, void** r, void** p0, int rc0,
                                           int m, double* host_rho) {
  return gcge_hip_cg_start_scaled_b_mv(mat, x, xc0, host_scale, r, p0, rc0, m, nullptr, 0, host_rho);
}

// ---- two steps of a V-cycle in one sweep each (GCGE_BACKEND.amg_residual / amg_prolong_add; csrc/host/lin_sol.c) ----------
// r[:, rc0:rc0+m) = b[:, bc0:bc0+m) - A x[:, xc0:xc0+m): the start sweep of the block CG with ONE store — the
// product is rounded on its own and then subtracted from b, exactly what MatDotMultiVec + MultiVecAxpby(1, b, -1, r) leave
// (reference src/ops_lin_sol.c:596-606): 3 block streams instead of 5.  Pattern matrices only; 0 = declined, nothing touched.
static int HIP_AmgResidual(void* mat, void** b, int bc0, void** x, int xc0, void** r, int rc0, int m, struct OPS_* ops) {
  (void)ops;
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  GcgeHipMV *vx = (GcgeHipMV*)x, *vb = (GcgeHipMV*)b, *vr = (GcgeHipMV*)r;
  if (m > 0 && A != nullptr && A->rect_ncols == 0 && vr != vb) g_sweep_stats[3] += start_sweep_odd_b_only(A, vx, xc0, vb, bc0, vr, vr, rc0, m);
  if (m <= 0 || !start_sweep_takes(A, vx, xc0, vb, bc0, vr, vr, rc0, m) || A->rect_ncols > 0 || vr == vb) return 0;
  if (xc0 < 0 || xc0 + m > vx->ncols || bc0 < 0 || bc0 + m > vb->ncols || rc0 < 0 || rc0 + m > vr->ncols) return 0;
  if (A->nrows != vx->nrows || A->nrows != vb->nrows || A->nrows != vr->nrows || A->nrows + A->nghost > vx->nrows_alloc) return 0;
  if (real_perm(vx->perm) != real_perm(A->perm) || real_perm(vb->perm) != real_perm(A->perm) || real_perm(vr->perm) != real_perm(A->perm)) return 0;
  gcge_hip_enter();
  ++g_sweep_stats[2];
  SlotTimer tm_("AMG residual (fused)", m);
  double* dd = gcge_hip_stage_d(6 * (size_t)m);                         // the sweep's column sums |r_j|^2: not used here
  const int rc = start_sweep(A, vx, xc0, vb, bc0, nullptr, vr, vr, rc0, m, dd);
  GCGE_REQUIRE(rc == 0, "AMG residual: kernel launch");
  return 1;
}

// xf[:, f0:f0+m) += P xc[:, c0:c0+m) for a prolongation with ONE entry per row (aggregation: gcge_multigrid.h) — the product is
// rounded, then added (no fused multiply-add), as MatDotMultiVec into a work block + MultiVecAxpby(1, work, 1, xf) do
// (reference src/ops_lin_sol.c:626-640): the fine block is read and written once, the work block not at all.
typedef double v2d_pa __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void prolong_add_kernel(long nrows, const int* __restrict__ colidx, const double* __restrict__ val,
    const double* __restrict__ xc, long ldc, double* __restrict__ xf, long ldf, int m2, int tpr) {
#pragma clang fp contract(off)
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  if (tx >= m2) return;
  const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + rpb - 1) / rpb * rpb;
  const long rend = min(nrows, ((long)blockIdx.x + 1) * slab);
  for (long row = (long)blockIdx.x * slab + ty; row < rend; row += 2L * rpb) {
    const long row2 = row + rpb;
    const bool two = row2 < rend;
    const long rb = two ? row2 : row;
    const int ca = colidx[row], cb = colidx[rb];
    const double va = val[row], vb = val[rb];
    const v2d_pa ea = *reinterpret_cast<const v2d_pa*>(xc + (long)ca * ldc + 2 * tx);
    const v2d_pa eb = *reinterpret_cast<const v2d_pa*>(xc + (long)cb * ldc + 2 * tx);
    const v2d_pa fa = __builtin_nontemporal_load(reinterpret_cast<const v2d_pa*>(xf + row * ldf + 2 * tx));
    const v2d_pa fb = __builtin_nontemporal_load(reinterpret_cast<const v2d_pa*>(xf + rb * ldf + 2 * tx));
    const v2d_pa ta = {va * ea.x, va * ea.y}, tb = {vb * eb.x, vb * eb.y};
    __builtin_nontemporal_store(v2d_pa{ta.x + fa.x, ta.y + fa.y}, reinterpret_cast<v2d_pa*>(xf + row * ldf + 2 * tx));
    if (two) __builtin_nontemporal_store(v2d_pa{tb.x + fb.x, tb.y + fb.y}, reinterpret_cast<v2d_pa*>(xf + rb * ldf + 2 * tx));
  }
}
static int HIP_AmgProlongAdd(void* matP, void** xc, int c0, void** xf, int f0, int m, struct OPS_* ops) {
  (void)ops;
  GCGE_HIP_MAT_* P = (GCGE_HIP_MAT_*)matP;
  GcgeHipMV *vc = (GcgeHipMV*)xc, *vf = (GcgeHipMV*)xf;
  if (P == nullptr || P->rect_ncols <= 0 || P->rect_one_per_row == 0 || m <= 0 || m / 2 > 256) return 0;
  if ((m & 1) || !pair_ok(vc, c0) || !pair_ok(vf, f0) || vc == vf) return 0;
  if (vc->nrows != P->rect_ncols || vf->nrows != P->nrows || c0 < 0 || c0 + m > vc->ncols || f0 < 0 || f0 + m > vf->ncols) return 0;
  gcge_hip_enter();
  SlotTimer tm_("AMG prolongation + correction (fused)", m);
  const int m2 = m / 2;
  int tpr = 1; while (tpr < m2) tpr *= 2;
  const int rpb = 256 / tpr;
  long g = ((long)P->nrows + (long)rpb * 8 - 1) / ((long)rpb * 8); if (g > 8192) g = 8192; if (g < 1) g = 1;
  hipLaunchKernelGGL(prolong_add_kernel, dim3((unsigned)g), dim3(256), 0, g_stream, (long)P->nrows, (const int*)P->d_colidx, (const double*)P->d_val,
                     (const double*)(vc->d + c0), (long)vc->ld, vf->d + f0, (long)vf->ld, m2, tpr);
  GCGE_REQUIRE(hipGetLastError() == hipSuccess, "AMG prolongation + correction: kernel launch");
  return 1;
}

// b[:, bc0:bc0+m) = x[:, xc0:xc0+m) diag(scale): the right-hand sides (lambda_j + sigma) x_j of the GCG driver's W systems for a
// BlockAMG that takes them as scale factors (GCGE_BACKEND.amg_form_rhs) — one read, one write, each product rounded once like the
// column scaling after a copy (MatDotMultiVec(B = NULL) + MultiVecLinearComb: reference src/ops_eig_sol_gcg.c:560-577)
__global__ __launch_bounds__(256) void scaled_copy_kernel(long nrows, const double* __restrict__ x, long ldx, double* __restrict__ b, long ldb,
    int m2, const double* __restrict__ scale, int tpr) {
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  if (tx >= m2) return;
  const v2d_pa sc = {scale[2 * tx], scale[2 * tx + 1]};
  const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + rpb - 1) / rpb * rpb;
  const long rend = min(nrows, ((long)blockIdx.x + 1) * slab);
  long row = (long)blockIdx.x * slab + ty;
  for (; row + 3L * rpb < rend; row += 4L * rpb) {
    v2d_pa a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d_pa*>(x + (row + (long)u * rpb) * ldx + 2 * tx));
#pragma unroll
    for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(v2d_pa{a[u].x * sc.x, a[u].y * sc.y}, reinterpret_cast<v2d_pa*>(b + (row + (long)u * rpb) * ldb + 2 * tx));
  }
  for (; row < rend; row += rpb) {
    const v2d_pa a = *reinterpret_cast<const v2d_pa*>(x + row * ldx + 2 * tx);
    *reinterpret_cast<v2d_pa*>(b + row * ldb + 2 * tx) = v2d_pa{a.x * sc.x, a.y * sc.y};
  }
}
static int HIP_AmgFormRhs(void** b, int bc0, void** x, int xc0, const double* scale, int m, struct OPS_* ops) {
  (void)ops;
  GcgeHipMV *vb = (GcgeHipMV*)b, *vx = (GcgeHipMV*)x;
  if (scale == nullptr || m <= 0 || m / 2 > 256 || (m & 1) || !pair_ok(vb, bc0) || !pair_ok(vx, xc0) || vb->nrows != vx->nrows) return 0;
  if (bc0 < 0 || bc0 + m > vb->ncols || xc0 < 0 || xc0 + m > vx->ncols) return 0;
  if (vb == vx && bc0 < xc0 + m && xc0 < bc0 + m) return 0;
  gcge_hip_enter();
  SlotTimer tm_("AMG right-hand sides (x diag(scale))", m);
  double* dd = gcge_hip_stage_d((size_t)m);
  double* hs = gcge_hip_stage_h((size_t)m);
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));   // the staging buffers are reused
  memcpy(hs, scale, m * sizeof(double));
  GCGE_HIP_CHECK(hipMemcpyAsync(dd, hs, m * sizeof(double), hipMemcpyHostToDevice, g_stream));
  const int m2 = m / 2;
  int tpr = 1; while (tpr < m2) tpr *= 2;
  const int rpb = 256 / tpr;
  long g = ((long)vx->nrows + (long)rpb * 8 - 1) / ((long)rpb * 8); if (g > 8192) g = 8192; if (g < 1) g = 1;
  hipLaunchKernelGGL(scaled_copy_kernel, dim3((unsigned)g), dim3(256), 0, g_stream, (long)vx->nrows, (const double*)(vx->d + xc0), (long)vx->ld,
                     vb->d + bc0, (long)vb->ld, m2, (const double*)dd, tpr);
  GCGE_REQUIRE(hipGetLastError() == hipSuccess, "AMG right-hand sides: kernel launch");
  return 1;
}

// Residuals of Ritz pairs of a standard problem in one read of x (GCGE_RESIDUAL_FN, include/gcge_ops.h; kernel MODE 4 of
// spmm_pattern.hip): res_sq[j] = sum over the local rows of ((A x_j) - lambda_j x_j)^2.  Declines (0) for B != NULL and
// blocks that cannot be walked in 16-byte column pairs; matrices without pattern form take resid_sq_stored above.  Odd
// column ranges are widened to even ones (the extra columns are computed and dropped).
// ... and for the matrices whose product cannot carry the sums (no pattern form: the plane sweep, dense blocks, pad-8): the product
// into a scratch block, then ONE sweep over it and x — 2 block streams behind the product instead of the 9 of the five slot calls
// (round 4; config 5: 13 -> 5 ms per outer iteration).  Chunks of <= 64 columns (the halo buffers' width on slabs).
// Round 5: the GENERALISED problem (B != NULL; reference src/ops_eig_sol_gcg.c:195-315: A x, B x, lambda B x, the difference, its
// column norms = 11 block streams through five slots) takes the same route with two scratch blocks: A x and B x by the products
// (whatever K1 form each matrix has), then ONE sweep sum_r ((A x)[r,j] - lambda_j (B x)[r,j])^2 over the two — 2 + 2 + 2 streams.
static int resid_sq_stored(GCGE_HIP_MAT_* A, GcgeHipMV* vx, int start, int end, const double* lambda, double* res_sq, GCGE_HIP_MAT_* Bm = nullptr) {
  if (getenv("GCGE_NO_STORED_RESIDUAL_HOOK") != nullptr) return 0;
  if (!pair_ok(vx, 0) || A->nrows + A->nghost > vx->nrows_alloc) return 0;
  if (Bm != nullptr && (Bm->nrows != A->nrows || Bm->rect_ncols > 0 || Bm->nrows + Bm->nghost > vx->nrows_alloc)) return 0;
  const int c0 = start & ~1, c1 = (end + 1) & ~1;
  if (c1 > vx->ld) return 0;
  const int chunk = 64;
  const size_t bytes = (size_t)A->nrows * chunk * sizeof(double);
  double* t = (double*)gcge_hip_pool_alloc(bytes);
  double* tb = Bm != nullptr ? (double*)gcge_hip_pool_alloc(bytes) : nullptr;
  int ok = 1;
  for (int b0 = c0; b0 < c1 && ok; b0 += chunk) {
    const int m = std::min(chunk, c1 - b0);
    if (A->nghost > 0 && m > A->buf_cols) { ok = 0; break; }
    if (Bm != nullptr && Bm->nghost > 0 && m > Bm->buf_cols) { ok = 0; break; }
    double* dd = gcge_hip_stage_d(2 * (size_t)m);
    GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));   // the pinned staging may still feed an upload of the previous chunk / slot call
    double* hl = gcge_hip_stage_h(2 * (size_t)m);
    for (int j = 0; j < m; ++j) hl[j] = (b0 + j >= start && b0 + j < end) ? lambda[b0 + j - start] : 0.0;
    GCGE_HIP_CHECK(hipMemcpyAsync(dd + m, hl, m * sizeof(double), hipMemcpyHostToDevice, g_stream));
    const int rc = spmm_halo(A, vx, b0, t, (long)m, m, nullptr, nullptr);
    GCGE_REQUIRE(rc == 0, "residual norms: product");
    if (Bm != nullptr) GCGE_REQUIRE(spmm_halo(Bm, vx, b0, tb, (long)m, m, nullptr, nullptr) == 0, "residual norms: product with B");
    GCGE_REQUIRE(gcge_hip_resid_sq(A->nrows, t, (long)m, Bm != nullptr ? tb : vx->d + b0, Bm != nullptr ? (long)m : vx->ld, m, dd + m, dd, g_stream) == 0, "residual norms: sweep");
    const double* hr = sums_to_host(dd, (size_t)m);   // (behind the upload from the same pinned block in stream order)
    for (int j = 0; j < m; ++j) if (b0 + j >= start && b0 + j < end) res_sq[b0 + j - start] = hr[j];
  }
  gcge_hip_pool_free(t, bytes);
  if (tb != nullptr) gcge_hip_pool_free(tb, bytes);
  return ok;
}
static int HIP_ResidualSq(void* mat, void* matB, void** x, int start, int end, const double* lambda, double* res_sq) {
  gcge_hip_enter();
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat; GcgeHipMV* vx = (GcgeHipMV*)x;
  if (A == nullptr || end <= start) return 0;
  const int c0 = start & ~1, c1 = (end + 1) & ~1, m = c1 - c0;
  if (c1 > vx->ld || A->nrows != vx->nrows) return 0;
  if (matB != nullptr) return getenv("GCGE_NO_GENERAL_RESIDUAL_HOOK") == nullptr ? resid_sq_stored(A, vx, start, end, lambda, res_sq, (GCGE_HIP_MAT_*)matB) : 0;
  if (!gcge_hip_cg_fusable(mat, x, m)) return resid_sq_stored(A, vx, start, end, lambda, res_sq);
  double* dd = gcge_hip_stage_d(7 * (size_t)m);
  double* d_lam = dd + 6 * (size_t)m;
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));   // the pinned staging may still feed an upload of the previous slot call
  double* hl = gcge_hip_stage_h(2 * (size_t)m);
  for (int j = 0; j < m; ++j) hl[j] = (c0 + j >= start && c0 + j < end) ? lambda[c0 + j - start] : 0.0;
  GCGE_HIP_CHECK(hipMemcpyAsync(d_lam, hl, m * sizeof(double), hipMemcpyHostToDevice, g_stream));
  const CgPass cg = {4, nullptr, 0, nullptr, 0, d_lam, nullptr, nullptr, nullptr, 0};
  const int rc = spmm_halo(A, vx, c0, nullptr, 0, m, dd, nullptr, &cg);
  GCGE_REQUIRE(rc == 0, "residual norms: kernel launch");
  const double* hr = sums_to_host(dd, (size_t)m);   // (behind the upload from the same pinned block in stream order)
  for (int j = start; j < end; ++j) res_sq[j - start] = hr[j - c0];
  return 1;
}

extern "C" void* gcge_hip_residual_hook(void) { return (void*)HIP_ResidualSq; }   /* for tests */

// app_ccs.c:140-150 — symmetric matrices: the product itself; a rectangular matrix (a prolongation P_l, used transposed as the
// restriction by DefaultMultiVecFromItoJ, src/ops_multi_grid.c:95-113) through the transposed CSR triple kept beside it
static void HIP_MatTransDotMultiVec(void* mat, void** x, void** y, int* start, int* end, struct OPS_* ops) {
  GCGE_HIP_MAT_* A = (GCGE_HIP_MAT_*)mat;
  if (A == nullptr || A->rect_ncols == 0) { HIP_MatDotMultiVec(mat, x, y, start, end, ops); return; }
  GcgeHipMV *vx = (GcgeHipMV*)x, *vy = (GcgeHipMV*)y;
  const int m = end[0] - start[0];
  gcge_hip_enter();
  SlotTimer tm_("MatTransDotMultiVec", m);
  GCGE_REQUIRE(m == end[1] - start[1], "MatTransDotMultiVec: equal column counts");
  if (m <= 0) return;
  GCGE_REQUIRE(start[0] >= 0 && end[0] <= vx->ncols && start[1] >= 0 && end[1] <= vy->ncols, "MatTransDotMultiVec: column ranges");
  GCGE_REQUIRE(vx != vy && vx->nrows == A->nrows && vy->nrows == A->rect_ncols, "MatTransDotMultiVec: shapes of a rectangular matrix");
  GCGE_REQUIRE(gcge_hip_csr_spmm(A->rect_ncols, A->d_t_rowptr, A->d_t_colidx, A->d_t_val, vx->d + start[0], vx->ld, vy->d + start[1], vy->ld, m, g_stream) == 0,
               "MatTransDotMultiVec: kernel launch (rectangular matrix)");
}

// what this file fills of the table and the back-end record OPS_HIP_Set hands out
extern "C" void gcge_hip_product_slots(struct OPS_* ops, GCGE_BACKEND* be) {
  ops->MatDotMultiVec      = HIP_MatDotMultiVec;
  ops->MatTransDotMultiVec = HIP_MatTransDotMultiVec;
  be->residual_sq     = HIP_ResidualSq;
  be->amg_residual    = HIP_AmgResidual;          // r = b - A x and x += P e as one sweep each
  be->amg_prolong_add = HIP_AmgProlongAdd;
  be->amg_form_rhs    = HIP_AmgFormRhs;           // b = x diag(scale) in one sweep
  be->cheb_step       = HIP_ChebStep;             // one step of a Chebyshev filter: fused on pattern matrices, product + one sweep otherwise
  be->cheb_accum      = HIP_ChebAccum;            // two iterates of a band-pass filter added to its sum in one sweep
  be->cheb_step_dots  = HIP_ChebStepDots;         // the step with the two column sums of the kernel polynomial method, no pass of their own
}
