// app_hip — the MI355X back-end behind GCGE's operator table.
//
// Counterpart of the reference's app/app_ccs.c (sparse matrix + block of vectors)
// with every O(n) operand resident in HBM: OPS_HIP_Set fills the same slots
// OPS_CCS_Set does (app_ccs.c:213-249), each slot keeps the contract of SURVEY.md
// Appendix A, and small dense results are returned to HOST pointers, complete on
// return (the solver layers are synchronous).  Handles are opaque:
//   matrix       GCGE_HIP_MAT  (CSR + pad-8 copy on the device)      <- CCSMAT   (app_ccs.h:20-24)
//   multivector  GcgeHipMV     (row-major n x ld block on the device) <- LAPACKVEC (app_lapack.h:17-20)
#include <hip/hip_runtime.h>
#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <unordered_map>
#include <algorithm>

#include "gcge_hip.h"
#include "gcge_solver.h"
#include "gcge_hip_internal.h"

static hipStream_t g_stream = nullptr;
static int g_inited = 0;
static double* g_stage_d = nullptr; static size_t g_stage_d_len = 0;   // device staging (doubles)
static double* g_stage_h = nullptr; static size_t g_stage_h_len = 0;   // pinned host staging
static int g_spmm_path = 0;   // 0: automatic (pattern > dense blocks + remainder > X tiles > pad-8 > CSR), 2: no pattern path, 3: pad-8 / CSR only, 4: no block form (tile form if present)
extern "C" void gcge_hip_set_spmm_path(int path) { g_spmm_path = path; }
static int g_offset_patterns = 1;   // 1: stencils with row-dependent coefficients take the pattern kernels with streamed values
extern "C" void gcge_hip_set_offset_patterns(int on) { g_offset_patterns = on; }
static int g_rand_mode = 0; static unsigned long long g_rand_seed = 0x5DEECE66Dull;

// ------------------------------------------------------------------ per-slot wall time (measurement aid, off by default)
// gcge_hip_slot_timing(1): every slot call is followed by a stream synchronisation and its wall time is added to a bucket
// (slot, width class of the column range it worked on); gcge_hip_slot_timing_report prints the buckets.  Used to see where
// a solver stack that was NOT written for this layout spends its time (tests/refstack_on_hip.py).
#include <map>
#include <tuple>
#include <string>
static int g_slot_timing = 0;
static std::map<std::string, std::pair<long, double>> g_slot_time;
SlotTimer::SlotTimer(const char* n, int c) : name(n), cols(c), on(g_slot_timing != 0) { if (on) t0 = std::chrono::steady_clock::now(); }
SlotTimer::~SlotTimer() {
  if (!on) return;
  hipStreamSynchronize(g_stream);
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const char* cls = cols <= 1 ? "1 col" : cols <= 8 ? "2-8 cols" : cols <= 32 ? "9-32 cols" : "> 32 cols";
  auto& b = g_slot_time[std::string(name) + " [" + cls + "]"];
  b.first += 1; b.second += dt;
}
extern "C" void gcge_hip_slot_timing(int on) { g_slot_timing = on; if (on) g_slot_time.clear(); }
extern "C" int gcge_hip_slot_timing_report(char* buf, int len) {
  std::string out;
  for (auto& kv : g_slot_time) {
    char line[256];
    snprintf(line, sizeof line, "%-44s calls %8ld  %9.3f s  %8.3f ms/call\n", kv.first.c_str(), kv.second.first, kv.second.second,
             1e3 * kv.second.second / (double)kv.second.first);
    out += line;
  }
  if (buf != nullptr && len > 0) { strncpy(buf, out.c_str(), (size_t)len - 1); buf[len - 1] = 0; }
  return (int)out.size();
}

// ------------------------------------------------------------------ in-solve rate of the dense kernels per shape (measurement aid)
// gcge_hip_dense_profile(1): every Gram (K2) and panel update (K3) launched by the slots is bracketed by two HIP events on the
// back-end's stream (no synchronisation); gcge_hip_dense_profile_report sums them per (kernel, k, m): calls, average time and
// 2 n k m flop / time — the TF a solve actually sees for each shape, not a stand-alone benchmark's.
struct DenseEvent { hipEvent_t e0, e1; int kind, k, m; long n; double bytes; };   // kind 0: Gram, 1: panel update; bytes the launch must move
static std::vector<DenseEvent> g_dense_prof;
static std::map<std::tuple<int, int, int>, std::tuple<long, double, double, double>> g_dense_acc;   // (kind, k, m) -> calls, ms, flop, bytes: events already folded
static int g_dense_prof_on = 0;
// events are recycled (~1e5 launches per bench must not create and destroy 2e5 events inside the timed region)
static std::vector<hipEvent_t> g_dense_ev_pool;
static hipEvent_t dense_ev_get() {
  if (!g_dense_ev_pool.empty()) { hipEvent_t e = g_dense_ev_pool.back(); g_dense_ev_pool.pop_back(); return e; }
  hipEvent_t e; GCGE_HIP_CHECK(hipEventCreate(&e)); return e;
}
// fold the recorded intervals into the per-shape sums (all of them: the caller has synchronised; otherwise the completed front)
static void dense_prof_fold(bool all) {
  size_t i = 0;
  for (; i < g_dense_prof.size(); ++i) {
    DenseEvent& e = g_dense_prof[i];
    if (!all && hipEventQuery(e.e1) != hipSuccess) break;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.e0, e.e1) == hipSuccess) {
      auto& a = g_dense_acc[std::make_tuple(e.kind, e.k, e.m)];
      std::get<0>(a) += 1; std::get<1>(a) += ms; std::get<2>(a) += 2.0 * (double)e.n * e.k * e.m; std::get<3>(a) += e.bytes;
    }
    g_dense_ev_pool.push_back(e.e0); g_dense_ev_pool.push_back(e.e1);
  }
  g_dense_prof.erase(g_dense_prof.begin(), g_dense_prof.begin() + (long)i);
}
extern "C" void gcge_hip_dense_profile(int on) {
  for (auto& e : g_dense_prof) { g_dense_ev_pool.push_back(e.e0); g_dense_ev_pool.push_back(e.e1); }
  g_dense_prof.clear();
  g_dense_acc.clear();
  g_dense_prof_on = on;
  if (on) while (g_dense_ev_pool.size() < 8192) { hipEvent_t e; GCGE_HIP_CHECK(hipEventCreate(&e)); g_dense_ev_pool.push_back(e); }   // before anything is timed
}
struct DenseProfScope {
  DenseEvent ev; bool on;
  DenseProfScope(int kind, long n, int k, int m, double bytes) : on(g_dense_prof_on != 0) {
    if (!on) return;
    ev.kind = kind; ev.k = k; ev.m = m; ev.n = n; ev.bytes = bytes;
    ev.e0 = dense_ev_get(); ev.e1 = dense_ev_get();
    GCGE_HIP_CHECK(hipEventRecord(ev.e0, g_stream));
  }
  ~DenseProfScope() {
    if (!on) return;
    hipEventRecord(ev.e1, g_stream); g_dense_prof.push_back(ev);
    if (g_dense_prof.size() >= 4096) dense_prof_fold(false);          // (a bench of 20 solves brackets ~1e5 launches)
  }
};
// the same sums as numbers: rows of 7 doubles (kind 0 Gram / 1 panel update, k, m, calls, milliseconds in all, flop in all, bytes the
// launches had to move in all: both operands once, + the panel read where beta != 0 and it is not updated in place), at most max_rows
// of them, largest total time first; returns the number of shapes seen
extern "C" int gcge_hip_dense_profile_shapes(double* out, int max_rows) {
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
  dense_prof_fold(true);
  std::vector<std::pair<double, std::tuple<int, int, int>>> order;
  for (auto& kv : g_dense_acc) order.emplace_back(-std::get<1>(kv.second), kv.first);
  std::sort(order.begin(), order.end());
  int r = 0;
  for (auto& o : order) {
    if (r >= max_rows) break;
    const auto& a = g_dense_acc[o.second];
    double* q = out + 7 * (size_t)r++;
    q[0] = std::get<0>(o.second); q[1] = std::get<1>(o.second); q[2] = std::get<2>(o.second);
    q[3] = (double)std::get<0>(a); q[4] = std::get<1>(a); q[5] = std::get<2>(a); q[6] = std::get<3>(a);
  }
  return (int)order.size();
}
extern "C" int gcge_hip_dense_profile_report(char* buf, int len) {
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
  dense_prof_fold(true);
  std::string out;
  for (auto& kv : g_dense_acc) {
    char line[256];
    const long calls = std::get<0>(kv.second); const double ms = std::get<1>(kv.second), fl = std::get<2>(kv.second);
    snprintf(line, sizeof line, "%-13s k = %4d  m = %4d  calls %6ld  %9.3f ms per call  %6.1f TF  (%.1f ms in all)\n",
             std::get<0>(kv.first) == 0 ? "Gram" : "panel update", std::get<1>(kv.first), std::get<2>(kv.first), calls, ms / calls,
             ms > 0 ? fl / (ms * 1e-3) * 1e-12 : 0.0, ms);
    out += line;
  }
  if (buf != nullptr && len > 0) { strncpy(buf, out.c_str(), (size_t)len - 1); buf[len - 1] = 0; }
  return (int)out.size();
}

// ------------------------------------------------------------------ column-wise Gram-Schmidt over the slots, one sweep per column
// The reference's OrthSelf (src/ops_orth.c:45-118) issues per column k: QtAP (k x 1 Gram of the remaining panel with x_k), a
// scaling of x_k, a rank-1 update of the columns behind it — three strided sweeps over the panel.  The back-end fuses them
// WITHOUT changing what is computed: the scaling is held back until the next call; if that call is the rank-1 update from
// that very column, one kernel scales x_k, updates the panel and accumulates the Gram column of x_{k+1} that the next
// QtAP will ask for — same operands, same products, and the SAME order of the row sums as the separate kernel
// (vec_kernels.hip: mgs_step_kernel mirrors panel_dot1_partial), so the fused path is bit-identical to the unfused one; a
// Gram column that differs in the last bit is enough to change which noise-level columns a degenerate block drops.
// Anything else flushes the held-back scaling first.  The speculative Gram column is served only to the IMMEDIATELY following data call (epoch
// check) on the same block and column range; every entry point that touches block data goes through enter().
static unsigned long g_epoch = 0;
// the squared column norms of the panel the last MultiVecLinearComb wrote, where it summed them (GCGE_BACKEND.panel_norms_sq)
static double* g_norms_d = nullptr; static GcgeHipMV* g_norms_owner = nullptr; static int g_norms_c0 = 0, g_norms_c1 = 0; static unsigned long g_norms_epoch = 0;
static GcgeHipMV* g_pend_owner = nullptr;   // the one block with a held-back scaling (its pend_col >= 0), or NULL
static int g_mgs_fuse = 1;
extern "C" void gcge_hip_set_mgs_fusion(int on) { g_mgs_fuse = on; }
static long g_mgs_fused_steps = 0, g_mgs_spec_hits = 0;
extern "C" void gcge_hip_mgs_fusion_stats(long* fused_steps, long* served_grams) { if (fused_steps) *fused_steps = g_mgs_fused_steps; if (served_grams) *served_grams = g_mgs_spec_hits; }
static void flush_pending();
static inline void enter(bool keep_pending = false) { ++g_epoch; if (!keep_pending && g_pend_owner != nullptr) flush_pending(); }
extern "C" void gcge_hip_enter(void) { enter(); }   // for mat_product.hip
// the same without counting as a call (the epoch decides whether a speculative Gram column is still the latest word on its block):
// called at the top of every EXPORTED raw kernel that takes device pointers (gcge_hip.h "raw kernels") — a caller may hold a
// pointer from before the scaling was held back
extern "C" void gcge_hip_apply_pending(void) { if (g_pend_owner != nullptr) flush_pending(); }

extern "C" double* gcge_hip_stage_d(size_t len) {
  if (len > g_stage_d_len) {
    if (g_stage_d) GCGE_HIP_CHECK(hipFree(g_stage_d));
    g_stage_d_len = len + len / 4 + 4096;
    GCGE_HIP_CHECK(hipMalloc(&g_stage_d, g_stage_d_len * sizeof(double)));
  }
  return g_stage_d;
}
static double* g_stage_d2 = nullptr; static size_t g_stage_d2_len = 0;   // second device staging (split products)
extern "C" double* gcge_hip_stage_d2(size_t len) {
  if (len > g_stage_d2_len) {
    if (g_stage_d2) GCGE_HIP_CHECK(hipFree(g_stage_d2));
    g_stage_d2_len = len * 2 + 1024;
    GCGE_HIP_CHECK(hipMalloc(&g_stage_d2, g_stage_d2_len * sizeof(double)));
  }
  return g_stage_d2;
}
extern "C" double* gcge_hip_stage_h(size_t len) {
  if (len > g_stage_h_len) {
    if (g_stage_h) GCGE_HIP_CHECK(hipHostFree(g_stage_h));
    g_stage_h_len = len + len / 4 + 4096;
    GCGE_HIP_CHECK(hipHostMalloc(&g_stage_h, g_stage_h_len * sizeof(double)));
  }
  return g_stage_h;
}

extern "C" int gcge_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
extern "C" int gcge_hip_init(int device) {
  if (g_inited) return 0;
  if (gcge_hip_device_count() <= 0) {
    fprintf(stderr, "gcge_hip_init: no HIP device visible — the HIP back-end has no CPU fallback\n");
    return -1;
  }
  if (device >= 0) GCGE_HIP_CHECK(hipSetDevice(device));
  g_stream = nullptr;   // the legacy default stream: ordered with torch's current stream and hipMemcpy
  g_inited = 1;
  return 0;
}
extern "C" void gcge_hip_finalize(void) {
  gcge_hip_pool_release();
  if (g_stage_d) hipFree(g_stage_d);
  if (g_stage_h) hipHostFree(g_stage_h);
  g_stage_d = nullptr; g_stage_h = nullptr; g_stage_d_len = g_stage_h_len = 0; g_inited = 0;
}
extern "C" void gcge_hip_sync(void) { GCGE_HIP_CHECK(hipStreamSynchronize(g_stream)); }
extern "C" void* gcge_hip_stream(void) { return (void*)g_stream; }
extern "C" void gcge_hip_set_random_mode(int mode, unsigned long long seed) { g_rand_mode = mode; g_rand_seed = seed; }

// (matrix handle: upload, analysis into the K1 forms, halo plan, destruction — csrc/hip/mat_upload.hip; every product with it, the
//  fused CG passes and the launch profile — csrc/hip/mat_product.hip)
extern "C" int gcge_hip_spmm_path_get(void) { return g_spmm_path; }
extern "C" int gcge_hip_offset_patterns_get(void) { return g_offset_patterns; }

// ------------------------------------------------------------------ device buffer pool
// hipMalloc / hipFree of the multi-GB blocks cost 0.25-0.3 s each on this stack (page-table set-up; hipFree also
// synchronises the device): ~1.9 s of a 21 s solve.  Freed blocks are kept by exact size and handed out again —
// every use of the back-end happens on one stream, so a recycled block is ordered behind the kernels that last
// touched it.  The reference allocates its work blocks per solve as well (test_eig_sol_gcg.c:66-92); a second
// solve of the same shape then allocates nothing.  gcge_hip_pool_release() returns everything to the driver.
static std::unordered_map<size_t, std::vector<void*>> g_pool;
static size_t g_pool_bytes = 0;
static int g_pool_on = 1;
extern "C" void gcge_hip_pool_release(void) {
  for (auto& kv : g_pool) for (void* q : kv.second) hipFree(q);
  g_pool.clear(); g_pool_bytes = 0;
}
extern "C" void gcge_hip_pool_enable(int on) { g_pool_on = on; if (!on) gcge_hip_pool_release(); }
// bytes the pool holds at the moment (free for MultiVecCreate*, but "used" in hipMemGetInfo)
extern "C" size_t gcge_hip_pool_cached_bytes(void) { return g_pool_bytes; }
extern "C" void* gcge_hip_pool_alloc(size_t bytes) {
  auto it = g_pool.find(bytes);
  if (it != g_pool.end() && !it->second.empty()) {
    void* q = it->second.back(); it->second.pop_back(); g_pool_bytes -= bytes;
    return q;
  }
  void* q = nullptr;
  if (hipMalloc(&q, bytes) != hipSuccess) {   // out of memory: give the cached blocks back and try once more
    (void)hipGetLastError();
    gcge_hip_pool_release();
    GCGE_HIP_CHECK(hipMalloc(&q, bytes));
  }
  return q;
}
extern "C" void gcge_hip_pool_free(void* q, size_t bytes) {
  if (!g_pool_on || bytes < ((size_t)1 << 20)) {   // small blocks are not worth tracking
    GCGE_HIP_CHECK(hipStreamSynchronize(g_stream)); hipFree(q); return;
  }
  g_pool[bytes].push_back(q); g_pool_bytes += bytes;
}

// ------------------------------------------------------------------ multivector
static GcgeHipMV* mv_new(int nrows, int nghost, int ncols, const GCGE_HIP_MAT_* mat, GcgePerm* perm) {
  GcgeHipMV* v = (GcgeHipMV*)calloc(1, sizeof(GcgeHipMV));
  v->nrows = nrows; v->nrows_alloc = nrows + nghost; v->ncols = ncols; v->mat = mat; v->pend_col = -1;
  v->perm = real_perm(perm) != nullptr ? gcge_hip_perm_acquire(perm) : nullptr;   // (the caller's order needs no record: only matrices pin "as given" for their size)
  v->ld = ((long)(ncols > 0 ? ncols : 1) + 7) / 8 * 8;
  const size_t bytes = (size_t)v->nrows_alloc * v->ld * sizeof(double);
  v->bytes = bytes ? bytes : 8;
  v->d = (double*)gcge_hip_pool_alloc(v->bytes);
  GCGE_HIP_CHECK(hipMemsetAsync(v->d, 0, bytes, g_stream));   // zero-filled like app_ccs.c:47
  return v;
}
static void HIP_MultiVecCreateByMat(void*** mv, int num_vec, void* mat, struct OPS_* ops) {
  const GCGE_HIP_MAT_* A = (const GCGE_HIP_MAT_*)mat;
  if (A->rect_ncols > 0) { *mv = (void**)mv_new(A->rect_ncols, 0, num_vec, nullptr, nullptr); return; }   // app_ccs.c:43: rows = the matrix's COLUMNS
  *mv = (void**)mv_new(A->nrows, A->nghost, num_vec, A, A->perm);
}
static void HIP_MultiVecCreateByMultiVec(void*** mv, int num_vec, void** src, struct OPS_* ops) {
  const GcgeHipMV* s = (const GcgeHipMV*)src;
  *mv = (void**)mv_new(s->nrows, s->nrows_alloc - s->nrows, num_vec, s->mat, s->perm);
}
static void HIP_MultiVecDestroy(void*** mv, int num_vec, struct OPS_* ops) {
  GcgeHipMV* v = *(GcgeHipMV**)mv;
  enter();
  if (v != nullptr && v == g_norms_owner) g_norms_owner = nullptr;
  if (v) { delete v->spec_dots; gcge_hip_pool_free(v->d, v->bytes); gcge_hip_perm_release(v->perm); free(v); }
  *mv = nullptr;
}
static void flush_pending() {
  GcgeHipMV* v = g_pend_owner;
  g_pend_owner = nullptr;
  if (v != nullptr && v->pend_col >= 0) {
    const int col = v->pend_col;
    v->pend_col = -1;
    gcge_hip_colscale1(v->nrows, v->d + col, v->ld, v->pend_fac, g_stream);
  }
}
extern "C" int gcge_hip_mv_nrows(void** mv) { return ((GcgeHipMV*)mv)->nrows; }
// id of the row order a block lives in (0: the caller's): scratch blocks kept between calls belong to ONE order (block_pcg.hip)
extern "C" unsigned gcge_hip_mv_row_order_id(void** mv) { const GcgePerm* p = real_perm(((GcgeHipMV*)mv)->perm); return p ? p->id : 0u; }
extern "C" int gcge_hip_mv_ncols(void** mv) { return ((GcgeHipMV*)mv)->ncols; }
extern "C" double* gcge_hip_mv_device_ptr(void** mv, long* ld) {
  enter();
  GcgeHipMV* v = (GcgeHipMV*)mv; if (ld) *ld = v->ld; return v->d;
}

// host column-major  <->  device row-major, in panels so the staging stays bounded
extern "C" void gcge_hip_mv_from_host(void** mv, int c0, int c1, const double* host, long ldh) {
  enter();
  GcgeHipMV* v = (GcgeHipMV*)mv;
  const int n = v->nrows;
  GCGE_REQUIRE(c0 >= 0 && c1 <= v->ncols && ldh >= n, "gcge_hip_mv_from_host: ranges");
  const int panel = 32;
  const GcgePerm* P = real_perm(v->perm);          // the block lives in the back-end's own row order: device row i = the caller's row perm[i]
  std::vector<double> tmp;
  if (P != nullptr) tmp.resize((size_t)n * panel);
  for (int c = c0; c < c1; c += panel) {
    const int m = (c1 - c < panel) ? c1 - c : panel;
    double* st = gcge_hip_stage_d((size_t)n * m);
    const double* src = host + (size_t)(c - c0) * ldh; size_t lds_ = (size_t)ldh;
    if (P != nullptr) {
      for (int j = 0; j < m; ++j) { const double* hj = host + (size_t)(c - c0 + j) * ldh; double* tj = tmp.data() + (size_t)j * n; for (int i = 0; i < n; ++i) tj[i] = hj[P->perm[i]]; }
      src = tmp.data(); lds_ = (size_t)n;
    }
    GCGE_HIP_CHECK(hipMemcpy2DAsync(st, (size_t)n * sizeof(double), src, lds_ * sizeof(double), (size_t)n * sizeof(double), m,
                                    hipMemcpyHostToDevice, g_stream));
    gcge_hip_colmajor_to_rowmajor(n, m, st, n, v->d + c, v->ld, g_stream);
    GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
  }
}
extern "C" void gcge_hip_mv_to_host(void** mv, int c0, int c1, double* host, long ldh) {
  enter();
  GcgeHipMV* v = (GcgeHipMV*)mv;
  const int n = v->nrows;
  GCGE_REQUIRE(c0 >= 0 && c1 <= v->ncols && ldh >= n, "gcge_hip_mv_to_host: ranges");
  const int panel = 32;
  const GcgePerm* P = real_perm(v->perm);
  std::vector<double> tmp;
  if (P != nullptr) tmp.resize((size_t)n * panel);
  for (int c = c0; c < c1; c += panel) {
    const int m = (c1 - c < panel) ? c1 - c : panel;
    double* st = gcge_hip_stage_d((size_t)n * m);
    gcge_hip_rowmajor_to_colmajor(n, m, v->d + c, v->ld, st, n, g_stream);
    double* dst = P != nullptr ? tmp.data() : host + (size_t)(c - c0) * ldh;
    GCGE_HIP_CHECK(hipMemcpy2DAsync(dst, (P != nullptr ? (size_t)n : (size_t)ldh) * sizeof(double), st,
                                    (size_t)n * sizeof(double), (size_t)n * sizeof(double), m,
                                    hipMemcpyDeviceToHost, g_stream));
    GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
    if (P != nullptr)
      for (int j = 0; j < m; ++j) { double* hj = host + (size_t)(c - c0 + j) * ldh; const double* tj = tmp.data() + (size_t)j * n; for (int i = 0; i < n; ++i) hj[P->perm[i]] = tj[i]; }
  }
}

static void HIP_MultiVecView(void** x, int start, int end, struct OPS_* ops) {
  GcgeHipMV* v = (GcgeHipMV*)x;
  const int m = end - start;
  if (m <= 0) return;
  std::vector<double> h((size_t)v->nrows * m);
  gcge_hip_mv_to_host(x, start, end, h.data(), v->nrows);
  for (int r = 0; r < v->nrows; ++r) {
    for (int c = 0; c < m; ++c) ops->Printf("%6.4e\t", h[(size_t)c * v->nrows + r]);
    ops->Printf("\n");
  }
}

// app_lapack.c:322-333 — mode 0: the reference's rand() stream, column by column
static void HIP_MultiVecSetRandomValue(void** x, int start, int end, struct OPS_* ops) {
  enter();
  GcgeHipMV* v = (GcgeHipMV*)x;
  const int m = end - start;
  if (m <= 0) return;
  GCGE_REQUIRE(start >= 0 && end <= v->ncols, "MultiVecSetRandomValue: column range");
  if (g_rand_mode == 1) {
    const long rb = v->mat ? v->mat->row_begin : 0, ng = v->mat ? v->mat->nglobal : v->nrows;
    gcge_hip_fill_uniform(v->nrows, rb, ng, v->d, v->ld, start, m, g_rand_seed, g_stream);
    g_rand_seed += 0x9E3779B97F4A7C15ull;   // a later fill of the same columns differs
    return;
  }
  // Row slabs: every rank walks the GLOBAL rand() sequence (columns outer, global rows inner) and keeps its own
  // rows, so the start block is the single-rank one whatever the number of ranks (identical local streams would
  // make it periodic in the slab index).  O(n_global) draws per column: use mode 1 for large n.
  const long before = (v->mat && v->mat->nglobal > v->nrows) ? v->mat->row_begin : 0;
  const long after = (v->mat && v->mat->nglobal > v->nrows) ? (long)v->mat->nglobal - v->mat->row_begin - v->nrows : 0;
  const int panel = 16;
  std::vector<double> h((size_t)v->nrows * panel);
  for (int c = start; c < end; c += panel) {
    const int mm = (end - c < panel) ? end - c : panel;
    for (int j = 0; j < mm; ++j) {
      for (long k = 0; k < before; ++k) (void)rand();
      for (int r = 0; r < v->nrows; ++r) h[(size_t)j * v->nrows + r] = ((double)rand()) / ((double)RAND_MAX + 1);
      for (long k = 0; k < after; ++k) (void)rand();
    }
    gcge_hip_mv_from_host(x, c, c + mm, h.data(), v->nrows);
  }
}

// app_lapack.c:334-395
static void HIP_MultiVecAxpby(double alpha, void** x, double beta, void** y, int* start, int* end, struct OPS_* ops) {
  GcgeHipMV *vx = (GcgeHipMV*)x, *vy = (GcgeHipMV*)y;
  const int m = end[1] - start[1];
  enter();
  SlotTimer tm_(x ? "MultiVecAxpby" : "MultiVecAxpby (scale)", m);
  GCGE_REQUIRE(end[0] - start[0] == m, "MultiVecAxpby: equal column counts");
  if (m <= 0 || vy->nrows == 0) return;
  GCGE_REQUIRE(start[1] >= 0 && end[1] <= vy->ncols, "MultiVecAxpby: y column range");
  if (vx) {
    GCGE_REQUIRE(vx->nrows == vy->nrows, "MultiVecAxpby: equal row counts");
    GCGE_REQUIRE(start[0] >= 0 && end[0] <= vx->ncols, "MultiVecAxpby: x column range");
  }
  if (vx == nullptr && m == 1 && beta != 0.0) {   // one column scaled in place (q_k = x_k / r_kk of a column-wise Gram-Schmidt)
    if (g_mgs_fuse) { g_pend_owner = vy; vy->pend_col = start[1]; vy->pend_fac = beta; return; }   // held back: see enter()
    gcge_hip_colscale1(vy->nrows, vy->d + start[1], vy->ld, beta, g_stream);
    return;
  }
  gcge_hip_axpby(vy->nrows, alpha, vx ? vx->d + start[0] : nullptr, vx ? vx->ld : 0, beta, vy->d + start[1],
                 vy->ld, m, g_stream);
}

// GCGE_BACKEND.block_moves (include/gcge_ops.h): X, the W start vectors and b of an outer iteration in one sweep over the rows of
// ritz[:, x0..x1) (vec_kernels.hip: block_moves_kernel).  0 with nothing touched for what the kernel does not take: rows wider than
// 512 columns, blocks in different row orders, V as b, V as source with an X move asked for, runs outside [x0, x1) or targets outside
// their blocks.  V as the source of the runs alone (ritz == V, x0 == x1: the Ritz vectors already live in V): the sweep walks the
// column pairs from the first run to the last and writes the W start vectors and b only.
static int HIP_BlockMoves(void** ritz, void** V, int x0, int x1, const int* runs, int w0, void** b, int b0, const double* scale, struct OPS_* ops) {
  (void)ops;
  GcgeHipMV *vr = (GcgeHipMV*)ritz, *vv = (GcgeHipMV*)V, *vb = (GcgeHipMV*)b;
  if (vr == nullptr || vv == nullptr || vb == vv || runs == nullptr || x0 < 0) return 0;
  const bool from_v = vr == vv;
  if (from_v ? (x1 != x0 || runs[0] < 1) : (x1 <= x0)) return 0;
  const int s0 = from_v ? runs[1] : x0, s1 = from_v ? runs[2 * runs[0]] : x1;      // the source columns the sweep walks
  if (s0 < 0 || s1 <= s0) return 0;
  if (s1 > vr->ncols || s1 > vv->ncols || vr->nrows != vv->nrows || vr->nrows <= 0 || real_perm(vr->perm) != real_perm(vv->perm)) return 0;
  if ((vr->ld & 1) || (vv->ld & 1) || ((uintptr_t)vr->d & 15) || ((uintptr_t)vv->d & 15)) return 0;
  if (vb != nullptr && (scale == nullptr || vb->nrows != vr->nrows || (vb->ld & 1) || ((uintptr_t)vb->d & 15) || real_perm(vb->perm) != real_perm(vr->perm))) return 0;
  const int c0 = s0 & ~1, c1 = (s1 + 1) & ~1, npairs = (c1 - c0) / 2;
  if (npairs > 256 || c1 > vr->ld) return 0;
  int total = 0, prev = s0;
  for (int i = 0; i < runs[0]; ++i) {
    const int lo = runs[2 * i + 1], hi = runs[2 * i + 2];
    if (lo < prev || hi <= lo || hi > s1) return 0;
    total += hi - lo; prev = hi;
  }
  if (w0 < s1 || w0 + total > vv->ncols) return 0;
  if (vb != nullptr && (b0 < 0 || b0 + total > vb->ncols)) return 0;
  enter();
  SlotTimer tm_(from_v ? "block moves (W start, b)" : "block moves (X, W start, b)", s1 - s0);
  // staging: [0, total) the factors, behind them the 2 npairs positions in the packed runs as ints
  const size_t nd = (size_t)total + (size_t)npairs;
  double* dd = gcge_hip_stage_d(nd);
  double* hs = gcge_hip_stage_h(nd);
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));   // the staging buffers are reused
  int* hmap = (int*)(hs + total);
  for (int k = 0; k < 2 * npairs; ++k) hmap[k] = -1;
  for (int i = 0, blk = 0; i < runs[0]; ++i)
    for (int col = runs[2 * i + 1]; col < runs[2 * i + 2]; ++col) hmap[col - c0] = blk++;
  for (int k = 0; k < total; ++k) hs[k] = vb != nullptr ? scale[k] : 0.0;
  GCGE_HIP_CHECK(hipMemcpyAsync(dd, hs, nd * sizeof(double), hipMemcpyHostToDevice, g_stream));
  GCGE_REQUIRE(gcge_hip_block_moves(vr->nrows, vr->d + c0, vr->ld, vv->d, vv->ld, vb != nullptr ? vb->d : nullptr, vb != nullptr ? vb->ld : 0, c0, npairs,
                                    from_v ? 0 : x0, from_v ? 0 : x1, (const int*)(dd + total), dd, w0, b0, g_stream) == 0, "block moves: kernel launch");
  return 1;
}
extern "C" int gcge_hip_block_moves_mv(void** ritz, void** V, int x0, int x1, const int* runs, int w0, void** b, int b0, const double* scale) {
  return HIP_BlockMoves(ritz, V, x0, x1, runs, w0, b, b0, scale, nullptr);
}

// app_lapack.c:463-534
static void HIP_MultiVecLinearComb(void** x, void** y, int is_vec, int* start, int* end, double* coef, int ldc,
                                   double* beta, int incb, struct OPS_* ops) {
  GcgeHipMV *vx = (GcgeHipMV*)x, *vy = (GcgeHipMV*)y;
  const int k = end[0] - start[0], m = end[1] - start[1];
  enter(true);   // a held-back scaling of x_k survives until it is known whether this is its rank-1 update
  SlotTimer tm_(k == 1 ? "MultiVecLinearComb (rank 1)" : "MultiVecLinearComb", m);
  {
    const bool step = g_mgs_fuse && k == 1 && vx == vy && vx != nullptr && coef != nullptr && start[1] == start[0] + 1 && m >= 1 && m <= 64 &&
                      beta != nullptr && incb == 0 && *beta == 1.0 && start[0] >= 0 && end[1] <= vy->ncols && vy->nrows > 0;
    double fac = 1.0;
    if (g_pend_owner != nullptr) {
      if (step && g_pend_owner == vx && vx->pend_col == start[0]) { fac = vx->pend_fac; vx->pend_col = -1; g_pend_owner = nullptr; }
      else flush_pending();
    }
    if (step) {
      // x_k *= fac, columns (k, k + m] += x_k coef^T, and the Gram column of x_{k+1} with the updated panel in the same sweep
      GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));   // staging buffers are reused
      double* hc = gcge_hip_stage_h(2 * (size_t)m);
      for (int j = 0; j < m; ++j) hc[j] = coef[(size_t)j * ldc];
      double* dc = gcge_hip_stage_d(2 * (size_t)m);
      GCGE_HIP_CHECK(hipMemcpyAsync(dc, hc, m * sizeof(double), hipMemcpyHostToDevice, g_stream));
      const int rc = gcge_hip_mgs_step(vy->nrows, vy->d + start[0], vy->ld, fac, dc, m, dc + m, g_stream);
      GCGE_REQUIRE(rc == 0, "MultiVecLinearComb: kernel launch");
      GCGE_HIP_CHECK(hipMemcpyAsync(hc + m, dc + m, m * sizeof(double), hipMemcpyDeviceToHost, g_stream));
      GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
      vy->spec_c0 = start[1]; vy->spec_c1 = end[1]; vy->spec_epoch = g_epoch;
      if (vy->spec_dots == nullptr) vy->spec_dots = new std::vector<double>();
      vy->spec_dots->assign(hc + m, hc + 2 * m);
      ++g_mgs_fused_steps;
      return;
    }
  }
  if (k == 0 || m == 0 || vy->nrows == 0) return;
  GCGE_REQUIRE(start[1] >= 0 && end[1] <= vy->ncols && m > 0, "MultiVecLinearComb: y column range");
  if (vx != nullptr && coef != nullptr) {
    GCGE_REQUIRE(vx->nrows == vy->nrows, "MultiVecLinearComb: equal row counts");
    GCGE_REQUIRE(start[0] >= 0 && end[0] <= vx->ncols && k > 0 && ldc >= k, "MultiVecLinearComb: x column range / ldc");
  }
  if (vx == nullptr || coef == nullptr) {       // scaling only: y_j *= beta_j
    if (beta == nullptr) return;
    if (incb == 0) { gcge_hip_axpby(vy->nrows, 0.0, nullptr, 0, *beta, vy->d + start[1], vy->ld, m, g_stream); return; }
    double* hb = gcge_hip_stage_h(m);
    GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
    for (int j = 0; j < m; ++j) hb[j] = beta[(size_t)j * incb];
    double* db = gcge_hip_stage_d(m);
    GCGE_HIP_CHECK(hipMemcpyAsync(db, hb, m * sizeof(double), hipMemcpyHostToDevice, g_stream));
    gcge_hip_colscale(vy->nrows, vy->d + start[1], vy->ld, m, db, g_stream);
    return;
  }
  if (k == 1) {   // rank-1 update y_j = x c_j + beta_j y_j: one sweep over the m contiguous columns of every row
    const size_t len = 2 * (size_t)m;
    GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));   // staging buffers are reused
    double* hc = gcge_hip_stage_h(len);
    for (int j = 0; j < m; ++j) { hc[j] = coef[(size_t)j * ldc]; hc[m + j] = beta == nullptr ? 0.0 : (incb == 0 ? *beta : beta[(size_t)j * incb]); }
    double* dc = gcge_hip_stage_d(len);
    GCGE_HIP_CHECK(hipMemcpyAsync(dc, hc, len * sizeof(double), hipMemcpyHostToDevice, g_stream));
    const bool unit_beta = beta != nullptr && incb == 0 && *beta == 1.0;
    int rc = gcge_hip_rank1_update(vy->nrows, vx->d + start[0], vx->ld, dc, unit_beta ? nullptr : dc + m, vy->d + start[1], vy->ld, m, g_stream);
    GCGE_REQUIRE(rc == 0, "MultiVecLinearComb: kernel launch");
    return;
  }
  // panels of <= 128 output columns; coefficient panel uploaded row-major (k x mp) [+ beta]
  for (int j0 = 0; j0 < m; j0 += 128) {
    const int mp = (m - j0 < 128) ? m - j0 : 128;
    const size_t len = (size_t)k * mp + mp;
    GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));   // staging buffers are reused
    double* hc = gcge_hip_stage_h(len);
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < mp; ++j) hc[(size_t)i * mp + j] = coef[(size_t)(j0 + j) * ldc + i];
    if (beta != nullptr) for (int j = 0; j < mp; ++j) hc[(size_t)k * mp + j] = (incb == 0) ? *beta : beta[(size_t)(j0 + j) * incb];
    double* dc = gcge_hip_stage_d(len);
    GCGE_HIP_CHECK(hipMemcpyAsync(dc, hc, len * sizeof(double), hipMemcpyHostToDevice, g_stream));
    // bytes a launch moves: X read, the panel written; the panel is READ as well where beta != 0 — unless it is updated in place
    // (y == x with the output columns inside the input range: the rows of X just read hold it)
    const bool inplace_ = vx == vy && start[1] + j0 >= start[0] && start[1] + j0 + mp <= end[0];
    DenseProfScope prof_(1, vy->nrows, k, mp, 8.0 * (double)vy->nrows * (k + mp + ((beta != nullptr && !inplace_) ? mp : 0)));
    // an update y = x c + y diag(beta) of one panel of <= 64 columns also sums the squares of what it stores where the register
    // form takes it (GCGE_BACKEND.panel_norms_sq: the "twice is enough" test of the orthonormalisation asks for them next)
    int rc = 1;
    if (beta != nullptr && m <= 64 && getenv("GCGE_NO_PANEL_NORMS") == nullptr) {
      if (g_norms_d == nullptr) GCGE_HIP_CHECK(hipMalloc(&g_norms_d, 64 * sizeof(double)));
      rc = gcge_hip_lincomb_norms(vy->nrows, vx->d + start[0], vx->ld, k, dc, mp, dc + (size_t)k * mp, vy->d + start[1], vy->ld, g_norms_d, g_stream);
      if (rc == 0) { g_norms_owner = vy; g_norms_c0 = start[1]; g_norms_c1 = end[1]; g_norms_epoch = g_epoch; }
    }
    if (rc == 1) rc = gcge_hip_lincomb(vy->nrows, vx->d + start[0], vx->ld, k, dc, mp, beta ? dc + (size_t)k * mp : nullptr,
                                       vy->d + start[1] + j0, vy->ld, g_stream);
    GCGE_REQUIRE(rc == 0, "MultiVecLinearComb: kernel launch");
  }
}

// GCGE_BACKEND.panel_norms_sq (include/gcge_ops.h): the squared column norms the last MultiVecLinearComb summed on its way
static int HIP_PanelNormsSq(void** y, int start, int end, double* out, struct OPS_* ops) {
  (void)ops;
  const bool fresh = (GcgeHipMV*)y == g_norms_owner && g_norms_owner != nullptr && start == g_norms_c0 && end == g_norms_c1 && g_norms_epoch == g_epoch;
  enter();
  if (!fresh || out == nullptr) return 0;
  const int m = end - start;
  double* hd = gcge_hip_stage_h(m);
  GCGE_HIP_CHECK(hipMemcpyAsync(hd, g_norms_d, m * sizeof(double), hipMemcpyDeviceToHost, g_stream));
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
  for (int j = 0; j < m; ++j) out[j] = hd[j];
  return 1;
}
extern "C" int gcge_hip_panel_norms_sq_mv(void** y, int start, int end, double* out) { return HIP_PanelNormsSq(y, start, end, out, nullptr); }

// GCGE_BACKEND.ritz_in_place (include/gcge_ops.h): V[:, n0..x1) = V[:, n0..w1) C in place and V[:, p0..p0 + np) = S[:, 0..np) behind
// it, one launch of the panel update's register form with the row copy in its epilogue (lincomb_mfma.hip).
static int HIP_RitzInPlace(void** V, int n0, int x1, int w1, const double* coef, int ldc, void** S, int p0, int np, struct OPS_* ops) {
  (void)ops;
  GcgeHipMV *vv = (GcgeHipMV*)V, *vs = (GcgeHipMV*)S;
  const int k = w1 - n0, m = x1 - n0;
  if (vv == nullptr || coef == nullptr || n0 < 0 || m < 1 || m > 128 || k < m || w1 > vv->ncols || ldc < k || np < 0) return 0;
  if ((vv->ld & 1) || ((uintptr_t)vv->d & 15)) return 0;
  if (np > 0) {
    if (vs == nullptr || vs == vv || np > vs->ncols || p0 < 0 || p0 + np > vv->ncols || (p0 < x1 && p0 + np > n0)) return 0;
    if (vs->nrows != vv->nrows || real_perm(vs->perm) != real_perm(vv->perm)) return 0;
  }
  if (vv->nrows <= 0) return 1;
  enter();
  SlotTimer tm_("Ritz vectors in place + P", m);
  const size_t len = (size_t)k * m;
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));   // staging buffers are reused
  double* hc = gcge_hip_stage_h(len);
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < m; ++j) hc[(size_t)i * m + j] = coef[(size_t)j * ldc + i];
  double* dc = gcge_hip_stage_d(len);
  GCGE_HIP_CHECK(hipMemcpyAsync(dc, hc, len * sizeof(double), hipMemcpyHostToDevice, g_stream));
  DenseProfScope prof_(1, vv->nrows, k, m, 8.0 * (double)vv->nrows * (k + m + 2 * np));
  const int rc = gcge_hip_lincomb_copy(vv->nrows, vv->d + n0, vv->ld, k, dc, m, nullptr, vv->d + n0, vv->ld, np > 0 ? vs->d : nullptr,
                                       np > 0 ? vs->ld : 0, vv->d + p0, vv->ld, np, g_stream);
  GCGE_REQUIRE(rc == 0 || rc == 1, "ritz in place: kernel launch");
  return rc == 0;
}
extern "C" int gcge_hip_ritz_in_place_mv(void** V, int n0, int x1, int w1, const double* coef, int ldc, void** S, int p0, int np) {
  return HIP_RitzInPlace(V, n0, x1, w1, coef, ldc, S, p0, np, nullptr);
}

// app_lapack.c:299-313 -> DenseMatQtAP(matA == NULL) :64-183.  Result to HOST, column-major ldIP.
static void reduce_inner_prod(char nsd, int nr, int nc, double* ip, int ldIP);
// reduce != 0: the SUM OVER THE RANKS is returned; returns 1 if that sum was formed (on the device, before the one copy to the host:
// RCCL inside the back-end), 0 if the caller still has to reduce the host result through GCGE_COMM (another transport; the served
// Gram column of a fused Gram-Schmidt step)
static int local_inner_prod(char nsd, void** x, void** y, int is_vec, int* start, int* end, double* ip, int ldIP, struct OPS_* ops, int reduce = 0);
// the slot: the local rows' part — or, where the caller opted in (GCGE_SetLocalInnerProdReduces: stacks that sum through MPI only,
// the reference's BlockPCG src/ops_lin_sol.c:306-321), the sum over the ranks
static void HIP_MultiVecLocalInnerProd(char nsd, void** x, void** y, int is_vec, int* start, int* end, double* ip, int ldIP, struct OPS_* ops) {
  const int want = GCGE_GetLocalInnerProdReduces();
  if (!local_inner_prod(nsd, x, y, is_vec, start, end, ip, ldIP, ops, want) && want) reduce_inner_prod(nsd, end[0] - start[0], end[1] - start[1], ip, ldIP);
}
extern "C" void gcge_hip_local_inner_prod(char nsd, void** x, void** y, int* start, int* end, double* ip, int ldIP, struct OPS_* ops) {
  local_inner_prod(nsd, x, y, 0, start, end, ip, ldIP, ops);           // for block_pcg.hip: the local rows' part, never reduced
}
static int local_inner_prod(char nsd, void** x, void** y, int is_vec, int* start, int* end,
                                       double* ip, int ldIP, struct OPS_* ops, int reduce) {
  GcgeHipMV *vx = (GcgeHipMV*)x, *vy = (GcgeHipMV*)y;
  const int k = end[0] - start[0], m = end[1] - start[1];
  enter();
  SlotTimer tm_(m == 1 ? "MultiVecLocalInnerProd (k x 1)" : "MultiVecLocalInnerProd", m == 1 ? k : m);
  if (k <= 0 || m <= 0) return 0;
  // Round 5: with RCCL inside the back-end the partial Gram is summed over the ranks WHERE IT IS — on the device,
  // on the back-end's stream, in front of the one device-to-host copy — instead of host -> pinned -> device -> ncclAllReduce -> pinned
  // -> host behind it: one stream synchronisation per inner product instead of two, no second staging.  ~1 700 inner products per
  // solve are latency, not bytes.  Reference: MPI_Allreduce of the local result, src/ops_multi_vec.c:206-228.
  GCGE_COMM* comm_ = reduce ? GCGE_GetComm() : nullptr;
  const bool dev_reduce = comm_ != nullptr && gcge_hip_comm_is_native(comm_) && getenv("GCGE_GRAM_HOST_REDUCE") == nullptr;
  if (m == 1 && nsd != 'D' && vx == vy && vx->spec_dots != nullptr && !vx->spec_dots->empty() && vx->spec_epoch + 1 == g_epoch &&
      start[0] == vx->spec_c0 && start[1] == vx->spec_c0 && end[0] == vx->spec_c1 && (int)vx->spec_dots->size() == k && ldIP >= k) {
    // the Gram column the previous call (the rank-1 update of a Gram-Schmidt step ON THIS BLOCK) accumulated on its way: no
    // call of any kind has been made since (epoch), same block, same column range
    for (int i = 0; i < k; ++i) ip[i] = (*vx->spec_dots)[i];
    vx->spec_dots->clear(); ++g_mgs_spec_hits;
    return 0;
  }
  if (vx->spec_dots != nullptr) vx->spec_dots->clear();
  if (vy->spec_dots != nullptr) vy->spec_dots->clear();
  GCGE_REQUIRE(vx->nrows == vy->nrows, "MultiVecInnerProd: equal row counts");
  GCGE_REQUIRE(start[0] >= 0 && end[0] <= vx->ncols && start[1] >= 0 && end[1] <= vy->ncols, "MultiVecInnerProd: column ranges");
  GCGE_REQUIRE(nsd == 'D' ? ldIP >= 1 : ldIP >= k, "MultiVecInnerProd: ldIP");
  if (nsd == 'D') {
    GCGE_REQUIRE(k == m, "MultiVecInnerProd 'D': square");
    double* dd = gcge_hip_stage_d(m);
    gcge_hip_coldots(vx->nrows, vx->d + start[0], vx->ld, vy->d + start[1], vy->ld, m, dd, g_stream);
    if (dev_reduce) gcge_hip_comm_allreduce_device(dd, m);
    double* hd = gcge_hip_stage_h(m);
    GCGE_HIP_CHECK(hipMemcpyAsync(hd, dd, m * sizeof(double), hipMemcpyDeviceToHost, g_stream));
    GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
    for (int j = 0; j < m; ++j) ip[(size_t)ldIP * j] = hd[j];
    return dev_reduce ? 1 : 0;
  }
  double* dg = gcge_hip_stage_d((size_t)k * m);
  if (m == 1) gcge_hip_panel_dot1(vx->nrows, vx->d + start[0], vx->ld, k, vy->d + start[1], vy->ld, dg, g_stream);   // panel . column
  else { DenseProfScope prof_(0, vx->nrows, k, m, 8.0 * (double)vx->nrows * ((vx == vy && start[0] == start[1] && k == m) ? k : k + m)); gcge_hip_gram(vx->nrows, vx->d + start[0], vx->ld, k, vy->d + start[1], vy->ld, m, dg, g_stream); }
  if (dev_reduce) gcge_hip_comm_allreduce_device(dg, k * m);      // (the whole k x m block: contiguous on the device whatever ldIP is)
  double* hg = gcge_hip_stage_h((size_t)k * m);
  GCGE_HIP_CHECK(hipMemcpyAsync(hg, dg, (size_t)k * m * sizeof(double), hipMemcpyDeviceToHost, g_stream));
  GCGE_HIP_CHECK(hipStreamSynchronize(g_stream));
  if (nsd == 'S') {   // lower triangle is authoritative, mirrored (app_lapack.c:119-130)
    GCGE_REQUIRE(k == m, "MultiVecInnerProd 'S': square");
    for (int j = 0; j < m; ++j)
      for (int i = j; i < k; ++i) { const double v = hg[(size_t)i * m + j]; ip[(size_t)ldIP * j + i] = v; ip[(size_t)ldIP * i + j] = v; }
  } else {
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < k; ++i) ip[(size_t)ldIP * j + i] = hg[(size_t)i * m + j];
  }
  return dev_reduce ? 1 : 0;
}

// Local part + sum over the ranks of the communicator registered at call time (GCGE_GetComm(): RCCL inside the back-end,
// csrc/hip/rccl_comm.hip, or a caller's transport); results packed for the reduction when ld != rows.  Own functions
// (not the Default* of a solver library): whichever OPS_Setup completes the table — ours or the reference's, whose
// default of the same name only reduces under OPS_USE_MPI, src/ops_multi_vec.c:202-230 — finds these slots filled.
static void HIP_MultiVecInnerProd(char nsd, void** x, void** y, int is_vec, int* start, int* end, double* ip, int ldIP,
                                  struct OPS_* ops) {
  if (!local_inner_prod(nsd, x, y, is_vec, start, end, ip, ldIP, ops, 1))
    reduce_inner_prod(nsd, end[0] - start[0], end[1] - start[1], ip, ldIP);
}
static void reduce_inner_prod(char nsd, int nr, int nc, double* ip, int ldIP) {
  GCGE_COMM* comm = GCGE_GetComm();
  if (comm == nullptr || nr <= 0 || nc <= 0) return;
  if (nsd == 'D') nr = 1;   // one value per column, stride ldIP
  if (nr == ldIP) { comm->allreduce_sum(ip, nr * nc, comm->ctx); return; }
  std::vector<double> pack((size_t)nr * nc);
  for (int c = 0; c < nc; ++c) memcpy(pack.data() + (size_t)c * nr, ip + (size_t)c * ldIP, nr * sizeof(double));
  comm->allreduce_sum(pack.data(), nr * nc, comm->ctx);
  for (int c = 0; c < nc; ++c) memcpy(ip + (size_t)c * ldIP, pack.data() + (size_t)c * nr, nr * sizeof(double));
}
// src/ops_multi_vec.c:351-411: qAp = Q[:, s0:e0)^T A P[:, s1:e1); A != NULL leaves A P in mv_ws[:, 0:m) (the
// orthonormalisation re-uses it); 'T' stores the transpose (m x k)
static void HIP_MultiVecQtAP(char ntsA, char ntsd, void** mvQ, void* matA, void** mvP, int is_vec, int* startQP, int* endQP,
                             double* qAp, int ldQAP, void** mv_ws, struct OPS_* ops) {
  int s[2], e[2];
  const int k = endQP[0] - startQP[0], m = endQP[1] - startQP[1];
  if (k <= 0 || m <= 0) return;
  if (matA == nullptr) {
    if (ntsd == 'T') {
      s[0] = startQP[1]; e[0] = endQP[1]; s[1] = startQP[0]; e[1] = endQP[0];
      ops->MultiVecInnerProd('N', mvP, mvQ, is_vec, s, e, qAp, ldQAP, ops);
    } else ops->MultiVecInnerProd(ntsd, mvQ, mvP, is_vec, startQP, endQP, qAp, ldQAP, ops);
    return;
  }
  s[0] = startQP[1]; e[0] = endQP[1]; s[1] = 0; e[1] = m;
  if (ntsA == 'T') ops->MatTransDotMultiVec(matA, mvP, mv_ws, s, e, ops);
  else ops->MatDotMultiVec(matA, mvP, mv_ws, s, e, ops);
  if (ntsd == 'T') {
    s[0] = 0; e[0] = m; s[1] = startQP[0]; e[1] = endQP[0];
    ops->MultiVecInnerProd('N', mv_ws, mvQ, is_vec, s, e, qAp, ldQAP, ops);
  } else {
    s[0] = startQP[0]; e[0] = endQP[0]; s[1] = 0; e[1] = m;
    ops->MultiVecInnerProd(ntsd, mvQ, mv_ws, is_vec, s, e, qAp, ldQAP, ops);
  }
}

// PAS (csrc/host/pas.c): the bordered product of its composite table (pas_border.hip), the identity of a standard problem whose
// hierarchy holds the coarse masses P^T P, and the row-order check of the levels (the prolongations are in the hierarchy's order)
static void* HIP_MatIdentity(void* like) {
  const GCGE_HIP_MAT_* A = (const GCGE_HIP_MAT_*)like;
  if (A == nullptr || A->rect_ncols > 0 || A->nghost > 0 || A->part_world > 1) return nullptr;   // whole matrices on one rank
  const int n = A->nrows;
  std::vector<int> rp((size_t)n + 1), ci((size_t)n); std::vector<double> va((size_t)n, 1.0);
  for (int r = 0; r <= n; ++r) rp[r] = r;
  for (int r = 0; r < n; ++r) ci[r] = r;
  return (void*)gcge_hip_mat_create(n, n, 0, rp.data(), ci.data(), va.data());
}
static void HIP_MatFree(void* m) { gcge_hip_mat_destroy((GCGE_HIP_MAT*)m); }
static int HIP_MatRowsAsGiven(void* m) { const GCGE_HIP_MAT_* A = (const GCGE_HIP_MAT_*)m; return A == nullptr || real_perm(A->perm) == nullptr; }

extern "C" void OPS_HIP_Set(struct OPS_* ops) {
  if (gcge_hip_init(-1) != 0) {
    fprintf(stderr, "OPS_HIP_Set: HIP back-end unavailable (no GPU): aborting — there is no CPU fallback\n");
    abort();
  }
  ops->Printf                   = DefaultPrintf;
  ops->GetWtime                 = DefaultGetWtime;
  ops->GetOptionFromCommandLine = DefaultGetOptionFromCommandLine;
  ops->MultiVecCreateByMat      = HIP_MultiVecCreateByMat;
  ops->MultiVecCreateByMultiVec = HIP_MultiVecCreateByMultiVec;
  ops->MultiVecDestroy          = HIP_MultiVecDestroy;
  ops->MultiVecView             = HIP_MultiVecView;
  ops->MultiVecLocalInnerProd   = HIP_MultiVecLocalInnerProd;
  ops->MultiVecInnerProd        = HIP_MultiVecInnerProd;   // installed HERE, not left to OPS_Setup: see above
  ops->MultiVecSetRandomValue   = HIP_MultiVecSetRandomValue;
  ops->MultiVecAxpby            = HIP_MultiVecAxpby;
  ops->MultiVecLinearComb       = HIP_MultiVecLinearComb;
  ops->MultiVecQtAP             = HIP_MultiVecQtAP;
  // the hierarchy behind BlockAMG (src/ops.h:134-139; multigrid.hip)
  ops->MultiGridCreate          = gcge_hip_multigrid_create;
  ops->MultiGridDestroy         = gcge_hip_multigrid_destroy;
  // what this table offers the solver stack beyond its slots (GCGE_BACKEND, include/gcge_ops.h)
  GCGE_BACKEND be = {};
  // panel updates work row by row on the row-major blocks (lincomb_mfma.hip: a block / wave reads only the rows it
  // writes, and writes them after its last read): one panel of <= 128 output columns may be updated in place
  be.inplace_lincomb_cols = 128;
  // K7 on the device for the projected matrices where the host solver dominates an outer iteration (eig_device.hip)
  be.symeig = gcge_hip_symeig; be.symeig_min_n = 192;
  gcge_hip_product_slots(ops, &be);           // MatDotMultiVec / MatTransDotMultiVec, the residual hook, the V-cycle's fused sweeps
  gcge_hip_bpcg_backend(&be);                 // the fused device CG: BlockAMG's smoother, and the solver of unformed b = x diag(scale)
  gcge_hip_pcg_backend(&be);                  // the sweeps of GCGE_PCGSolve's step, one launch each (pcg_sweeps.hip)
  be.pas_border = gcge_hip_pas_border;        // PAS: y += QX t and g = QX^T q in one pass over QX
  be.block_moves = HIP_BlockMoves;            // GCG's X / W start / b moves of an outer iteration in one sweep
  be.ritz_in_place = HIP_RitzInPlace;         // GCG's Ritz vectors written over X, P moved in behind them: no ComputeX
  be.panel_norms_sq = HIP_PanelNormsSq;       // column norms summed by the panel update that wrote the columns
  be.multigrid_refresh_check = gcge_hip_multigrid_refresh_check;
  be.multigrid_refresh = gcge_hip_multigrid_refresh;   // a live hierarchy after level 0 took new values in place (multigrid.hip)
  be.mat_identity = HIP_MatIdentity; be.mat_free = HIP_MatFree; be.mat_rows_as_given = HIP_MatRowsAsGiven;
  GCGE_SetBackend(ops, &be);
}
