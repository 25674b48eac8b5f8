// Matrix handle of the HIP back-end (the CCSMAT counterpart, reference app/app_ccs.h:20-24): upload of the host CSR arrays,
// their analysis into the forms the K1 kernels take (pad-8 copy, row patterns, star + remainder, dense blocks, tiles), the halo
// plan of a row slab, destruction.  Split off app_hip.hip in round 4; the multivector slots live there, the products in mat_product.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <map>
#include <unordered_map>
#include <vector>

#include "gcge_hip.h"
#include "gcge_hip_internal.h"
#include "pattern_table.h"
#include "star_split.h"

#define g_spmm_path (gcge_hip_spmm_path_get())
#define g_offset_patterns (gcge_hip_offset_patterns_get())

// ------------------------------------------------------------------ matrix
// Pattern format: rows written as {(column - row, value)} in CSR order; at most 64 KB of table.  Leaves
// A->d_pid == NULL when the matrix has too many distinct rows (irregular matrices give up after a few
// hundred rows, so the scan costs nothing there).
typedef GcgePatEntry PatEntryH;
// by_offsets: rows are compared by their column offsets only; the table then carries 1.0 for every present entry and the
// values travel per row (A->d_rowval: 8 doubles per row in table-slot order, tables of at most 8 slots): stencils with
// variable coefficients keep the pattern kernels at 64 more bytes per row and 16-column pass.
static void build_patterns(GCGE_HIP_MAT* A, int nrows, int ncols_local, const int* rowptr, const int* colidx, const double* val,
                           bool by_offsets = false) {
  A->d_pid = nullptr; A->d_tab = nullptr; A->npat = 0; A->pat_lt = 0; A->pat_near = 0; A->d_rowval = nullptr;
  int maxlen = 0;
  for (int r = 0; r < nrows; ++r) maxlen = std::max(maxlen, rowptr[r + 1] - rowptr[r]);
  const int lt = gcge_hip_pattern_width(maxlen);
  if (lt == 0 || nrows == 0 || (by_offsets && lt > 8)) return;
  const int maxpat = gcge_pat_max_patterns(lt);
  std::vector<PatEntryH> tab;
  std::unordered_map<uint64_t, std::vector<int>> byhash;
  std::vector<unsigned short> pid((size_t)nrows);
  auto same = [&](int p, int r) {
    const PatEntryH* e = &tab[(size_t)p * lt];
    const int len = rowptr[r + 1] - rowptr[r];
    for (int k = 0; k < len; ++k) {
      const int q = rowptr[r] + k;
      if (e[k].off != (long)colidx[q] - r || (!by_offsets && memcmp(&e[k].val, &val[q], sizeof(double)) != 0)) return false;
      if (by_offsets && e[k].val == 0.0) return false;   // (a padding slot: the table row is shorter)
    }
    for (int k = len; k < lt; ++k) if (e[k].off != 0 || e[k].val != 0.0) return false;
    return true;
  };
  int prev = -1;
  for (int r = 0; r < nrows; ++r) {
    if (prev >= 0 && same(prev, r)) { pid[r] = (unsigned short)prev; continue; }
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)(rowptr[r + 1] - rowptr[r]);
    for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) {
      uint64_t vb; memcpy(&vb, &val[q], 8);
      if (by_offsets) vb = 1;
      h = (h ^ (uint64_t)((long)colidx[q] - r)) * 0xBF58476D1CE4E5B9ull; h ^= h >> 29;
      h = (h ^ vb) * 0x94D049BB133111EBull; h ^= h >> 32;
    }
    int found = -1;
    std::vector<int>& cand = byhash[h];
    for (int p : cand) if (same(p, r)) { found = p; break; }
    if (found < 0) {
      if ((int)(tab.size() / lt) >= maxpat) return;   // not a pattern matrix
      found = (int)(tab.size() / lt);
      for (int k = 0; k < lt; ++k) {
        const int q = rowptr[r] + k;
        PatEntryH e = {0.0, 0};
        if (q < rowptr[r + 1]) { e.val = by_offsets ? 1.0 : val[q]; e.off = (long)colidx[q] - r; }
        tab.push_back(e);
      }
      cand.push_back(found);
    }
    pid[r] = (unsigned short)found; prev = found;
  }
  // (b) the table side, shared with the device search (pattern_table.h): spans of the most frequent pattern, then the chain layout
  // from the rows' distinct (pattern, head, tail, mask) keys in order of first occurrence
  A->npat = (int)(tab.size() / lt); A->pat_lt = lt;
  std::vector<long> freq((size_t)A->npat, 0);
  for (int r = 0; r < nrows; ++r) ++freq[pid[r]];
  GcgePatPlan plan;
  gcge_pat_plan(tab, freq, lt, plan);
  A->pat_span = plan.span; A->pat_span2 = plan.span2;
  if (plan.chain) {
    std::unordered_map<uint64_t, int> id_of;
    std::vector<uint64_t> keys;
    std::vector<unsigned short> cpid((size_t)nrows);
    bool ok = true;
    for (int r = 0; r < nrows; ++r) {
      const uint64_t key = gcge_pat_row_key(plan, pid[r], r, nrows, ncols_local);
      auto it = id_of.find(key);
      if (it == id_of.end()) {
        if ((int)keys.size() >= maxpat) { ok = false; break; }
        it = id_of.emplace(key, (int)keys.size()).first;
        keys.push_back(key);
      }
      cpid[r] = (unsigned short)it->second;
    }
    std::vector<PatEntryH> ctab;
    if (ok && gcge_pat_chain_table(plan, keys, ctab)) {
      tab.swap(ctab); pid.swap(cpid);
      A->npat = (int)(tab.size() / lt);
      gcge_pat_chain_spans(plan, tab, &A->pat_span2, &A->pat_near);
    }
  }
  if (by_offsets) {
    // the row's values in the slot order of ITS table row: an entry sits in the slot that carries its offset (the
    // diagonal in slot 1 of a chain-layout table, where slots whose address would leave the block also read offset 0)
    const bool chain_layout = A->pat_span2 <= -1;
    std::vector<double> rv((size_t)nrows * 8, 0.0);
    bool ok = true;
    for (int r = 0; r < nrows && ok; ++r) {
      const PatEntryH* e = &tab[(size_t)pid[r] * lt];
      unsigned used = 0;
      for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) {
        const long off = (long)colidx[q] - r;
        int slot = -1;
        if (chain_layout && off == 0) slot = 1;
        else for (int k = 0; k < lt; ++k) if (!(used >> k & 1) && e[k].off == off && e[k].val != 0.0 && !(chain_layout && off == 0 && k != 1)) { slot = k; break; }
        if (slot < 0 || (used >> slot & 1)) { ok = false; break; }
        used |= 1u << slot;
        rv[(size_t)r * 8 + slot] = val[q];
      }
    }
    if (!ok) { A->npat = 0; return; }   // (cannot happen for tables built above; the matrix then keeps the generic kernels)
    GCGE_HIP_CHECK(hipMalloc(&A->d_rowval, rv.size() * sizeof(double)));
    GCGE_HIP_CHECK(hipMemcpy(A->d_rowval, rv.data(), rv.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  GCGE_HIP_CHECK(hipMalloc(&A->d_pid, (size_t)nrows * sizeof(unsigned short)));
  GCGE_HIP_CHECK(hipMalloc(&A->d_tab, tab.size() * sizeof(PatEntryH)));
  GCGE_HIP_CHECK(hipMemcpy(A->d_pid, pid.data(), (size_t)nrows * sizeof(unsigned short), hipMemcpyHostToDevice));
  GCGE_HIP_CHECK(hipMemcpy(A->d_tab, tab.data(), tab.size() * sizeof(PatEntryH), hipMemcpyHostToDevice));
}

// ---------------------------------------------------------------------------------------------------------------- geometry
// The masked grid a whole matrix lives on stays on the handle — named by the caller (kind 1) or recovered at upload (kind 2) —
// independent of the K1 form: host and device copies of the box array.  A geometry that is not one (box indices out of the box or
// not strictly ascending) is not recorded.
static void mat_set_geometry(GCGE_HIP_MAT* A, int kind, int nx, int ny, int nz, const int* box) {
  const long nbox = (long)nx * ny * nz;
  if (A == nullptr || box == nullptr || nx < 1 || ny < 1 || nz < 1 || nbox > 2147483647L || A->nghost != 0 || A->row_begin != 0) return;
  for (int r = 0; r < A->nrows; ++r) if (box[r] < 0 || box[r] >= nbox || (r > 0 && box[r] <= box[r - 1])) return;
  free(A->h_box); if (A->d_box) hipFree(A->d_box);
  A->h_box = (int*)malloc((size_t)(A->nrows ? A->nrows : 1) * sizeof(int));
  memcpy(A->h_box, box, (size_t)A->nrows * sizeof(int));
  GCGE_HIP_CHECK(hipMalloc(&A->d_box, (size_t)(A->nrows ? A->nrows : 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMemcpy(A->d_box, box, (size_t)A->nrows * sizeof(int), hipMemcpyHostToDevice));
  A->geom_kind = kind; A->geom_dims[0] = nx; A->geom_dims[1] = ny; A->geom_dims[2] = nz;
}
extern "C" int gcge_hip_mat_geometry(const GCGE_HIP_MAT* A, int* dims, int* box_of_row) {
  if (A == nullptr || A->geom_kind == 0) return 0;
  if (dims != nullptr) { dims[0] = A->geom_dims[0]; dims[1] = A->geom_dims[1]; dims[2] = A->geom_dims[2]; }
  if (box_of_row != nullptr) memcpy(box_of_row, A->h_box, (size_t)A->nrows * sizeof(int));
  return A->geom_kind;
}

// rows of one slab with LOCAL column indices in [0, ncols_local); columns >= nrows are halo rows.  ghost_global (may be NULL): the
// global rows behind the halo columns, ascending — with it (and nglobal) a slab of a grid matrix cut on plane boundaries keeps the
// plane sweep of spmm_star.hip: the planes below and above the slab are then found among the halo rows.  geom (may be NULL): the
// masked grid the caller names; one named for a whole matrix (cols false) also means that none is recovered for the handle.
// Value maps (value_maps.h, mat_values_forms.hip): with the switch on when a matrix is created, a handle that takes the star or the dense form
// also keeps, on the device, where each of its stored values came from — what gcge_hip_mat_update_values_device needs to give such a
// handle new values in place.  The forms and every stored array are those of the switch off; the maps cost about 4 bytes per block slot
// and remainder slot plus 1 byte per CSR entry under a star (gcge_hip_mat_value_maps).  Default 0.
static int g_keep_value_maps = 0;
extern "C" int gcge_hip_mat_keep_value_maps(int on) { const int was = g_keep_value_maps; g_keep_value_maps = on != 0; return was; }   // returns the setting it replaces
extern "C" long gcge_hip_mat_value_maps(const GCGE_HIP_MAT* A) {
  if (A == nullptr || !gcge_hip_mat_holds_value_maps(A)) return 0;
  const void* DM = A->star != nullptr ? A->star_rem : A->dense;
  return gcge_hip_star_maps_bytes(A->star_maps) + gcge_hip_dense_value_maps(DM, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}
static double upload_now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
static GCGE_HIP_MAT* mat_create_local(int nrows, int ncols_local, int nglobal, int row_begin, const int* rowptr, const int* colidx, const double* val,
                                      const int* ghost_global, const GcgeGridGeom* geom) {
  if (gcge_hip_init(-1) != 0) return nullptr;
  const bool timing = getenv("GCGE_UPLOAD_TIMING") != nullptr;   // phases of the host-side analysis on stderr
  double t_phase = upload_now();
  auto phase = [&](const char* what) { if (timing) { const double t = upload_now(); fprintf(stderr, "gcge_hip upload: %-28s %.3f s\n", what, t - t_phase); t_phase = t; } };
  GCGE_HIP_MAT* A = (GCGE_HIP_MAT*)calloc(1, sizeof(GCGE_HIP_MAT));
  A->nrows = nrows; A->nglobal = nglobal; A->row_begin = row_begin; A->nnz = rowptr[nrows];
  A->nghost = ncols_local - nrows;
  GCGE_REQUIRE(A->nghost >= 0, "gcge_hip_mat_create_local: ncols_local >= nrows");
  if (ghost_global != nullptr && A->nghost > 0) {
    A->h_ghost_global = (int*)malloc((size_t)A->nghost * sizeof(int));
    memcpy(A->h_ghost_global, ghost_global, (size_t)A->nghost * sizeof(int));
  }
  {
    const int nt = gcge_upload_threads();
    std::vector<int> bad((size_t)nt, 0);
    gcge_parallel_chunks(A->nnz, nt, [&](int c, long k0, long k1) { int b = 0; for (long k = k0; k < k1; ++k) b |= (colidx[k] < 0) | (colidx[k] >= ncols_local); bad[c] = b; });
    for (int c = 0; c < nt; ++c) GCGE_REQUIRE(bad[c] == 0, "gcge_hip_mat_create_local: column index in range");
  }
  const size_t nnz = (size_t)A->nnz;
  GCGE_HIP_CHECK(hipMalloc(&A->d_rowptr, ((size_t)nrows + 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&A->d_colidx, (nnz ? nnz : 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&A->d_val, (nnz ? nnz : 1) * sizeof(double)));
  GCGE_HIP_CHECK(hipMemcpy(A->d_rowptr, rowptr, ((size_t)nrows + 1) * sizeof(int), hipMemcpyHostToDevice));
  GCGE_HIP_CHECK(hipMemcpy(A->d_colidx, colidx, nnz * sizeof(int), hipMemcpyHostToDevice));
  GCGE_HIP_CHECK(hipMemcpy(A->d_val, val, nnz * sizeof(double), hipMemcpyHostToDevice));
  // pad-8 copy: every row padded to a multiple of 8 entries with (own column, 0.0).  The kernel LOADS the X row a pad names (weight
  // 0), so a pad's column must be a row of X: row r is one because ncols_local >= nrows (required above, nghost >= 0).  Matrices
  // with more rows than columns (multigrid.hip's prolongations) have no pad-8 copy and take gcge_hip_csr_spmm.
  std::vector<int> orp((size_t)nrows + 1);
  size_t noct = 0;
  for (int r = 0; r < nrows; ++r) { orp[r] = (int)noct; noct += ((size_t)(rowptr[r + 1] - rowptr[r]) + 7) / 8; }
  orp[nrows] = (int)noct;
  std::vector<int> pc(noct * 8);
  std::vector<double> pv(noct * 8);
  gcge_parallel_chunks(nrows, gcge_upload_threads(), [&](int, long r0, long r1) {
    for (long r = r0; r < r1; ++r) {
      size_t o = (size_t)orp[r] * 8; int k;
      for (k = rowptr[r]; k < rowptr[r + 1]; ++k, ++o) { pc[o] = colidx[k]; pv[o] = val[k]; }
      for (; o < (size_t)orp[r + 1] * 8; ++o) { pc[o] = (int)r; pv[o] = 0.0; }
    }
  });
  A->noct = (long)noct;
  GCGE_HIP_CHECK(hipMalloc(&A->d_orp, ((size_t)nrows + 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&A->d_pcol, (noct ? noct * 8 : 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&A->d_pval, (noct ? noct * 8 : 1) * sizeof(double)));
  GCGE_HIP_CHECK(hipMemcpy(A->d_orp, orp.data(), ((size_t)nrows + 1) * sizeof(int), hipMemcpyHostToDevice));
  GCGE_HIP_CHECK(hipMemcpy(A->d_pcol, pc.data(), noct * 8 * sizeof(int), hipMemcpyHostToDevice));
  GCGE_HIP_CHECK(hipMemcpy(A->d_pval, pv.data(), noct * 8 * sizeof(double), hipMemcpyHostToDevice));
  phase("CSR + pad-8 copies");
  build_patterns(A, nrows, ncols_local, rowptr, colidx, val);
  if (A->d_pid == nullptr && g_offset_patterns) build_patterns(A, nrows, ncols_local, rowptr, colidx, val, true);   // same stencil, other coefficients in every row
  // matrices without a pattern form whose rows are mostly ONE star stencil on a grid (free diagonal): those rows leave the CSR
  // arrays for the plane sweep of spmm_star.hip, the others (rows inside dense blocks, ...) keep every entry and take the block form
  phase("pattern search");
  A->star = nullptr; A->star_rem = nullptr;
  // (a row slab keeps them like a whole matrix: the maps index the CSR entries of the local arrays, which are the caller's entries —
  //  gcge_dist_localize only renames columns —, and every stored value of a slab derives from the rank's own rows)
  const int keep_maps = g_keep_value_maps;
  if (A->d_pid == nullptr) {
    // (the sweep needs to know where the slab sits in the grid: a whole matrix, or a slab with its global size and halo rows named)
    const bool whole = row_begin == 0 && ncols_local == nrows && (nglobal <= 0 || nglobal == nrows);
    const bool slab = !whole && nglobal > 0 && (ncols_local == nrows || ghost_global != nullptr);
    gcge::StarHost* H = nullptr;                    // the split behind S: ours
    void* S = (whole || slab) ? gcge_hip_star_build(nrows, ncols_local, row_begin, whole ? nrows : nglobal, ghost_global, rowptr, colidx, val, geom, &H, keep_maps) : nullptr;
    phase("star split");
    if (S != nullptr && whole && (geom == nullptr || geom->cols) && gcge_hip_star_masked_form(S) != 0) {
      // a masked grid nobody named for the whole matrix: what the build recovered from the rows goes on the handle, whatever becomes of the
      // grid form below (own_box empty: a world of ONE slab with its local columns named — the handle still carries what the rows show)
      int* od = H->own_dims;
      if (!H->own_box.empty() || gcge::star_infer_box(nrows, rowptr, colidx, &H->own_box, &od[0], &od[1], &od[2]))
        mat_set_geometry(A, 2, od[0], od[1], od[2], H->own_box.data());
      phase("geometry for the handle");
    }
    if (S != nullptr) {
      void* D = gcge_hip_dense_build_rows(nrows, ncols_local, H->rem_rowptr.data(), H->rem_col.data(), H->rem_val.data(),
                                          (const unsigned char*)H->clean.data(), keep_maps);   // (its pad-8 part lists the other rows only)
      if (D != nullptr) { A->star = S; A->star_rem = D; } else gcge_hip_star_free(S);   // (the block form switched off, gcge_hip_spmm_dense_mode(-1): the forms below)
      if (D != nullptr && keep_maps) A->star_maps = gcge_hip_star_maps_create(H, A->nnz);
      delete H;
      phase("blocks + listed rows");
    }
  }
  // matrices without a pattern form: dense row blocks (supernodes) on MFMA + remainder CSR, where such blocks exist
  A->dense = (A->d_pid == nullptr && A->star == nullptr) ? gcge_hip_dense_build(nrows, ncols_local, rowptr, colidx, val, keep_maps) : nullptr;
  // ... and, where switched on, row tiles with LDS-staged X rows
  A->tile = ((A->d_pid == nullptr && A->star == nullptr) || gcge_hip_spmm_tile_mode_get() == 2) ? gcge_hip_tile_build(nrows, ncols_local, rowptr, colidx, val) : nullptr;
  // interior rows: none of them references a halo column (slabs: everything but the first and the last plane)
  A->ov_lo = 0; A->ov_hi = nrows;
  if (A->nghost > 0) {
    for (int r = 0; r < nrows; ++r) {
      bool g = false;
      for (int k = rowptr[r]; k < rowptr[r + 1] && !g; ++k) g = colidx[k] >= nrows;
      if (!g) continue;
      if (r < nrows / 2) A->ov_lo = r + 1; else { A->ov_hi = r; break; }
    }
  }
  return A;
}
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_local_ghosts(int nrows, int ncols_local, int nglobal, int row_begin, const int* rowptr, const int* colidx,
                                                          const double* val, const int* ghost_global) {
  return mat_create_local(nrows, ncols_local, nglobal, row_begin, rowptr, colidx, val, ghost_global, nullptr);
}
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_local(int nrows, int ncols_local, int nglobal, int row_begin, const int* rowptr, const int* colidx, const double* val) {
  return mat_create_local(nrows, ncols_local, nglobal, row_begin, rowptr, colidx, val, nullptr, nullptr);
}
// a ROW SLAB of a masked grid: the box index of every local column — the own rows, then the halo rows (ascending by global row); NULL: none
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_local_ghosts_grid(int nrows, int ncols_local, int nglobal, int row_begin, const int* rowptr, const int* colidx,
                                                               const double* val, const int* ghost_global, int nx, int ny, int nz, const int* box_of_local_col) {
  const GcgeGridGeom geom = {nx, ny, nz, box_of_local_col, ncols_local, true};
  return mat_create_local(nrows, ncols_local, nglobal, row_begin, rowptr, colidx, val, ghost_global, box_of_local_col != nullptr ? &geom : nullptr);
}
// ---------------------------------------------------------------------------------------------------------------- row orders
// (round 5)  A whole matrix (one rank) that shows neither a pattern form nor a grid in the order it arrives in is
// re-ordered INSIDE the handle: grid coordinates recovered from the graph of a star stencil (gcge_hip_reorder_star_grid: scan order,
// the plane sweep applies again) or reverse Cuthill-McKee (a banded matrix gathers from a window of X).  The solver never sees it:
// handles are opaque, blocks of vectors created for the matrix live in the new order, gcge_hip_mv_to_host / from_host
// and the reference-order random fill translate.  mode: 0 automatic (matrices of >= 65 536 rows without a fast form), 1 every matrix
// without a fast form (tests), -1 never.
static int g_reorder_mode = 0;
extern "C" void gcge_hip_spmm_reorder_mode(int mode) { g_reorder_mode = mode; }
static std::vector<GcgePerm*> g_perms;          // live orders, one per n
static unsigned g_perm_next_id = 1;
static char g_reorder_kind[64] = "";
extern "C" const char* gcge_hip_mat_row_order(const GCGE_HIP_MAT* A) {
  if (A == nullptr || A->perm == nullptr || A->perm->identity) return "as given";
  return g_reorder_kind[0] ? g_reorder_kind : "reordered";
}
extern "C" GcgePerm* gcge_hip_perm_acquire(GcgePerm* p) { if (p) ++p->refs; return p; }
extern "C" void gcge_hip_perm_release(GcgePerm* p) {
  if (p == nullptr || --p->refs > 0) return;
  for (size_t i = 0; i < g_perms.size(); ++i) if (g_perms[i] == p) { g_perms.erase(g_perms.begin() + (long)i); break; }
  free(p->perm); free(p->iperm); free(p);
}
static GcgePerm* perm_find(int n) { for (GcgePerm* p : g_perms) if (p->n == n) return p; return nullptr; }
static GcgePerm* perm_register(int n, const int* perm /* NULL: identity */) {
  GcgePerm* p = (GcgePerm*)calloc(1, sizeof(GcgePerm));
  p->n = n; p->identity = perm == nullptr; p->id = g_perm_next_id++;
  if (perm != nullptr) {
    p->perm = (int*)malloc((size_t)n * sizeof(int)); p->iperm = (int*)malloc((size_t)n * sizeof(int));
    memcpy(p->perm, perm, (size_t)n * sizeof(int));
    for (int i = 0; i < n; ++i) p->iperm[perm[i]] = i;
  }
  g_perms.push_back(p);
  return p;
}
// for mat_device.hip: the live order of size n (NULL: none), and the identity order of size n, registered when no order of that size
// is live (NULL: a re-ordered one is) — neither takes a reference
extern "C" GcgePerm* gcge_hip_perm_live(int n) { return perm_find(n); }
extern "C" GcgePerm* gcge_hip_perm_identity(int n) {
  GcgePerm* P = perm_find(n);
  if (P == nullptr) P = perm_register(n, nullptr);
  return P->identity ? P : nullptr;
}
// P A P^T as CSR with ascending columns: new row i = old row perm[i], old column c -> iperm[c].  Each entry rides through the sort
// with its index in the caller's arrays (the columns of a row are distinct: the order is decided by them alone); emap (may be NULL)
// takes it: emap[q] = k, the entry of the caller's arrays that sits at position q of the new ones — what an update of the values in
// place needs (mat_values.hip).  val and va may be NULL together: the structure alone.
static void permute_csr_into(int n, const int* rowptr, const int* colidx, const double* val, const int* perm, const int* iperm,
                             int* rp, int* ci, double* va, int* emap) {
  rp[0] = 0;
  for (int i = 0; i < n; ++i) rp[i + 1] = rp[i] + (rowptr[perm[i] + 1] - rowptr[perm[i]]);
  gcge_parallel_chunks(n, gcge_upload_threads(), [&](int, long r0, long r1) {
    std::vector<std::pair<int, int>> tmp;             // (new column, the caller's entry)
    for (long i = r0; i < r1; ++i) {
      const int o = perm[i];
      tmp.clear();
      for (int k = rowptr[o]; k < rowptr[o + 1]; ++k) tmp.emplace_back(iperm[colidx[k]], k);
      std::sort(tmp.begin(), tmp.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
      int q = rp[i];
      for (auto& e : tmp) {
        ci[q] = e.first;
        if (va != nullptr) va[q] = val[e.second];
        if (emap != nullptr) emap[q] = e.second;
        ++q;
      }
    }
  });
}
static void permute_csr(int n, const int* rowptr, const int* colidx, const double* val, const GcgePerm* P,
                        std::vector<int>& rp, std::vector<int>& ci, std::vector<double>& va, std::vector<int>* emap) {
  rp.resize((size_t)n + 1); ci.resize((size_t)rowptr[n] ? (size_t)rowptr[n] : 1); va.resize(ci.size());
  if (emap != nullptr) emap->resize(ci.size());
  permute_csr_into(n, rowptr, colidx, val, P->perm, P->iperm, rp.data(), ci.data(), va.data(), emap != nullptr ? emap->data() : nullptr);
}
// tests: the routine above on the caller's arrays, no device.  perm[new] = old; rowptr_new: n + 1 ints, colidx_new and emap: rowptr[n]
// ints each.  0: done; -1: perm is no permutation of [0, n), or n < 0
extern "C" int gcge_hip_reorder_entry_map(int n, const int* rowptr, const int* colidx, const int* perm, int* rowptr_new, int* colidx_new, int* emap) {
  if (n < 0 || rowptr_new == nullptr) return -1;
  if (n == 0) { rowptr_new[0] = 0; return 0; }
  if (rowptr == nullptr || perm == nullptr || colidx_new == nullptr || emap == nullptr || (colidx == nullptr && rowptr[n] > 0)) return -1;
  std::vector<int> iperm((size_t)n, -1);
  for (int i = 0; i < n; ++i) {
    if (perm[i] < 0 || perm[i] >= n || iperm[perm[i]] >= 0) return -1;
    iperm[perm[i]] = i;
  }
  permute_csr_into(n, rowptr, colidx, nullptr, perm, iperm.data(), rowptr_new, colidx_new, nullptr, emap);
  return 0;
}
// The entry map of a re-ordered handle goes to the device when gcge_hip_mat_keep_value_maps is on at creation (4 bytes per entry: too
// much to keep unasked); with the switch off the handle is what it is without this record.
static void mat_keep_entry_map(GCGE_HIP_MAT* A, const std::vector<int>& emap) {
  if (A == nullptr) return;
  GCGE_HIP_CHECK(hipMalloc(&A->d_emap, (size_t)(A->nnz > 0 ? A->nnz : 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMemcpy(A->d_emap, emap.data(), (size_t)A->nnz * sizeof(int), hipMemcpyHostToDevice));
}
extern "C" long gcge_hip_mat_entry_map(const GCGE_HIP_MAT* A) { return (A != nullptr && A->d_emap != nullptr) ? (long)A->nnz * (long)sizeof(int) : 0; }
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create(int nrows, int nglobal, int row_begin, const int* rowptr,
                                             const int* colidx, const double* val) {
  if (row_begin != 0 || nrows != nglobal) {
    fprintf(stderr, "gcge_hip_mat_create: a row slab needs gcge_dist_localize + gcge_hip_mat_create_local\n");
    return nullptr;
  }
  const bool timing = getenv("GCGE_UPLOAD_TIMING") != nullptr;
  std::vector<int> rp, ci; std::vector<double> va;
  std::vector<int> em;                                      // the entry map, recorded only where an update in place was asked for
  std::vector<int>* emap = g_keep_value_maps ? &em : nullptr;
  // a matrix of this size lives in this process already: the new one shares its row order (B after A of a generalised problem; its
  // structure is its own, and so is its entry map)
  if (GcgePerm* P = perm_find(nrows)) {
    if (P->identity) {
      GCGE_HIP_MAT* A = gcge_hip_mat_create_local(nrows, nrows, nglobal, 0, rowptr, colidx, val);
      if (A != nullptr) A->perm = gcge_hip_perm_acquire(P);
      return A;
    }
    permute_csr(nrows, rowptr, colidx, val, P, rp, ci, va, emap);
    GCGE_HIP_MAT* A = gcge_hip_mat_create_local(nrows, nrows, nglobal, 0, rp.data(), ci.data(), va.data());
    if (A != nullptr) A->perm = gcge_hip_perm_acquire(P);
    if (A != nullptr && emap != nullptr) mat_keep_entry_map(A, em);
    return A;
  }
  GCGE_HIP_MAT* A = gcge_hip_mat_create_local(nrows, nrows, nglobal, 0, rowptr, colidx, val);
  if (A == nullptr) return nullptr;
  const bool fast = A->d_pid != nullptr || A->star != nullptr;
  const bool want = g_reorder_mode == 1 || (g_reorder_mode == 0 && nrows >= 65536);
  if (fast || !want || nrows < 64) { A->perm = gcge_hip_perm_acquire(perm_register(nrows, nullptr)); return A; }
  // no fast form in the order given: look for a better one
  double t0 = upload_now();
  std::vector<int> perm((size_t)nrows), box((size_t)nrows);
  int dims[3] = {0, 0, 0};
  bool have = false, grid = false;
  const long placed = gcge_hip_reorder_star_grid(nrows, rowptr, colidx, val, dims, box.data());
  if (placed > 0) {                                       // scan order of the recovered grid: ascending box index
    for (int i = 0; i < nrows; ++i) perm[i] = i;
    std::sort(perm.begin(), perm.end(), [&](int a, int b) { return box[a] < box[b]; });
    have = grid = true;
    snprintf(g_reorder_kind, sizeof g_reorder_kind, "grid %d x %d x %d recovered from the star couplings", dims[0], dims[1], dims[2]);
  } else if (gcge_hip_reorder_rcm(nrows, rowptr, colidx, perm.data()) == 0) {
    std::vector<int> ip((size_t)nrows);
    for (int i = 0; i < nrows; ++i) ip[perm[i]] = i;
    const double b0 = gcge_hip_mean_bandwidth(nrows, rowptr, colidx, nullptr), b1 = gcge_hip_mean_bandwidth(nrows, rowptr, colidx, ip.data());
    have = b1 < 0.5 * b0;                                 // (a matrix that is banded already stays as it is)
    snprintf(g_reorder_kind, sizeof g_reorder_kind, "reverse Cuthill-McKee (mean |i - j| %.0f -> %.0f)", b0, b1);
  }
  if (timing) fprintf(stderr, "gcge_hip upload: %-28s %.3f s (%s)\n", "row order", upload_now() - t0, have ? g_reorder_kind : "kept as given");
  if (!have) { A->perm = gcge_hip_perm_acquire(perm_register(nrows, nullptr)); return A; }
  gcge_hip_mat_destroy(A);
  GcgePerm* P = perm_register(nrows, perm.data());
  permute_csr(nrows, rowptr, colidx, val, P, rp, ci, va, emap);
  const bool masked = grid && (long)dims[0] * dims[1] * dims[2] != nrows;   // a ball: name the geometry for the plane sweep's row map
  std::vector<int> bsorted(masked ? (size_t)nrows : 0);
  for (int i = 0; i < nrows && masked; ++i) bsorted[i] = box[perm[i]];
  const GcgeGridGeom geom = {dims[0], dims[1], dims[2], bsorted.data(), nrows, false};
  A = mat_create_local(nrows, nrows, nglobal, 0, rp.data(), ci.data(), va.data(), nullptr, masked ? &geom : nullptr);
  if (A == nullptr) { gcge_hip_perm_release(gcge_hip_perm_acquire(P)); return nullptr; }
  A->perm = gcge_hip_perm_acquire(P);
  if (emap != nullptr) mat_keep_entry_map(A, em);
  return A;
}
// A matrix on a MASKED grid (one rank): row r is grid point box_of_row[r] = x + nx (y + ny z) of an nx x ny x nz box, rows in scan
// order — the real-space DFT matrices behind BASELINE config 5 live on the grid points inside a sphere (PARSEC).  With the
// geometry named, the rows that are a star stencil on that grid take the plane sweep of spmm_star.hip (through a row map);
// without it such a matrix is served by dense blocks + the pad-8 kernel.  The geometry only selects kernels: results are those
// of gcge_hip_mat_create on the same arrays.
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_grid(int nrows, const int* rowptr, const int* colidx, const double* val,
                                                  int nx, int ny, int nz, const int* box_of_row) {
  // (the caller named the geometry: the rows stay as given and nothing is recovered from them for the handle, even if what was named is none)
  const bool named = box_of_row != nullptr && nx > 0 && ny > 0 && nz > 0;
  const GcgeGridGeom geom = {nx, ny, nz, named ? box_of_row : nullptr, nrows, false};
  GCGE_HIP_MAT* A = mat_create_local(nrows, nrows, nrows, 0, rowptr, colidx, val, nullptr, &geom);
  if (A != nullptr) { GcgePerm* P = perm_find(nrows); if (P == nullptr) P = perm_register(nrows, nullptr); if (P->identity) A->perm = gcge_hip_perm_acquire(P); }
  if (A != nullptr && named) mat_set_geometry(A, 1, nx, ny, nz, box_of_row);
  return A;
}
// A whole matrix whose rows stay as given whatever the row order search would do and whatever order another matrix of its size lives
// in: the coarse levels of a hierarchy whose prolongations are numbered like its rows (multigrid.hip).  It shares the identity order of
// its size when there is one (or none yet); beside a re-ordered matrix of the same size it carries no order record, which means the
// caller's order to every block created for it.
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_as_given(int nrows, const int* rowptr, const int* colidx, const double* val) {
  GCGE_HIP_MAT* A = gcge_hip_mat_create_local(nrows, nrows, nrows, 0, rowptr, colidx, val);
  if (A == nullptr) return nullptr;
  GcgePerm* P = perm_find(nrows);
  if (P == nullptr) P = perm_register(nrows, nullptr);
  if (P->identity) A->perm = gcge_hip_perm_acquire(P);
  return A;
}
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_csr(const GCGE_CSR* A) {
  if (A->row_begin == 0 && A->nrows == A->ncols) return gcge_hip_mat_create(A->nrows, A->ncols, 0, A->rowptr, A->colidx, A->val);
  // a localized slab: ncols = nrows + nghost (gcge_dist_localize)
  return gcge_hip_mat_create_local(A->nrows, A->ncols, -1, A->row_begin, A->rowptr, A->colidx, A->val);
}
// halo plan: send_rows = local rows to ship (grouped by destination rank, ascending), buffers hold
// buf_cols columns of nsend / nghost rows; exchange() moves sendbuf -> the peers' recvbuf.
extern "C" void gcge_hip_mat_set_halo(GCGE_HIP_MAT* A, int nglobal, int nsend, const int* send_rows, double* sendbuf,
                                      double* recvbuf, int buf_cols, gcge_halo_exchange_fn fn, void* ctx) {
  A->nglobal = nglobal; A->nsend = nsend; A->sendbuf = sendbuf; A->recvbuf = recvbuf; A->buf_cols = buf_cols;
  A->exchange = fn; A->exchange_ctx = ctx;
  for (int i = 0; i < nsend; ++i) GCGE_REQUIRE(send_rows[i] >= 0 && send_rows[i] < A->nrows, "halo send row in range");
  if (A->d_send_rows) hipFree(A->d_send_rows);
  GCGE_HIP_CHECK(hipMalloc(&A->d_send_rows, (nsend ? nsend : 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMemcpy(A->d_send_rows, send_rows, nsend * sizeof(int), hipMemcpyHostToDevice));
}
// optional: a split form of the exchange installed by gcge_hip_mat_set_halo — begin(sendbuf, recvbuf, ncols, ctx)
// posts the transfers of the packed rows and returns, end(ctx) returns when recvbuf is complete
extern "C" void gcge_hip_mat_set_halo_async(GCGE_HIP_MAT* A, gcge_halo_exchange_fn begin, void (*end)(void*)) {
  A->exchange_begin = begin; A->exchange_end = end;
}
extern "C" void gcge_hip_mat_destroy(GCGE_HIP_MAT* A) {
  if (!A) return;
  hipFree(A->d_rowptr); hipFree(A->d_colidx); hipFree(A->d_val);
  if (A->rect_ncols > 0) { hipFree(A->d_t_rowptr); hipFree(A->d_t_colidx); hipFree(A->d_t_val); gcge_hip_perm_release(A->perm); free(A); return; }   // a prolongation (multigrid.hip)
  hipFree(A->d_orp); hipFree(A->d_pcol); hipFree(A->d_pval);
  if (A->d_pid) { hipFree(A->d_pid); hipFree(A->d_tab); }
  if (A->d_rowval) hipFree(A->d_rowval);
  if (A->d_send_rows) hipFree(A->d_send_rows);
  if (A->tile != nullptr) gcge_hip_tile_free(A->tile);
  if (A->dense != nullptr) gcge_hip_dense_free(A->dense);
  if (A->star_rem != nullptr) gcge_hip_dense_free(A->star_rem);
  if (A->star != nullptr) gcge_hip_star_free(A->star);
  if (A->star_maps != nullptr) gcge_hip_star_maps_free(A->star_maps);
  if (A->d_emap != nullptr) hipFree(A->d_emap);
  if (A->native_halo != nullptr) gcge_hip_halo_native_free(A);   // RCCL plan + the exchange buffers it owns (rccl_comm.hip)
  free(A->h_ghost_global); free(A->h_part);
  free(A->h_box); if (A->d_box) hipFree(A->d_box);
  gcge_hip_perm_release(A->perm);
  free(A);
}
// the row partition of all ranks a slab belongs to (world + 1 offsets): recorded by gcge_hip_mat_create_slab, or by whoever built
// the slab through gcge_hip_mat_create_local_ghosts + its own halo plan — MultiGridCreate coarsens a slab only when it knows it
extern "C" void gcge_hip_mat_set_partition(GCGE_HIP_MAT* A, const long* part, int world) {
  free(A->h_part); A->h_part = nullptr; A->part_world = 0;
  if (part == nullptr || world < 1) return;
  A->h_part = (long*)malloc((size_t)(world + 1) * sizeof(long));
  memcpy(A->h_part, part, (size_t)(world + 1) * sizeof(long));
  A->part_world = world;
}
extern "C" int gcge_hip_mat_nrows(const GCGE_HIP_MAT* A) { return A->nrows; }
extern "C" long gcge_hip_mat_nnz(const GCGE_HIP_MAT* A) { return A->nnz; }
// number of row patterns the SpMM pattern path works with (0: the matrix is served by the generic pad-8 kernels)
extern "C" int gcge_hip_mat_patterns(const GCGE_HIP_MAT* A) { return A->d_pid ? A->npat : 0; }
// 1: the pattern table is in chain layout (the +-S rows of the stencil stay in registers between iterations);
// 2: additionally slots 3,4 hold the +-L rows that the waves of a block exchange through LDS
extern "C" int gcge_hip_mat_pattern_chain(const GCGE_HIP_MAT* A) {
  if (!A->d_pid || A->pat_span2 > -1) return 0;
  return A->pat_span2 <= -8 ? 2 : 1;
}

// which K1 form MatDotMultiVec takes for this matrix at block widths >= 16 (bench.py names the kernel in its roofline)
extern "C" const char* gcge_hip_mat_spmm_form(const GCGE_HIP_MAT* A) {
  if (A->d_pid != nullptr && g_spmm_path == 0) {
    const int ch = gcge_hip_mat_pattern_chain(A);
    if (A->d_rowval != nullptr) return ch == 2 ? "spmm_pattern_chain2+values" : "spmm_pattern+values";   // offsets-only table, values per row
    return ch == 2 ? "spmm_pattern_chain2" : ch == 1 ? "spmm_pattern_chain" : "spmm_pattern";
  }
  if (A->star != nullptr && g_spmm_path == 0) return gcge_hip_dense_remainder_is_tiled(A->star_rem) ? "spmm_star+spmm_dense+spmm_tile" : "spmm_star+spmm_dense+spmm_pad8";
  if (A->dense != nullptr && g_spmm_path != 1 && g_spmm_path != 3 && g_spmm_path != 4) return gcge_hip_dense_remainder_is_tiled(A->dense) ? "spmm_dense+spmm_tile" : "spmm_dense+spmm_pad8";
  if (A->tile != nullptr && g_spmm_path != 1 && g_spmm_path != 3) return "spmm_tile";
  return "spmm_pad8";
}

// what the upload made of a matrix without a pattern form (measurement aid): out[0..4] = dense blocks, row blocks of 32, non-zeros
// in blocks, stored block entries, remainder non-zeros; out[5..11] = tiles of the remainder (0: pad-8), X rows staged per matrix
// row, ELL entries per non-zero, overflow entries, brick dimensions.  0: the matrix has no block form.
extern "C" int gcge_hip_mat_form_stats(const GCGE_HIP_MAT* A, double* out) {
  for (int i = 0; i < 12; ++i) out[i] = 0.0;
  const void* DM = A->star != nullptr ? A->star_rem : A->dense;       // (with a grid form: the block form of the rows it leaves)
  if (DM == nullptr) return 0;
  long nb = 0, items = 0, dn = 0, de = 0, rn = 0;
  gcge_hip_dense_stats(DM, &nb, &items, &dn, &de, &rn);
  out[0] = (double)nb; out[1] = (double)items; out[2] = (double)dn; out[3] = (double)de; out[4] = (double)rn;
  if (const void* T = gcge_hip_dense_remainder_tile(DM)) {
    long nt = 0, ov = 0; double xr = 0, el = 0; int brick[3] = {0, 0, 0}; long strides[2];
    gcge_hip_tile_stats(T, &nt, &ov, &xr, &el, brick, strides);
    out[5] = (double)nt; out[6] = xr; out[7] = el; out[8] = (double)ov; out[9] = brick[0]; out[10] = brick[1]; out[11] = brick[2];
  }
  return 1;
}
extern "C" int gcge_hip_mat_star_masked_form(const GCGE_HIP_MAT* A) { return A->star != nullptr ? gcge_hip_star_masked_form(A->star) : 0; }
// the grid form (spmm_star.hip): out[0..5] = nx, ny, nz, arm length of the star, rows it multiplies, rows of the matrix.  0: none.
extern "C" int gcge_hip_mat_star_stats(const GCGE_HIP_MAT* A, long* out) {
  if (A->star == nullptr) return 0;
  gcge_hip_star_stats(A->star, out);
  return 1;
}

