// New values for a live matrix handle from a DEVICE array (gcge_hip_mat_update_values_device, include/gcge_hip.h): the sparsity
// structure stays, so everything that depends on it alone — rowptr, colidx, the pad-8 index arrays, pid, the offsets of the pattern
// table, spans, the chain layout — is kept, and only what holds values is re-derived, by kernels, without the host:
//   d_val + d_pval   k_mv_values: an 8-lane group per row walks its octets; lane i of octet j reads the new value 8 j + i of the row
//                    (a group reads a contiguous run) and writes it to d_val and to the pad-8 copy, pads 0.0 — a wave's stores to the
//                    pad-8 copy are the contiguous octets of 8 consecutive rows (512 bytes for rows of at most 8 entries);
//   d_rowval         k_mv_rowval: an 8-lane group per row; lane t loads entry t of the row, the group hands the entries round by
//                    shuffles, every lane runs the slot rule (gcge_pat_value_slot, pattern_table.h) and keeps the value that lands in
//                    ITS slot: 64 contiguous bytes per row, 512 per wave;
//   the table        k_mv_table: npat * lt threads; slot k of class p takes the value the slot rule puts there for the FIRST row of
//                    the class (k_mv_first: atomicMin over the run heads of pid, the idiom of k_md_insert in mat_device.hip), written
//                    into a new table that replaces the old one (no thread reads what another writes).
// All checks run BEFORE the first store (k_mv_check, one thread per row, the table read through the cache: at most 64 KB): the row's
// count of present table slots against its length (an explicitly stored +-0.0), every entry placed by the slot rule, and for a value
// table the row's new values against those of the first row of its class, entry by entry as bits (rows of one class carry the same
// offsets in the same order, so equal entries are equal slots), none of them +-0.0.  One flag word comes back.
// A handle with a star or a dense form that kept its value maps (gcge_hip_mat_keep_value_maps) takes the check and the write of
// mat_values_forms.hip around k_mv_values instead; without maps it is declined from the handle alone, as every tile form is.
// A re-ordered handle that kept its entry map (the same switch) first gathers the caller's values into its own order
// (k_mv_gather_entries) and then takes the update above on that block; without the map it is declined from the handle alone.
// A row slab (halo columns, a halo plan) takes all of the above on its own rows: nothing here indexes by column, the offsets of the
// pattern rule are those of the local columns the table was built from.  The call is rank-local: no collective, no exchange.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "gcge_hip.h"
#include "gcge_hip_internal.h"
#include "pattern_table.h"

static long g_mu_stats[6] = {0, 0, 0, 0, 0, 0};
extern "C" void gcge_hip_mat_update_stats(long out[6]) { for (int i = 0; i < 6; ++i) out[i] = g_mu_stats[i]; }

#define MV_BS 256
static unsigned mv_blocks(long n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// first[p] = the first row of class p; only a run head (a row whose pid differs from row r - 1's) touches it
__global__ void k_mv_first_init(int npat, int* __restrict__ first) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < npat) first[p] = INT_MAX;
}
__global__ void k_mv_first(int n, int npat, const unsigned short* __restrict__ pid, int* __restrict__ first) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int p = pid[r];
  if (p >= npat || (r > 0 && pid[r - 1] == p)) return;
  atomicMin(&first[p], (int)r);
}
// flag bits: 1 a row's count of present slots differs from its length, 2 an entry without a slot (or a pid outside the table, or a
// row whose length differs from its class's first row), 4 the classes are not uniform under the new values
__global__ void k_mv_check(int n, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ nv,
                           const unsigned short* __restrict__ pid, const GcgePatEntry* __restrict__ tab, int npat, int lt, int chain_layout,
                           const int* __restrict__ first, int* __restrict__ flag) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int p = pid[r];
  if (p >= npat) { atomicOr(flag, 2); return; }
  const GcgePatEntry* e = tab + (size_t)p * lt;
  const int q0 = rp[r], len = rp[r + 1] - q0;
  int bad = 0;
  if (len > lt || gcge_pat_present_slots(e, lt) != len) bad |= 1;
  unsigned used = 0;
  for (int k = 0; k < len && !(bad & 1); ++k)
    if (gcge_pat_value_slot(e, lt, chain_layout != 0, (long)ci[q0 + k] - r, &used) < 0) { bad |= 2; break; }
  if (first != nullptr && bad == 0) {       // a value table: uniform classes?
    const int f = first[p];
    if (f < 0 || f >= n || rp[f + 1] - rp[f] != len) bad |= 2;
    else {
      const int g0 = rp[f];
      bool same = true;
      for (int k = 0; k < len; ++k) {
        const double v = nv[q0 + k];
        same = same && v != 0.0 && __double_as_longlong(v) == __double_as_longlong(nv[g0 + k]);
      }
      if (!same) bad |= 4;
    }
  }
  if (bad != 0 && (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bad) != bad) atomicOr(flag, bad);
}

// d_val and the pad-8 values of every row (k_md_pad8_fill without the columns): group g = row, lane i of the group
__global__ __launch_bounds__(MV_BS) void k_mv_values(int n, const int* __restrict__ rp, const int* __restrict__ orp, const double* __restrict__ nv,
                                                     double* __restrict__ va, double* __restrict__ pv) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long r = t >> 3;
  const int i = (int)(t & 7);
  if (r >= n) return;
  const int q0 = rp[r], len = rp[r + 1] - q0;
  const size_t o0 = (size_t)orp[r] * 8, o1 = (size_t)orp[r + 1] * 8;
  int k = i;
  for (size_t o = o0 + i; o < o1; o += 8, k += 8) {
    double v = 0.0;
    if (k < len) { v = nv[q0 + k]; va[q0 + k] = v; }
    pv[o] = v;
  }
}
// d_rowval[8 r + slot] by the slot rule (tables of at most 8 slots: rows of at most 8 entries, which k_mv_check has vouched for)
__global__ __launch_bounds__(MV_BS) void k_mv_rowval(int n, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ nv,
                                                     const unsigned short* __restrict__ pid, const GcgePatEntry* __restrict__ tab, int lt,
                                                     int chain_layout, double* __restrict__ rowval) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long r = t >> 3;                      // (blockDim.x is a multiple of 64: the 8 lanes of a group share a wave)
  const int i = (int)(t & 7), lane = (int)(threadIdx.x & 63);
  const bool live = r < n;
  int len = 0; long off = 0; double v = 0.0;
  const GcgePatEntry* e = tab;
  if (live) {
    const int q0 = rp[r];
    len = min(rp[r + 1] - q0, 8);
    e = tab + (size_t)pid[r] * lt;
    if (i < len) { off = (long)ci[q0 + i] - r; v = nv[q0 + i]; }
  }
  double mine = 0.0;
  unsigned used = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {               // every lane of the wave takes part in the shuffles
    const int src = (lane & ~7) | k;
    const long ok = ((long)__shfl((int)(off >> 32), src, 64) << 32) | (unsigned)__shfl((int)off, src, 64);
    const double vk = __hiloint2double(__shfl(__double2hiint(v), src, 64), __shfl(__double2loint(v), src, 64));
    if (k < len) { const int s = gcge_pat_value_slot(e, lt, chain_layout != 0, ok, &used); if (s == i) mine = vk; }
  }
  if (live) rowval[(size_t)r * 8 + i] = mine;
}
// the new table: offsets as they are, the value of every present slot from the class's first row
__global__ void k_mv_table(int npat, int lt, int chain_layout, const int* __restrict__ first, const int* __restrict__ rp, const int* __restrict__ ci,
                           const double* __restrict__ nv, const GcgePatEntry* __restrict__ tab, GcgePatEntry* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= npat * lt) return;
  const int p = idx / lt, k = idx % lt, f = first[p];
  const GcgePatEntry* e = tab + (size_t)p * lt;
  GcgePatEntry o = e[k];
  if (f != INT_MAX && o.val != 0.0) {         // (a class without rows keeps its entry)
    unsigned used = 0;
    for (int q = rp[f]; q < rp[f + 1]; ++q)
      if (gcge_pat_value_slot(e, lt, chain_layout != 0, (long)ci[q] - f, &used) == k) { o.val = nv[q]; break; }
  }
  out[idx] = o;
}

// A re-ordered handle (mat_upload.hip "row orders") holds P A P^T: its CSR values are a fixed permutation of the caller's, recorded at
// creation as emap (GCGE_HIP_MAT_::d_emap).  out[q] = in[emap[q]]: a thread per PAIR of entries of the handle — one 8-byte load of the
// map, two 8-byte loads of values, one 16-byte store (emap and out are allocations of their own and q is even: aligned) —, so a wave
// loads 512 contiguous bytes of map and stores 1024 contiguous bytes; the sources of one re-ordered row are one row of the caller's
// array, permuted inside the row, so the loads of a wave fall into a few row-sized windows.  The last thread takes an odd entry alone.
// (Measured against one entry per thread on the permuted 128^3 matrix of profiles/mat_update_reordered: 3.24 against 3.35 ms per update.)
__global__ __launch_bounds__(MV_BS) void k_mv_gather_entries(long nnz, const int* __restrict__ emap, const double* __restrict__ in,
                                                             double* __restrict__ out) {
  const long q = 2 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (q + 1 < nnz) {
    const int2 e = *(const int2*)(emap + q);
    *(double2*)(out + q) = make_double2(in[e.x], in[e.y]);
  } else if (q < nnz) out[q] = in[emap[q]];
}

// the update of a handle whose values are stored in the order of d_val (the handle has passed the checks on the handle alone)
static int mv_update(GCGE_HIP_MAT* A, const double* d_val) {
  const bool forms = gcge_hip_mat_has_value_form(A) != 0;
  hipStream_t st = (hipStream_t)gcge_hip_stream();
  const int n = A->nrows, lt = A->pat_lt, npat = A->npat;
  if (forms) {
    if (A->d_pid != nullptr || gcge_hip_mat_forms_check(A, d_val, &g_mu_stats[5]) != 0) { g_mu_stats[3] += 1; return 1; }
    if (n > 0) k_mv_values<<<mv_blocks(8L * n, MV_BS), MV_BS, 0, st>>>(n, A->d_rowptr, A->d_orp, d_val, A->d_val, A->d_pval);
    gcge_hip_mat_forms_write(A, d_val);
    GCGE_HIP_CHECK(hipGetLastError());
    GCGE_HIP_CHECK(hipStreamSynchronize(st));
    g_mu_stats[0] += 1;
    return 0;
  }
  const int chain_layout = A->pat_span2 <= -1 ? 1 : 0;
  const GcgePatEntry* tab = (const GcgePatEntry*)A->d_tab;
  const bool value_table = A->d_pid != nullptr && A->d_rowval == nullptr;
  int* d_first = nullptr;
  bool rewrite = false, convert = false;
  if (A->d_pid != nullptr) {
    int* d_flag = nullptr;
    GCGE_HIP_CHECK(hipMalloc(&d_flag, sizeof(int)));
    GCGE_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    if (value_table) {
      GCGE_HIP_CHECK(hipMalloc(&d_first, (size_t)npat * sizeof(int)));
      k_mv_first_init<<<mv_blocks(npat, MV_BS), MV_BS, 0, st>>>(npat, d_first);
      k_mv_first<<<mv_blocks(n, MV_BS), MV_BS, 0, st>>>(n, npat, A->d_pid, d_first);
    }
    k_mv_check<<<mv_blocks(n, MV_BS), MV_BS, 0, st>>>(n, A->d_rowptr, A->d_colidx, d_val, A->d_pid, tab, npat, lt, chain_layout, d_first, d_flag);
    GCGE_HIP_CHECK(hipGetLastError());
    int flag = 0;
    GCGE_HIP_CHECK(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    GCGE_HIP_CHECK(hipStreamSynchronize(st));
    g_mu_stats[5] += (long)sizeof(int);
    hipFree(d_flag);
    rewrite = value_table && (flag & 4) == 0;
    convert = value_table && !rewrite;
    if ((flag & 3) != 0 || (convert && lt > 8)) {
      if (d_first != nullptr) hipFree(d_first);
      g_mu_stats[3] += 1;
      return 1;
    }
  }
  // from here on the handle is written
  if (n > 0) k_mv_values<<<mv_blocks(8L * n, MV_BS), MV_BS, 0, st>>>(n, A->d_rowptr, A->d_orp, d_val, A->d_val, A->d_pval);
  GcgePatEntry* d_newtab = nullptr;
  if (rewrite) {
    GCGE_HIP_CHECK(hipMalloc(&d_newtab, (size_t)npat * lt * sizeof(GcgePatEntry)));
    k_mv_table<<<mv_blocks((long)npat * lt, MV_BS), MV_BS, 0, st>>>(npat, lt, chain_layout, d_first, A->d_rowptr, A->d_colidx, d_val, tab, d_newtab);
  } else if (A->d_pid != nullptr) {
    if (convert) {
      GCGE_HIP_CHECK(hipMalloc(&A->d_rowval, (size_t)(n ? n : 1) * 8 * sizeof(double)));   // (the scatter writes all 8 slots of every row: unused ones 0.0)
    }
    k_mv_rowval<<<mv_blocks(8L * n, MV_BS), MV_BS, 0, st>>>(n, A->d_rowptr, A->d_colidx, d_val, A->d_pid, tab, lt, chain_layout, A->d_rowval);
  }
  GCGE_HIP_CHECK(hipGetLastError());
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  if (rewrite) { hipFree(A->d_tab); A->d_tab = d_newtab; g_mu_stats[1] += 1; }
  if (d_first != nullptr) hipFree(d_first);
  if (convert) g_mu_stats[2] += 1; else g_mu_stats[0] += 1;
  return 0;
}

extern "C" int gcge_hip_mat_update_values_device(GCGE_HIP_MAT* A, long nnz, const double* d_val) {
  if (A == nullptr || d_val == nullptr || nnz != A->nnz) { g_mu_stats[4] += 1; return -1; }
  // declined from the handle alone: tile forms, star / dense forms without value maps (gcge_hip_mat_forms_check), rectangular handles,
  // re-ordered handles without an entry map.  A row slab is taken like a whole matrix: its d_val is in the caller's entry order
  // (gcge_dist_localize only renames columns; a slab never has a row order of its own) and every stored copy of a value derives from
  // the rank's own rows, so the call stays rank-local and collective-free.
  if (A->tile != nullptr || A->rect_ncols > 0 || (real_perm(A->perm) != nullptr && A->d_emap == nullptr) || A->d_orp == nullptr ||
      (A->d_pid != nullptr && (A->d_tab == nullptr || A->pat_lt < 1 || A->pat_lt > 16 || A->npat < 1 || (A->d_rowval != nullptr && A->pat_lt > 8)))) {
    g_mu_stats[3] += 1;
    return 1;
  }
  // a slab's halo exchange moves X, not matrix values, but a split product may still be reading the handle: the back-end's stream and,
  // where the exchange runs over a transfer stream of the back-end's own, that stream drain before the first store
  if (A->nghost > 0 || A->exchange != nullptr || A->exchange_begin != nullptr || A->native_halo != nullptr) {
    GCGE_HIP_CHECK(hipStreamSynchronize((hipStream_t)gcge_hip_stream()));
    if (A->native_halo != nullptr) gcge_hip_comm_transfer_sync();
  }
  if (A->d_emap == nullptr) return mv_update(A, d_val);
  // a re-ordered handle: the caller's values in the handle's order, in a block of the pool, then the update as it is.  The gather writes
  // the block only, so a decline has still written nothing to the handle; everything runs on one stream, and the block goes back after
  // the stream has drained (the caller's array is no longer read either).
  hipStream_t st = (hipStream_t)gcge_hip_stream();
  const size_t bytes = (size_t)(nnz > 0 ? nnz : 1) * sizeof(double);
  double* work = (double*)gcge_hip_pool_alloc(bytes);
  if (nnz > 0) k_mv_gather_entries<<<mv_blocks((nnz + 1) / 2, MV_BS), MV_BS, 0, st>>>(nnz, A->d_emap, d_val, work);
  GCGE_HIP_CHECK(hipGetLastError());
  const int rc = mv_update(A, work);
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  gcge_hip_pool_free(work, bytes);
  return rc;
}
