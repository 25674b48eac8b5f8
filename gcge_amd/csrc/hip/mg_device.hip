// The aggregation hierarchy on the device: the kernels behind the device path of MultiGridCreate (multigrid.hip).
//
// What csrc/host/multigrid.c does on host CSR arrays, done here on the device-resident CSR of a level, with the same results bit for
// bit: grid aggregation (gcge_mg_aggregate_grid: 2 x 2 x 2 cells, the last cell of an odd direction one layer thick), the members of
// every aggregate in ascending fine-row order (aggregate_members), the cells of a masked grid (gcge_mg_aggregate_masked: the occupied
// cells counted, numbered by a sum, their members found in the sorted box array), the Galerkin product Ac = scale P^T A P for a piecewise-constant
// P (gcge_mg_galerkin) and the two CSR triples of P / P^T (gcge_mg_prolongation).
//
// Galerkin product: one wave per coarse row I.  Its entries are the entries of its member rows, member rows ascending, each row in
// storage order, walked in chunks of 64 (one entry per lane).  Pass 1 (count): the distinct coarse columns agg[col] go into an LDS
// hash table (integer atomics only); their number is the row's length.  Pass 2 (fill): the same set, ranked (the columns ascending),
// then the values: the lane that owns a column (rank % 64) adds the chunk's matching values one after the other in entry order, from
// 0.0, and multiplies by scale at the end only when scale != 1.0 — the host's summation order, so the same doubles.  A row with more
// than MG_DCAP distinct coarse columns sets a flag and the caller falls back to the host build.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "gcge_hip.h"
#include "gcge_multigrid.h"
#include "gcge_hip_internal.h"

#define MG_WAVE 64
#define MG_HT 1024      // hash slots per coarse row (power of two)
#define MG_DCAP 512     // distinct coarse columns per coarse row handled here (more: the flag, then the host build)

static hipStream_t mg_stream() { return (hipStream_t)gcge_hip_stream(); }

// ------------------------------------------------------------------------------------------------------------ aggregation of a grid
__global__ void k_mg_agg_grid(int nx, int ny, long nf, int cx, int cy, int* __restrict__ agg) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nf) return;
  const int x = (int)(r % nx), y = (int)((r / nx) % ny), z = (int)(r / ((long)nx * ny));
  agg[r] = cx * ((y / 2) + cy * (z / 2)) + x / 2;
}
// members of cell I: count (pass 0, into ptr[I + 1]) or the fine rows ascending (pass 1, at ptr[I])
__global__ void k_mg_members_grid(int nx, int ny, int nz, int cx, int cy, int nc, int pass, int* __restrict__ ptr, int* __restrict__ mem) {
  const int I = blockIdx.x * blockDim.x + threadIdx.x;
  if (I >= nc) return;
  const int ix = I % cx, iy = (I / cx) % cy, iz = I / (cx * cy);
  const int wx = 2 * ix + 1 < nx ? 2 : 1, wy = 2 * iy + 1 < ny ? 2 : 1, wz = 2 * iz + 1 < nz ? 2 : 1;
  if (pass == 0) { ptr[I + 1] = wx * wy * wz; return; }
  int q = ptr[I];
  for (int dz = 0; dz < wz; ++dz)
    for (int dy = 0; dy < wy; ++dy)
      for (int dx = 0; dx < wx; ++dx) mem[q++] = (2 * ix + dx) + nx * ((2 * iy + dy) + ny * (2 * iz + dz));
}

// ------------------------------------------------------------------------------------------------------------ aggregation of a masked grid
// gcge_mg_aggregate_masked on the device: row r is box point box[r] (strictly ascending) of the box nx x ny x nz, its cell the
// 2 x 2 x 2 cell of that point.  Integer atomics count the rows of every cell (a count does not depend on the order of its
// increments); two sums over the cells number the occupied ones and place their members; the members themselves are FOUND, not
// collected: a cell's points in ascending box index are its rows in ascending order, and box is sorted, so each is a binary search.
__device__ inline int mg_cell_of(int b, int nx, int ny, int cx, int cy) {
  const int x = b % nx, y = (b / nx) % ny, z = b / (nx * ny);
  return cx * ((y / 2) + cy * (z / 2)) + x / 2;
}
// cnt[1 + cell] = rows in the cell
__global__ void k_mg_masked_count(int nf, const int* __restrict__ box, int nx, int ny, int cx, int cy, int* __restrict__ cnt) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < nf) atomicAdd(&cnt[1 + mg_cell_of(box[r], nx, ny, cx, cy)], 1);
}
__global__ void k_mg_masked_flag(int ncell, const int* __restrict__ cnt, int* __restrict__ occ) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < ncell) occ[1 + c] = cnt[1 + c] > 0;
}
// after the sums: occ[c] = occupied cells before c (the number of cell c when it is one), cnt[c] = rows in the cells before c
__global__ void k_mg_masked_agg(int nf, const int* __restrict__ box, int nx, int ny, int cx, int cy, const int* __restrict__ occ, int* __restrict__ agg) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < nf) agg[r] = occ[mg_cell_of(box[r], nx, ny, cx, cy)];
}
__global__ void k_mg_masked_cells(int nf, const int* __restrict__ box, int nx, int ny, int nz, int cx, int cy, int ncell, int nc,
                                  const int* __restrict__ occ, const int* __restrict__ cnt, int* __restrict__ ptr, int* __restrict__ mem,
                                  int* __restrict__ cbox) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) ptr[nc] = nf;
  if (c >= ncell || cnt[c + 1] == cnt[c]) return;
  const int I = occ[c], ix = c % cx, iy = (c / cx) % cy, iz = c / (cx * cy);
  int q = cnt[c];
  const int q1 = cnt[c + 1];
  ptr[I] = q; cbox[I] = c;
  for (int dz = 0; dz < 2; ++dz)
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx) {
        const int x = 2 * ix + dx, y = 2 * iy + dy, z = 2 * iz + dz;
        if (x >= nx || y >= ny || z >= nz || q >= q1) continue;
        const int b = x + nx * (y + ny * z);
        int lo = 0, hi = nf;                          // first row with box[row] >= b
        while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (box[mid] < b) lo = mid + 1; else hi = mid; }
        if (lo < nf && box[lo] == b) mem[q++] = lo;
      }
}

// ------------------------------------------------------------------------------------------------------------ Galerkin product
struct MgRowLds {
  int keys[MG_HT];       // coarse column in the slot, -1: empty
  int kpos[MG_HT];       // its index in dl
  int dl[MG_DCAP];       // the distinct columns in arrival order
  int rnk[MG_DCAP];      // their ranks (ascending column order)
  double acc[MG_DCAP];   // sums by rank
  int mbeg[MG_WAVE], moff[MG_WAVE + 1];   // a batch of member rows: start in A, offset in the batch's entry list
  int cr[MG_WAVE]; double cv[MG_WAVE];                   // a chunk: rank and value of every entry
  int ndist, over;
};

__device__ inline unsigned mg_hash(int c) { return ((unsigned)c * 2654435761u) >> (32 - 10); }     // log2(MG_HT) = 10
static_assert(MG_HT == 1024, "mg_hash assumes 1024 slots");

// slot of column c in the table (inserting it when absent); -1 when the row has overflowed
__device__ inline int mg_insert(MgRowLds& s, int c) {
  unsigned h = mg_hash(c);
  for (int probe = 0; probe < MG_HT; ++probe, h = (h + 1) & (MG_HT - 1)) {
    const int old = atomicCAS(&s.keys[h], -1, c);
    if (old == -1) {
      const int p = atomicAdd(&s.ndist, 1);
      if (p < MG_DCAP) { s.dl[p] = c; s.kpos[h] = p; } else s.over = 1;
      return (int)h;
    }
    if (old == c) return (int)h;
  }
  s.over = 1;
  return -1;
}
__device__ inline int mg_lookup(const MgRowLds& s, int c) {
  unsigned h = mg_hash(c);
  for (int probe = 0; probe < MG_HT; ++probe, h = (h + 1) & (MG_HT - 1)) if (s.keys[h] == c) return (int)h;
  return -1;
}

// walk the entries of coarse row I in the host's order: fn(c, v, i, n) per chunk of n <= 64 entries, lane i holds entry i (c = -1:
// no entry / a column >= nf); every lane calls fn the same number of times (block = one wave, __syncthreads orders LDS).  S: the
// kernel's LDS record, of which the walk uses mbeg / moff
template <class S, class F>
__device__ inline void mg_walk_row(S& s, int I, int nf, const int* __restrict__ ptr, const int* __restrict__ mem, const int* __restrict__ rowptr,
                                   const int* __restrict__ colidx, const double* __restrict__ val, const int* __restrict__ agg, bool want_val, F fn) {
  const int lane = threadIdx.x;
  const int q0 = ptr[I], q1 = ptr[I + 1];
  for (int qb = q0; qb < q1; qb += MG_WAVE) {
    const int nm = min(MG_WAVE, q1 - qb);
    int len = 0;
    if (lane < nm) { const int r = mem[qb + lane]; s.mbeg[lane] = rowptr[r]; len = rowptr[r + 1] - s.mbeg[lane]; }
    s.moff[lane + 1] = len;
    __syncthreads();
    if (lane == 0) { s.moff[0] = 0; for (int m = 0; m < nm; ++m) s.moff[m + 1] += s.moff[m]; }
    __syncthreads();
    const int tot = s.moff[nm];
    for (int eb = 0; eb < tot; eb += MG_WAVE) {
      const int e = eb + lane, n = min(MG_WAVE, tot - eb);
      int c = -1; double v = 0.0;
      if (e < tot) {
        int lo = 0, hi = nm - 1;                      // member m with moff[m] <= e < moff[m + 1]
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s.moff[mid] <= e) lo = mid; else hi = mid - 1; }
        const int k = s.mbeg[lo] + (e - s.moff[lo]);
        const int col = colidx[k];
        if (col >= 0 && col < nf) c = agg[col];
        if (want_val) v = val[k];
      }
      fn(c, v, lane, n);
    }
    __syncthreads();
  }
}

// pass 1 (FILL = false): cnt[I] = distinct coarse columns of row I;  pass 2: colidx / val of row I at rowptr_c[I]
template <bool FILL>
__global__ void __launch_bounds__(MG_WAVE) k_mg_galerkin(int nc, int nf, const int* __restrict__ ptr, const int* __restrict__ mem,
    const int* __restrict__ rowptr, const int* __restrict__ colidx, const double* __restrict__ val, const int* __restrict__ agg, double scale,
    long long* __restrict__ cnt, const int* __restrict__ rowptr_c, int* __restrict__ colidx_c, double* __restrict__ val_c, int* __restrict__ flag) {
  __shared__ MgRowLds s;
  const int lane = threadIdx.x;
  for (int I = blockIdx.x; I < nc; I += gridDim.x) {
    for (int h = lane; h < MG_HT; h += MG_WAVE) s.keys[h] = -1;
    if (lane == 0) { s.ndist = 0; s.over = 0; }
    __syncthreads();
    mg_walk_row(s, I, nf, ptr, mem, rowptr, colidx, val, agg, false, [&](int c, double, int, int) {
      if (c >= 0 && !s.over) mg_insert(s, c);
      __syncthreads();
    });
    const int nd = s.ndist;
    if (s.over) { if (lane == 0) { if (!FILL) cnt[I] = nd; *flag = 1; } __syncthreads(); continue; }
    if (!FILL) { if (lane == 0) cnt[I] = nd; __syncthreads(); continue; }
    // ranks: the position of every distinct column in ascending order
    for (int j = lane; j < nd; j += MG_WAVE) {
      const int cj = s.dl[j]; int r = 0;
      for (int i = 0; i < nd; ++i) r += s.dl[i] < cj;
      s.rnk[j] = r; s.acc[r] = 0.0;
    }
    __syncthreads();
    mg_walk_row(s, I, nf, ptr, mem, rowptr, colidx, val, agg, true, [&](int c, double v, int i, int n) {
      const int h = c >= 0 ? mg_lookup(s, c) : -1;
      s.cr[i] = h >= 0 ? s.rnk[s.kpos[h]] : -1; s.cv[i] = v;
      __syncthreads();
      for (int t = 0; t < n; ++t) { const int r = s.cr[t]; if (r >= 0 && (r & (MG_WAVE - 1)) == lane) s.acc[r] += s.cv[t]; }
      __syncthreads();
    });
    const int base = rowptr_c[I];
    for (int j = lane; j < nd; j += MG_WAVE) {
      const int r = s.rnk[j];
      colidx_c[base + r] = s.dl[j];
      double a = s.acc[r];
      if (scale != 1.0) a *= scale;
      val_c[base + r] = a;
    }
    __syncthreads();
  }
}

// Values only, for a coarse structure that exists (gcge_hip_mg_galerkin_values_device: the refresh of a live hierarchy, multigrid.hip):
// the row's ascending coarse columns staged in LDS, every entry's place among them by binary search — no hash, no count pass —, then the
// sums of k_mg_galerkin<true>: the lane that owns a rank adds its values one by one in walk order from 0.0, times scale at the end when
// scale != 1.0.  7.3 KB of LDS per wave.  A row is written whole or not at all: an entry whose coarse column the row does not hold, or
// a row of more than MG_DCAP columns, sets the flag and leaves the row's values alone.
// SLAB (a level of a row-slab hierarchy, multigrid.hip): agg is the level's colagg — one entry per LOCAL column, halo columns included
// (nf counts them all) — and the coarse row lists its columns in ascending GLOBAL order under local names: own columns [0, nown), then
// the halo columns, of which the first nlo lie below the slab.  mg_slab_key turns a local column into its rank in that global order, so
// the staged row is ascending again and the search is the same; the sums are the build's (gcge_mg_build_slab adds a coarse entry's
// contributions in walk order from 0.0, then times scale).
__device__ inline int mg_slab_key(int c, int nown, int nlo) { return c < nown ? c + nlo : (c - nown < nlo ? c - nown : c); }
struct MgValLds {
  int col[MG_DCAP];      // the coarse row's columns, ascending
  double acc[MG_DCAP];   // sums by rank
  int mbeg[MG_WAVE], moff[MG_WAVE + 1];
  int cr[MG_WAVE]; double cv[MG_WAVE];
  int miss;
};
template <bool SLAB>
__global__ void __launch_bounds__(MG_WAVE) k_mg_galerkin_values(int nc, int nf, const int* __restrict__ ptr, const int* __restrict__ mem,
    const int* __restrict__ rowptr, const int* __restrict__ colidx, const double* __restrict__ val, const int* __restrict__ agg, double scale,
    const int* __restrict__ rowptr_c, const int* __restrict__ colidx_c, double* __restrict__ val_c, int* __restrict__ flag, int nown, int nlo) {
  __shared__ MgValLds s;
  const int lane = threadIdx.x;
  for (int I = blockIdx.x; I < nc; I += gridDim.x) {
    const int base = rowptr_c[I], nd = rowptr_c[I + 1] - base;
    if (nd < 0 || nd > MG_DCAP) { if (lane == 0) *flag = 1; continue; }       // (uniform over the wave)
    for (int j = lane; j < nd; j += MG_WAVE) { const int cj = colidx_c[base + j]; s.col[j] = SLAB ? mg_slab_key(cj, nown, nlo) : cj; s.acc[j] = 0.0; }
    if (lane == 0) s.miss = 0;
    __syncthreads();
    mg_walk_row(s, I, nf, ptr, mem, rowptr, colidx, val, agg, true, [&](int c, double v, int i, int n) {
      int r = -1;
      if (SLAB && c >= 0) c = mg_slab_key(c, nown, nlo);
      if (c >= 0) {
        int lo = 0, hi = nd;                          // first column >= c
        while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (s.col[mid] < c) lo = mid + 1; else hi = mid; }
        if (lo < nd && s.col[lo] == c) r = lo; else s.miss = 1;
      }
      s.cr[i] = r; s.cv[i] = v;
      __syncthreads();
      for (int t = 0; t < n; ++t) { const int q = s.cr[t]; if (q >= 0 && (q & (MG_WAVE - 1)) == lane) s.acc[q] += s.cv[t]; }
      __syncthreads();
    });
    if (s.miss) { if (lane == 0) *flag = 1; }
    else
      for (int j = lane; j < nd; j += MG_WAVE) {
        double a = s.acc[j];
        if (scale != 1.0) a *= scale;
        val_c[base + j] = a;
      }
    __syncthreads();
  }
}

__global__ void k_mg_ll_to_int(long n, const long long* __restrict__ a, int* __restrict__ b) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) b[i] = (int)a[i];
}
__global__ void k_mg_prolong(long nf, int* __restrict__ rowptr, double* __restrict__ val, double* __restrict__ t_val) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r <= nf) rowptr[r] = (int)r;
  if (r < nf) { val[r] = 1.0; t_val[r] = 1.0; }
}

// grid detection from the sampled rows r = i * step only: their entries with a column > r (all gcge_mg_detect_grid reads) as offsets
// col - r, counted (pass 0: cnt[i], the largest count and offset in mx[0..1]) then written at pos[i] (pass 1; 16 bits when they fit)
__global__ void k_mg_detect(int pass, long ns, long step, const int* __restrict__ rowptr, const int* __restrict__ colidx, int* __restrict__ cnt,
                            int* __restrict__ mx, const long long* __restrict__ pos, int wide, void* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  const long r = i * step;
  long q = pass == 1 ? pos[i] : 0; int c = 0, mo = 0;
  for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) {
    const long col = colidx[k];
    if (col <= r) continue;
    if (pass == 0) { ++c; mo = max(mo, (int)(col - r)); }
    else if (wide) ((int*)out)[q++] = (int)(col - r);
    else ((unsigned short*)out)[q++] = (unsigned short)(col - r);
  }
  if (pass == 0) { cnt[i] = c; atomicMax(&mx[0], c); atomicMax(&mx[1], mo); }
}
__global__ void k_mg_pack(long ns, const int* __restrict__ cnt, int wide, void* __restrict__ out, long long* __restrict__ pos) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  if (wide) ((int*)out)[i] = cnt[i]; else ((unsigned char*)out)[i] = (unsigned char)cnt[i];
  pos[i + 1] = cnt[i];
}

static unsigned mg_blocks(long n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// in-place inclusive sum of n >= 1 values on the back-end's stream
template <class T>
static void mg_inclusive_sum(T* d, long n) {
  size_t bytes = 0;
  GCGE_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, bytes, d, d, (int)n, mg_stream()));
  void* tmp = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&tmp, bytes ? bytes : 8));
  GCGE_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(tmp, bytes, d, d, (int)n, mg_stream()));
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  GCGE_HIP_CHECK(hipFree(tmp));
}

// ------------------------------------------------------------------------------------------------------------ host entry points
// gcge_mg_detect_grid on a whole matrix's device CSR without downloading it: the rows the host function samples, with their entries
// above the diagonal (counts in 8 bits and offsets in 16 bits when they fit), on a host CSR whose other rows are empty — the same
// answer by construction
extern "C" int gcge_hip_mg_detect_grid_device(int n, const int* d_rowptr, const int* d_colidx, int dims[3], long* d2h) {
  if (n < 8) return 0;
  const long step = n > (1 << 20) ? n / (1 << 20) : 1, ns = (n + step - 1) / step;
  int *d_cnt = nullptr, *d_mx = nullptr; long long* d_pos = nullptr; void* d_c = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d_cnt, (size_t)ns * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_mx, 2 * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_pos, ((size_t)ns + 1) * sizeof(long long)));
  GCGE_HIP_CHECK(hipMalloc(&d_c, (size_t)ns * sizeof(int)));
  GCGE_HIP_CHECK(hipMemsetAsync(d_mx, 0, 2 * sizeof(int), mg_stream()));
  GCGE_HIP_CHECK(hipMemsetAsync(d_pos, 0, sizeof(long long), mg_stream()));
  hipLaunchKernelGGL(k_mg_detect, dim3(mg_blocks(ns, 256)), dim3(256), 0, mg_stream(), 0, ns, step, d_rowptr, d_colidx, d_cnt, d_mx,
                     (const long long*)nullptr, 0, (void*)nullptr);
  GCGE_HIP_CHECK(hipGetLastError());
  int mx[2] = {0, 0};
  GCGE_HIP_CHECK(hipMemcpyAsync(mx, d_mx, sizeof mx, hipMemcpyDeviceToHost, mg_stream()));
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  const int wide_c = mx[0] > 255, wide_o = mx[1] > 65535;
  hipLaunchKernelGGL(k_mg_pack, dim3(mg_blocks(ns, 256)), dim3(256), 0, mg_stream(), ns, (const int*)d_cnt, wide_c, d_c, d_pos);
  mg_inclusive_sum(d_pos + 1, ns);
  long long tot = 0;
  GCGE_HIP_CHECK(hipMemcpy(&tot, d_pos + ns, sizeof tot, hipMemcpyDeviceToHost));
  void* d_o = nullptr;
  const size_t osz = wide_o ? sizeof(int) : sizeof(unsigned short), csz = wide_c ? sizeof(int) : 1;
  GCGE_HIP_CHECK(hipMalloc(&d_o, (size_t)(tot ? tot : 1) * osz));
  hipLaunchKernelGGL(k_mg_detect, dim3(mg_blocks(ns, 256)), dim3(256), 0, mg_stream(), 1, ns, step, d_rowptr, d_colidx, (int*)nullptr,
                     (int*)nullptr, (const long long*)d_pos, wide_o, d_o);
  GCGE_HIP_CHECK(hipGetLastError());
  std::vector<unsigned char> hc((size_t)ns * csz), ho((size_t)(tot ? tot : 1) * osz);
  GCGE_HIP_CHECK(hipMemcpy(hc.data(), d_c, (size_t)ns * csz, hipMemcpyDeviceToHost));
  if (tot > 0) GCGE_HIP_CHECK(hipMemcpy(ho.data(), d_o, (size_t)tot * osz, hipMemcpyDeviceToHost));
  if (d2h) *d2h += (long)(sizeof mx + sizeof tot + (size_t)ns * csz + (size_t)tot * osz);
  hipFree(d_cnt); hipFree(d_mx); hipFree(d_pos); hipFree(d_c); hipFree(d_o);
  std::vector<int> rp((size_t)n + 1, 0), ci((size_t)(tot ? tot : 1));
  long q = 0;
  for (long r = 0; r < n; ++r) {
    if (r % step == 0) {
      const long i = r / step;
      const int c = wide_c ? ((const int*)hc.data())[i] : hc[i];
      for (int j = 0; j < c; ++j, ++q) ci[q] = (int)r + (wide_o ? ((const int*)ho.data())[q] : ((const unsigned short*)ho.data())[q]);
    }
    rp[r + 1] = (int)q;
  }
  GCGE_CSR S; memset(&S, 0, sizeof S);
  S.nrows = n; S.ncols = n; S.row_begin = 0; S.nnz = q; S.rowptr = rp.data(); S.colidx = ci.data(); S.val = nullptr;
  return gcge_mg_detect_grid(&S, dims, nullptr);
}

extern "C" void gcge_hip_mg_agg_grid_device(const int dims[3], int* d_agg, int* d_ptr, int* d_mem, int cdims[3]) {
  const int nx = dims[0], ny = dims[1], nz = dims[2];
  const int cx = (nx + 1) / 2, cy = (ny + 1) / 2, cz = (nz + 1) / 2;
  const long nf = (long)nx * ny * nz; const int nc = cx * cy * cz;
  cdims[0] = cx; cdims[1] = cy; cdims[2] = cz;
  hipLaunchKernelGGL(k_mg_agg_grid, dim3(mg_blocks(nf, 256)), dim3(256), 0, mg_stream(), nx, ny, nf, cx, cy, d_agg);
  GCGE_HIP_CHECK(hipMemsetAsync(d_ptr, 0, sizeof(int), mg_stream()));
  hipLaunchKernelGGL(k_mg_members_grid, dim3(mg_blocks(nc, 256)), dim3(256), 0, mg_stream(), nx, ny, nz, cx, cy, nc, 0, d_ptr, d_mem);
  mg_inclusive_sum(d_ptr + 1, nc);
  hipLaunchKernelGGL(k_mg_members_grid, dim3(mg_blocks(nc, 256)), dim3(256), 0, mg_stream(), nx, ny, nz, cx, cy, nc, 1, d_ptr, d_mem);
  GCGE_HIP_CHECK(hipGetLastError());
}

// the cells of a masked grid from its device-resident box array (nf strictly ascending box indices of the box dims, checked by
// whoever put the geometry on the handle): d_agg / d_mem (nf ints, the caller's) are filled, *d_ptr_out (nc + 1 ints) and *d_cbox_out
// (nc ints: the coarse level's box array) are allocated here (hipFree).  Returns the number of aggregates; one int comes back.
extern "C" int gcge_hip_mg_agg_masked_device(const int dims[3], const int* d_box, int nf, int* d_agg, int* d_mem, int** d_ptr_out,
                                             int** d_cbox_out, int cdims[3], long* d2h) {
  const int nx = dims[0], ny = dims[1], nz = dims[2];
  const int cx = (nx + 1) / 2, cy = (ny + 1) / 2, cz = (nz + 1) / 2;
  const long ncell_l = (long)cx * cy * cz;
  GCGE_REQUIRE(nf > 0 && (long)nx * ny * nz <= 2147483647L && nf <= (long)nx * ny * nz, "gcge_hip_mg_agg_masked_device: the rows are points of the box");
  const int ncell = (int)ncell_l;
  cdims[0] = cx; cdims[1] = cy; cdims[2] = cz;
  int *d_cnt = nullptr, *d_occ = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d_cnt, ((size_t)ncell + 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_occ, ((size_t)ncell + 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMemsetAsync(d_cnt, 0, ((size_t)ncell + 1) * sizeof(int), mg_stream()));
  GCGE_HIP_CHECK(hipMemsetAsync(d_occ, 0, sizeof(int), mg_stream()));
  hipLaunchKernelGGL(k_mg_masked_count, dim3(mg_blocks(nf, 256)), dim3(256), 0, mg_stream(), nf, d_box, nx, ny, cx, cy, d_cnt);
  hipLaunchKernelGGL(k_mg_masked_flag, dim3(mg_blocks(ncell, 256)), dim3(256), 0, mg_stream(), ncell, (const int*)d_cnt, d_occ);
  GCGE_HIP_CHECK(hipGetLastError());
  mg_inclusive_sum(d_cnt + 1, ncell);
  mg_inclusive_sum(d_occ + 1, ncell);
  int nc = 0;
  GCGE_HIP_CHECK(hipMemcpy(&nc, d_occ + ncell, sizeof nc, hipMemcpyDeviceToHost));
  if (d2h) *d2h += (long)sizeof nc;
  GCGE_REQUIRE(nc >= 1 && nc <= nf, "gcge_hip_mg_agg_masked_device: every row lies in a cell");
  int *d_ptr = nullptr, *d_cbox = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d_ptr, ((size_t)nc + 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_cbox, (size_t)nc * sizeof(int)));
  hipLaunchKernelGGL(k_mg_masked_agg, dim3(mg_blocks(nf, 256)), dim3(256), 0, mg_stream(), nf, d_box, nx, ny, cx, cy, (const int*)d_occ, d_agg);
  hipLaunchKernelGGL(k_mg_masked_cells, dim3(mg_blocks(ncell, 256)), dim3(256), 0, mg_stream(), nf, d_box, nx, ny, nz, cx, cy, ncell, nc,
                     (const int*)d_occ, (const int*)d_cnt, d_ptr, d_mem, d_cbox);
  GCGE_HIP_CHECK(hipGetLastError());
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  hipFree(d_cnt); hipFree(d_occ);
  *d_ptr_out = d_ptr; *d_cbox_out = d_cbox;
  return nc;
}

// the same for a host box array, everything copied back: agg, mem (nrows ints), ptr (nrows + 1 ints: nc + 1 used), cbox (nrows ints:
// nc used) — tests and tools.  Returns the number of aggregates, -2 for a geometry gcge_mg_aggregate_masked refuses.
extern "C" int gcge_hip_mg_aggregate_masked(const int dims[3], const int* box_of_row, int nrows, int* agg, int* ptr, int* mem, int* cbox, int cdims[3]) {
  if (gcge_hip_init(-1) != 0 || nrows < 1) return -1;
  const long nbox = (long)dims[0] * dims[1] * dims[2];
  if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || nbox > 2147483647L) return -2;
  for (int r = 0; r < nrows; ++r) if (box_of_row[r] < 0 || box_of_row[r] >= nbox || (r > 0 && box_of_row[r] <= box_of_row[r - 1])) return -2;
  int *d_box = nullptr, *d_agg = nullptr, *d_mem = nullptr, *d_ptr = nullptr, *d_cbox = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d_box, (size_t)nrows * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_agg, (size_t)nrows * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_mem, (size_t)nrows * sizeof(int)));
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  GCGE_HIP_CHECK(hipMemcpy(d_box, box_of_row, (size_t)nrows * sizeof(int), hipMemcpyHostToDevice));
  const int nc = gcge_hip_mg_agg_masked_device(dims, d_box, nrows, d_agg, d_mem, &d_ptr, &d_cbox, cdims, nullptr);
  GCGE_HIP_CHECK(hipMemcpy(agg, d_agg, (size_t)nrows * sizeof(int), hipMemcpyDeviceToHost));
  GCGE_HIP_CHECK(hipMemcpy(mem, d_mem, (size_t)nrows * sizeof(int), hipMemcpyDeviceToHost));
  GCGE_HIP_CHECK(hipMemcpy(ptr, d_ptr, ((size_t)nc + 1) * sizeof(int), hipMemcpyDeviceToHost));
  GCGE_HIP_CHECK(hipMemcpy(cbox, d_cbox, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost));
  hipFree(d_box); hipFree(d_agg); hipFree(d_mem); hipFree(d_ptr); hipFree(d_cbox);
  return nc;
}

// Ac = scale P^T A P on the device: A (nf rows) as device CSR, agg / ptr / mem device arrays of nc aggregates.  Fills the device
// CSR of Ac (allocated here; the caller frees it with hipFree) and returns 0, or 1 when a coarse row has more than MG_DCAP distinct
// columns or Ac more than 2^31 - 1 entries (nothing allocated: the caller builds on the host instead).  d2h: bytes copied back.
extern "C" int gcge_hip_mg_galerkin_device(int nf, const int* d_rowptr, const int* d_colidx, const double* d_val, const int* d_agg, int nc,
                                           const int* d_ptr, const int* d_mem, double scale, int** d_rp_out, int** d_ci_out, double** d_va_out,
                                           long* nnz_out, long* d2h) {
  long long* d_cnt = nullptr; int* d_flag = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d_cnt, ((size_t)nc + 1) * sizeof(long long)));
  GCGE_HIP_CHECK(hipMalloc(&d_flag, sizeof(int)));
  GCGE_HIP_CHECK(hipMemsetAsync(d_cnt, 0, sizeof(long long), mg_stream()));
  GCGE_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int), mg_stream()));
  const unsigned grid = (unsigned)(nc < 65536 * 16 ? nc : 65536 * 16);
  if (nc > 0)
    hipLaunchKernelGGL(k_mg_galerkin<false>, dim3(grid), dim3(MG_WAVE), 0, mg_stream(), nc, nf, d_ptr, d_mem, d_rowptr, d_colidx, d_val, d_agg,
                       scale, d_cnt + 1, (const int*)nullptr, (int*)nullptr, (double*)nullptr, d_flag);
  GCGE_HIP_CHECK(hipGetLastError());
  mg_inclusive_sum(d_cnt + 1, nc);
  long long tot = 0; int flag = 0;
  GCGE_HIP_CHECK(hipMemcpy(&tot, d_cnt + nc, sizeof tot, hipMemcpyDeviceToHost));
  GCGE_HIP_CHECK(hipMemcpy(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost));
  if (d2h) *d2h += (long)(sizeof tot + sizeof flag);
  if (flag != 0 || tot > 2147483647LL) { hipFree(d_cnt); hipFree(d_flag); return 1; }
  int* d_rp = nullptr; int* d_ci = nullptr; double* d_va = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d_rp, ((size_t)nc + 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_ci, (size_t)(tot ? tot : 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_va, (size_t)(tot ? tot : 1) * sizeof(double)));
  hipLaunchKernelGGL(k_mg_ll_to_int, dim3(mg_blocks((long)nc + 1, 256)), dim3(256), 0, mg_stream(), (long)nc + 1, (const long long*)d_cnt, d_rp);
  if (nc > 0)
    hipLaunchKernelGGL(k_mg_galerkin<true>, dim3(grid), dim3(MG_WAVE), 0, mg_stream(), nc, nf, d_ptr, d_mem, d_rowptr, d_colidx, d_val, d_agg,
                       scale, (long long*)nullptr, (const int*)d_rp, d_ci, d_va, d_flag);
  GCGE_HIP_CHECK(hipGetLastError());
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  hipFree(d_cnt); hipFree(d_flag);
  *d_rp_out = d_rp; *d_ci_out = d_ci; *d_va_out = d_va; *nnz_out = (long)tot;
  return 0;
}

// The values of Ac = scale P^T A P for a coarse structure that exists (d_rp_c / d_ci_c: nc rows, ascending columns — what
// gcge_hip_mg_galerkin_device made of a matrix of this structure), straight into d_va_c: the doubles gcge_hip_mg_galerkin_device and the
// host's gcge_mg_galerkin give for these values.  Returns 0, or 1 when an entry's coarse column is not in its coarse row (the structure is
// not this matrix's) or a coarse row holds more than MG_DCAP columns: such rows keep what d_va_c held, the others are written.  One word
// comes back.
static int mg_galerkin_values_into(bool slab, int nf, const int* d_rowptr, const int* d_colidx, const double* d_val, const int* d_agg, int nc,
                                   const int* d_ptr, const int* d_mem, double scale, const int* d_rp_c, const int* d_ci_c, double* d_va_c,
                                   int nlo, long* d2h) {
  if (nc <= 0) return 0;
  int* d_flag = (int*)gcge_hip_stage_d(1);              // (a word of the back-end's staging block: nothing else runs between the two calls)
  GCGE_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int), mg_stream()));
  const unsigned grid = (unsigned)(nc < 65536 * 16 ? nc : 65536 * 16);
  if (slab)
    hipLaunchKernelGGL(k_mg_galerkin_values<true>, dim3(grid), dim3(MG_WAVE), 0, mg_stream(), nc, nf, d_ptr, d_mem, d_rowptr, d_colidx, d_val, d_agg, scale,
                       d_rp_c, d_ci_c, d_va_c, d_flag, nc, nlo);
  else
    hipLaunchKernelGGL(k_mg_galerkin_values<false>, dim3(grid), dim3(MG_WAVE), 0, mg_stream(), nc, nf, d_ptr, d_mem, d_rowptr, d_colidx, d_val, d_agg, scale,
                       d_rp_c, d_ci_c, d_va_c, d_flag, nc, 0);
  GCGE_HIP_CHECK(hipGetLastError());
  int flag = 0;
  GCGE_HIP_CHECK(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, mg_stream()));
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  if (d2h) *d2h += (long)sizeof flag;
  return flag != 0;
}
extern "C" int gcge_hip_mg_galerkin_values_into(int nf, const int* d_rowptr, const int* d_colidx, const double* d_val, const int* d_agg, int nc,
                                                const int* d_ptr, const int* d_mem, double scale, const int* d_rp_c, const int* d_ci_c,
                                                double* d_va_c, long* d2h) {
  return mg_galerkin_values_into(false, nf, d_rowptr, d_colidx, d_val, d_agg, nc, d_ptr, d_mem, scale, d_rp_c, d_ci_c, d_va_c, 0, d2h);
}
// ... on one level of a row-slab hierarchy: the nrows_f own rows of the fine slab (d_ptr / d_mem: the members of the nc own coarse rows)
// over its ncols_f LOCAL columns, d_colagg[ncols_f] the local coarse column of each (gcge_mg_slab_colagg), nlo of the coarse slab's halo
// columns below it; the coarse structure is the coarse slab's own, local columns.  Same returns.
extern "C" int gcge_hip_mg_galerkin_values_slab_into(int ncols_f, const int* d_rowptr, const int* d_colidx, const double* d_val, const int* d_colagg,
                                                     int nc, const int* d_ptr, const int* d_mem, double scale, const int* d_rp_c, const int* d_ci_c,
                                                     double* d_va_c, int nlo, long* d2h) {
  return mg_galerkin_values_into(true, ncols_f, d_rowptr, d_colidx, d_val, d_colagg, nc, d_ptr, d_mem, scale, d_rp_c, d_ci_c, d_va_c, nlo, d2h);
}
// ... into d_va_c_out only when the whole product fits the structure: on a return of 1 d_va_c_out is as it was (the values go through
// a block of the pool)
extern "C" int gcge_hip_mg_galerkin_values_device(int nf, const int* d_rowptr, const int* d_colidx, const double* d_val, const int* d_agg, int nc,
                                                  const int* d_ptr, const int* d_mem, double scale, const int* d_rp_c, const int* d_ci_c,
                                                  double* d_va_c_out) {
  if (nc <= 0) return 0;
  int nnz = 0;
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  GCGE_HIP_CHECK(hipMemcpy(&nnz, d_rp_c + nc, sizeof nnz, hipMemcpyDeviceToHost));
  if (nnz <= 0) return 0;
  const size_t bytes = (size_t)nnz * sizeof(double);
  double* tmp = (double*)gcge_hip_pool_alloc(bytes);
  const int rc = gcge_hip_mg_galerkin_values_into(nf, d_rowptr, d_colidx, d_val, d_agg, nc, d_ptr, d_mem, scale, d_rp_c, d_ci_c, tmp, nullptr);
  if (rc == 0) {
    GCGE_HIP_CHECK(hipMemcpyAsync(d_va_c_out, tmp, bytes, hipMemcpyDeviceToDevice, mg_stream()));
    GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  }
  gcge_hip_pool_free(tmp, bytes);
  return rc;
}

// P (rowptr[r] = r, colidx = agg, 1.0) and P^T (the members, 1.0) from device arrays: what gcge_hip_mat_create_rect makes from the
// host arrays of gcge_mg_prolongation.  The arrays are copied; the caller keeps its own.
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_rect_device(int nf, int nc, const int* d_agg, const int* d_ptr, const int* d_mem) {
  if (gcge_hip_init(-1) != 0) return nullptr;
  GCGE_REQUIRE(nf > 0 && nc > 0, "gcge_hip_mat_create_rect_device: a non-empty prolongation");
  GCGE_HIP_MAT* P = (GCGE_HIP_MAT*)calloc(1, sizeof(GCGE_HIP_MAT));
  P->nrows = nf; P->nglobal = nf; P->nnz = nf; P->rect_ncols = nc; P->rect_one_per_row = 1;
  GCGE_HIP_CHECK(hipMalloc(&P->d_rowptr, ((size_t)nf + 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&P->d_colidx, (size_t)nf * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&P->d_val, (size_t)nf * sizeof(double)));
  GCGE_HIP_CHECK(hipMalloc(&P->d_t_rowptr, ((size_t)nc + 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&P->d_t_colidx, (size_t)nf * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&P->d_t_val, (size_t)nf * sizeof(double)));
  GCGE_HIP_CHECK(hipMemcpyAsync(P->d_colidx, d_agg, (size_t)nf * sizeof(int), hipMemcpyDeviceToDevice, mg_stream()));
  GCGE_HIP_CHECK(hipMemcpyAsync(P->d_t_rowptr, d_ptr, ((size_t)nc + 1) * sizeof(int), hipMemcpyDeviceToDevice, mg_stream()));
  GCGE_HIP_CHECK(hipMemcpyAsync(P->d_t_colidx, d_mem, (size_t)nf * sizeof(int), hipMemcpyDeviceToDevice, mg_stream()));
  hipLaunchKernelGGL(k_mg_prolong, dim3(mg_blocks((long)nf + 1, 256)), dim3(256), 0, mg_stream(), (long)nf, P->d_rowptr, P->d_val, P->d_t_val);
  GCGE_HIP_CHECK(hipGetLastError());
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  return P;
}

// members of every aggregate in ascending fine-row order (host; the counting sort of aggregate_members, csrc/host/multigrid.c)
void gcge_hip_mg_members_host(const int* agg, int nf, int nc, std::vector<int>& ptr, std::vector<int>& mem) {
  ptr.assign((size_t)nc + 1, 0); mem.resize(nf > 0 ? (size_t)nf : 1);
  for (int r = 0; r < nf; ++r) ++ptr[(size_t)agg[r] + 1];
  for (int I = 0; I < nc; ++I) ptr[I + 1] += ptr[I];
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (int r = 0; r < nf; ++r) mem[fill[agg[r]]++] = r;
}

// a device CSR of n rows as a host copy (malloc'd arrays: gcge_csr_free)
extern "C" int gcge_hip_mg_download_csr(int nrows, int ncols, long nnz, const int* d_rp, const int* d_ci, const double* d_va, GCGE_CSR* out, long* d2h) {
  memset(out, 0, sizeof *out);
  out->rowptr = (int*)malloc(((size_t)nrows + 1) * sizeof(int));
  out->colidx = (int*)malloc((size_t)(nnz ? nnz : 1) * sizeof(int));
  out->val = (double*)malloc((size_t)(nnz ? nnz : 1) * sizeof(double));
  if (!out->rowptr || !out->colidx || !out->val) { gcge_csr_free(out); return -3; }
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  GCGE_HIP_CHECK(hipMemcpy(out->rowptr, d_rp, ((size_t)nrows + 1) * sizeof(int), hipMemcpyDeviceToHost));
  if (nnz > 0) {
    GCGE_HIP_CHECK(hipMemcpy(out->colidx, d_ci, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost));
    GCGE_HIP_CHECK(hipMemcpy(out->val, d_va, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (d2h) *d2h += (long)(((size_t)nrows + 1) * sizeof(int) + (size_t)nnz * (sizeof(int) + sizeof(double)));
  out->nrows = nrows; out->ncols = ncols; out->row_begin = 0; out->nnz = nnz;
  return 0;
}

extern "C" int gcge_hip_mat_to_csr(const GCGE_HIP_MAT* A, GCGE_CSR* out) {
  if (A == nullptr || out == nullptr) return -1;
  return gcge_hip_mg_download_csr(A->nrows, A->rect_ncols > 0 ? A->rect_ncols : A->nrows, A->nnz, A->d_rowptr, A->d_colidx, A->d_val, out, nullptr);
}
extern "C" int gcge_hip_mat_to_csr_t(const GCGE_HIP_MAT* A, GCGE_CSR* out) {
  if (A == nullptr || out == nullptr || A->rect_ncols <= 0) return -1;
  return gcge_hip_mg_download_csr(A->rect_ncols, A->nrows, A->nnz, A->d_t_rowptr, A->d_t_colidx, A->d_t_val, out, nullptr);
}

// the device product on A's device CSR for a host agg: tests and tools
extern "C" int gcge_hip_mg_galerkin(const GCGE_HIP_MAT* A, const int* agg_host, int nc, double scale, GCGE_CSR* Ac_out) {
  if (A == nullptr || agg_host == nullptr || Ac_out == nullptr || A->rect_ncols > 0 || nc < 1) return -1;
  const int nf = A->nrows;
  for (int r = 0; r < nf; ++r) if (agg_host[r] < 0 || agg_host[r] >= nc) return -2;
  std::vector<int> ptr, mem;
  gcge_hip_mg_members_host(agg_host, nf, nc, ptr, mem);
  int *d_agg = nullptr, *d_ptr = nullptr, *d_mem = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d_agg, (size_t)(nf ? nf : 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_ptr, ptr.size() * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_mem, mem.size() * sizeof(int)));
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  GCGE_HIP_CHECK(hipMemcpy(d_agg, agg_host, (size_t)nf * sizeof(int), hipMemcpyHostToDevice));
  GCGE_HIP_CHECK(hipMemcpy(d_ptr, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice));
  GCGE_HIP_CHECK(hipMemcpy(d_mem, mem.data(), mem.size() * sizeof(int), hipMemcpyHostToDevice));
  int *d_rp = nullptr, *d_ci = nullptr; double* d_va = nullptr; long nnz = 0;
  int rc = gcge_hip_mg_galerkin_device(nf, A->d_rowptr, A->d_colidx, A->d_val, d_agg, nc, d_ptr, d_mem, scale, &d_rp, &d_ci, &d_va, &nnz, nullptr);
  hipFree(d_agg); hipFree(d_ptr); hipFree(d_mem);
  if (rc != 0) { memset(Ac_out, 0, sizeof *Ac_out); return 1; }
  rc = gcge_hip_mg_download_csr(nc, nc, nnz, d_rp, d_ci, d_va, Ac_out, nullptr);
  hipFree(d_rp); hipFree(d_ci); hipFree(d_va);
  return rc;
}

// the values-only product on A's device CSR for a host agg and a host coarse structure (nc rows): va_c goes up as it is, comes back as
// gcge_hip_mg_galerkin_values_device left it, and its return value is returned — tests and tools
extern "C" int gcge_hip_mg_galerkin_values(const GCGE_HIP_MAT* A, const int* agg_host, int nc, double scale, const int* rp_c, const int* ci_c,
                                           double* va_c) {
  if (A == nullptr || agg_host == nullptr || rp_c == nullptr || ci_c == nullptr || va_c == nullptr || A->rect_ncols > 0 || nc < 1) return -1;
  const int nf = A->nrows;
  for (int r = 0; r < nf; ++r) if (agg_host[r] < 0 || agg_host[r] >= nc) return -2;
  if (rp_c[0] != 0) return -2;
  for (int I = 0; I < nc; ++I) if (rp_c[I + 1] < rp_c[I]) return -2;
  const size_t nnz = (size_t)rp_c[nc];
  for (size_t k = 0; k < nnz; ++k) if (ci_c[k] < 0 || ci_c[k] >= nc) return -2;
  std::vector<int> ptr, mem;
  gcge_hip_mg_members_host(agg_host, nf, nc, ptr, mem);
  auto up = [](const void* h, size_t bytes) { void* d = nullptr; GCGE_HIP_CHECK(hipMalloc(&d, bytes ? bytes : 8)); GCGE_HIP_CHECK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); return d; };
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  int* d_agg = (int*)up(agg_host, (size_t)nf * sizeof(int));
  int* d_ptr = (int*)up(ptr.data(), ptr.size() * sizeof(int));
  int* d_mem = (int*)up(mem.data(), (size_t)nf * sizeof(int));
  int* d_rp = (int*)up(rp_c, ((size_t)nc + 1) * sizeof(int));
  int* d_ci = (int*)up(ci_c, nnz * sizeof(int));
  double* d_va = (double*)up(va_c, nnz * sizeof(double));
  const int rc = gcge_hip_mg_galerkin_values_device(nf, A->d_rowptr, A->d_colidx, A->d_val, d_agg, nc, d_ptr, d_mem, scale, d_rp, d_ci, d_va);
  GCGE_HIP_CHECK(hipStreamSynchronize(mg_stream()));
  if (nnz > 0) GCGE_HIP_CHECK(hipMemcpy(va_c, d_va, nnz * sizeof(double), hipMemcpyDeviceToHost));
  hipFree(d_agg); hipFree(d_ptr); hipFree(d_mem); hipFree(d_rp); hipFree(d_ci); hipFree(d_va);
  return rc;
}
