// MIS-2 aggregation of a matrix without a grid on the device: gcge_mg_aggregate_mis2 (csrc/host/multigrid.c; the definition is in
// include/gcge_multigrid.h) on the device-resident CSR of a level, with the same aggregates byte for byte, and their members.
//
// Nothing here depends on scheduling: every value a kernel writes is a function of arrays the kernels before it finished (a maximum,
// a count, a sum of integers, a stable sort), the only atomics add integers into counters, no kernel waits for another workgroup.
//
// Rows of very different length (several hundred entries beside 37 in the SiO2-like matrix) are served by a GROUP of G lanes per
// row, G = 4 .. 64 chosen from the mean row length: consecutive lanes read consecutive entries, the group's lanes run the same
// number of steps, and a row's result is a reduction over the group by shuffles (maxima and an ordered compaction by ballot).
//
//   strength   thr[r], then the strong edges of every row as a CSR of their own (count, sum, ordered fill: columns ascending like
//              the row's), with |a_rc| beside them: the rounds and the joins walk this smaller graph only.
//   roots      rounds driven by the host.  A round takes, for every row, the largest key among the undecided rows of its closed
//              strong neighbourhood, then the same once more (the distance-2 maximum); an undecided row whose own key is that
//              maximum becomes a root; the root flag is pushed two hops the same way and turns undecided rows into non-roots; the
//              number of rows still undecided comes back.  An undecided row with the largest key within two edges has no root of
//              higher priority near it, and every row of higher priority near it is decided: the greedy set, whatever the round.
//              Keys are distinct (the mixer is a bijection) and never 0 for a row index, so the key alone orders the rows and 0
//              stands for "no undecided row".
//   numbering  an inclusive sum over the root flags: the roots in ascending row order.
//   joins      join 1 reads the roots, join 2 reads join 1's array and writes another: a row placed in join 2 attracts nobody.
//   members    a stable radix sort of the rows by aggregate (the members ascending), ptr from the boundaries of the sorted ids.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "gcge_hip.h"
#include "gcge_multigrid.h"
#include "gcge_hip_internal.h"

#define AG_BLOCK 256
#define AG_MAX_ROUNDS 64
typedef unsigned long long ag_u64;

static hipStream_t ag_stream() { return (hipStream_t)gcge_hip_stream(); }
static unsigned ag_blocks(long n) { return (unsigned)((n + AG_BLOCK - 1) / AG_BLOCK); }

// the row and the lane of this thread in a kernel that gives every row a group of G lanes (AG_BLOCK / G rows per block)
template <int G> __device__ inline int ag_row() { return (int)(((long)blockIdx.x * AG_BLOCK + threadIdx.x) / G); }
template <int G> __device__ inline int ag_lane() { return (int)(threadIdx.x % G); }

template <int G> __device__ inline double ag_group_max(double v) {
  for (int o = G / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, G));
  return v;
}
template <int G> __device__ inline ag_u64 ag_group_max(ag_u64 v) {
  for (int o = G / 2; o > 0; o >>= 1) { const ag_u64 w = __shfl_xor(v, o, G); v = w > v ? w : v; }
  return v;
}
// the candidate (w, id) that wins a join: the larger w, then the smaller id (id == INT_MAX: none)
template <int G> __device__ inline void ag_group_best(double& w, int& id) {
  for (int o = G / 2; o > 0; o >>= 1) {
    const double w2 = __shfl_xor(w, o, G); const int id2 = __shfl_xor(id, o, G);
    if (w2 > w || (w2 == w && id2 < id)) { w = w2; id = id2; }
  }
}

// ------------------------------------------------------------------------------------------------------------ strength
template <int G>
__global__ void __launch_bounds__(AG_BLOCK) k_ag_thr(int n, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ va,
                                                      double theta, double* __restrict__ thr) {
  const int r = ag_row<G>(), l = ag_lane<G>();
  if (r >= n) return;
  double mx = 0.0;
  for (int k = rp[r] + l; k < rp[r + 1]; k += G) {
    const int c = ci[k];
    if (c != r && c >= 0 && c < n) mx = fmax(mx, fabs(va[k]));
  }
  mx = ag_group_max<G>(mx);
  if (l == 0) thr[r] = theta * mx;
}

// the strong edges of row r: their number (FILL = false, cnt[r]) or the edges themselves at srp[r], in the row's order
template <int G, bool FILL>
__global__ void __launch_bounds__(AG_BLOCK) k_ag_strong(int n, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ va,
                                                         const double* __restrict__ thr, int* __restrict__ cnt, const int* __restrict__ srp,
                                                         int* __restrict__ sci, double* __restrict__ sw) {
  const int r = ag_row<G>(), l = ag_lane<G>();
  if (r >= n) return;
  const double tr = thr[r];
  const int beg = rp[r], end = rp[r + 1];
  const int shift = (int)((threadIdx.x & 63) / G * G);       // the group's first lane in its wave
  int total = 0;
  for (int k0 = beg; k0 < end; k0 += G) {                    // (the same number of steps for the lanes of a group)
    const int k = k0 + l;
    int c = -1; double w = 0.0; bool s = false;
    if (k < end) {
      c = ci[k]; const double a = va[k]; w = fabs(a);
      if (c != r && c >= 0 && c < n && a != 0.0) { const double tc = thr[c]; s = w >= (tr < tc ? tr : tc); }
    }
    const ag_u64 b = __builtin_amdgcn_ballot_w64(s);
    const ag_u64 gb = G == 64 ? b : (b >> shift) & ((1ull << (G & 63)) - 1ull);
    if (FILL && s) {
      const int q = srp[r] + total + __popcll(gb & ((1ull << l) - 1ull));
      sci[q] = c; sw[q] = w;
    }
    total += __popcll(gb);
  }
  if (!FILL && l == 0) cnt[r] = total;
}

// ------------------------------------------------------------------------------------------------------------ root rounds
enum { AG_UNDECIDED = 0, AG_ROOT = 1, AG_COVERED = 2 };
// out[r] = the largest source value over the closed strong neighbourhood of r.  MODE 0: the key of an undecided row (0 otherwise),
// 1: in[], 2: the root flag
template <int MODE> __device__ inline ag_u64 ag_source(int c, const int* __restrict__ state, const ag_u64* __restrict__ in) {
  if (MODE == 0) return state[c] == AG_UNDECIDED ? (ag_u64)gcge_mg_mis2_key(c) : 0ull;
  if (MODE == 1) return in[c];
  return state[c] == AG_ROOT ? 1ull : 0ull;
}
template <int G, int MODE>
__global__ void __launch_bounds__(AG_BLOCK) k_ag_hop(int n, const int* __restrict__ srp, const int* __restrict__ sci, const int* __restrict__ state,
                                                      const ag_u64* __restrict__ in, ag_u64* __restrict__ out) {
  const int r = ag_row<G>(), l = ag_lane<G>();
  if (r >= n) return;
  ag_u64 v = l == 0 ? ag_source<MODE>(r, state, in) : 0ull;
  for (int k = srp[r] + l; k < srp[r + 1]; k += G) { const ag_u64 w = ag_source<MODE>(sci[k], state, in); v = w > v ? w : v; }
  v = ag_group_max<G>(v);
  if (l == 0) out[r] = v;
}
__global__ void __launch_bounds__(AG_BLOCK) k_ag_roots(int n, const ag_u64* __restrict__ m2, int* __restrict__ state) {
  const int r = blockIdx.x * AG_BLOCK + threadIdx.x;
  if (r < n && state[r] == AG_UNDECIDED && m2[r] == (ag_u64)gcge_mg_mis2_key(r)) state[r] = AG_ROOT;
}
// undecided rows within two edges of a root are none; *undecided += the rows left (one add per block)
__global__ void __launch_bounds__(AG_BLOCK) k_ag_cover(int n, const ag_u64* __restrict__ f2, int* __restrict__ state, int* __restrict__ undecided) {
  const int r = blockIdx.x * AG_BLOCK + threadIdx.x;
  int left = 0;
  if (r < n && state[r] == AG_UNDECIDED) {
    if (f2[r] != 0ull) state[r] = AG_COVERED; else left = 1;
  }
  const int c = __syncthreads_count(left);
  if (threadIdx.x == 0 && c > 0) atomicAdd(undecided, c);
}

// ------------------------------------------------------------------------------------------------------------ numbering, joins, members
__global__ void __launch_bounds__(AG_BLOCK) k_ag_root_flags(int n, const int* __restrict__ state, int* __restrict__ num) {
  const int r = blockIdx.x * AG_BLOCK + threadIdx.x;
  if (r < n) num[r] = state[r] == AG_ROOT;
}
// (after the sum: a root's aggregate is num[r] - 1)
template <int G>
__global__ void __launch_bounds__(AG_BLOCK) k_ag_join1(int n, const int* __restrict__ srp, const int* __restrict__ sci, const double* __restrict__ sw,
                                                        const int* __restrict__ state, const int* __restrict__ num, int* __restrict__ agg1) {
  const int r = ag_row<G>(), l = ag_lane<G>();
  if (r >= n) return;
  if (state[r] == AG_ROOT) { if (l == 0) agg1[r] = num[r] - 1; return; }
  double bw = -1.0; int bc = INT_MAX;
  for (int k = srp[r] + l; k < srp[r + 1]; k += G) {
    const int c = sci[k]; const double w = sw[k];
    if (state[c] == AG_ROOT && (w > bw || (w == bw && c < bc))) { bw = w; bc = c; }
  }
  ag_group_best<G>(bw, bc);
  if (l == 0) agg1[r] = bc != INT_MAX ? num[bc] - 1 : -1;
}
// a row join 2 leaves free cannot happen on a symmetric matrix: it is counted (the caller then gives the level to the host
// routine) and put into aggregate 0, so that the array never holds an index out of range
template <int G>
__global__ void __launch_bounds__(AG_BLOCK) k_ag_join2(int n, const int* __restrict__ srp, const int* __restrict__ sci, const double* __restrict__ sw,
                                                        const int* __restrict__ agg1, int* __restrict__ agg, int* __restrict__ leftover) {
  const int r = ag_row<G>(), l = ag_lane<G>();
  int left = 0;
  if (r < n) {
    const int a = agg1[r];
    if (a >= 0) { if (l == 0) agg[r] = a; }
    else {
      double bw = -1.0; int ba = INT_MAX;
      for (int k = srp[r] + l; k < srp[r + 1]; k += G) {
        const int ac = agg1[sci[k]]; const double w = sw[k];
        if (ac >= 0 && (w > bw || (w == bw && ac < ba))) { bw = w; ba = ac; }
      }
      ag_group_best<G>(bw, ba);
      if (l == 0) { agg[r] = ba != INT_MAX ? ba : 0; left = ba == INT_MAX; }
    }
  }
  const int c = __syncthreads_count(left);
  if (threadIdx.x == 0 && c > 0) atomicAdd(leftover, c);
}
__global__ void __launch_bounds__(AG_BLOCK) k_ag_iota(int n, int* __restrict__ v) {
  const int r = blockIdx.x * AG_BLOCK + threadIdx.x;
  if (r < n) v[r] = r;
}
// ptr from the sorted aggregate ids (every aggregate holds its root: none is empty)
__global__ void __launch_bounds__(AG_BLOCK) k_ag_ptr(int n, int nc, const int* __restrict__ sorted, int* __restrict__ ptr) {
  const int q = blockIdx.x * AG_BLOCK + threadIdx.x;
  if (q >= n) return;
  if (q == 0) ptr[nc] = n;
  if (q == 0 || sorted[q] != sorted[q - 1]) ptr[sorted[q]] = q;
}

// ------------------------------------------------------------------------------------------------------------ host side
static void ag_inclusive_sum(int* d, int n) {
  size_t bytes = 0;
  GCGE_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, bytes, d, d, n, ag_stream()));
  void* tmp = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&tmp, bytes ? bytes : 8));
  GCGE_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(tmp, bytes, d, d, n, ag_stream()));
  GCGE_HIP_CHECK(hipStreamSynchronize(ag_stream()));
  GCGE_HIP_CHECK(hipFree(tmp));
}
// lanes per row: the smallest of 4 .. 64 that holds a row of mean length
static int ag_group(long nnz, int n) {
  const long mean = n > 0 ? (nnz + n - 1) / n : 0;
  int g = 4;
  while (g < 64 && g < mean) g *= 2;
  return g;
}
// kern<G, ...>(args) over n rows with G lanes each
#define AG_LAUNCH(G_, n_, KERN, ...)                                                                                                   \
  do {                                                                                                                                  \
    switch (G_) {                                                                                                                       \
      case 4:  hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN(4)),  dim3(ag_blocks((long)(n_) * 4)),  dim3(AG_BLOCK), 0, ag_stream(), __VA_ARGS__); break; \
      case 8:  hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN(8)),  dim3(ag_blocks((long)(n_) * 8)),  dim3(AG_BLOCK), 0, ag_stream(), __VA_ARGS__); break; \
      case 16: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN(16)), dim3(ag_blocks((long)(n_) * 16)), dim3(AG_BLOCK), 0, ag_stream(), __VA_ARGS__); break; \
      case 32: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN(32)), dim3(ag_blocks((long)(n_) * 32)), dim3(AG_BLOCK), 0, ag_stream(), __VA_ARGS__); break; \
      default: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN(64)), dim3(ag_blocks((long)(n_) * 64)), dim3(AG_BLOCK), 0, ag_stream(), __VA_ARGS__); break; \
    }                                                                                                                                   \
    GCGE_HIP_CHECK(hipGetLastError());                                                                                                  \
  } while (0)
#define AG_K_THR(G) k_ag_thr<G>
#define AG_K_COUNT(G) k_ag_strong<G, false>
#define AG_K_FILL(G) k_ag_strong<G, true>
#define AG_K_HOP0(G) k_ag_hop<G, 0>
#define AG_K_HOP1(G) k_ag_hop<G, 1>
#define AG_K_HOP2(G) k_ag_hop<G, 2>
#define AG_K_JOIN1(G) k_ag_join1<G>
#define AG_K_JOIN2(G) k_ag_join2<G>

static int g_ag_round_cap = AG_MAX_ROUNDS, g_ag_rounds = 0;
extern "C" void gcge_hip_mg_graph_round_cap(int cap) { g_ag_round_cap = cap < 1 ? 1 : cap > AG_MAX_ROUNDS ? AG_MAX_ROUNDS : cap; }
extern "C" int gcge_hip_mg_graph_rounds(void) { return g_ag_rounds; }

// The aggregates of the n-row device CSR (local columns; a column outside [0, n) is no coupling): d_agg / d_mem (n ints, the caller's)
// are filled, *d_ptr_out (nc + 1 ints) is allocated here (hipFree) — agg / ptr / mem as gcge_hip_mg_agg_grid_device delivers them.
// Returns the number of aggregates, or -1 with nothing allocated when the rounds reached their cap (or a row was left free: an
// unsymmetric matrix): the caller aggregates the level on the host.  One int per round and two more come back.
extern "C" int gcge_hip_mg_agg_graph_device(int n, const int* d_rowptr, const int* d_colidx, const double* d_val, double theta, int* d_agg,
                                            int* d_mem, int** d_ptr_out, long* d2h) {
  GCGE_REQUIRE(n >= 1 && d_ptr_out != nullptr, "gcge_hip_mg_agg_graph_device: a matrix with rows");
  *d_ptr_out = nullptr; g_ag_rounds = 0;
  int nnz = 0;
  GCGE_HIP_CHECK(hipStreamSynchronize(ag_stream()));
  GCGE_HIP_CHECK(hipMemcpy(&nnz, d_rowptr + n, sizeof nnz, hipMemcpyDeviceToHost));
  if (d2h) *d2h += (long)sizeof nnz;
  const int G = ag_group(nnz, n);
  double *d_thr = nullptr, *d_sw = nullptr; int *d_srp = nullptr, *d_sci = nullptr, *d_state = nullptr, *d_num = nullptr, *d_agg1 = nullptr, *d_cnt = nullptr;
  ag_u64 *d_m1 = nullptr, *d_m2 = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d_thr, (size_t)n * sizeof(double)));
  GCGE_HIP_CHECK(hipMalloc(&d_srp, ((size_t)n + 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_state, (size_t)n * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_num, (size_t)n * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_agg1, (size_t)n * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_m1, (size_t)n * sizeof(ag_u64)));
  GCGE_HIP_CHECK(hipMalloc(&d_m2, (size_t)n * sizeof(ag_u64)));
  GCGE_HIP_CHECK(hipMalloc(&d_cnt, 2 * sizeof(int)));
  auto release = [&] {
    hipFree(d_thr); hipFree(d_sw); hipFree(d_srp); hipFree(d_sci); hipFree(d_state); hipFree(d_num); hipFree(d_agg1); hipFree(d_cnt);
    hipFree(d_m1); hipFree(d_m2);
  };
  // strength: thresholds, then the strong edges as a CSR of their own
  AG_LAUNCH(G, n, AG_K_THR, n, d_rowptr, d_colidx, d_val, theta, d_thr);
  GCGE_HIP_CHECK(hipMemsetAsync(d_srp, 0, sizeof(int), ag_stream()));
  AG_LAUNCH(G, n, AG_K_COUNT, n, d_rowptr, d_colidx, d_val, (const double*)d_thr, d_srp + 1, (const int*)nullptr, (int*)nullptr, (double*)nullptr);
  ag_inclusive_sum(d_srp + 1, n);
  int snnz = 0;
  GCGE_HIP_CHECK(hipMemcpy(&snnz, d_srp + n, sizeof snnz, hipMemcpyDeviceToHost));
  if (d2h) *d2h += (long)sizeof snnz;
  GCGE_REQUIRE(snnz >= 0 && snnz <= nnz, "gcge_hip_mg_agg_graph_device: the strong edges are entries of the matrix");
  GCGE_HIP_CHECK(hipMalloc(&d_sci, (size_t)(snnz ? snnz : 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_sw, (size_t)(snnz ? snnz : 1) * sizeof(double)));
  AG_LAUNCH(G, n, AG_K_FILL, n, d_rowptr, d_colidx, d_val, (const double*)d_thr, (int*)nullptr, (const int*)d_srp, d_sci, d_sw);
  const int GS = ag_group(snnz, n);
  // roots
  GCGE_HIP_CHECK(hipMemsetAsync(d_state, 0, (size_t)n * sizeof(int), ag_stream()));
  int undecided = n, rounds = 0;
  while (undecided > 0 && rounds < g_ag_round_cap) {
    GCGE_HIP_CHECK(hipMemsetAsync(d_cnt, 0, sizeof(int), ag_stream()));
    AG_LAUNCH(GS, n, AG_K_HOP0, n, (const int*)d_srp, (const int*)d_sci, (const int*)d_state, (const ag_u64*)nullptr, d_m1);
    AG_LAUNCH(GS, n, AG_K_HOP1, n, (const int*)d_srp, (const int*)d_sci, (const int*)d_state, (const ag_u64*)d_m1, d_m2);
    hipLaunchKernelGGL(k_ag_roots, dim3(ag_blocks(n)), dim3(AG_BLOCK), 0, ag_stream(), n, (const ag_u64*)d_m2, d_state);
    AG_LAUNCH(GS, n, AG_K_HOP2, n, (const int*)d_srp, (const int*)d_sci, (const int*)d_state, (const ag_u64*)nullptr, d_m1);
    AG_LAUNCH(GS, n, AG_K_HOP1, n, (const int*)d_srp, (const int*)d_sci, (const int*)d_state, (const ag_u64*)d_m1, d_m2);
    hipLaunchKernelGGL(k_ag_cover, dim3(ag_blocks(n)), dim3(AG_BLOCK), 0, ag_stream(), n, (const ag_u64*)d_m2, d_state, d_cnt);
    GCGE_HIP_CHECK(hipGetLastError());
    GCGE_HIP_CHECK(hipMemcpyAsync(&undecided, d_cnt, sizeof undecided, hipMemcpyDeviceToHost, ag_stream()));
    GCGE_HIP_CHECK(hipStreamSynchronize(ag_stream()));
    if (d2h) *d2h += (long)sizeof undecided;
    ++rounds;
  }
  g_ag_rounds = rounds;
  if (undecided > 0) { release(); return -1; }
  // numbering and joins
  hipLaunchKernelGGL(k_ag_root_flags, dim3(ag_blocks(n)), dim3(AG_BLOCK), 0, ag_stream(), n, (const int*)d_state, d_num);
  GCGE_HIP_CHECK(hipGetLastError());
  ag_inclusive_sum(d_num, n);
  GCGE_HIP_CHECK(hipMemsetAsync(d_cnt + 1, 0, sizeof(int), ag_stream()));
  AG_LAUNCH(GS, n, AG_K_JOIN1, n, (const int*)d_srp, (const int*)d_sci, (const double*)d_sw, (const int*)d_state, (const int*)d_num, d_agg1);
  AG_LAUNCH(GS, n, AG_K_JOIN2, n, (const int*)d_srp, (const int*)d_sci, (const double*)d_sw, (const int*)d_agg1, d_agg, d_cnt + 1);
  int back[2] = {0, 0};      // the number of roots, the rows left free
  GCGE_HIP_CHECK(hipMemcpyAsync(&back[0], d_num + (n - 1), sizeof(int), hipMemcpyDeviceToHost, ag_stream()));
  GCGE_HIP_CHECK(hipMemcpyAsync(&back[1], d_cnt + 1, sizeof(int), hipMemcpyDeviceToHost, ag_stream()));
  GCGE_HIP_CHECK(hipStreamSynchronize(ag_stream()));
  if (d2h) *d2h += (long)sizeof back;
  const int nc = back[0];
  if (back[1] != 0 || nc < 1 || nc > n) { release(); return -1; }
  // members: the rows sorted by aggregate (stable: ascending inside every aggregate)
  int *d_ptr = nullptr, *d_sorted = d_agg1, *d_rows = d_num;       // (both arrays are free again)
  GCGE_HIP_CHECK(hipMalloc(&d_ptr, ((size_t)nc + 1) * sizeof(int)));
  hipLaunchKernelGGL(k_ag_iota, dim3(ag_blocks(n)), dim3(AG_BLOCK), 0, ag_stream(), n, d_rows);
  int end_bit = 1;
  while (end_bit < 31 && (1L << end_bit) < (long)nc) ++end_bit;
  size_t bytes = 0;
  GCGE_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const int*)d_agg, d_sorted, (const int*)d_rows, d_mem, n, 0, end_bit, ag_stream()));
  void* tmp = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&tmp, bytes ? bytes : 8));
  GCGE_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, (const int*)d_agg, d_sorted, (const int*)d_rows, d_mem, n, 0, end_bit, ag_stream()));
  hipLaunchKernelGGL(k_ag_ptr, dim3(ag_blocks(n)), dim3(AG_BLOCK), 0, ag_stream(), n, nc, (const int*)d_sorted, d_ptr);
  GCGE_HIP_CHECK(hipGetLastError());
  GCGE_HIP_CHECK(hipStreamSynchronize(ag_stream()));
  hipFree(tmp);
  release();
  *d_ptr_out = d_ptr;
  return nc;
}

// the device routine for host arrays (n rows, ascending columns), everything copied back: agg, mem (n ints), ptr (n + 1 ints: nc + 1
// used) — tests and tools.  Returns the number of aggregates, -1 when the device routine gave the matrix up, -2 bad arguments.
extern "C" int gcge_hip_mg_aggregate_graph_csr(int n, const int* rowptr, const int* colidx, const double* val, double theta, int* agg, int* ptr, int* mem) {
  if (gcge_hip_init(-1) != 0) return -2;
  if (n < 1 || rowptr == nullptr || rowptr[0] != 0 || rowptr[n] < 0) return -2;
  for (int r = 0; r < n; ++r) if (rowptr[r + 1] < rowptr[r]) return -2;
  const size_t nnz = (size_t)rowptr[n];
  int *d_rp = nullptr, *d_ci = nullptr; double* d_va = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d_rp, ((size_t)n + 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_ci, (nnz ? nnz : 1) * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_va, (nnz ? nnz : 1) * sizeof(double)));
  GCGE_HIP_CHECK(hipMemcpy(d_rp, rowptr, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
  if (nnz > 0) {
    GCGE_HIP_CHECK(hipMemcpy(d_ci, colidx, nnz * sizeof(int), hipMemcpyHostToDevice));
    GCGE_HIP_CHECK(hipMemcpy(d_va, val, nnz * sizeof(double), hipMemcpyHostToDevice));
  }
  GCGE_HIP_MAT_ tmp; memset(&tmp, 0, sizeof tmp);
  tmp.nrows = n; tmp.nglobal = n; tmp.nnz = (long)nnz; tmp.d_rowptr = d_rp; tmp.d_colidx = d_ci; tmp.d_val = d_va;
  const int nc = gcge_hip_mg_aggregate_graph(&tmp, theta, agg, ptr, mem);
  hipFree(d_rp); hipFree(d_ci); hipFree(d_va);
  return nc;
}
extern "C" int gcge_hip_mg_aggregate_graph(const GCGE_HIP_MAT* A, double theta, int* agg, int* ptr, int* mem) {
  if (A == nullptr || A->rect_ncols > 0 || A->nghost > 0 || A->nrows < 1 || agg == nullptr || ptr == nullptr || mem == nullptr) return -2;
  const int n = A->nrows;
  int *d_agg = nullptr, *d_mem = nullptr, *d_ptr = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d_agg, (size_t)n * sizeof(int)));
  GCGE_HIP_CHECK(hipMalloc(&d_mem, (size_t)n * sizeof(int)));
  const int nc = gcge_hip_mg_agg_graph_device(n, A->d_rowptr, A->d_colidx, A->d_val, theta, d_agg, d_mem, &d_ptr, nullptr);
  if (nc >= 1) {
    GCGE_HIP_CHECK(hipMemcpy(agg, d_agg, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    GCGE_HIP_CHECK(hipMemcpy(mem, d_mem, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    GCGE_HIP_CHECK(hipMemcpy(ptr, d_ptr, ((size_t)nc + 1) * sizeof(int), hipMemcpyDeviceToHost));
  }
  hipFree(d_agg); hipFree(d_mem); hipFree(d_ptr);
  return nc;
}
