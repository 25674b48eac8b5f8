// The three vector sweeps of one step of GCGE_PCGSolve (csrc/host/block_fpcg.c: flexible block CG preconditioned by a BlockAMG
// V-cycle) and the shift of GCGE_PCGSolveDeflated's operator, each ONE pass over its blocks where the operator table's slots take
// several:
//
//   pcg_step       x += alpha p ; r -= alpha w ; rr_j = |r_j|^2      4 reads + 2 writes       slots: 2 Axpby per column + 'D' product  4 + 2 + 2
//   pcg_dots       zr_j = z_j . r_j ; zw_j = z_j . w_j               3 reads                  slots: two 'D' products                  4
//   pcg_direction  p = z + beta p  (or p = z)                        2 reads + 1 write        slots: 1 Axpby per column                the same
//                                                                                             streams, but one launch per COLUMN
//   pcg_shift      w -= shift q ; pw_j = p_j . w_j  (q = B p, or p itself)    3 reads + 1 write        slots: 1 Axpby per column + 'D' product  3 + 1 + 2
//                                                                         (q == p: 2 + 1)
// in block streams of the window's width.  Per-column scalars (alpha, beta) and flags come from the host; a column without a flag
// keeps the bits of everything the sweep writes (a select, not alpha = 0: -0.0 and non-finite neighbours stay what they were).
//
// Modelled on cg_update_all / cg_update_r of block_pcg.hip: 16-byte lanes (v2d, one column pair per thread) with non-temporal loads
// and stores when the width, the column origins and the leading dimensions are even (cg_vec_ok), a scalar-lane kernel (4 row lanes x
// 64 columns) otherwise; every workgroup leaves its partial sums in gcge_hip_partial_ws and reduce_partials adds them in a fixed
// order: the same bits on every run.  The grid is cg_grid's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gcge_hip.h"
#include "gcge_hip_internal.h"

namespace gcge {

typedef double v2d __attribute__((ext_vector_type(2)));

// the rows [row0, rend) of workgroup blockIdx.x, walked rpb = 256 / tpr at a time in groups of UNR
struct PcgRows { long first, end, step; };
__device__ __forceinline__ PcgRows pcg_rows(long nrows, int tpr, int unr) {
  const int rpb = 256 / tpr, ty = threadIdx.x / tpr;
  const long group = (long)rpb * unr;
  const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + group - 1) / group * group;
  return {(long)blockIdx.x * slab + ty, min(nrows, ((long)blockIdx.x + 1) * slab), (long)rpb};
}

// ---- pcg_step ------------------------------------------------------------------------------------------------------------------
template <int UNR>
__global__ __launch_bounds__(256) void pcg_step_v2(long nrows, const double* __restrict__ p, long ldp, const double* __restrict__ w, long ldw,
    double* __restrict__ x, long ldx, double* __restrict__ r, long ldr, int m, const double* __restrict__ alpha, const int* __restrict__ flag,
    double* __restrict__ partial, int tpr) {
  __shared__ double red[256][2];
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  double s0 = 0.0, s1 = 0.0;
  const bool mine = j < m;
  const int f0 = mine ? flag[j] : 0, f1 = mine ? flag[j + 1] : 0;
  if (mine && (f0 | f1)) {
    const double a0 = f0 ? alpha[j] : 0.0, a1 = f1 ? alpha[j + 1] : 0.0;
    const PcgRows q = pcg_rows(nrows, tpr, UNR);
    auto one = [&](long rr, v2d pv, v2d wv, v2d xv, v2d rv) {
      const v2d xn = {f0 ? fma(a0, pv.x, xv.x) : xv.x, f1 ? fma(a1, pv.y, xv.y) : xv.y};
      const v2d rn = {f0 ? fma(-a0, wv.x, rv.x) : rv.x, f1 ? fma(-a1, wv.y, rv.y) : rv.y};
      __builtin_nontemporal_store(xn, reinterpret_cast<v2d*>(x + rr * ldx + j));
      __builtin_nontemporal_store(rn, reinterpret_cast<v2d*>(r + rr * ldr + j));
      if (f0) s0 = fma(rn.x, rn.x, s0);
      if (f1) s1 = fma(rn.y, rn.y, s1);
    };
    long row = q.first;
    for (; row + (UNR - 1) * q.step < q.end; row += q.step * UNR) {
      v2d pv[UNR], wv[UNR], xv[UNR], rv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const long rr = row + u * q.step;
        pv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p + rr * ldp + j));
        wv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(w + rr * ldw + j));
        xv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(x + rr * ldx + j));
        rv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(r + rr * ldr + j));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(row + u * q.step, pv[u], wv[u], xv[u], rv[u]);
    }
    for (; row < q.end; row += q.step)
      one(row, *reinterpret_cast<const v2d*>(p + row * ldp + j), *reinterpret_cast<const v2d*>(w + row * ldw + j),
          *reinterpret_cast<const v2d*>(x + row * ldx + j), *reinterpret_cast<const v2d*>(r + row * ldr + j));
  }
  red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1;
  __syncthreads();
  if (ty == 0 && mine) {
    for (int k = 1; k < rpb; ++k) { s0 += red[k * tpr + tx][0]; s1 += red[k * tpr + tx][1]; }
    partial[(long)blockIdx.x * m + j] = s0;
    partial[(long)blockIdx.x * m + j + 1] = s1;
  }
}

// any width, origin and leading dimension: 4 row lanes x 64 columns, the columns in chunks of 64
__global__ __launch_bounds__(256) void pcg_step_s(long nrows, const double* __restrict__ p, long ldp, const double* __restrict__ w, long ldw,
    double* __restrict__ x, long ldx, double* __restrict__ r, long ldr, int m, const double* __restrict__ alpha, const int* __restrict__ flag,
    double* __restrict__ partial, long rows_per_block) {
  __shared__ double red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(nrows, r0 + rows_per_block);
  for (int c0 = 0; c0 < m; c0 += 64) {
    const int j = c0 + tx;
    double s = 0.0;
    if (j < m && flag[j]) {
      const double a = alpha[j];
      for (long row = r0 + ty; row < r1; row += 4) {
        x[row * ldx + j] = fma(a, p[row * ldp + j], x[row * ldx + j]);
        const double rn = fma(-a, w[row * ldw + j], r[row * ldr + j]);
        r[row * ldr + j] = rn;
        s = fma(rn, rn, s);
      }
    }
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && j < m) partial[(long)blockIdx.x * m + j] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
    __syncthreads();
  }
}

// ---- pcg_dots: partial[b * 2m + j] = sum z r, partial[b * 2m + m + j] = sum z w ------------------------------------------------------
template <int UNR>
__global__ __launch_bounds__(256) void pcg_dots_v2(long nrows, const double* __restrict__ z, long ldz, const double* __restrict__ r, long ldr,
    const double* __restrict__ w, long ldw, int m, double* __restrict__ partial, int tpr) {
  __shared__ double red[256][4];
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
  const bool mine = j < m;
  if (mine) {
    const PcgRows q = pcg_rows(nrows, tpr, UNR);
    auto one = [&](v2d zv, v2d rv, v2d wv) {
      s0 = fma(zv.x, rv.x, s0); s1 = fma(zv.y, rv.y, s1);
      t0 = fma(zv.x, wv.x, t0); t1 = fma(zv.y, wv.y, t1);
    };
    long row = q.first;
    for (; row + (UNR - 1) * q.step < q.end; row += q.step * UNR) {
      v2d zv[UNR], rv[UNR], wv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const long rr = row + u * q.step;
        zv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(z + rr * ldz + j));
        rv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(r + rr * ldr + j));
        wv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(w + rr * ldw + j));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(zv[u], rv[u], wv[u]);
    }
    for (; row < q.end; row += q.step)
      one(*reinterpret_cast<const v2d*>(z + row * ldz + j), *reinterpret_cast<const v2d*>(r + row * ldr + j),
          *reinterpret_cast<const v2d*>(w + row * ldw + j));
  }
  red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1; red[threadIdx.x][2] = t0; red[threadIdx.x][3] = t1;
  __syncthreads();
  if (ty == 0 && mine) {
    for (int k = 1; k < rpb; ++k) {
      s0 += red[k * tpr + tx][0]; s1 += red[k * tpr + tx][1]; t0 += red[k * tpr + tx][2]; t1 += red[k * tpr + tx][3];
    }
    double* out = partial + (long)blockIdx.x * 2 * m;
    out[j] = s0; out[j + 1] = s1; out[m + j] = t0; out[m + j + 1] = t1;
  }
}

__global__ __launch_bounds__(256) void pcg_dots_s(long nrows, const double* __restrict__ z, long ldz, const double* __restrict__ r, long ldr,
    const double* __restrict__ w, long ldw, int m, double* __restrict__ partial, long rows_per_block) {
  __shared__ double red[2][4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(nrows, r0 + rows_per_block);
  for (int c0 = 0; c0 < m; c0 += 64) {
    const int j = c0 + tx;
    double s = 0.0, t = 0.0;
    if (j < m)
      for (long row = r0 + ty; row < r1; row += 4) {
        const double zv = z[row * ldz + j];
        s = fma(zv, r[row * ldr + j], s);
        t = fma(zv, w[row * ldw + j], t);
      }
    red[0][ty][tx] = s; red[1][ty][tx] = t;
    __syncthreads();
    if (ty == 0 && j < m) {
      partial[(long)blockIdx.x * 2 * m + j] = (red[0][0][tx] + red[0][1][tx]) + (red[0][2][tx] + red[0][3][tx]);
      partial[(long)blockIdx.x * 2 * m + m + j] = (red[1][0][tx] + red[1][1][tx]) + (red[1][2][tx] + red[1][3][tx]);
    }
    __syncthreads();
  }
}

// ---- pcg_direction: flag 1: p = z + beta p, flag 2: p = z, flag 0: p keeps its bits --------------------------------------------------
template <int UNR>
__global__ __launch_bounds__(256) void pcg_direction_v2(long nrows, const double* __restrict__ z, long ldz, double* __restrict__ p, long ldp,
    int m, const double* __restrict__ beta, const int* __restrict__ flag, int tpr) {
  const int tx = threadIdx.x % tpr;
  const int j = 2 * tx;
  if (j >= m) return;
  const int f0 = flag[j], f1 = flag[j + 1];
  if (!(f0 | f1)) return;
  const double b0 = f0 == 1 ? beta[j] : 0.0, b1 = f1 == 1 ? beta[j + 1] : 0.0;
  const PcgRows q = pcg_rows(nrows, tpr, UNR);
  auto one = [&](long rr, v2d zv, v2d pv) {
    const v2d pn = {f0 == 1 ? fma(b0, pv.x, zv.x) : f0 ? zv.x : pv.x, f1 == 1 ? fma(b1, pv.y, zv.y) : f1 ? zv.y : pv.y};
    __builtin_nontemporal_store(pn, reinterpret_cast<v2d*>(p + rr * ldp + j));
  };
  long row = q.first;
  for (; row + (UNR - 1) * q.step < q.end; row += q.step * UNR) {
    v2d zv[UNR], pv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long rr = row + u * q.step;
      zv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(z + rr * ldz + j));
      pv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p + rr * ldp + j));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < UNR; ++u) one(row + u * q.step, zv[u], pv[u]);
  }
  for (; row < q.end; row += q.step)
    one(row, *reinterpret_cast<const v2d*>(z + row * ldz + j), *reinterpret_cast<const v2d*>(p + row * ldp + j));
}

__global__ __launch_bounds__(256) void pcg_direction_s(long nrows, const double* __restrict__ z, long ldz, double* __restrict__ p, long ldp,
    int m, const double* __restrict__ beta, const int* __restrict__ flag, long rows_per_block) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(nrows, r0 + rows_per_block);
  for (int j = tx; j < m; j += 64) {
    const int f = flag[j];
    if (f == 0) continue;
    const double b = beta[j];
    for (long row = r0 + ty; row < r1; row += 4)
      p[row * ldp + j] = f == 1 ? fma(b, p[row * ldp + j], z[row * ldz + j]) : z[row * ldz + j];
  }
}

// ---- pcg_shift: w -= shift q ; pw_j = sum p w_new, flagged columns only; QP: q is p (the row is read once) ---------------------------
template <int UNR, bool QP>
__global__ __launch_bounds__(256) void pcg_shift_v2(long nrows, const double* __restrict__ p, long ldp, const double* __restrict__ q, long ldq,
    double* __restrict__ w, long ldw, int m, const double* __restrict__ shift, const int* __restrict__ flag, double* __restrict__ partial,
    int tpr) {
  __shared__ double red[256][2];
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  double s0 = 0.0, s1 = 0.0;
  const bool mine = j < m;
  const int f0 = mine ? flag[j] : 0, f1 = mine ? flag[j + 1] : 0;
  if (mine && (f0 | f1)) {
    const double a0 = f0 ? shift[j] : 0.0, a1 = f1 ? shift[j + 1] : 0.0;
    const PcgRows rows = pcg_rows(nrows, tpr, UNR);
    auto one = [&](long rr, v2d pv, v2d qv, v2d wv) {
      const v2d wn = {f0 ? fma(-a0, qv.x, wv.x) : wv.x, f1 ? fma(-a1, qv.y, wv.y) : wv.y};
      __builtin_nontemporal_store(wn, reinterpret_cast<v2d*>(w + rr * ldw + j));
      if (f0) s0 = fma(pv.x, wn.x, s0);
      if (f1) s1 = fma(pv.y, wn.y, s1);
    };
    long row = rows.first;
    for (; row + (UNR - 1) * rows.step < rows.end; row += rows.step * UNR) {
      v2d pv[UNR], qv[UNR], wv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const long rr = row + u * rows.step;
        pv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p + rr * ldp + j));
        qv[u] = QP ? pv[u] : __builtin_nontemporal_load(reinterpret_cast<const v2d*>(q + rr * ldq + j));
        wv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(w + rr * ldw + j));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(row + u * rows.step, pv[u], qv[u], wv[u]);
    }
    for (; row < rows.end; row += rows.step) {
      const v2d pv = *reinterpret_cast<const v2d*>(p + row * ldp + j);
      one(row, pv, QP ? pv : *reinterpret_cast<const v2d*>(q + row * ldq + j), *reinterpret_cast<const v2d*>(w + row * ldw + j));
    }
  }
  red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1;
  __syncthreads();
  if (ty == 0 && mine) {
    for (int k = 1; k < rpb; ++k) { s0 += red[k * tpr + tx][0]; s1 += red[k * tpr + tx][1]; }
    partial[(long)blockIdx.x * m + j] = s0;
    partial[(long)blockIdx.x * m + j + 1] = s1;
  }
}

template <bool QP>
__global__ __launch_bounds__(256) void pcg_shift_s(long nrows, const double* __restrict__ p, long ldp, const double* __restrict__ q, long ldq,
    double* __restrict__ w, long ldw, int m, const double* __restrict__ shift, const int* __restrict__ flag, double* __restrict__ partial,
    long rows_per_block) {
  __shared__ double red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(nrows, r0 + rows_per_block);
  for (int c0 = 0; c0 < m; c0 += 64) {
    const int j = c0 + tx;
    double s = 0.0;
    if (j < m && flag[j]) {
      const double a = shift[j];
      for (long row = r0 + ty; row < r1; row += 4) {
        const double pv = p[row * ldp + j];
        const double wn = fma(-a, QP ? pv : q[row * ldq + j], w[row * ldw + j]);
        w[row * ldw + j] = wn;
        s = fma(pv, wn, s);
      }
    }
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && j < m) partial[(long)blockIdx.x * m + j] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
    __syncthreads();
  }
}
}  // namespace gcge

using namespace gcge;

// the scalars of one call on the device and in pinned memory: [coefficients (m doubles) | flags (m ints)], grown on demand
static double *g_d_sc = nullptr, *g_h_sc = nullptr; static int g_sc_cap = 0;
static void pcg_scalars(int m, hipStream_t st) {
  if (m > g_sc_cap) {
    if (g_d_sc) { GCGE_HIP_CHECK(hipStreamSynchronize(st)); GCGE_HIP_CHECK(hipFree(g_d_sc)); GCGE_HIP_CHECK(hipHostFree(g_h_sc)); }
    g_sc_cap = m + 64;
    GCGE_HIP_CHECK(hipMalloc(&g_d_sc, 2 * (size_t)g_sc_cap * sizeof(double)));
    GCGE_HIP_CHECK(hipHostMalloc(&g_h_sc, 2 * (size_t)g_sc_cap * sizeof(double)));
  }
}
// coef (NULL: none) and flag go up; returns the device flags (the coefficients are g_d_sc)
static const int* pcg_upload(int m, const double* coef, const int* flag, hipStream_t st) {
  pcg_scalars(m, st);
  GCGE_HIP_CHECK(hipStreamSynchronize(st));      // the pinned buffer is reused
  if (coef != nullptr) memcpy(g_h_sc, coef, m * sizeof(double));
  else memset(g_h_sc, 0, m * sizeof(double));
  memcpy(g_h_sc + g_sc_cap, flag, m * sizeof(int));
  GCGE_HIP_CHECK(hipMemcpyAsync(g_d_sc, g_h_sc, m * sizeof(double), hipMemcpyHostToDevice, st));
  GCGE_HIP_CHECK(hipMemcpyAsync(g_d_sc + g_sc_cap, g_h_sc + g_sc_cap, m * sizeof(int), hipMemcpyHostToDevice, st));
  return reinterpret_cast<const int*>(g_d_sc + g_sc_cap);
}
// the len sums nb workgroups left in part come back to the host, added in reduce_partials' fixed order
static void pcg_sums_to_host(double* part, long nb, int len, double* out, hipStream_t st) {
  pcg_scalars(len, st);
  gcge_hip_reduce_partials(part, (int)nb, len, part + (size_t)nb * len, st);
  GCGE_HIP_CHECK(hipMemcpyAsync(g_h_sc, part + (size_t)nb * len, len * sizeof(double), hipMemcpyDeviceToHost, st));
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  memcpy(out, g_h_sc, len * sizeof(double));
}

extern "C" int gcge_hip_pcg_step(int nrows, const double* d_p, long ldp, const double* d_w, long ldw, double* d_x, long ldx, double* d_r, long ldr,
                                 int m, const double* alpha, const int* flag, double* rr, void* stream) {
  gcge_hip_apply_pending();
  if (m <= 0) return 0;
  for (int j = 0; j < m; ++j) rr[j] = 0.0;
  if (nrows <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const CgGrid grid = cg_grid(nrows);
  const int* d_flag = pcg_upload(m, alpha, flag, st);
  double* part = gcge_hip_partial_ws((size_t)grid.nb * m + m);
  if (m <= 512 && cg_vec_ok(m, {d_p, d_w, d_x, d_r}, {ldp, ldw, ldx, ldr}))
    hipLaunchKernelGGL(pcg_step_v2<4>, dim3((unsigned)grid.nb), dim3(256), 0, st, (long)nrows, d_p, ldp, d_w, ldw, d_x, ldx, d_r, ldr, m,
                       (const double*)g_d_sc, d_flag, part, cg_tpr(m));
  else
    hipLaunchKernelGGL(pcg_step_s, dim3((unsigned)grid.nb), dim3(256), 0, st, (long)nrows, d_p, ldp, d_w, ldw, d_x, ldx, d_r, ldr, m,
                       (const double*)g_d_sc, d_flag, part, grid.rpb);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  pcg_sums_to_host(part, grid.nb, m, rr, st);
  return 0;
}

extern "C" int gcge_hip_pcg_dots(int nrows, const double* d_z, long ldz, const double* d_r, long ldr, const double* d_w, long ldw, int m,
                                 double* zr, double* zw, void* stream) {
  gcge_hip_apply_pending();
  if (m <= 0) return 0;
  for (int j = 0; j < m; ++j) zr[j] = zw[j] = 0.0;
  if (nrows <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const CgGrid grid = cg_grid(nrows);
  double* part = gcge_hip_partial_ws((size_t)grid.nb * 2 * m + 2 * m);
  if (m <= 512 && cg_vec_ok(m, {d_z, d_r, d_w}, {ldz, ldr, ldw}))
    hipLaunchKernelGGL(pcg_dots_v2<4>, dim3((unsigned)grid.nb), dim3(256), 0, st, (long)nrows, d_z, ldz, d_r, ldr, d_w, ldw, m, part, cg_tpr(m));
  else
    hipLaunchKernelGGL(pcg_dots_s, dim3((unsigned)grid.nb), dim3(256), 0, st, (long)nrows, d_z, ldz, d_r, ldr, d_w, ldw, m, part, grid.rpb);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  std::vector<double> both(2 * (size_t)m);
  pcg_sums_to_host(part, grid.nb, 2 * m, both.data(), st);
  memcpy(zr, both.data(), m * sizeof(double));
  memcpy(zw, both.data() + m, m * sizeof(double));
  return 0;
}

extern "C" int gcge_hip_pcg_direction(int nrows, const double* d_z, long ldz, double* d_p, long ldp, int m, const double* beta, const int* flag,
                                      void* stream) {
  gcge_hip_apply_pending();
  if (m <= 0 || nrows <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const CgGrid grid = cg_grid(nrows);
  const int* d_flag = pcg_upload(m, beta, flag, st);
  if (m <= 512 && cg_vec_ok(m, {d_z, d_p}, {ldz, ldp}))
    hipLaunchKernelGGL(pcg_direction_v2<4>, dim3((unsigned)grid.nb), dim3(256), 0, st, (long)nrows, d_z, ldz, d_p, ldp, m, (const double*)g_d_sc,
                       d_flag, cg_tpr(m));
  else
    hipLaunchKernelGGL(pcg_direction_s, dim3((unsigned)grid.nb), dim3(256), 0, st, (long)nrows, d_z, ldz, d_p, ldp, m, (const double*)g_d_sc,
                       d_flag, grid.rpb);
  return (int)hipGetLastError();
}

extern "C" int gcge_hip_pcg_shift(int nrows, const double* d_p, long ldp, const double* d_q, long ldq, double* d_w, long ldw, int m,
                                  const double* shift, const int* flag, double* pw, void* stream) {
  gcge_hip_apply_pending();
  if (m <= 0) return 0;
  for (int j = 0; j < m; ++j) pw[j] = 0.0;
  if (nrows <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const CgGrid grid = cg_grid(nrows);
  const int* d_flag = pcg_upload(m, shift, flag, st);
  double* part = gcge_hip_partial_ws((size_t)grid.nb * m + m);
  const bool qp = d_q == d_p && ldq == ldp;
  const bool vec = m <= 512 && cg_vec_ok(m, {d_p, d_q, d_w}, {ldp, ldq, ldw});
#define GCGE_PCG_SHIFT_LAUNCH(kernel, last)                                                                                          \
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid.nb), dim3(256), 0, st, (long)nrows, d_p, ldp, d_q, ldq, d_w, ldw, m, (const double*)g_d_sc, \
                     d_flag, part, last)
  if (vec && qp) GCGE_PCG_SHIFT_LAUNCH((pcg_shift_v2<4, true>), cg_tpr(m));
  else if (vec) GCGE_PCG_SHIFT_LAUNCH((pcg_shift_v2<4, false>), cg_tpr(m));
  else if (qp) GCGE_PCG_SHIFT_LAUNCH(pcg_shift_s<true>, grid.rpb);
  else GCGE_PCG_SHIFT_LAUNCH(pcg_shift_s<false>, grid.rpb);
#undef GCGE_PCG_SHIFT_LAUNCH
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  pcg_sums_to_host(part, grid.nb, m, pw, st);
  return 0;
}

// ---- the hooks of the HIP table's back-end record (GCGE_BACKEND, include/gcge_ops.h): the same sweeps on blocks of this back-end ----
// a window of m columns from column c0 of a block with the rows and the row order of `like`
static bool window_ok(const GcgeHipMV* v, int c0, int m, const GcgeHipMV* like) {
  return v != nullptr && c0 >= 0 && c0 + m <= v->ncols && v->nrows == like->nrows && real_perm(v->perm) == real_perm(like->perm);
}
static int HIP_PcgStep(void** p, int p0, void** w, int w0, void** x, int x0, void** r, int r0, int m, const double* alpha, const int* flag,
                       double* rr, struct OPS_* ops) {
  (void)ops;
  GcgeHipMV *vp = (GcgeHipMV*)p, *vw = (GcgeHipMV*)w, *vx = (GcgeHipMV*)x, *vr = (GcgeHipMV*)r;
  if (m <= 0 || vx == nullptr || alpha == nullptr || flag == nullptr || rr == nullptr) return 0;
  if (!window_ok(vp, p0, m, vx) || !window_ok(vw, w0, m, vx) || !window_ok(vx, x0, m, vx) || !window_ok(vr, r0, m, vx)) return 0;
  if (vx == vr || vx == vp || vx == vw || vr == vp || vr == vw) return 0;      // (what is written is no other operand)
  gcge_hip_enter();
  SlotTimer tm_("PCG step (x, r, |r|^2)", m);
  const int rc = gcge_hip_pcg_step(vx->nrows, vp->d + p0, vp->ld, vw->d + w0, vw->ld, vx->d + x0, vx->ld, vr->d + r0, vr->ld, m, alpha, flag, rr,
                                   gcge_hip_stream());
  GCGE_REQUIRE(rc == 0, "PCG step: kernel launch");
  return 1;
}
static int HIP_PcgDots(void** z, int z0, void** r, int r0, void** w, int w0, int m, double* zr, double* zw, struct OPS_* ops) {
  (void)ops;
  GcgeHipMV *vz = (GcgeHipMV*)z, *vr = (GcgeHipMV*)r, *vw = (GcgeHipMV*)w;
  if (m <= 0 || vz == nullptr || zr == nullptr || zw == nullptr) return 0;
  if (!window_ok(vz, z0, m, vz) || !window_ok(vr, r0, m, vz) || !window_ok(vw, w0, m, vz)) return 0;
  gcge_hip_enter();
  SlotTimer tm_("PCG dots (z.r, z.w)", m);
  const int rc = gcge_hip_pcg_dots(vz->nrows, vz->d + z0, vz->ld, vr->d + r0, vr->ld, vw->d + w0, vw->ld, m, zr, zw, gcge_hip_stream());
  GCGE_REQUIRE(rc == 0, "PCG dots: kernel launch");
  return 1;
}
static int HIP_PcgDirection(void** z, int z0, void** p, int p0, int m, const double* beta, const int* flag, struct OPS_* ops) {
  (void)ops;
  GcgeHipMV *vz = (GcgeHipMV*)z, *vp = (GcgeHipMV*)p;
  if (m <= 0 || vp == nullptr || beta == nullptr || flag == nullptr || vz == vp) return 0;
  if (!window_ok(vz, z0, m, vp) || !window_ok(vp, p0, m, vp)) return 0;
  gcge_hip_enter();
  SlotTimer tm_("PCG direction (p = z + beta p)", m);
  const int rc = gcge_hip_pcg_direction(vp->nrows, vz->d + z0, vz->ld, vp->d + p0, vp->ld, m, beta, flag, gcge_hip_stream());
  GCGE_REQUIRE(rc == 0, "PCG direction: kernel launch");
  return 1;
}
static int HIP_PcgShift(void** p, int p0, void** q, int q0, void** w, int w0, int m, const double* shift, const int* flag, double* pw,
                        struct OPS_* ops) {
  (void)ops;
  GcgeHipMV *vp = (GcgeHipMV*)p, *vq = (GcgeHipMV*)q, *vw = (GcgeHipMV*)w;
  if (m <= 0 || vw == nullptr || shift == nullptr || flag == nullptr || pw == nullptr) return 0;
  if (!window_ok(vp, p0, m, vw) || !window_ok(vq, q0, m, vw) || !window_ok(vw, w0, m, vw)) return 0;
  if (vw == vp || vw == vq) return 0;      // (what is written is no other operand)
  gcge_hip_enter();
  SlotTimer tm_("PCG shift (w -= shift q, p.w)", m);
  const int rc = gcge_hip_pcg_shift(vw->nrows, vp->d + p0, vp->ld, vq->d + q0, vq->ld, vw->d + w0, vw->ld, m, shift, flag, pw, gcge_hip_stream());
  GCGE_REQUIRE(rc == 0, "PCG shift: kernel launch");
  return 1;
}
// iterations of the fused CG's last call (the solver amg_smoother_setup installs)
static int bpcg_last_niter(struct OPS_* ops) {
  (void)ops;
  int n = 0;
  gcge_hip_bpcg_stats(nullptr, nullptr, &n);
  return n;
}

extern "C" void gcge_hip_pcg_backend(GCGE_BACKEND* be) {
  be->pcg_step = HIP_PcgStep;
  be->pcg_dots = HIP_PcgDots;
  be->pcg_direction = HIP_PcgDirection;
  be->pcg_shift = HIP_PcgShift;
  be->amg_smoother_niter = bpcg_last_niter;
}
