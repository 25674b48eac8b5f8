// The vector sweep of one step of a Chebyshev filter (GCGE_ChebFilter, csrc/host/chfsi.c): with out holding the product A y,
//
//   cheb_sweep     out <- alpha (out - c y) - beta z          3 reads + 1 write        slots: 2 Axpby (3 streams each)
//                                                             (beta == 0: 2 + 1, z is not read)
// in block streams of the width m, in place on out, in ONE pass.  The step Y_{j+1} = alpha_j (A - c I) Y_j - beta_j Y_{j-1} of the
// three-term recurrence is then the product (2 streams) and this sweep: 6 streams instead of the 8 of product + two Axpby.
//
// Order of operations, the same in both kernels and on every run (no sums, no atomics, every entry computed by one thread from its
// own three operands):
//     u   = fma(-c, y, out)                       one rounding
//     out = fma(alpha, u, -(beta * z))            beta * z rounded, then one rounding            (beta != 0)
//     out = alpha * u                             one rounding; z may be NULL or hold anything   (beta == 0: a filter's first step)
// alpha, c and beta are the same for every column: kernel arguments, nothing is staged.
//
// Modelled on pcg_shift of pcg_sweeps.hip: 16-byte lanes (v2d, one column pair per thread) with non-temporal loads and stores when
// the width, the column origins and the leading dimensions are even (cg_vec_ok), a scalar-lane kernel (4 row lanes x 64 columns)
// otherwise; row groups of 4 with all loads issued before the arithmetic; the grid is cg_grid's.
//
// Beside it, in the same shape, the sums of the band-pass filter (GCGE_ChebBandFilter):
//
//   cheb_accum     acc <- [acc +] mu_a ta + mu_b tb                3 reads + 1 write        slots: 2 Axpby (3 streams each)
//                                                                  (init: 2 + 1, acc is not read; one term: tb is not read)
//
// And the sweep that also returns the inner products of the kernel polynomial method (GCGE_ChebMoments), with the sums alone beside it:
//
//   cheb_sweep_dots   cheb_sweep, and oo_j = sum_r out_new[r, j]^2, oy_j = sum_r out_new[r, j] y[r, j]      3 reads + 1 write
//                                                                  slots: the sweep, then two 'D' products (3 to 4 more reads)
//   cheb_dots         tt_j = sum_r t[r, j]^2, ty_j = sum_r t[r, j] y[r, j]                                  2 reads
// per-workgroup partial sums in gcge_hip_partial_ws, added by reduce_partials in a fixed order as in pcg_sweeps.hip: no atomics, the
// same bits on every run; the sums come back to the host, so these two wait for the stream.
//
// Also here: the device staging of the fused step's scalars (gcge_hip_cheb_step_mv, mat_product.hip), filled by a one-block kernel
// so that nothing is copied from the host and nothing is waited for.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "gcge_hip.h"
#include "gcge_hip_internal.h"

namespace gcge {

typedef double v2d __attribute__((ext_vector_type(2)));

template <int UNR, bool HASZ>
__global__ __launch_bounds__(256) void cheb_sweep_v2(long nrows, double* __restrict__ out, long ldo, const double* __restrict__ y, long ldy,
    const double* __restrict__ z, long ldz, int m, double alpha, double c, double beta, int tpr) {
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  if (j >= m) return;
  // the rows of workgroup blockIdx.x, walked rpb at a time in groups of UNR (pcg_rows of pcg_sweeps.hip)
  const long group = (long)rpb * UNR;
  const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + group - 1) / group * group;
  const long rend = min(nrows, ((long)blockIdx.x + 1) * slab), step = rpb;
  auto one = [&](long rr, v2d ov, v2d yv, v2d zv) {
    const v2d u = {fma(-c, yv.x, ov.x), fma(-c, yv.y, ov.y)};
    const v2d r = HASZ ? v2d{fma(alpha, u.x, -(beta * zv.x)), fma(alpha, u.y, -(beta * zv.y))} : v2d{alpha * u.x, alpha * u.y};
    __builtin_nontemporal_store(r, reinterpret_cast<v2d*>(out + rr * ldo + j));
  };
  long row = (long)blockIdx.x * slab + ty;
  for (; row + (UNR - 1) * step < rend; row += step * UNR) {
    v2d ov[UNR], yv[UNR], zv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long rr = row + u * step;
      ov[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(out + rr * ldo + j));
      yv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(y + rr * ldy + j));
      zv[u] = HASZ ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(z + rr * ldz + j)) : v2d{0.0, 0.0};
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < UNR; ++u) one(row + u * step, ov[u], yv[u], zv[u]);
  }
  for (; row < rend; row += step)
    one(row, *reinterpret_cast<const v2d*>(out + row * ldo + j), *reinterpret_cast<const v2d*>(y + row * ldy + j),
        HASZ ? *reinterpret_cast<const v2d*>(z + row * ldz + j) : v2d{0.0, 0.0});
}

// any width, origin and leading dimension: 4 row lanes x 64 columns, the columns in chunks of 64
template <bool HASZ>
__global__ __launch_bounds__(256) void cheb_sweep_s(long nrows, double* __restrict__ out, long ldo, const double* __restrict__ y, long ldy,
    const double* __restrict__ z, long ldz, int m, double alpha, double c, double beta, long rows_per_block) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(nrows, r0 + rows_per_block);
  for (int j = tx; j < m; j += 64)
    for (long row = r0 + ty; row < r1; row += 4) {
      const double u = fma(-c, y[row * ldy + j], out[row * ldo + j]);
      out[row * ldo + j] = HASZ ? fma(alpha, u, -(beta * z[row * ldz + j])) : alpha * u;
    }
}

// ---- the sums of a band-pass filter (GCGE_ChebBandFilter): acc <- [acc +] mu_a ta + mu_b tb, two iterates of the recurrence in ONE
// pass: 3 reads + 1 write (INIT: acc is not read, 2 + 1; !HASB: one term, tb is not read) where the slots take two Axpby of 3 streams
// each.  s = fma(mu_a, ta, acc) (INIT: mu_a * ta), then acc = fma(mu_b, tb, s) (one term: acc = s): every entry by one thread from
// its own operands, the same bits in both kernels and on every run.  The launch shape is cheb_sweep's.
template <int UNR, bool INIT, bool HASB>
__global__ __launch_bounds__(256) void cheb_accum_v2(long nrows, double* __restrict__ acc, long lda, const double* __restrict__ ta, long ldta,
    const double* __restrict__ tb, long ldtb, int m, double mu_a, double mu_b, int tpr) {
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  if (j >= m) return;
  const long group = (long)rpb * UNR;
  const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + group - 1) / group * group;
  const long rend = min(nrows, ((long)blockIdx.x + 1) * slab), step = rpb;
  const v2d zero = {0.0, 0.0};
  auto one = [&](long rr, v2d cv, v2d av, v2d bv) {
    const v2d s = INIT ? v2d{mu_a * av.x, mu_a * av.y} : v2d{fma(mu_a, av.x, cv.x), fma(mu_a, av.y, cv.y)};
    const v2d r = HASB ? v2d{fma(mu_b, bv.x, s.x), fma(mu_b, bv.y, s.y)} : s;
    __builtin_nontemporal_store(r, reinterpret_cast<v2d*>(acc + rr * lda + j));
  };
  long row = (long)blockIdx.x * slab + ty;
  for (; row + (UNR - 1) * step < rend; row += step * UNR) {
    v2d cv[UNR], av[UNR], bv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long rr = row + u * step;
      cv[u] = INIT ? zero : __builtin_nontemporal_load(reinterpret_cast<const v2d*>(acc + rr * lda + j));
      av[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(ta + rr * ldta + j));
      bv[u] = HASB ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(tb + rr * ldtb + j)) : zero;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < UNR; ++u) one(row + u * step, cv[u], av[u], bv[u]);
  }
  for (; row < rend; row += step)
    one(row, INIT ? zero : *reinterpret_cast<const v2d*>(acc + row * lda + j), *reinterpret_cast<const v2d*>(ta + row * ldta + j),
        HASB ? *reinterpret_cast<const v2d*>(tb + row * ldtb + j) : zero);
}

template <bool INIT, bool HASB>
__global__ __launch_bounds__(256) void cheb_accum_s(long nrows, double* __restrict__ acc, long lda, const double* __restrict__ ta, long ldta,
    const double* __restrict__ tb, long ldtb, int m, double mu_a, double mu_b, long rows_per_block) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(nrows, r0 + rows_per_block);
  for (int j = tx; j < m; j += 64)
    for (long row = r0 + ty; row < r1; row += 4) {
      const double s = INIT ? mu_a * ta[row * ldta + j] : fma(mu_a, ta[row * ldta + j], acc[row * lda + j]);
      acc[row * lda + j] = HASB ? fma(mu_b, tb[row * ldtb + j], s) : s;
    }
}

// ---- the step's sweep WITH the two column sums of the kernel polynomial method (GCGE_ChebMoments): cheb_sweep's arithmetic, entry by
// entry the same expressions, so out gets the same bits; from the value r it stores each thread also adds r^2 and r y into its own
// sums (fma, rows in ascending order), the workgroup adds its row lanes in LDS in ascending lane order and leaves
//     partial[b * 2m + j] = sum r^2,   partial[b * 2m + m + j] = sum r y        (pcg_dots' layout)
// for reduce_partials: a fixed order, no atomics, the same bits on every run.  3 reads + 1 write (!HASZ: 2 + 1), as the sweep alone.
template <int UNR, bool HASZ>
__global__ __launch_bounds__(256) void cheb_sweep_dots_v2(long nrows, double* __restrict__ out, long ldo, const double* __restrict__ y, long ldy,
    const double* __restrict__ z, long ldz, int m, double alpha, double c, double beta, double* __restrict__ partial, int tpr) {
  __shared__ double red[256][4];
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
  const bool mine = j < m;
  if (mine) {
    const long group = (long)rpb * UNR;
    const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + group - 1) / group * group;
    const long rend = min(nrows, ((long)blockIdx.x + 1) * slab), step = rpb;
    auto one = [&](long rr, v2d ov, v2d yv, v2d zv) {
      const v2d u = {fma(-c, yv.x, ov.x), fma(-c, yv.y, ov.y)};
      const v2d r = HASZ ? v2d{fma(alpha, u.x, -(beta * zv.x)), fma(alpha, u.y, -(beta * zv.y))} : v2d{alpha * u.x, alpha * u.y};
      __builtin_nontemporal_store(r, reinterpret_cast<v2d*>(out + rr * ldo + j));
      s0 = fma(r.x, r.x, s0); s1 = fma(r.y, r.y, s1);
      t0 = fma(r.x, yv.x, t0); t1 = fma(r.y, yv.y, t1);
    };
    long row = (long)blockIdx.x * slab + ty;
    for (; row + (UNR - 1) * step < rend; row += step * UNR) {
      v2d ov[UNR], yv[UNR], zv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const long rr = row + u * step;
        ov[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(out + rr * ldo + j));
        yv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(y + rr * ldy + j));
        zv[u] = HASZ ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(z + rr * ldz + j)) : v2d{0.0, 0.0};
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(row + u * step, ov[u], yv[u], zv[u]);
    }
    for (; row < rend; row += step)
      one(row, *reinterpret_cast<const v2d*>(out + row * ldo + j), *reinterpret_cast<const v2d*>(y + row * ldy + j),
          HASZ ? *reinterpret_cast<const v2d*>(z + row * ldz + j) : v2d{0.0, 0.0});
  }
  red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1; red[threadIdx.x][2] = t0; red[threadIdx.x][3] = t1;
  __syncthreads();
  if (ty == 0 && mine) {
    for (int k = 1; k < rpb; ++k) {
      s0 += red[k * tpr + tx][0]; s1 += red[k * tpr + tx][1]; t0 += red[k * tpr + tx][2]; t1 += red[k * tpr + tx][3];
    }
    double* p = partial + (long)blockIdx.x * 2 * m;
    p[j] = s0; p[j + 1] = s1; p[m + j] = t0; p[m + j + 1] = t1;
  }
}

template <bool HASZ>
__global__ __launch_bounds__(256) void cheb_sweep_dots_s(long nrows, double* __restrict__ out, long ldo, const double* __restrict__ y, long ldy,
    const double* __restrict__ z, long ldz, int m, double alpha, double c, double beta, double* __restrict__ partial, long rows_per_block) {
  __shared__ double red[2][4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(nrows, r0 + rows_per_block);
  for (int c0 = 0; c0 < m; c0 += 64) {
    const int j = c0 + tx;
    double s = 0.0, t = 0.0;
    if (j < m)
      for (long row = r0 + ty; row < r1; row += 4) {
        const double yv = y[row * ldy + j];
        const double u = fma(-c, yv, out[row * ldo + j]);
        const double r = HASZ ? fma(alpha, u, -(beta * z[row * ldz + j])) : alpha * u;
        out[row * ldo + j] = r;
        s = fma(r, r, s);
        t = fma(r, yv, t);
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

// ---- the same two sums of an iterate that is in memory already (behind the fused step): tt = sum t^2, ty = sum t y from ONE read of
// t and y, 2 reads; the launch shape and the partials' layout are cheb_sweep_dots'.
template <int UNR>
__global__ __launch_bounds__(256) void cheb_dots_v2(long nrows, const double* __restrict__ t, long ldt, const double* __restrict__ y, long ldy, int m,
    double* __restrict__ partial, int tpr) {
  __shared__ double red[256][4];
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
  const bool mine = j < m;
  if (mine) {
    const long group = (long)rpb * UNR;
    const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + group - 1) / group * group;
    const long rend = min(nrows, ((long)blockIdx.x + 1) * slab), step = rpb;
    auto one = [&](v2d tv, v2d yv) {
      s0 = fma(tv.x, tv.x, s0); s1 = fma(tv.y, tv.y, s1);
      t0 = fma(tv.x, yv.x, t0); t1 = fma(tv.y, yv.y, t1);
    };
    long row = (long)blockIdx.x * slab + ty;
    for (; row + (UNR - 1) * step < rend; row += step * UNR) {
      v2d tv[UNR], yv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const long rr = row + u * step;
        tv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(t + rr * ldt + j));
        yv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(y + rr * ldy + j));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(tv[u], yv[u]);
    }
    for (; row < rend; row += step)
      one(*reinterpret_cast<const v2d*>(t + row * ldt + j), *reinterpret_cast<const v2d*>(y + row * ldy + j));
  }
  red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1; red[threadIdx.x][2] = t0; red[threadIdx.x][3] = t1;
  __syncthreads();
  if (ty == 0 && mine) {
    for (int k = 1; k < rpb; ++k) {
      s0 += red[k * tpr + tx][0]; s1 += red[k * tpr + tx][1]; t0 += red[k * tpr + tx][2]; t1 += red[k * tpr + tx][3];
    }
    double* p = partial + (long)blockIdx.x * 2 * m;
    p[j] = s0; p[j + 1] = s1; p[m + j] = t0; p[m + j + 1] = t1;
  }
}

__global__ __launch_bounds__(256) void cheb_dots_s(long nrows, const double* __restrict__ t, long ldt, const double* __restrict__ y, long ldy, int m,
    double* __restrict__ partial, long rows_per_block) {
  __shared__ double red[2][4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(nrows, r0 + rows_per_block);
  for (int c0 = 0; c0 < m; c0 += 64) {
    const int j = c0 + tx;
    double s = 0.0, q = 0.0;
    if (j < m)
      for (long row = r0 + ty; row < r1; row += 4) {
        const double tv = t[row * ldt + j];
        s = fma(tv, tv, s);
        q = fma(tv, y[row * ldy + j], q);
      }
    red[0][ty][tx] = s; red[1][ty][tx] = q;
    __syncthreads();
    if (ty == 0 && j < m) {
      partial[(long)blockIdx.x * 2 * m + j] = (red[0][0][tx] + red[0][1][tx]) + (red[0][2][tx] + red[0][3][tx]);
      partial[(long)blockIdx.x * 2 * m + m + j] = (red[1][0][tx] + red[1][1][tx]) + (red[1][2][tx] + red[1][3][tx]);
    }
    __syncthreads();
  }
}

// the scalars of one fused step, the same for every column: coef = [al | cb | bp] (3 m doubles), flag = m ones
__global__ void cheb_scalars_fill(int m, double al, double cb, double bp, double* __restrict__ coef, int* __restrict__ flag) {
  for (int j = threadIdx.x; j < m; j += blockDim.x) { coef[j] = al; coef[m + j] = cb; coef[2 * m + j] = bp; flag[j] = 1; }
}
}  // namespace gcge

using namespace gcge;

extern "C" int gcge_hip_cheb_sweep(long n, double* out, long ldo, const double* y, long ldy, const double* z, long ldz, int m, double alpha,
                                   double c, double beta, void* stream) {
  gcge_hip_apply_pending();
  if (n < 0 || m < 0 || out == nullptr || y == nullptr || (beta != 0.0 && z == nullptr) || out == y || out == z) return -1;
  if (n == 0 || m == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const CgGrid grid = cg_grid(n);
  const bool hasz = beta != 0.0;
  if (!hasz) { z = y; ldz = ldy; }      // (never read; keeps the alignment test below on the operands that are)
  const bool vec = m <= 512 && cg_vec_ok(m, {out, y, z}, {ldo, ldy, ldz});
#define GCGE_CHEB_LAUNCH(kernel, last)                                                                                              \
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid.nb), dim3(256), 0, st, n, out, ldo, y, ldy, z, ldz, m, alpha, c, beta, last)
  if (vec && hasz) GCGE_CHEB_LAUNCH((cheb_sweep_v2<4, true>), cg_tpr(m));
  else if (vec) GCGE_CHEB_LAUNCH((cheb_sweep_v2<4, false>), cg_tpr(m));
  else if (hasz) GCGE_CHEB_LAUNCH(cheb_sweep_s<true>, grid.rpb);
  else GCGE_CHEB_LAUNCH(cheb_sweep_s<false>, grid.rpb);
#undef GCGE_CHEB_LAUNCH
  return (int)hipGetLastError();
}

// the 2 m sums nb workgroups left in part come back to the host, added in reduce_partials' fixed order (one stream synchronisation)
static void cheb_sums_to_host(double* part, long nb, int m, double* first, double* second, hipStream_t st) {
  double* h = gcge_hip_stage_h(2 * (size_t)m);
  gcge_hip_reduce_partials(part, (int)nb, 2 * m, part + (size_t)nb * 2 * m, st);
  GCGE_HIP_CHECK(hipMemcpyAsync(h, part + (size_t)nb * 2 * m, 2 * (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  memcpy(first, h, m * sizeof(double));
  memcpy(second, h + m, m * sizeof(double));
}

extern "C" int gcge_hip_cheb_sweep_dots(long n, double* out, long ldo, const double* y, long ldy, const double* z, long ldz, int m, double alpha,
                                        double c, double beta, double* oo, double* oy, void* stream) {
  gcge_hip_apply_pending();
  if (n < 0 || m < 0 || out == nullptr || y == nullptr || (beta != 0.0 && z == nullptr) || out == y || out == z || oo == nullptr || oy == nullptr)
    return -1;
  for (int j = 0; j < m; ++j) oo[j] = oy[j] = 0.0;
  if (n == 0 || m == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const CgGrid grid = cg_grid(n);
  const bool hasz = beta != 0.0;
  if (!hasz) { z = y; ldz = ldy; }      // (never read; keeps the alignment test below on the operands that are)
  const bool vec = m <= 512 && cg_vec_ok(m, {out, y, z}, {ldo, ldy, ldz});
  double* part = gcge_hip_partial_ws((size_t)grid.nb * 2 * m + 2 * m);
#define GCGE_CHEB_LAUNCH(kernel, last)                                                                                              \
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid.nb), dim3(256), 0, st, n, out, ldo, y, ldy, z, ldz, m, alpha, c, beta, part, last)
  if (vec && hasz) GCGE_CHEB_LAUNCH((cheb_sweep_dots_v2<4, true>), cg_tpr(m));
  else if (vec) GCGE_CHEB_LAUNCH((cheb_sweep_dots_v2<4, false>), cg_tpr(m));
  else if (hasz) GCGE_CHEB_LAUNCH(cheb_sweep_dots_s<true>, grid.rpb);
  else GCGE_CHEB_LAUNCH(cheb_sweep_dots_s<false>, grid.rpb);
#undef GCGE_CHEB_LAUNCH
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  cheb_sums_to_host(part, grid.nb, m, oo, oy, st);
  return 0;
}

extern "C" int gcge_hip_cheb_dots(long n, const double* t, long ldt, const double* y, long ldy, int m, double* tt, double* ty, void* stream) {
  gcge_hip_apply_pending();
  if (n < 0 || m < 0 || t == nullptr || y == nullptr || tt == nullptr || ty == nullptr) return -1;
  for (int j = 0; j < m; ++j) tt[j] = ty[j] = 0.0;
  if (n == 0 || m == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const CgGrid grid = cg_grid(n);
  double* part = gcge_hip_partial_ws((size_t)grid.nb * 2 * m + 2 * m);
  if (m <= 512 && cg_vec_ok(m, {t, y}, {ldt, ldy}))
    hipLaunchKernelGGL(cheb_dots_v2<4>, dim3((unsigned)grid.nb), dim3(256), 0, st, n, t, ldt, y, ldy, m, part, cg_tpr(m));
  else
    hipLaunchKernelGGL(cheb_dots_s, dim3((unsigned)grid.nb), dim3(256), 0, st, n, t, ldt, y, ldy, m, part, grid.rpb);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  cheb_sums_to_host(part, grid.nb, m, tt, ty, st);
  return 0;
}

extern "C" int gcge_hip_cheb_accum(long n, double* acc, long lda, const double* ta, long ldta, double mu_a, const double* tb, long ldtb,
                                   double mu_b, int m, int init, void* stream) {
  gcge_hip_apply_pending();
  if (n < 0 || m < 0 || acc == nullptr || ta == nullptr || acc == ta || acc == tb) return -1;
  if (n == 0 || m == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const CgGrid grid = cg_grid(n);
  const bool hasb = tb != nullptr;
  if (!hasb) { tb = ta; ldtb = ldta; mu_b = 0.0; }      // (never read; keeps the alignment test below on the operands that are)
  const bool vec = m <= 512 && cg_vec_ok(m, {acc, ta, tb}, {lda, ldta, ldtb});
#define GCGE_ACCUM_LAUNCH(kernel, last)                                                                                             \
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid.nb), dim3(256), 0, st, n, acc, lda, ta, ldta, tb, ldtb, m, mu_a, mu_b, last)
#define GCGE_ACCUM_FORMS(V2, S)                                                                                                     \
  do { if (vec) GCGE_ACCUM_LAUNCH(V2, cg_tpr(m)); else GCGE_ACCUM_LAUNCH(S, grid.rpb); } while (0)
  if (init && hasb) GCGE_ACCUM_FORMS((cheb_accum_v2<4, true, true>), (cheb_accum_s<true, true>));
  else if (init) GCGE_ACCUM_FORMS((cheb_accum_v2<4, true, false>), (cheb_accum_s<true, false>));
  else if (hasb) GCGE_ACCUM_FORMS((cheb_accum_v2<4, false, true>), (cheb_accum_s<false, true>));
  else GCGE_ACCUM_FORMS((cheb_accum_v2<4, false, false>), (cheb_accum_s<false, false>));
#undef GCGE_ACCUM_FORMS
#undef GCGE_ACCUM_LAUNCH
  return (int)hipGetLastError();
}

// The staging area of the fused step: 3 m doubles and m ints on the device, grown on demand, written by a kernel on `stream` (in
// stream order behind the step that read it last).  d_alpha = -alpha, d_beta = -alpha c - 1, d_betaprev = beta, every flag 1: the
// mapping of the step onto kernel MODE 7 (mat_product.hip, gcge_hip_cheb_step_mv).
static double* g_d_cheb = nullptr; static int g_cheb_cap = 0;
extern "C" void gcge_hip_cheb_scalars(int m, double alpha, double c, double beta, void* stream, const double** d_alpha, const double** d_beta,
                                      const double** d_betaprev, const int** d_flag) {
  hipStream_t st = (hipStream_t)stream;
  if (m > g_cheb_cap) {
    if (g_d_cheb) { GCGE_HIP_CHECK(hipStreamSynchronize(st)); GCGE_HIP_CHECK(hipFree(g_d_cheb)); }
    g_cheb_cap = m + 64;
    GCGE_HIP_CHECK(hipMalloc(&g_d_cheb, 4 * (size_t)g_cheb_cap * sizeof(double)));
  }
  int* flag = reinterpret_cast<int*>(g_d_cheb + 3 * (size_t)m);
  hipLaunchKernelGGL(cheb_scalars_fill, dim3(1), dim3(64), 0, st, m, -alpha, -alpha * c - 1.0, beta, g_d_cheb, flag);
  *d_alpha = g_d_cheb; *d_beta = g_d_cheb + m; *d_betaprev = g_d_cheb + 2 * (size_t)m; *d_flag = flag;
}
