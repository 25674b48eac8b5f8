// The bordered product of PAS's composite table (include/gcge_pas.h) in one pass over QX:
//     y[:, y0 .. y0+m) = beta y[:, y0 .. y0+m) + QX t        g = QX^T q[:, q0 .. q0+m)
// QX is the tall n_H x s border of the augmented matrix [[A_H, QX], [QX^T, XX]]; with the slots the two products are a
// LinearComb and a Gram that read QX from HBM twice: 8 n (2 s + 3 m) bytes.  Here every 16-row tile of QX is read by one
// workgroup for both products (the second read of a tile hits the caches): 8 n (s + 3 m) bytes — QX and q once, y read
// and written once (s <= 128; a wider border is taken in chunks of 128 columns, y then once per chunk).
//
// Both products run on v_mfma_f64_16x16x4_f64 (D(16x16) += A(16x4) B(4x16); lane l: A[l & 15][l >> 4], B[l >> 4][l & 15],
// D[4 t + (l >> 4)][l & 15] in register t) over the ROW-major blocks of the back-end:
//   y tile  (16 rows x 16 columns of m):  A = QX[r + i][k + kk],      B = t[k + kk][j]
//   g tile  (16 of s x 16 of m):          A = QX[r + kk][c + i],      B = q[r + kk][j]     (split-K over the rows)
// Every workgroup sums its rows' g partials in registers and writes them to its own slab; a second kernel adds the slabs
// in a fixed order (bitwise reproducible, no atomics: the scheme of gram_mfma.hip).
//
// Shapes: 1 <= m <= 128, 1 <= s (chunks of 128), any n and column offsets; loads outside the shape read 0, stores are masked.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "gcge_hip_internal.h"

namespace {
typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int SC = 128;   // border columns per pass: 8 tiles of 16, two per wave
constexpr int MT = 8;     // at most 8 tiles of 16 columns of m

__device__ __forceinline__ double ld_or0(const double* p, bool ok) { return ok ? *p : 0.0; }

// one workgroup = 4 waves, rows [tile_lo * 16, tile_hi * 16) of the chunk of border columns [c0, c0 + SC)
__global__ __launch_bounds__(256) void pas_border_kernel(long n, const double* __restrict__ qx, long ldqx, int s, int c0,
    const double* __restrict__ q, long ldq, double* __restrict__ y, long ldy, int m, double beta, int first,
    const double* __restrict__ t, long ldt, double* __restrict__ slab, long tiles_per_wg, long ntiles) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int li = lane & 15, lk = lane >> 4;
  const int mtiles = (m + 15) >> 4;
  const long tile_lo = (long)blockIdx.x * tiles_per_wg;
  const long tile_hi = tile_lo + tiles_per_wg < ntiles ? tile_lo + tiles_per_wg : ntiles;
  v4d gacc[2][MT];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < MT; ++b) gacc[a][b] = v4d{0.0, 0.0, 0.0, 0.0};
  // the border columns of this wave's two g tiles, and this wave's two y column tiles (wave, wave + 4)
  const int gc[2] = {c0 + 16 * wave + li, c0 + 16 * (wave + 4) + li};
  for (long tile = tile_lo; tile < tile_hi; ++tile) {
    const long r0 = tile * 16;
    // ---- y tile: 16 rows x columns 16 (wave) .. and 16 (wave + 4) ..  (k over the chunk's border columns)
    v4d yacc[2] = {v4d{0.0, 0.0, 0.0, 0.0}, v4d{0.0, 0.0, 0.0, 0.0}};
    const long ry = r0 + li;
    const bool rok = ry < n;
    for (int k = 0; k < SC; k += 4) {
      const int kc = c0 + k + lk;
      const double a = ld_or0(qx + ry * ldqx + kc, rok && kc < s);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int j = 16 * (wave + 4 * u) + li;
        const double b = ld_or0(t + (long)kc * ldt + j, kc < s && j < m);
        yacc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, yacc[u], 0, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = 16 * (wave + 4 * u) + li;
      if (j >= m) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long row = r0 + 4 * r + lk;
        if (row >= n) continue;
        double* py = y + row * ldy + j;
        *py = (first ? (beta == 0.0 ? 0.0 : beta * *py) : *py) + yacc[u][r];
      }
    }
    // ---- g partial: (border columns of the two tiles) x m, split-K over the 16 rows
#pragma unroll
    for (int kk = 0; kk < 16; kk += 4) {
      const long row = r0 + kk + lk;
      const bool ok = row < n;
      double a[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) a[u] = ld_or0(qx + row * ldqx + gc[u], ok && gc[u] < s);
#pragma unroll
      for (int b = 0; b < MT; ++b) {
        if (b >= mtiles) break;
        const int j = 16 * b + li;
        const double bq = ld_or0(q + row * ldq + j, ok && j < m);
#pragma unroll
        for (int u = 0; u < 2; ++u) gacc[u][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], bq, gacc[u][b], 0, 0, 0);
      }
    }
  }
  // this workgroup's partial of the chunk: slab[wg][i][j], i < SC border columns, j < 16 mtiles
  double* out = slab + (long)blockIdx.x * SC * (16 * MT);
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int b = 0; b < MT; ++b) {
      if (b >= mtiles) break;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * (wave + 4 * u) + 4 * r + lk;
        out[(long)i * (16 * MT) + 16 * b + li] = gacc[u][b][r];
      }
    }
}

// g[c0 + i, j] = sum over the workgroups in order of slab[wg][i][j]  (column-major g, leading dimension s)
__global__ __launch_bounds__(256) void pas_border_reduce(const double* __restrict__ slab, int nwg, int s, int c0, int m,
                                                          double* __restrict__ g) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(idx / m), j = (int)(idx % m);
  if (i >= SC || c0 + i >= s) return;
  double acc = 0.0;
  for (int w = 0; w < nwg; ++w) acc += slab[((long)w * SC + i) * (16 * MT) + j];
  g[(long)j * s + c0 + i] = acc;
}

double* g_dev = nullptr; size_t g_dev_len = 0;     // t (row-major s x m) then g (column-major s x m)
std::vector<double> g_host;
}  // namespace

// GCGE_BACKEND.pas_border of OPS_HIP_Set (GCGE_PAS_BORDER_FN, include/gcge_pas.h)
extern "C" int gcge_hip_pas_border(void** QX, int s, void** q, int q0, void** y, int y0, int m, double beta,
                                   const double* t, int ldt, double* g, int ldg) {
  if (s < 1 || m < 1) return s < 1 && m >= 0 ? 0 : -1;
  if (m > 16 * MT) return -1;   // wider blocks: the slots
  gcge_hip_apply_pending();
  const int n = gcge_hip_mv_nrows(QX);
  GCGE_REQUIRE(gcge_hip_mv_nrows(q) == n && gcge_hip_mv_nrows(y) == n, "pas_border: QX, q and y have the same rows");
  GCGE_REQUIRE(s <= gcge_hip_mv_ncols(QX) && q0 >= 0 && q0 + m <= gcge_hip_mv_ncols(q) && y0 >= 0 && y0 + m <= gcge_hip_mv_ncols(y),
               "pas_border: column ranges");
  GCGE_REQUIRE(ldt >= s && ldg >= s, "pas_border: leading dimensions of t and g");
  GCGE_REQUIRE(q != y || q0 + m <= y0 || y0 + m <= q0, "pas_border: q and y ranges must not overlap");
  long ldqx, ldq, ldy;
  const double* dqx = gcge_hip_mv_device_ptr(QX, &ldqx);
  const double* dq = gcge_hip_mv_device_ptr(q, &ldq) + q0;
  double* dy = gcge_hip_mv_device_ptr(y, &ldy) + y0;
  hipStream_t st = (hipStream_t)gcge_hip_stream();
  // t to the device, row-major s x m (leading dimension m), then room for g (s x m)
  const size_t len = 2 * (size_t)s * m;
  if (len > g_dev_len) {
    if (g_dev != nullptr) { GCGE_HIP_CHECK(hipStreamSynchronize(st)); GCGE_HIP_CHECK(hipFree(g_dev)); }
    GCGE_HIP_CHECK(hipMalloc(&g_dev, len * sizeof(double))); g_dev_len = len;
  }
  g_host.resize(len);
  for (int k = 0; k < s; ++k)
    for (int j = 0; j < m; ++j) g_host[(size_t)k * m + j] = t[(size_t)j * ldt + k];
  GCGE_HIP_CHECK(hipMemcpyAsync(g_dev, g_host.data(), (size_t)s * m * sizeof(double), hipMemcpyHostToDevice, st));
  double* dt = g_dev; double* dg = g_dev + (size_t)s * m;
  const long ntiles = ((long)n + 15) / 16;
  const long nwg_want = ntiles < 1024 ? ntiles : 1024;
  const long tiles_per_wg = nwg_want > 0 ? (ntiles + nwg_want - 1) / nwg_want : 1;
  const int nwg = (int)(ntiles > 0 ? (ntiles + tiles_per_wg - 1) / tiles_per_wg : 0);
  if (nwg == 0) {
    for (int j = 0; j < m; ++j) memset(g + (size_t)j * ldg, 0, (size_t)s * sizeof(double));
    return 0;
  }
  double* slab = gcge_hip_partial_ws((size_t)nwg * SC * 16 * MT);
  for (int c0 = 0; c0 < s; c0 += SC) {
    hipLaunchKernelGGL(pas_border_kernel, dim3(nwg), dim3(256), 0, st, (long)n, dqx, ldqx, s, c0, dq, ldq, dy, ldy, m, beta,
                       c0 == 0 ? 1 : 0, (const double*)dt, (long)m, slab, tiles_per_wg, ntiles);
    GCGE_HIP_CHECK(hipGetLastError());
    const long cells = (long)SC * m;
    hipLaunchKernelGGL(pas_border_reduce, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, (const double*)slab, nwg, s, c0, m, dg);
    GCGE_HIP_CHECK(hipGetLastError());
  }
  GCGE_HIP_CHECK(hipMemcpyAsync(g_host.data(), dg, (size_t)s * m * sizeof(double), hipMemcpyDeviceToHost, st));
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  for (int j = 0; j < m; ++j) memcpy(g + (size_t)j * ldg, g_host.data() + (size_t)j * s, (size_t)s * sizeof(double));
  return 0;
}
