// Sampled outer product on a CSR pattern: for every stored entry e of row i with column j = colidx[e]
//
//     out[e] = alpha * sum_{c < k} w[c] * U[i, c] * V[j, c]
//
// — the value of the rank-k product U diag(w) V^T on the stored entries only.  It is what the gradients of eigenvalues
// (d lambda_c / d A_ij = x_ic x_jc) and of a linear solve (d L / d A_ij = -(A^-1 g)_i x_j) with respect to the matrix
// VALUES are (gcge_amd/grad.py).  U and V are row-major blocks, element (r, c) at [r * ld + c], as every block of vectors
// on the device is.
//
// Bytes (HBM bound):  8 n k (U once) + 8 nnz k requested from V (a banded pattern names each row of V from neighbouring
// rows, so most of these are cache hits: 8 n k from memory) + 4 (n + 1 + nnz) structure + 8 nnz written.
//
// One kernel, sample_outer<LPE, CPL, MULTI>:
//   * a wave takes a run of ROWS_PER_WAVE rows and cuts the ENTRIES of that run into G = 64 / LPE contiguous pieces, one
//     per group of LPE lanes: short rows idle no group, a row longer than a wave is shared by the groups;
//   * a group walks its piece row by row; lane s of the group holds columns [s CPL, s CPL + CPL) of the row's U slice,
//     times w, in registers across the row's entries, and loads the same columns of V[j, :] for every entry (CPL = 2:
//     one 16-byte load; CPL = 1: one 8-byte load), UNROLL entries in flight;
//   * the partial sums are added over the group's lanes by an xor butterfly (every lane ends with the same bits) and
//     lane (p mod LPE) keeps the result of the piece's p-th entry, so that a group stores LPE consecutive doubles at
//     once;
//   * MULTI (k > 64 CPL): the columns run in chunks of 64 CPL inside the entry, the sum stays in the lane's register;
//     the chunk of the U slice is then read again for every entry (it stays in the CU's vector cache).
// No atomics; a lane adds its columns in ascending chunks and the butterfly is fixed by LPE, so the order of summation
// depends on (k, CPL) alone and two runs give the same bits.
//
// Branches (gcge_hip_csr_sample_outer):
//   CPL = 2 when ldu and ldv are even and U and V start on 16 bytes, else 1;
//   LPE = the power of two >= ceil(k / CPL), at most 64;  MULTI when k > 64 CPL.
//   CPL = 2 with an odd k reads one double past column k - 1 of a row — inside the row's ld, since ld is even and
//   >= k — and drops it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gcge_hip_internal.h"

namespace gcge {

constexpr int SO_ROWS_PER_WAVE = 16;
constexpr int SO_UNROLL = 4;

// columns [c, c + CPL) of a row that starts at p, zero from column k on
template <int CPL>
__device__ __forceinline__ void so_load(const double* __restrict__ p, int c, int k, double (&r)[CPL]) {
  if (CPL == 2) {
    if (c < k) {
      const double2 t = *reinterpret_cast<const double2*>(p + c);
      r[0] = t.x;
      r[CPL - 1] = c + 1 < k ? t.y : 0.0;
    } else {
      r[0] = 0.0;
      r[CPL - 1] = 0.0;
    }
  } else {
    r[0] = c < k ? p[c] : 0.0;
  }
}

template <int LPE, int CPL, bool MULTI>
__global__ __launch_bounds__(256) void sample_outer(int nrows, const int* __restrict__ rowptr,
                                                    const int* __restrict__ colidx, const double* __restrict__ u, size_t ldu,
                                                    const double* __restrict__ v, size_t ldv, int k,
                                                    const double* __restrict__ w, double alpha, double* __restrict__ out) {
  constexpr int G = 64 / LPE, CW = LPE * CPL;
  const int lane = threadIdx.x & 63, g = lane / LPE, sub = lane % LPE;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long r0l = wave * SO_ROWS_PER_WAVE;
  if (r0l >= nrows) return;
  const int r0 = (int)r0l, r1 = (int)min((long)nrows, r0l + SO_ROWS_PER_WAVE);
  const int e0 = rowptr[r0], e1 = rowptr[r1];
  const int per = (e1 - e0 + G - 1) / G;                       // entries of a piece
  const int gs = (int)min((long)e1, (long)e0 + (long)g * per), ge = (int)min((long)e1, (long)gs + per);
  if (gs >= ge) return;                                        // (no shuffle leaves the group: a group may leave alone)
  int r = r0;
  while (rowptr[r + 1] <= gs) ++r;                             // the row of the piece's first entry (gs < e1: r < r1)
  const int c = sub * CPL;                                     // this lane's first column of a chunk
  double wr[CPL];
  if (!MULTI) {
    for (int q = 0; q < CPL; ++q) wr[q] = (w != nullptr && c + q < k) ? w[c + q] : 1.0;
  }
  double keep = 0.0;
  for (int a = gs; a < ge; ++r) {
    const int b = min(rowptr[r + 1], ge);
    if (b <= a) continue;                                      // an empty row
    const double* __restrict__ urow = u + (size_t)r * ldu;
    double ur[CPL];
    if (!MULTI) {
      so_load<CPL>(urow, c, k, ur);
      for (int q = 0; q < CPL; ++q) ur[q] *= wr[q];
    }
    for (; a < b; a += SO_UNROLL) {
      int col[SO_UNROLL];
      double s[SO_UNROLL];
#pragma unroll
      for (int t = 0; t < SO_UNROLL; ++t) col[t] = a + t < b ? colidx[a + t] : -1;
      if (!MULTI) {
        double vr[SO_UNROLL][CPL];
#pragma unroll
        for (int t = 0; t < SO_UNROLL; ++t) {
          if (col[t] >= 0) so_load<CPL>(v + (size_t)col[t] * ldv, c, k, vr[t]);
          else for (int q = 0; q < CPL; ++q) vr[t][q] = 0.0;
        }
#pragma unroll
        for (int t = 0; t < SO_UNROLL; ++t) {
          s[t] = ur[0] * vr[t][0];
          if (CPL == 2) s[t] += ur[CPL - 1] * vr[t][CPL - 1];
        }
      } else {
#pragma unroll
        for (int t = 0; t < SO_UNROLL; ++t) s[t] = 0.0;
        for (int c0 = 0; c0 < k; c0 += CW) {
          double uc[CPL];
          so_load<CPL>(urow, c0 + c, k, uc);
          if (w != nullptr)
            for (int q = 0; q < CPL; ++q) uc[q] *= c0 + c + q < k ? w[c0 + c + q] : 1.0;
#pragma unroll
          for (int t = 0; t < SO_UNROLL; ++t) {
            if (col[t] < 0) continue;
            double vc[CPL];
            so_load<CPL>(v + (size_t)col[t] * ldv, c0 + c, k, vc);
            for (int q = 0; q < CPL; ++q) s[t] += uc[q] * vc[q];
          }
        }
      }
#pragma unroll
      for (int t = 0; t < SO_UNROLL; ++t) {
        if (a + t >= b) break;                                 // (the same in every lane of the group)
#pragma unroll
        for (int off = LPE / 2; off > 0; off >>= 1) s[t] += __shfl_xor(s[t], off, 64);
        const int e = a + t, slot = (e - gs) & (LPE - 1);
        if (sub == slot) keep = alpha * s[t];
        if (slot == LPE - 1 || e == ge - 1) {
          if (sub <= slot) out[(size_t)(e - slot) + sub] = keep;
        }
      }
    }
    a = b;
  }
}

template <int LPE, int CPL, bool MULTI>
static void so_launch(int nrows, const int* rowptr, const int* colidx, const double* u, long ldu, const double* v, long ldv,
                      int k, const double* w, double alpha, double* out, hipStream_t st) {
  const long waves = ((long)nrows + SO_ROWS_PER_WAVE - 1) / SO_ROWS_PER_WAVE;
  const unsigned grid = (unsigned)((waves + 3) / 4);
  hipLaunchKernelGGL((sample_outer<LPE, CPL, MULTI>), dim3(grid), dim3(256), 0, st, nrows, rowptr, colidx, u, (size_t)ldu, v,
                     (size_t)ldv, k, w, alpha, out);
}

template <int CPL>
static void so_dispatch(int nrows, const int* rowptr, const int* colidx, const double* u, long ldu, const double* v, long ldv,
                        int k, const double* w, double alpha, double* out, hipStream_t st) {
  const int need = (k + CPL - 1) / CPL;                        // lanes that hold a column
#define GCGE_SO(L, M) so_launch<L, CPL, M>(nrows, rowptr, colidx, u, ldu, v, ldv, k, w, alpha, out, st)
  if (need > 64) GCGE_SO(64, true);
  else if (need > 32) GCGE_SO(64, false);
  else if (need > 16) GCGE_SO(32, false);
  else if (need > 8) GCGE_SO(16, false);
  else if (need > 4) GCGE_SO(8, false);
  else if (need > 2) GCGE_SO(4, false);
  else if (need > 1) GCGE_SO(2, false);
  else GCGE_SO(1, false);
#undef GCGE_SO
}

}  // namespace gcge

// C-ABI: see include/gcge_hip.h.
extern "C" int gcge_hip_csr_sample_outer(int nrows, const int* d_rowptr, const int* d_colidx, const double* d_u, long ldu,
                                         const double* d_v, long ldv, int k, const double* d_w, double alpha, double* d_out,
                                         void* stream) {
  if (nrows < 0 || k < 1 || ldu < k || ldv < k) return -1;
  if (nrows == 0) return 0;
  if (d_rowptr == nullptr || d_colidx == nullptr || d_u == nullptr || d_v == nullptr || d_out == nullptr) return -1;
  gcge_hip_apply_pending();
  hipStream_t st = (hipStream_t)stream;
  const bool vec2 = ((ldu | ldv) % 2 == 0) && (((uintptr_t)d_u | (uintptr_t)d_v) % 16 == 0);
  if (vec2) gcge::so_dispatch<2>(nrows, d_rowptr, d_colidx, d_u, ldu, d_v, ldv, k, d_w, alpha, d_out, st);
  else gcge::so_dispatch<1>(nrows, d_rowptr, d_colidx, d_u, ldu, d_v, ldv, k, d_w, alpha, d_out, st);
  return (int)hipGetLastError();
}
