// K5 — block conjugate gradients with the vector work fused on the device.
//
// Same recurrence, stopping rules and per-column retirement as the reference's BlockPCG (src/ops_lin_sol.c:140-437) — every
// right-hand side has its own alpha, beta, rho and leaves the iteration on its own — but instead of ~3 b single-column
// MultiVecAxpby calls + 2 inner products per iteration (13 block streams + the SpMM) an iteration is a few
// launches on whole blocks.  Retired columns get alpha = 0 / a keep-flag, so their x, r, p stay bit for bit untouched, as if
// they had been skipped.  A call is planned once (CgPlan, cg_plan) and then runs ONE of three loops:
//
// 1. Device-scalar loop (cg_loop_device_scalars) — the default.  alpha, beta, rho, the stopping test and the active flags stay
//    on the device (cg_scalars_a / cg_scalars_b); the host only learns, one iteration late, how many columns are still active.
//    Taken when the four blocks can be walked with 16-byte lanes (even width, even column origins and leading dimensions, at
//    most 512 columns: the "one-pass scheme"), there is no shift, the transport over ranks is native (or there is none), the
//    solver was set up for at most 4000 iterations, GCGE_CG_HOST_SCALARS is unset, and the matrix has one of two forms:
//    * recompute form (pattern matrices in chain + line-exchange layout, a ring of directions): w = A p is never stored.
//        pass 1: pTw_j, wTw_j from one read of p                      (spmm_pattern.hip MODE 2, gcge_hip_cg_pass1_dev)
//        pass 2: w rebuilt in the SpMM kernel's registers, r -= alpha_j w ; p' = r + beta_j p ; rho_j
//                (reads p, r; writes r, p' into the next ring slot)   (MODE 3, gcge_hip_cg_pass2_dev)
//      x is brought up to date from the ring every J = R - 1 iterations (cg_accum_x, J + 2 streams): 1 + 4 + 1.1 = 6.1 block
//      streams per iteration with the ring of 16.  Without a stored residual (below) pass 2 reads p_k, p_{k-1} and writes
//      p_{k+1} (MODE 7, gcge_hip_cg_pass2i_dev): 3 streams instead of 4, 5.1 per iteration.
//    * stored product (matrices without a pattern form; GCGE_CG_STORED_HOST unset, a ring of >= 2 slots, operands
//      gcge_hip_spmm_dot2_dev takes): the SpMM with both column sums in its epilogue (2 streams), then one sweep
//      cg_update_rp (w, r, p_k in; r, p_{k+1} out: 5 streams) or, without a stored residual, cg_update_p_implicit (4), and
//      the same x flush: 2 + 5 + 1.1, or 2 + 4 + 1.1.
//    beta_j = rho_pred_j / rho_j with rho_pred = alpha^2 wTw - rho (what r_new . r_new is in exact arithmetic for CG
//    directions); the measured rho_j of the sweep drives the next alpha and the stopping test.
//    The residual is not stored — r_k = p_k - beta_{k-1} p_{k-1} is rebuilt from the two directions the ring holds — where
//    the ring has >= 3 slots and the stopping rule is loose (rate >= 1e-4 within <= 100 iterations; gcge_hip_bpcg_residual_form
//    overrides either way).  With the recompute form the start sweep then stores p0 alone (3 streams instead of 4).
//
// 2. Host-scalar loop (cg_loop_host_scalars) — the one-pass scheme with the b scalars of an iteration on the host, as in the
//    reference (two tiny device->host reads per iteration, which is also where the cross-rank all-reduce of
//    ops_lin_sol.c:317,365 happens).  Taken by one-pass operands that loop 1 does not take: a shift, a callback transport
//    (torch.distributed rehearsals), more than 4000 iterations, GCGE_CG_HOST_SCALARS / GCGE_CG_STORED_HOST, no ring.
//    Same kernels: recompute form 1 + 4 + 1.1 (gcge_hip_cg_pass1_mv / pass2_mv, residual always stored); stored product with
//    a ring 2 + 5 (cg_update_rp) or 2 + 4 (cg_update_p_implicit) + 1.1; without a ring (memory short, fewer than 3
//    iterations) x is updated in every sweep: cg_update_all, 4 reads + 3 writes = 7 block streams + the SpMM.
//
// 3. Two-sweep loop (cg_loop_two_sweeps) — the fallback when a block cannot be walked with 16-byte lanes (odd widths, odd
//    column origins, more than 512 columns).  It needs no prediction of rho:
//        x += alpha'_j p ; p = r + beta_j p       (cg_update_xp: the x update of the PREVIOUS step is deferred into this pass:
//                                                  3 reads + 2 writes)
//        w = A p ; pTw_j = p_j . w_j
//        r -= alpha_j w ; rho_j = r_j . r_j       (cg_update_r: 2 reads + 1 write)
//    8 block streams + the SpMM, scalars on the host.
//
// The start r = b - A x, p0 = r, rho (cg_start) is one sweep on pattern matrices (MODE 5; MODE 6 from the scale factors of
// b = x diag(scale), GCGE_LINSOL_ARGS.rhs_scale), product + one sweep (cg_start_scaled_stored: 4 streams instead of 10) for
// scale factors on a stored product, and product, axpby, column sums, copy otherwise.  tol_type "rel" needs |b|: b is formed.
//
// A shift published by the caller (GCGE_LINSOL_ARGS: our GCG does it for -gcge_compW_cg_shift, the
// reference leaves sigma to a user-defined solver, ops_eig_sol_gcg.c:584-618) turns the operator into
// A + sigma B (second SpMM + axpy per application; B == NULL: + sigma I).
//
// Installed as ops->MultiLinearSolver by gcge_hip_bpcg_setup(); GCG calls it through
// the reference's user_defined_multi_linear_solver = 1 hook (ops_eig_sol_gcg.c:584-618).
#include <hip/hip_runtime.h>
#include <assert.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "gcge_hip.h"
#include "gcge_hip_internal.h"

namespace gcge {

// x_j += aprev_j p_j (flag bit 2: deferred x update of the previous step), then
// p_j = r_j (flag bits 0-1 == 2, first step) or p_j = r_j + beta_j p_j (== 1); 0: p untouched
__global__ __launch_bounds__(256) void cg_update_xp(long nrows, const double* __restrict__ r, long ldr,
    double* __restrict__ p, long ldp, double* __restrict__ x, long ldx, int m, const double* __restrict__ beta,
    const double* __restrict__ aprev, const int* __restrict__ flag) {
  const long total = nrows * (long)m;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; idx < total; idx += stride) {
    const long row = idx / m;
    const int j = (int)(idx - row * m);
    const int f = flag[j];
    if (f == 0) continue;
    double* pp = p + row * ldp + j;
    double pv = 0.0;
    if ((f & 4) || (f & 3) == 1) pv = *pp;
    if (f & 4) { double* px = x + row * ldx + j; *px = fma(aprev[j], pv, *px); }
    if ((f & 3) == 2) *pp = r[row * ldr + j];
    else if ((f & 3) == 1) *pp = fma(beta[j], pv, r[row * ldr + j]);
  }
}

// r_j -= alpha_j w_j (flagged columns) ; partial[b*m + j] = sum_rows r_j^2
__global__ __launch_bounds__(256) void cg_update_r(long nrows, const double* __restrict__ w, long ldw,
    double* __restrict__ r, long ldr, int m, const double* __restrict__ alpha, const int* __restrict__ flag,
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
        const double rv = fma(-a, w[row * ldw + j], r[row * ldr + j]);
        r[row * ldr + j] = rv;
        s = fma(rv, rv, s);
      }
    }
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && j < m)
      partial[(long)blockIdx.x * m + j] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
    __syncthreads();
  }
}

typedef double v2d __attribute__((ext_vector_type(2)));

// ---- one-pass step -------------------------------------------------------------------------------------------
// r -= alpha w ; x += alpha p ; p = r_new + beta p ; partial[b*m + j] = sum over the block's rows of r_new^2
// in ONE sweep (4 reads + 3 writes instead of the 5 + 3 streams of the two kernels above).  beta = rho_new / rho
// is needed before r_new exists, so the caller predicts rho_new = alpha^2 (w.w) - rho from the column sums the
// SpMM kernel delivers for free (exact in exact arithmetic: r_new.r_new = rho - 2 alpha r.w + alpha^2 w.w and
// r.w = p.w = rho / alpha for CG directions); the TRUE rho_new comes back from this sweep and is what the next
// alpha and the stopping test use.  Retired columns: alpha = 0, (cr, cb) = (0, 1): r, x, p stay bit-identical.
template <int UNR>
__global__ __launch_bounds__(256) void cg_update_all(long nrows, const double* __restrict__ w, long ldw,
    double* __restrict__ r, long ldr, double* __restrict__ p, long ldp, double* __restrict__ x, long ldx, int m,
    const double* __restrict__ alpha, const double* __restrict__ beta, const int* __restrict__ flag,
    double* __restrict__ partial, int tpr) {
  __shared__ double red[256][2];
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  double s0 = 0.0, s1 = 0.0;
  const bool mine = j < m;
  const int f0 = mine ? flag[j] : 0, f1 = mine ? flag[j + 1] : 0;
  if (mine && (f0 | f1)) {
    const double a0 = f0 ? alpha[j] : 0.0, a1 = f1 ? alpha[j + 1] : 0.0;
    const double cr0 = f0 ? 1.0 : 0.0, cr1 = f1 ? 1.0 : 0.0;
    const double cb0 = f0 ? beta[j] : 1.0, cb1 = f1 ? beta[j + 1] : 1.0;
    const long step = rpb, group = (long)rpb * UNR;
    const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + group - 1) / group * group;
    const long rend = min(nrows, ((long)blockIdx.x + 1) * slab);
    auto one = [&](long rr, v2d wv, v2d rv, v2d pv, v2d xv) {
      v2d rn = {fma(-a0, wv.x, rv.x), fma(-a1, wv.y, rv.y)};
      v2d xn = {fma(a0, pv.x, xv.x), fma(a1, pv.y, xv.y)};
      v2d pn = {fma(cb0, pv.x, cr0 * rn.x), fma(cb1, pv.y, cr1 * rn.y)};
      __builtin_nontemporal_store(rn, reinterpret_cast<v2d*>(r + rr * ldr + j));
      __builtin_nontemporal_store(xn, reinterpret_cast<v2d*>(x + rr * ldx + j));
      __builtin_nontemporal_store(pn, reinterpret_cast<v2d*>(p + rr * ldp + j));
      s0 = fma(cr0 * rn.x, rn.x, s0); s1 = fma(cr1 * rn.y, rn.y, s1);
    };
    long row = (long)blockIdx.x * slab + ty;
    for (; row + (UNR - 1) * step < rend; row += step * UNR) {
      v2d wv[UNR], rv[UNR], pv[UNR], xv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const long rr = row + u * step;
        wv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(w + rr * ldw + j));
        rv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(r + rr * ldr + j));
        pv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p + rr * ldp + j));
        xv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(x + rr * ldx + j));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(row + u * step, wv[u], rv[u], pv[u], xv[u]);
    }
    for (; row < rend; row += step)
      one(row, *reinterpret_cast<const v2d*>(w + row * ldw + j), *reinterpret_cast<const v2d*>(r + row * ldr + j),
          *reinterpret_cast<const v2d*>(p + row * ldp + j), *reinterpret_cast<const v2d*>(x + row * ldx + j));
  }
  red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1;
  __syncthreads();
  if (ty == 0 && mine) {
    for (int q = 1; q < rpb; ++q) { s0 += red[q * tpr + tx][0]; s1 += red[q * tpr + tx][1]; }
    partial[(long)blockIdx.x * m + j] = s0;
    partial[(long)blockIdx.x * m + j + 1] = s1;
  }
}

// ---- p-ring variant of the one-pass step ------------------------------------------------------------------------
// x is only needed when the solve ends, but x += alpha p costs a read and a write of a whole block in every
// iteration (2 of the 7 streams).  With memory to spare the directions are kept instead: iteration k reads p_k from
// ring slot k and writes p_{k+1} to slot k+1 (5 streams: w, r, p_k in; r, p_{k+1} out), and every J iterations one
// sweep adds the J pending terms to x (J + 2 streams).  J = 15: 6.1 streams per iteration instead of 7.
template <int UNR>
__global__ __launch_bounds__(256) void cg_update_rp(long nrows, const double* __restrict__ w, long ldw,
    double* __restrict__ r, long ldr, const double* __restrict__ pold, double* __restrict__ pnew, long ldp, int m,
    const double* __restrict__ alpha, const double* __restrict__ beta, const int* __restrict__ flag,
    double* __restrict__ partial, int tpr) {
  __shared__ double red[256][2];
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  double s0 = 0.0, s1 = 0.0;
  const bool mine = j < m;
  const int f0 = mine ? flag[j] : 0, f1 = mine ? flag[j + 1] : 0;
  if (mine) {   // retired columns are still COPIED to the next slot (alpha = 0, cr = 0, cb = 1): the ring must stay complete
    const double a0 = f0 ? alpha[j] : 0.0, a1 = f1 ? alpha[j + 1] : 0.0;
    const double cr0 = f0 ? 1.0 : 0.0, cr1 = f1 ? 1.0 : 0.0;
    const double cb0 = f0 ? beta[j] : 1.0, cb1 = f1 ? beta[j + 1] : 1.0;
    const long step = rpb, group = (long)rpb * UNR;
    const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + group - 1) / group * group;
    const long rend = min(nrows, ((long)blockIdx.x + 1) * slab);
    auto one = [&](long rr, v2d wv, v2d rv, v2d pv) {
      v2d rn = {fma(-a0, wv.x, rv.x), fma(-a1, wv.y, rv.y)};
      v2d pn = {fma(cb0, pv.x, cr0 * rn.x), fma(cb1, pv.y, cr1 * rn.y)};
      __builtin_nontemporal_store(rn, reinterpret_cast<v2d*>(r + rr * ldr + j));
      __builtin_nontemporal_store(pn, reinterpret_cast<v2d*>(pnew + rr * ldp + j));
      s0 = fma(cr0 * rn.x, rn.x, s0); s1 = fma(cr1 * rn.y, rn.y, s1);
    };
    long row = (long)blockIdx.x * slab + ty;
    for (; row + (UNR - 1) * step < rend; row += step * UNR) {
      v2d wv[UNR], rv[UNR], pv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const long rr = row + u * step;
        wv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(w + rr * ldw + j));
        rv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(r + rr * ldr + j));
        pv[u] = *reinterpret_cast<const v2d*>(pold + rr * ldp + j);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(row + u * step, wv[u], rv[u], pv[u]);
    }
    for (; row < rend; row += step)
      one(row, *reinterpret_cast<const v2d*>(w + row * ldw + j), *reinterpret_cast<const v2d*>(r + row * ldr + j),
          *reinterpret_cast<const v2d*>(pold + row * ldp + j));
  }
  red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1;
  __syncthreads();
  if (ty == 0 && mine) {
    for (int q = 1; q < rpb; ++q) { s0 += red[q * tpr + tx][0]; s1 += red[q * tpr + tx][1]; }
    partial[(long)blockIdx.x * m + j] = s0;
    partial[(long)blockIdx.x * m + j + 1] = s1;
  }
}

// The same step without a stored residual (ring of >= 3 slots): r_k = p_k - beta_{k-1} p_{k-1} is rebuilt from the two directions
// the ring holds, so the sweep reads w, p_k, p_{k-1} and writes p_{k+1} — 4 streams instead of 5.  bprev = 0 in the first
// iteration and after a restart (p_k = r_k); retired columns are copied to the next slot.  The rebuilt residual carries an error
// of eps |p| instead of eps |r|: only where the stopping rule is loose (cg_plan: rate >= 1e-4, <= 100 iterations).
template <int UNR>
__global__ __launch_bounds__(256) void cg_update_p_implicit(long nrows, const double* __restrict__ w, long ldw,
    const double* __restrict__ pprev, const double* __restrict__ pold, double* __restrict__ pnew, long ldp, int m,
    const double* __restrict__ alpha, const double* __restrict__ beta, const double* __restrict__ bprev, const int* __restrict__ flag,
    double* __restrict__ partial, int tpr) {
  __shared__ double red[256][2];
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  double s0 = 0.0, s1 = 0.0;
  const bool mine = j < m;
  const int f0 = mine ? flag[j] : 0, f1 = mine ? flag[j + 1] : 0;
  if (mine) {
    const double a0 = f0 ? alpha[j] : 0.0, a1 = f1 ? alpha[j + 1] : 0.0;
    const double cr0 = f0 ? 1.0 : 0.0, cr1 = f1 ? 1.0 : 0.0;
    const double cb0 = f0 ? beta[j] : 1.0, cb1 = f1 ? beta[j + 1] : 1.0;
    const double bp0 = f0 ? bprev[j] : 0.0, bp1 = f1 ? bprev[j + 1] : 0.0;
    const long step = rpb, group = (long)rpb * UNR;
    const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + group - 1) / group * group;
    const long rend = min(nrows, ((long)blockIdx.x + 1) * slab);
    auto one = [&](long rr, v2d wv, v2d qv, v2d pv) {
      v2d rn = {fma(-a0, wv.x, fma(-bp0, qv.x, pv.x)), fma(-a1, wv.y, fma(-bp1, qv.y, pv.y))};
      v2d pn = {fma(cb0, pv.x, cr0 * rn.x), fma(cb1, pv.y, cr1 * rn.y)};
      __builtin_nontemporal_store(pn, reinterpret_cast<v2d*>(pnew + rr * ldp + j));
      s0 = fma(cr0 * rn.x, rn.x, s0); s1 = fma(cr1 * rn.y, rn.y, s1);
    };
    long row = (long)blockIdx.x * slab + ty;
    for (; row + (UNR - 1) * step < rend; row += step * UNR) {
      v2d wv[UNR], qv[UNR], pv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const long rr = row + u * step;
        wv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(w + rr * ldw + j));
        qv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(pprev + rr * ldp + j));
        pv[u] = *reinterpret_cast<const v2d*>(pold + rr * ldp + j);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(row + u * step, wv[u], qv[u], pv[u]);
    }
    for (; row < rend; row += step)
      one(row, *reinterpret_cast<const v2d*>(w + row * ldw + j), *reinterpret_cast<const v2d*>(pprev + row * ldp + j),
          *reinterpret_cast<const v2d*>(pold + row * ldp + j));
  }
  red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1;
  __syncthreads();
  if (ty == 0 && mine) {
    for (int q = 1; q < rpb; ++q) { s0 += red[q * tpr + tx][0]; s1 += red[q * tpr + tx][1]; }
    partial[(long)blockIdx.x * m + j] = s0;
    partial[(long)blockIdx.x * m + j + 1] = s1;
  }
}

// Start of a solve whose right-hand sides are b = x diag(scale) (GCGE_LINSOL_ARGS.rhs_scale) on a matrix whose product is stored:
// after w = A x, ONE sweep forms r = x diag(scale) - w, writes it as r and as p0 and sums r.r per column — instead of copying x to b,
// scaling b, r = b - w, the column sums and the copy p0 = r (10 block streams; here 4).
template <int UNR>
__global__ __launch_bounds__(256) void cg_start_scaled_stored(long nrows, const double* __restrict__ x, long ldx, const double* __restrict__ w,
    long ldw, double* __restrict__ r, long ldr, double* __restrict__ p0, long ldp, int m, const double* __restrict__ scale,
    double* __restrict__ partial, int tpr) {
  __shared__ double red[256][2];
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  double s0 = 0.0, s1 = 0.0;
  const bool mine = j < m;
  if (mine) {
    const double c0 = scale[j], c1 = scale[j + 1];
    const long step = rpb, group = (long)rpb * UNR;
    const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + group - 1) / group * group;
    const long rend = min(nrows, ((long)blockIdx.x + 1) * slab);
    auto one = [&](long rr, v2d xv, v2d wv) {
#pragma clang fp contract(off)
      v2d rn = {c0 * xv.x - wv.x, c1 * xv.y - wv.y};                   // rounded like the column scaling followed by the subtraction
      __builtin_nontemporal_store(rn, reinterpret_cast<v2d*>(r + rr * ldr + j));
      __builtin_nontemporal_store(rn, reinterpret_cast<v2d*>(p0 + rr * ldp + j));
      s0 = fma(rn.x, rn.x, s0); s1 = fma(rn.y, rn.y, s1);
    };
    long row = (long)blockIdx.x * slab + ty;
    for (; row + (UNR - 1) * step < rend; row += step * UNR) {
      v2d xv[UNR], wv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const long rr = row + u * step;
        xv[u] = *reinterpret_cast<const v2d*>(x + rr * ldx + j);
        wv[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(w + rr * ldw + j));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(row + u * step, xv[u], wv[u]);
    }
    for (; row < rend; row += step)
      one(row, *reinterpret_cast<const v2d*>(x + row * ldx + j), *reinterpret_cast<const v2d*>(w + row * ldw + j));
  }
  red[threadIdx.x][0] = s0; red[threadIdx.x][1] = s1;
  __syncthreads();
  if (ty == 0 && mine) {
    for (int q = 1; q < rpb; ++q) { s0 += red[q * tpr + tx][0]; s1 += red[q * tpr + tx][1]; }
    partial[(long)blockIdx.x * m + j] = s0;
    partial[(long)blockIdx.x * m + j + 1] = s1;
  }
}

struct RingPtrs { const double* p[16]; };
// x[:, j] = xsrc[:, j] + sum_{q < cnt} coef[q * m + j] * ring[q][:, j]      (cnt <= 16)
// xsrc: the x the terms are added to — x itself, or, in the first flush of a call whose initial guess lies elsewhere
// (GCGE_LINSOL_ARGS.x_src), those columns, which are only read (cnt == 0: a plain copy)
__global__ __launch_bounds__(256) void cg_accum_x(long nrows, RingPtrs ring, int cnt, long ldp, const double* xsrc, long ldxs, double* x,
    long ldx, int m, const double* __restrict__ coef, int tpr) {
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  const int j = 2 * tx;
  if (j >= m) return;
  const long slab = (((nrows + gridDim.x - 1) / gridDim.x) + rpb - 1) / rpb * rpb;
  const long rend = min(nrows, ((long)blockIdx.x + 1) * slab);
  for (long row = (long)blockIdx.x * slab + ty; row < rend; row += rpb) {
    v2d xv = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(xsrc + row * ldxs + j));
#pragma unroll 4
    for (int q = 0; q < cnt; ++q) {
      const v2d pv = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(ring.p[q] + row * ldp + j));
      xv.x = fma(coef[q * m + j], pv.x, xv.x); xv.y = fma(coef[q * m + j + 1], pv.y, xv.y);
    }
    __builtin_nontemporal_store(xv, reinterpret_cast<v2d*>(x + row * ldx + j));
  }
}

// ---- the scalars of an iteration on the device (recompute form) ---------------------------------------------------
// alpha_j = rho_j / (p_j . A p_j); beta_j = rho_pred_j / rho_j with rho_pred = alpha^2 |A p|^2 - rho (clamped at 0: the
// column restarts from r); retired columns get flag 0 / alpha 0 so the passes leave them bit-for-bit untouched.
// ahist: this iteration's row of the pending-x-update coefficients (cg_accum_x).
__global__ __launch_bounds__(256) void cg_scalars_a(int m, const double* __restrict__ rho2, const double* __restrict__ pw_ww,
    const int* __restrict__ active, double* __restrict__ alpha, double* __restrict__ beta, int* __restrict__ flag,
    double* __restrict__ ahist) {
  for (int j = threadIdx.x; j < m; j += 256) {
    double al = 0.0, be = 0.0; int fl = 0;
    if (active[j]) {
      al = rho2[j] / pw_ww[j];
      double pred = al * al * pw_ww[m + j] - rho2[j];
      if (!(pred > 0.0) || !isfinite(pred)) pred = 0.0;
      be = pred / rho2[j]; fl = 1;
    }
    alpha[j] = al; beta[j] = be; flag[j] = fl; ahist[j] = al;
  }
}
// rho_j <- measured r_j . r_j of the sweep, stopping test of src/ops_lin_sol.c:372-380 per column; the number of columns
// still active goes to nact_out (host-mapped memory: the host reads it one iteration later)
__global__ __launch_bounds__(256) void cg_scalars_b(int m, const double* __restrict__ newrho, double rate, double tol,
    const double* __restrict__ norm_b, const double* __restrict__ init_res, double* __restrict__ rho2, int* __restrict__ active,
    double* __restrict__ last_res, int* __restrict__ nact_out) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int mine = 0;
  for (int j = threadIdx.x; j < m; j += 256) {
    if (!active[j]) continue;
    const double rv = newrho[j];
    rho2[j] = rv;
    const double lr = sqrt(rv);
    last_res[j] = lr;
    const int a = (lr > rate * init_res[j]) && (lr > tol * norm_b[j]);
    active[j] = a; mine += a;
  }
  if (mine) atomicAdd(&cnt, mine);
  __syncthreads();
  if (threadIdx.x == 0) { *nact_out = cnt; __threadfence_system(); }
}
}  // namespace gcge

using namespace gcge;

// (cg_vec_ok, cg_tpr, cg_grid: gcge_hip_internal.h, shared with pcg_sweeps.hip)

static void launch_update_xp(long n, const double* r, long ldr, double* p, long ldp, double* x, long ldx, int mw,
                             const double* beta, const double* aprev, const int* flag, hipStream_t st) {
  long total = n * mw, g = (total + 255) / 256; if (g > 8192) g = 8192;
  hipLaunchKernelGGL(cg_update_xp, dim3((unsigned)g), dim3(256), 0, st, n, r, ldr, p, ldp, x, ldx, mw, beta, aprev, flag);
}
static void launch_start_scaled_stored(long n, CgGrid grid, const double* x, long ldx, const double* w, long ldw, double* r, long ldr,
                                       double* p0, long ldp, int m, const double* scale, double* part, hipStream_t st) {
  hipLaunchKernelGGL(cg_start_scaled_stored<4>, dim3((unsigned)grid.nb), dim3(256), 0, st, n, x, ldx, w, ldw, r, ldr, p0, ldp, m, scale, part,
                     cg_tpr(m));
}

// The solver's blocks for one problem shape.  A solver that alternates between systems of different size — the levels of a
// multigrid cycle (BlockAMG smooths every level with this CG) — must not rebuild its blocks and ring on every call: the set of the
// shape that is left is PARKED (up to 8 row counts) and taken out again when that shape comes back.
struct BpcgBlocks {
  void** mv_ws[4] = {};            // r, p, w (+ B p scratch when a shift with B != NULL is active), created lazily
  void** ring[17] = {}; int ring_len = 0;   // p-ring of the one-pass scheme (ring[0] aliases mv_ws[1])
  int ws_cols = 0, ws_rows = 0;
  unsigned order = 0;              // row order (mat_upload.hip "row orders") of the blocks: they were created like the x block of that call
};
struct HipBpcg {
  int max_iter = 30; double rate = 1e-2, tol = 1e-14; char tol_type[8] = "abs";
  BpcgBlocks blk;                  // the blocks of the shape the last call had
  int niter = 0; double residual = -1.0;
  long spmm_calls = 0, spmm_cols = 0;   // statistics for bench.py
  double* d_coef = nullptr; int* d_flag = nullptr; double* h_pin = nullptr; int cap = 0;
  long recompute_iters = 0;        // iterations run in the two-pass form with the product recomputed (pattern matrices)
  long col_iters = 0, active_col_iters = 0;   // columns streamed per iteration, summed / of which still active (one-pass scheme)
  long total_iters = 0; double total_seconds = 0.0;   // CG iterations and host wall time over all calls (bench.py: ms per CG iteration)
  double* d_sc = nullptr; int* d_sci = nullptr; int* h_nact = nullptr; int sc_cap = 0; hipEvent_t ev_it[2] = {};   // device-side scalars
  long dev_scalar_iters = 0;
  long implicit_r_iters = 0;       // iterations that rebuilt r from two directions (no stored residual)
  long stored_dev_iters = 0;       // iterations of the device-scalar loop with the product stored (matrices without a pattern form)
  long legacy_start_sums = 0;      // one-sweep starts whose |r|^2 was summed again by the column-dot kernel (right-hand sides moved off an odd column)
  long fused_starts = 0;           // solves started by product + one sweep (cg_start_scaled_stored)
  long surplus_iters = 0;          // iterations enqueued after the last column had retired (no-ops on the data, but they stream)
  long trimmed_iters = 0;          // last iterations of the device-scalar loop whose second pass ran over fewer columns or not at all
  long starts_in_place = 0, starts_materialised = 0;   // calls with the initial guess elsewhere (args.x_src): started from it in one sweep / copied first
};
static HipBpcg g_bpcg;

static int g_residual_form = 0;   // 0 automatic, 1 never stored (rebuilt from two directions), 2 always stored
extern "C" void gcge_hip_bpcg_residual_form(int form) { g_residual_form = form; }

static void reduce_over_ranks(double* v, int n) {
  GCGE_COMM* c = GCGE_GetComm();
  if (c != nullptr && n > 0) c->allreduce_sum(v, n, c->ctx);
}

static BpcgBlocks g_parked[8]; static int g_nparked = 0;
static void bpcg_destroy_set(BpcgBlocks* q, struct OPS_* ops) {
  for (int i = 1; i < q->ring_len; ++i) if (q->ring[i]) ops->MultiVecDestroy(&q->ring[i], q->ws_cols, ops);
  for (int i = 0; i < 4; ++i) if (q->mv_ws[i]) ops->MultiVecDestroy(&q->mv_ws[i], q->ws_cols, ops);
  *q = BpcgBlocks();
}
static void bpcg_unpark(int i) {   // entry i leaves the list (its blocks are the caller's now, or destroyed)
  for (--g_nparked; i < g_nparked; ++i) g_parked[i] = g_parked[i + 1];
}
// r, p, w (and the shift's scratch block on demand) for this problem shape.  A change of the column count within a shape drops that
// shape's ring.
static void bpcg_shape(HipBpcg* s, int n, int nrhs, void** mv_x, struct OPS_* ops) {
  BpcgBlocks& k = s->blk;
  const unsigned order = gcge_hip_mv_row_order_id(mv_x);
  if (k.ws_cols >= nrhs && k.ws_rows == n && k.order == order) return;
  if (k.ws_rows == n && k.order != order && k.mv_ws[0] != nullptr) bpcg_destroy_set(&k, ops);   // same size, another row order: the blocks belong to the other matrix
  if (k.ws_rows != n) {
    if (k.ws_rows > 0 && k.mv_ws[0] != nullptr) {          // park the current set
      if (g_nparked == 8) { bpcg_destroy_set(&g_parked[0], ops); bpcg_unpark(0); }
      g_parked[g_nparked++] = k;
      k = BpcgBlocks();
    }
    for (int i = 0; i < g_nparked; ++i) if (g_parked[i].ws_rows == n && g_parked[i].order != order) {   // parked for another row order: gone
      bpcg_destroy_set(&g_parked[i], ops);
      bpcg_unpark(i); --i;
    }
    for (int i = 0; i < g_nparked; ++i) if (g_parked[i].ws_rows == n) {     // a parked set of this row count comes back
      k = g_parked[i];
      bpcg_unpark(i);
      break;
    }
    if (k.ws_cols >= nrhs && k.ws_rows == n) return;
  }
  for (int i = 1; i < k.ring_len; ++i) if (k.ring[i]) ops->MultiVecDestroy(&k.ring[i], k.ws_cols, ops);
  k.ring_len = 0;
  for (int i = 0; i < 4; ++i) {
    if (k.mv_ws[i]) ops->MultiVecDestroy(&k.mv_ws[i], k.ws_cols, ops);
    if (i < 3) ops->MultiVecCreateByMultiVec(&k.mv_ws[i], nrhs, mv_x, ops);
  }
  k.ws_cols = nrhs; k.ws_rows = n; k.order = order;
}
static void bpcg_ring(HipBpcg* s, void* mat, void** mv_x, double sigma, struct OPS_* ops) {
  BpcgBlocks& k = s->blk;
  long ldp = 0;
  (void)gcge_hip_mv_device_ptr(k.mv_ws[1], &ldp);
  // p-ring (see cg_update_rp): as many slots as memory allows, at most 16; fewer than 4 pending terms do not pay
  const int ring_max = getenv("GCGE_CG_RING") ? atoi(getenv("GCGE_CG_RING")) : 16;   // (read when a ring is created)
  // (a ring that was created for a solver with fewer iterations — the smoothing runs of a multigrid cycle — grows when a later
  //  set-up asks for more)
  const int have = k.ring_len > 0 ? k.ring_len - 1 : 0;
  if (s->max_iter >= 3 && have < 15 && have < s->max_iter) {   // (every rank gets here in the same call: the vote below is collective)
    size_t fr = 0, tot = 0;
    GCGE_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    fr += gcge_hip_pool_cached_bytes();   // blocks parked in the back-end's pool are available to MultiVecCreate*
    const size_t slot = (size_t)gcge_hip_mv_nrows(k.mv_ws[1]) * (size_t)ldp * sizeof(double) + ((size_t)64 << 20);
    const size_t keep = (size_t)12 << 30;   // leave room for staging, partial sums and the caller
    long want = fr > keep ? (long)((fr - keep) / slot) : 0;
    if (want > ring_max - 1) want = ring_max - 1;
    // smallest ring worth having: with the product recomputed (1 + 4 streams per iteration) even two extra slots pay —
    // x then costs (2 + 2) / 2 = 2 streams per iteration, 7 in all against 8.1 of the stored-w form; that is the case of
    // BASELINE config 4's shape, where 244 of 288 GB are taken by the solver's own blocks
    // (with the product stored — generic matrices, shifts — a ring only pays from 4 extra slots on: 2 + 5 + (J + 2) / J
    // streams against the 9 of the ring-less sweep)
    const int min_ring = (sigma == 0.0 && gcge_hip_cg_recompute_pays(mat)) ? 2 : 4;
    if (want < min_ring) want = 0;
    want += have;                                  // (slots this shape already holds are not "free memory" any more)
    if (want > ring_max - 1) want = ring_max - 1;
    if (want > s->max_iter) want = s->max_iter;
    // Row-partitioned runs: the ring length decides the column window [alo, ahi) and with it the LENGTH of the two
    // all-reduces of an iteration, so every rank must use the same one — the minimum over the ranks (free memory
    // differs between slabs cut by non-zeros and between ranks sharing a device).  GCGE_COMM only sums: rank r's
    // "can hold at least q+1 extra slots" indicators are summed, the agreed length is the count of unanimous entries.
    if (GCGE_COMM* c = GCGE_GetComm()) {
      double vote[16];
      for (int q = 0; q < 16; ++q) vote[q] = q < want ? 1.0 : 0.0;
      c->allreduce_sum(vote, 16, c->ctx);
      long agreed = 0;
      while (agreed < 16 && vote[agreed] > (double)c->size - 0.5) ++agreed;
      want = agreed;
    }
    if (k.ring_len == 0) { k.ring[0] = k.mv_ws[1]; k.ring_len = 1; }
    for (long i = have; i < want; ++i) { ops->MultiVecCreateByMultiVec(&k.ring[k.ring_len], k.ws_cols, mv_x, ops); ++k.ring_len; }
  }
}

// ---- one call ---------------------------------------------------------------------------------------------------------------
// The environment switches of DESIGN.md §4, read at every call (the tests flip them inside one process).
struct CgSwitches { bool host_scalars, stored_host, no_w_slot, no_idle_slots, no_fused_start; };
static CgSwitches cg_switches() {
  return {getenv("GCGE_CG_HOST_SCALARS") != nullptr, getenv("GCGE_CG_STORED_HOST") != nullptr, getenv("GCGE_CG_NO_W_SLOT") != nullptr,
          getenv("GCGE_CG_NO_IDLE_SLOTS") != nullptr, getenv("GCGE_CG_NO_FUSED_START") != nullptr};
}

// What a call works on: the operands, what the caller published, the solver's blocks on the device, and the host's scalars of
// the columns (the device-scalar loop uploads them once, the other two keep them current).
struct CgCall {
  HipBpcg* s; struct OPS_* ops; hipStream_t st;
  void* mat; void** mv_b; void** mv_x; int bc0, xc0;     // b and x with their first columns
  int n, nrhs;
  GCGE_LINSOL_ARGS args;                                   // (include/gcge_ops.h); operator: A, or A + sigma B when it published a shift
  CgSwitches env;
  double *dx, *dr, *dp, *dw; long ldx, ldr, ldp, ldw;      // x at its first column; r, p, w
  const double* dxs; long ldxs;                            // what the next x flush reads: x, or args.x_src until x has been written once
  bool one_pass;                                           // all four can be walked with 16-byte lanes
  CgGrid grid;
  std::vector<double> norm_b, rho1, rho2, pTw, init_res, last_res, coef;
  std::vector<int> active, flag;
  int nact;

  // y[:, ys:ys+k) = (A + sigma B) x[:, xs:xs+k); dots != NULL: dots[j] = x_j . y_j (local part), yy likewise y_j . y_j
  void apply(void** xin, int xs, void** yout, int ys, int k, double* dots, double* yy = nullptr) const {
    const double sigma = args.sigma;
    int a2[2] = {xs, ys}, b2[2] = {xs + k, ys + k};
    if (sigma == 0.0) {
      if (dots) gcge_hip_spmm_dot2_mv(mat, xin, yout, a2, b2, dots, yy, ops);
      else ops->MatDotMultiVec(mat, xin, yout, a2, b2, ops);
      return;
    }
    ops->MatDotMultiVec(mat, xin, yout, a2, b2, ops);
    if (args.matB != nullptr) {
      int a3[2] = {xs, 0}, b3[2] = {xs + k, k};
      ops->MatDotMultiVec(args.matB, xin, s->blk.mv_ws[3], a3, b3, ops);
      int a4[2] = {0, ys}, b4[2] = {k, ys + k};
      ops->MultiVecAxpby(sigma, s->blk.mv_ws[3], 1.0, yout, a4, b4, ops);
    } else {
      ops->MultiVecAxpby(sigma, xin, 1.0, yout, a2, b2, ops);
    }
    if (dots) gcge_hip_local_inner_prod('D', xin, yout, a2, b2, dots, 1, ops);
    if (yy) { int a5[2] = {ys, ys}, b5[2] = {ys + k, ys + k}; gcge_hip_local_inner_prod('D', yout, yout, a5, b5, yy, 1, ops); }
  }
  // d_coef = [c0v | c1v] (2 * cap doubles), d_flag = fl, columns [lo, lo + mw), through the pinned staging buffer
  void upload(int lo, int mw, const double* c0v, const double* c1v, const int* fl) const {
    GCGE_HIP_CHECK(hipStreamSynchronize(st));
    memcpy(s->h_pin, c0v + lo, mw * sizeof(double));
    memcpy(s->h_pin + s->cap, c1v + lo, mw * sizeof(double));
    memcpy(s->h_pin + 2 * s->cap, fl + lo, mw * sizeof(int));
    GCGE_HIP_CHECK(hipMemcpyAsync(s->d_coef, s->h_pin, mw * sizeof(double), hipMemcpyHostToDevice, st));
    GCGE_HIP_CHECK(hipMemcpyAsync(s->d_coef + s->cap, s->h_pin + s->cap, mw * sizeof(double), hipMemcpyHostToDevice, st));
    GCGE_HIP_CHECK(hipMemcpyAsync(s->d_flag, s->h_pin + 2 * s->cap, mw * sizeof(int), hipMemcpyHostToDevice, st));
  }
  // the sums a sweep left in part[0 .. nb * m) come back summed over the workgroups and the ranks
  void partial_sums_to_host(double* part, int m, double* out) const {
    gcge_hip_reduce_partials(part, (int)grid.nb, m, part + (size_t)grid.nb * m, st);
    GCGE_HIP_CHECK(hipMemcpyAsync(s->h_pin, part + (size_t)grid.nb * m, m * sizeof(double), hipMemcpyDeviceToHost, st));
    GCGE_HIP_CHECK(hipStreamSynchronize(st));
    memcpy(out, s->h_pin, m * sizeof(double));
    reduce_over_ranks(out, m);
  }
  // rho_j <- the sweep's measured r_j . r_j for the active columns of [alo, ahi); stopping test of src/ops_lin_sol.c:372-380
  void retire_columns(int alo, int ahi, const double* newrho) {
    nact = 0;
    for (int j = alo; j < ahi; ++j) {
      if (!active[j]) continue;
      rho1[j] = rho2[j]; rho2[j] = newrho[j - alo];
      last_res[j] = sqrt(rho2[j]);
      active[j] = (last_res[j] > s->rate * init_res[j]) && (last_res[j] > s->tol * norm_b[j]);
      nact += active[j];
    }
  }
};

enum CgLoop { CG_DEVICE_SCALARS, CG_HOST_SCALARS, CG_TWO_SWEEPS };
// Everything the call branches on, decided once (cg_plan).
struct CgPlan {
  CgLoop loop;
  bool recompute;          // one-pass scheme on a pattern matrix with a ring: the product is formed twice and never stored
  void** slots[17]; int R; // the direction slots of this call: the ring, the w block, the caller's idle blocks; 1: x is updated in every iteration
  bool stored_dev;         // stored product whose SpMM leaves its sums on the device
  bool implicit_r;         // the residual is not stored: the sweep rebuilds it from two directions
  bool start_without_r;    // ... and is never read: the one-sweep starts store p0 alone
  int last_cols;           // columns of the second pass of the last iteration the device-scalar loop can enqueue
};
// Sizes the ring (collective: every rank plans in the same call) and picks the loop.
static CgPlan cg_plan(const CgCall& c) {
  HipBpcg* s = c.s; BpcgBlocks& k = s->blk;
  const double sigma = c.args.sigma;
  CgPlan p = {};
  p.loop = CG_TWO_SWEEPS; p.R = 1; p.slots[0] = k.mv_ws[1];
  if (!c.one_pass) return p;
  bpcg_ring(s, c.mat, c.mv_x, sigma, c.ops);
  // Pattern matrices (stencils) with a ring: the product is formed twice and never stored (recompute form above).  Same recurrences,
  // same operands, so alpha, beta and the iterates agree with the stored-w form to rounding of the sums.
  const int R0 = k.ring_len >= 2 ? k.ring_len : 1;
  p.recompute = R0 > 1 && sigma == 0.0 && gcge_hip_cg_recompute_pays(c.mat) && gcge_hip_cg_fusable(c.mat, k.ring[0], c.nrhs) && !(c.nrhs & 1);
  // the slots of this call: the ring, plus the w block — which the recompute form never writes — as one more slot
  // (matters where memory is short: at BASELINE config 4's shape a ring of 3 becomes one of 4, x costs 5/3 instead of
  // 2 block streams per iteration)
  p.R = R0;
  for (int q = 0; q < R0; ++q) p.slots[q] = R0 > 1 ? k.ring[q] : k.mv_ws[1];
  if (p.recompute && p.R < 16 && !c.env.no_w_slot) p.slots[p.R++] = k.mv_ws[2];
  // ... and the blocks the caller declared idle for the duration of the solve (args.idle_blocks), where
  // they have the shape of the ring's own blocks (same rows, same leading dimension, 16-byte aligned, room for the halo)
  if (p.recompute && !c.env.no_idle_slots) {
    const int nidle = c.args.idle_blocks != nullptr ? c.args.n_idle : 0; void*** idle = c.args.idle_blocks;
    for (int q = 0; q < nidle && p.R < 16; ++q) {
      void** hb = idle[q];
      if (hb == nullptr || hb == c.mv_x || hb == c.mv_b || gcge_hip_mv_nrows(hb) != c.n || gcge_hip_mv_ncols(hb) < c.nrhs) continue;
      bool dup = false;
      for (int t = 0; t < p.R; ++t) dup |= p.slots[t] == hb;
      for (int t = 0; t < 4; ++t) dup |= k.mv_ws[t] == hb;
      long ldq = 0;
      if (dup || gcge_hip_mv_device_ptr(hb, &ldq) == nullptr || ldq != c.ldp || !gcge_hip_cg_fusable(c.mat, hb, c.nrhs)) continue;
      p.slots[p.R++] = hb;
    }
  }
  // The stored-product form (matrices without a pattern form: the plane sweep, dense blocks, pad-8; no shift) keeps its scalars on
  // the device too, from round 4 on: product + sums left on the device (gcge_hip_spmm_dot2_dev), the direction update reading
  // alpha / beta / flags where cg_scalars_a put them.  Before, every iteration made two host round trips (sums down, coefficients up,
  // new rho down): 0.6 of 6.2 ms per iteration on the SiO2-like matrix.
  // (only where gcge_hip_spmm_dot2_dev will take these operands — a row slab whose halo buffers are narrower than the
  //  block, or a slot without room for the halo rows, keeps the host-scalar loop, which chunks the columns)
  p.stored_dev = !p.recompute && p.R >= 2 && sigma == 0.0 && c.mat != nullptr && !c.env.stored_host &&
                 gcge_hip_spmm_dot2_dev_ok(c.mat, p.slots[0], k.mv_ws[2], 0, 0, c.nrhs);
  // Scalars on the device: over ranks the sums are reduced on the device by RCCL (gcge_hip_comm_allreduce_device); a callback
  // transport (torch.distributed rehearsals) keeps the host-scalar loop.  h_nact holds one count per iteration: <= 4000.
  GCGE_COMM* comm = GCGE_GetComm();
  const bool dev_scalars = (p.recompute || p.stored_dev) && !c.env.host_scalars && s->max_iter <= 4000 &&
                           (comm == nullptr || gcge_hip_comm_is_native(comm));
  p.loop = dev_scalars ? CG_DEVICE_SCALARS : CG_HOST_SCALARS;
  // The residual is not stored (gcge_hip_bpcg_residual_form(2): it is) but rebuilt from the previous direction, which the ring
  // still holds (3 slots suffice: p_{k-1}, p_k, p_{k+1}).  Same recurrence in exact arithmetic; in floating point the rebuilt r_k
  // carries a rounding error of eps |p_k| instead of eps |r_k| — immaterial for systems solved to a relative 1e-2.
  // Taken where the systems are solved to a moderate reduction (rate >= 1e-4 within <= 100 iterations: the GCG driver's
  // 1e-2 in 30); a caller asking for more keeps the stored residual — gcge_hip_bpcg_residual_form overrides
  // either way, tests/test_hip_parity.py::test_fused_cg_tight_tolerances compares the two forms down to 1e-13.
  // (the host-scalar loop's recompute passes, gcge_hip_cg_pass2_mv, only exist with a stored residual)
  p.implicit_r = p.R >= 3 && (g_residual_form == 1 || (g_residual_form == 0 && s->rate >= 1e-4 && s->max_iter <= 100)) &&
                 (dev_scalars || !p.recompute);
  // Then the block r is never read by the recompute passes, and the one-sweep starts store p0 alone (r and p0 name the same block:
  // single store, 3 block streams instead of 4 — the two smoothing calls of a V-cycle start this way).
  p.start_without_r = dev_scalars && p.recompute && p.implicit_r;
  // The last iteration the device-scalar loop can enqueue (max_iter - 1) needs its first pass and alpha — x takes alpha p from the
  // pending coefficients — but its second pass only writes p_{k+1}, which nothing reads, and measures rho_{k+1}, which only the
  // caller can read (the residual this call reports, column 0's).  A caller that reads no residual, or that of the leading
  // columns only (GCGE_LINSOL_ARGS.final_residual_cols: BlockAMG's smoothing calls), gets no second pass in that
  // iteration, or one over the 16-column passes that hold those columns: the kernel launches its column passes with the
  // same blocks and partial sums whatever the column count (spmm_pattern.hip), so their rho are the full pass's bit for bit.
  // The stored-product form has no such cut (its sweep's row split follows the column count): it skips the sweep for none.
  const int frc = c.args.final_residual_cols;
  const int fin = frc < 0 ? 0 : (frc == 0 ? c.nrhs : std::min(frc, c.nrhs));
  p.last_cols = fin == c.nrhs ? c.nrhs : (p.recompute ? std::min(c.nrhs, (fin + 15) / 16 * 16) : (fin > 0 ? c.nrhs : 0));
  return p;
}

// The scales of the stopping rule tol * scale_j (src/ops_lin_sol.c:175-197); "rel" reads the formed b.
static void cg_stopping_scales(CgCall& c) {
  HipBpcg* s = c.s;
  if (0 == strcmp(s->tol_type, "rel")) {
    int st2[2] = {c.bc0, c.bc0}, en2[2] = {c.bc0 + c.nrhs, c.bc0 + c.nrhs};
    c.ops->MultiVecInnerProd('D', c.mv_b, c.mv_b, 0, st2, en2, c.norm_b.data(), 1, c.ops);
    for (int i = 0; i < c.nrhs; ++i) c.norm_b[i] = sqrt(c.norm_b[i]);
  } else if (0 == strcmp(s->tol_type, "user")) {
    // src/ops_lin_sol.c:186-192: the caller's scales, |lambda_j + sigma| from the GCG driver (args.user_scale)
    const int nsc = c.args.user_scale != nullptr ? c.args.n_user_scale : 0;
    const double* usc = c.args.user_scale;
    if (usc == nullptr || nsc < c.nrhs) {
      fprintf(stderr, "HIP_BlockPCG: tol_type \"user\" but the caller published %d scales for %d right-hand sides "
                      "(GCGE_LINSOL_ARGS.user_scale, include/gcge_ops.h)\n", nsc, c.nrhs);
      abort();
    }
    for (int i = 0; i < c.nrhs; ++i) c.norm_b[i] = fabs(usc[i]);
  } else {
    for (int i = 0; i < c.nrhs; ++i) c.norm_b[i] = 1.0;   // "abs" (gcge_hip_bpcg_setup refuses anything else)
  }
}

extern "C" int gcge_hip_block_moves_mv(void** ritz, void** V, int x0, int x1, const int* runs, int w0, void** b, int b0, const double* scale);

// The initial guess lies in columns [x_src_col, x_src_col + nrhs) of the block args.x_src, which this call only reads; the result
// goes to mv_x, and with rhs_scale b = x_src diag(rhs_scale) is left in mv_b (GCGE_LINSOL_ARGS, include/gcge_ops.h).
// one_sweep (pattern matrix, no shift, not "rel", a ring: x is only written by the flushes) and operands the sweep takes: kernel
// MODE 8 reads x where it lies, stores r / p0 and b and sums rho — nothing is copied, the first x flush reads x_src (c.dxs).
// Returns true then (p0 in place, c.rho2 summed).  Everything else: x and b are made first, by the block-move sweep where it takes
// them and by the slots otherwise — the same bits — and the call goes on as if it had been handed them (false).
static bool cg_start_elsewhere(CgCall& c, void** start_r, bool one_sweep) {
  HipBpcg* s = c.s; BpcgBlocks& k = s->blk; struct OPS_* ops = c.ops;
  void** src = c.args.x_src; const int sc0 = c.args.x_src_col, nrhs = c.nrhs;
  const double* scale = c.args.rhs_scale;
  c.args.x_src = nullptr; c.args.x_src_col = 0;
  if (gcge_hip_mv_nrows(src) != c.n || gcge_hip_mv_row_order_id(src) != gcge_hip_mv_row_order_id(c.mv_x) || sc0 < 0 || sc0 + nrhs > gcge_hip_mv_ncols(src) ||
      (src == c.mv_x && sc0 < c.xc0 + nrhs && c.xc0 < sc0 + nrhs)) {
    fprintf(stderr, "HIP_BlockPCG: the initial guess (GCGE_LINSOL_ARGS.x_src) does not match x in shape or overlaps it\n"); abort();
  }
  long lds = 0;
  const double* ds = gcge_hip_mv_device_ptr(src, &lds);
  if (one_sweep && scale != nullptr && c.one_pass && !(lds & 1) && !((uintptr_t)(ds + sc0) & 15) &&
      gcge_hip_cg_start_scaled_b_mv(c.mat, src, sc0, scale, start_r, k.mv_ws[1], 0, nrhs, c.mv_b, c.bc0, c.rho2.data()) == 0) {
    reduce_over_ranks(c.rho2.data(), nrhs);
    c.dxs = ds + sc0; c.ldxs = lds;
    c.args.rhs_scale = nullptr;          // b is formed
    ++s->starts_in_place;
    return true;
  }
  const int runs[3] = {1, sc0, sc0 + nrhs};
  if (!(scale != nullptr && src == c.mv_x && gcge_hip_block_moves_mv(src, c.mv_x, sc0 + nrhs, sc0 + nrhs, runs, c.xc0, c.mv_b, c.bc0, scale))) {
    int st2[2] = {sc0, c.xc0}, en2[2] = {sc0 + nrhs, c.xc0 + nrhs};
    ops->MultiVecAxpby(1.0, src, 0.0, c.mv_x, st2, en2, ops);
    if (scale != nullptr) {
      st2[0] = c.xc0; en2[0] = c.xc0 + nrhs; st2[1] = c.bc0; en2[1] = c.bc0 + nrhs;
      ops->MultiVecAxpby(1.0, c.mv_x, 0.0, c.mv_b, st2, en2, ops);
      std::vector<double> sc(scale, scale + nrhs);
      ops->MultiVecLinearComb(NULL, c.mv_b, 0, st2, en2, NULL, 0, sc.data(), 1, ops);
    }
  }
  c.args.rhs_scale = nullptr;            // b is formed: an ordinary right-hand side from here on
  ++s->starts_materialised;
  return false;
}

// r = b - A x ; c.rho2 = diag(r^T r) summed over the ranks ; c.norm_b.  Returns whether p0 = r is in place as well (the one-sweep
// routes write both; without_r: they write p0 alone).
// The caller may have declared b = x diag(scale) without forming it (args.rhs_scale: our GCG driver's systems
// A w = (lambda + sigma) x, started from w = x).  The one-sweep starts then take the scale factors
// and neither read nor need b; every other route forms b first, here, on the device.
static bool cg_start(CgCall& c, bool without_r, bool ring_recompute) {
  HipBpcg* s = c.s; BpcgBlocks& k = s->blk; struct OPS_* ops = c.ops;
  const int nrhs = c.nrhs;
  const bool rel = 0 == strcmp(s->tol_type, "rel");                                     // needs |b|: b is formed
  const bool pattern = c.args.sigma == 0.0 && gcge_hip_cg_recompute_pays(c.mat);        // r, p0 and rho in one sweep (kernel MODES 5, 6, 8)
  void** start_r = without_r ? k.mv_ws[1] : k.mv_ws[0];
  bool p0_done = false;
  if (c.args.x_src != nullptr) p0_done = cg_start_elsewhere(c, start_r, !rel && pattern && ring_recompute);
  const double* rhs_scale = c.args.rhs_scale;
  if (p0_done) {
  } else if (rhs_scale != nullptr && !rel && pattern &&
      gcge_hip_cg_start_scaled_mv(c.mat, c.mv_x, c.xc0, rhs_scale, start_r, k.mv_ws[1], 0, nrhs, c.rho2.data()) == 0) {
    reduce_over_ranks(c.rho2.data(), nrhs);
    p0_done = true;
  } else if (rhs_scale != nullptr && !rel && c.args.sigma == 0.0 && c.mat != nullptr && c.one_pass && !c.env.no_fused_start) {
    // matrices whose product is stored (no pattern form): w = A x, then one sweep for r = x diag(scale) - w, p0 = r, r.r
    // (cg_start_scaled_stored: 4 block streams behind the product instead of 10)
    c.apply(c.mv_x, c.xc0, k.mv_ws[2], 0, nrhs, nullptr);
    double* part = gcge_hip_partial_ws((size_t)c.grid.nb * nrhs + nrhs);
    GCGE_HIP_CHECK(hipStreamSynchronize(c.st));          // the pinned staging may still feed an earlier upload
    memcpy(s->h_pin, rhs_scale, nrhs * sizeof(double));
    GCGE_HIP_CHECK(hipMemcpyAsync(s->d_coef, s->h_pin, nrhs * sizeof(double), hipMemcpyHostToDevice, c.st));
    launch_start_scaled_stored((long)c.n, c.grid, c.dx, c.ldx, c.dw, c.ldw, c.dr, c.ldr, c.dp, c.ldp, nrhs, s->d_coef, part, c.st);
    c.partial_sums_to_host(part, nrhs, c.rho2.data());
    p0_done = true;
    ++s->fused_starts;
  } else if (rhs_scale != nullptr) {
    int st2[2] = {c.xc0, c.bc0}, en2[2] = {c.xc0 + nrhs, c.bc0 + nrhs};
    ops->MultiVecAxpby(1.0, c.mv_x, 0.0, c.mv_b, st2, en2, ops);
    std::vector<double> sc(rhs_scale, rhs_scale + nrhs);
    ops->MultiVecLinearComb(NULL, c.mv_b, 0, st2, en2, NULL, 0, sc.data(), 1, ops);
  }
  cg_stopping_scales(c);
  if (p0_done) return true;   // started from the scale factors above
  if (pattern && gcge_hip_cg_start_mv(c.mat, c.mv_x, c.xc0, c.mv_b, c.bc0, start_r, k.mv_ws[1], 0, nrhs, c.rho2.data()) == 0) {
    // right-hand sides the driver moved off an odd column (GCGE_SetRealignedRhs): from there the sweep was declined and |r|^2 came
    // from the column-dot kernel below, in another order of the row sums.  r is the same bit for bit either way; take those sums
    // (one more read of r), so that the solve does not depend on where b lies
    int rb0 = 0;
    if (GCGE_GetRealignedRhs(&rb0) == c.mv_b && rb0 == c.bc0) {
      int st2[2] = {0, 0}, en2[2] = {nrhs, nrhs};
      ops->MultiVecInnerProd('D', start_r, start_r, 0, st2, en2, c.rho2.data(), 1, ops);
      ++s->legacy_start_sums;
    } else reduce_over_ranks(c.rho2.data(), nrhs);
    return true;
  }
  // product, axpby, column dots (and the copy p0 = r, which is the caller's)
  c.apply(c.mv_x, c.xc0, k.mv_ws[0], 0, nrhs, nullptr);
  int st2[2] = {c.bc0, 0}, en2[2] = {c.bc0 + nrhs, nrhs};
  ops->MultiVecAxpby(1.0, c.mv_b, -1.0, k.mv_ws[0], st2, en2, ops);
  st2[0] = 0; en2[0] = nrhs;
  ops->MultiVecInnerProd('D', k.mv_ws[0], k.mv_ws[0], 0, st2, en2, c.rho2.data(), 1, ops);
  return false;
}

// The pending x updates of a call with a ring: p_k lives in slots[cur]; x still lacks the terms of the npend directions from
// slots[first_slot] on.
struct CgPending { int npend = 0, first_slot = 0, cur = 0; };
static void launch_accum_x(long n, const RingPtrs& rp, int cnt, long ldp, const double* xs, long ldxs, double* x, long ldx, int m, const double* d_coef,
                           hipStream_t st) {
  const int tpr = cg_tpr(m);
  long g = (n + (256 / tpr) * 8 - 1) / ((256 / tpr) * 8); if (g > 8192) g = 8192; if (g < 1) g = 1;
  hipLaunchKernelGGL(cg_accum_x, dim3((unsigned)g), dim3(256), 0, st, n, rp, cnt, ldp, xs, ldxs, x, ldx, m, d_coef, tpr);
}
// the flush on operator-table blocks with host coefficients (include/gcge_hip.h; tests)
extern "C" int gcge_hip_cg_accum_x_mv(void** src, int sc0, void** x, int xc0, int m, void*** ring, int cnt, const double* host_coef) {
  long lds = 0, ldx = 0, ldp = 0;
  const double* ds = gcge_hip_mv_device_ptr(src, &lds);
  double* dx = gcge_hip_mv_device_ptr(x, &ldx);
  if (ds == nullptr || dx == nullptr || m <= 0 || m > 512 || cnt < 0 || cnt > 16 || (cnt > 0 && (ring == nullptr || host_coef == nullptr))) return -1;
  const int n = gcge_hip_mv_nrows(x);
  if (gcge_hip_mv_nrows(src) != n || sc0 < 0 || sc0 + m > gcge_hip_mv_ncols(src) || xc0 < 0 || xc0 + m > gcge_hip_mv_ncols(x)) return -1;
  if (!cg_vec_ok(m, {ds + sc0, dx + xc0}, {lds, ldx})) return -1;
  RingPtrs rp;
  for (int q = 0; q < 16; ++q) {
    long ldq = 0;
    void** slot = cnt > 0 ? ring[q < cnt ? q : 0] : src;
    rp.p[q] = gcge_hip_mv_device_ptr(slot, &ldq);
    if (cnt > 0 && (rp.p[q] == nullptr || gcge_hip_mv_nrows(slot) != n || gcge_hip_mv_ncols(slot) < m || (q > 0 && ldq != ldp) || !cg_vec_ok(m, {rp.p[q]}, {ldq}))) return -1;
    if (q == 0) ldp = ldq;
  }
  hipStream_t st = (hipStream_t)gcge_hip_stream();
  double* d_coef = nullptr;
  if (cnt > 0) {
    GCGE_HIP_CHECK(hipMalloc(&d_coef, (size_t)cnt * m * sizeof(double)));
    GCGE_HIP_CHECK(hipMemcpy(d_coef, host_coef, (size_t)cnt * m * sizeof(double), hipMemcpyHostToDevice));
  }
  launch_accum_x((long)n, rp, cnt, ldp, ds + sc0, lds, dx + xc0, ldx, m, d_coef, st);
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  if (d_coef != nullptr) GCGE_HIP_CHECK(hipFree(d_coef));
  return 0;
}
// x += sum over the pending directions q of p_q diag(d_coef[q * nrhs ..])  (cg_accum_x); d_coef: device memory
static void cg_flush_x(CgCall& c, const CgPlan& p, CgPending& w, const double* d_coef) {
  if (w.npend == 0 && c.dxs == c.dx) return;   // (nothing pending but x never written: a plain copy of the initial guess)
  RingPtrs rp;
  for (int q = 0; q < 16; ++q) { long ldq; rp.p[q] = gcge_hip_mv_device_ptr(p.slots[(w.first_slot + (q < w.npend ? q : 0)) % p.R], &ldq); }
  launch_accum_x((long)c.n, rp, w.npend, c.ldp, c.dxs, c.ldxs, c.dx, c.ldx, c.nrhs, d_coef, c.st);
  c.dxs = c.dx; c.ldxs = c.ldx;
  w.first_slot = (w.first_slot + w.npend) % p.R; w.npend = 0;
}

struct CgResult { int niter; double residual; };   // iterations that started with an active column; column 0's last residual

// ---- loop 1: the scalars on the device, no host round trip inside an iteration ------------------------------------------------
// pass 1 -> [all-reduce] -> cg_scalars_a -> pass 2 -> [all-reduce] -> cg_scalars_b, all on the back-end's stream.  The iteration
// the host enqueued before it learnt that no column was active any more is a no-op on the data (all flags 0: r untouched, p
// copied, zero coefficients for the pending x update).
static CgResult cg_loop_device_scalars(CgCall& c, const CgPlan& p) {
  HipBpcg* s = c.s; BpcgBlocks& k = s->blk; hipStream_t st = c.st;
  const int n = c.n, nrhs = c.nrhs, R = p.R, J = R - 1;
  const bool recompute = p.recompute, implicit_r = p.implicit_r;
  if (s->sc_cap < nrhs) {
    GCGE_HIP_CHECK(hipStreamSynchronize(st));
    if (s->d_sc) { hipFree(s->d_sc); hipFree(s->d_sci); hipHostFree(s->h_nact); }
    else { GCGE_HIP_CHECK(hipEventCreateWithFlags(&s->ev_it[0], hipEventDisableTiming)); GCGE_HIP_CHECK(hipEventCreateWithFlags(&s->ev_it[1], hipEventDisableTiming)); }
    s->sc_cap = nrhs + 64;
    GCGE_HIP_CHECK(hipMalloc(&s->d_sc, (size_t)(30 + 16) * s->sc_cap * sizeof(double)));
    GCGE_HIP_CHECK(hipMalloc(&s->d_sci, (size_t)2 * s->sc_cap * sizeof(int)));
    GCGE_HIP_CHECK(hipHostMalloc(&s->h_nact, 4096 * sizeof(int)));
  }
  const size_t cap = (size_t)s->sc_cap;
  double *d_rho2 = s->d_sc, *d_init = d_rho2 + cap, *d_normb = d_init + cap, *d_last = d_normb + cap, *d_alpha = d_last + cap,
         *d_beta = d_alpha + cap, *d_sums = d_beta + cap /* 6 cap */, *d_newrho = d_sums + 6 * cap /* 6 cap */,
         *d_ahist = d_newrho + 6 * cap /* 16 cap, starts at 18 cap: (30 + 16) cap in total */;
  int *d_active = s->d_sci, *d_flag = d_active + cap;
  double* d_betaB = d_ahist + 16 * cap;   // second beta buffer: beta_k and beta_{k-1} alternate between the two
  if (implicit_r) {
    GCGE_HIP_CHECK(hipMemsetAsync(d_beta, 0, cap * sizeof(double), st));
    GCGE_HIP_CHECK(hipMemsetAsync(d_betaB, 0, cap * sizeof(double), st));
  }
  {   // start values (rho, initial residuals, scales, active flags were computed on the host)
    std::vector<double> up(3 * (size_t)nrhs);
    memcpy(up.data(), c.rho2.data(), nrhs * sizeof(double)); memcpy(up.data() + nrhs, c.init_res.data(), nrhs * sizeof(double));
    memcpy(up.data() + 2 * nrhs, c.norm_b.data(), nrhs * sizeof(double));
    GCGE_HIP_CHECK(hipMemcpyAsync(d_rho2, up.data(), nrhs * sizeof(double), hipMemcpyHostToDevice, st));
    GCGE_HIP_CHECK(hipMemcpyAsync(d_init, up.data() + nrhs, nrhs * sizeof(double), hipMemcpyHostToDevice, st));
    GCGE_HIP_CHECK(hipMemcpyAsync(d_normb, up.data() + 2 * nrhs, nrhs * sizeof(double), hipMemcpyHostToDevice, st));
    GCGE_HIP_CHECK(hipMemcpyAsync(d_last, up.data() + nrhs, nrhs * sizeof(double), hipMemcpyHostToDevice, st));
    GCGE_HIP_CHECK(hipMemcpyAsync(d_active, c.active.data(), nrhs * sizeof(int), hipMemcpyHostToDevice, st));
    GCGE_HIP_CHECK(hipStreamSynchronize(st));   // `up` leaves scope
  }
  const bool reduce = GCGE_GetComm() != nullptr;
  CgPending w;
  int enq = 0;            // iterations enqueued
  int done = -1;          // index of the last iteration whose active count the host has seen
  int stop_at = -1;       // first iteration that found no active column at its start
  bool trimmed = false;   // the last iteration's second pass left columns out: its active count is not a count of all
  while (enq < s->max_iter && enq < 4096) {
    void** pcur = p.slots[w.cur];
    const int m2 = enq == s->max_iter - 1 ? p.last_cols : nrhs;   // columns of this iteration's second pass
    trimmed = m2 < nrhs;
    if (recompute) {
      if (gcge_hip_cg_pass1_dev(c.mat, pcur, 0, nrhs, d_sums) != 0) { fprintf(stderr, "HIP_BlockPCG: first CG pass refused operands it had accepted\n"); abort(); }
    } else if (gcge_hip_spmm_dot2_dev(c.mat, pcur, k.mv_ws[2], 0, 0, nrhs, d_sums) != 0) {
      fprintf(stderr, "HIP_BlockPCG: product with column sums refused operands the one-pass scheme had accepted\n"); abort();
    }
    if (reduce) gcge_hip_comm_allreduce_device(d_sums, 2 * nrhs);
    double* bcur = (implicit_r && (enq & 1)) ? d_betaB : d_beta;
    const double* bprev = (enq & 1) ? d_beta : d_betaB;
    hipLaunchKernelGGL(cg_scalars_a, dim3(1), dim3(256), 0, st, nrhs, d_rho2, d_sums, d_active, d_alpha, bcur, d_flag,
                       d_ahist + (size_t)w.npend * nrhs);
    int rc2 = 0;
    if (m2 == 0) {        // no second pass: p_{k+1}, rho_{k+1} and the active flags are left as they are (counted as before)
      if (implicit_r) ++s->implicit_r_iters;
      if (!recompute) ++s->stored_dev_iters;
    } else if (!recompute) {     // w is stored: one sweep over w, the directions (and r where it is stored) — cg_update_p_implicit / cg_update_rp
      long ldq;
      const double* pold = gcge_hip_mv_device_ptr(p.slots[w.cur], &ldq);
      double* pnew = gcge_hip_mv_device_ptr(p.slots[(w.cur + 1) % R], &ldq);
      double* part = gcge_hip_partial_ws((size_t)c.grid.nb * nrhs);
      if (implicit_r) {
        const double* pprev = gcge_hip_mv_device_ptr(p.slots[(w.cur + R - 1) % R], &ldq);
        hipLaunchKernelGGL(cg_update_p_implicit<4>, dim3((unsigned)c.grid.nb), dim3(256), 0, st, (long)n, (const double*)c.dw, c.ldw, enq == 0 ? pold : pprev,
                           pold, pnew, c.ldp, nrhs, (const double*)d_alpha, (const double*)bcur, bprev, (const int*)d_flag, part, cg_tpr(nrhs));
        ++s->implicit_r_iters;
      } else
        hipLaunchKernelGGL(cg_update_rp<4>, dim3((unsigned)c.grid.nb), dim3(256), 0, st, (long)n, (const double*)c.dw, c.ldw, c.dr, c.ldr, pold, pnew, c.ldp, nrhs,
                           (const double*)d_alpha, (const double*)d_beta, (const int*)d_flag, part, cg_tpr(nrhs));
      gcge_hip_reduce_partials(part, (int)c.grid.nb, nrhs, d_newrho, st);
      ++s->stored_dev_iters;
    } else if (implicit_r) {
      rc2 = gcge_hip_cg_pass2i_dev(c.mat, pcur, enq == 0 ? pcur : p.slots[(w.cur + R - 1) % R], p.slots[(w.cur + 1) % R], 0, m2, d_alpha, bcur,
                                   d_flag, bprev, d_newrho);
      ++s->implicit_r_iters;
    } else rc2 = gcge_hip_cg_pass2_dev(c.mat, pcur, k.mv_ws[0], p.slots[(w.cur + 1) % R], 0, m2, d_alpha, d_beta, d_flag, d_newrho);
    if (rc2 != 0) { fprintf(stderr, "HIP_BlockPCG: second CG pass refused operands it had accepted\n"); abort(); }
    if (m2 > 0) {   // (m2 is the same on every rank: max_iter and the caller's final_residual_cols are)
      if (reduce) gcge_hip_comm_allreduce_device(d_newrho, m2);
      hipLaunchKernelGGL(cg_scalars_b, dim3(1), dim3(256), 0, st, m2, d_newrho, s->rate, s->tol, d_normb, d_init, d_rho2, d_active,
                         d_last, s->h_nact + enq);
    }
    if (trimmed) ++s->trimmed_iters;
    GCGE_HIP_CHECK(hipEventRecord(s->ev_it[enq & 1], st));
    ++w.npend; w.cur = (w.cur + 1) % R; if (recompute) ++s->recompute_iters; ++s->dev_scalar_iters; s->spmm_calls++; s->spmm_cols += nrhs;
    ++enq;
    if (w.npend == J) cg_flush_x(c, p, w, d_ahist);
    if (enq >= 2) {   // what did iteration enq - 2 leave?  (iteration enq - 1 is already in the queue)
      GCGE_HIP_CHECK(hipEventSynchronize(s->ev_it[(enq - 2) & 1]));
      done = enq - 2;
      if (s->h_nact[done] == 0) { stop_at = done + 1; break; }
    }
  }
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  // niter, the column statistics and the surplus count never look at a trimmed last iteration's active count
  if (stop_at < 0) {      // the queue ran dry at max_iter (or the last iterations have not been looked at yet)
    stop_at = enq;        // (a trimmed last iteration q = enq - 1 left no count of all columns; it would give q + 1 = enq anyway)
    for (int q = done + 1; q < enq - (trimmed ? 1 : 0); ++q) if (s->h_nact[q] == 0) { stop_at = q + 1; break; }
  }
  const int niter = stop_at;   // iterations that started with at least one active column, as the reference counts them
  cg_flush_x(c, p, w, d_ahist);
  GCGE_HIP_CHECK(hipMemcpyAsync(s->h_pin, d_last, sizeof(double), hipMemcpyDeviceToHost, st));
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  // columns streamed: every enqueued iteration walks all nrhs columns (the ring must stay complete), including the up to
  // two iterations enqueued before the host saw that nothing was active any more; columns still active at the START of
  // iteration q: the count iteration q - 1 left in h_nact
  s->col_iters += (long)nrhs * enq; s->surplus_iters += enq - niter;
  { long act = c.nact; for (int q = 1; q < niter; ++q) act += s->h_nact[q - 1]; s->active_col_iters += act; }
  return {niter, s->h_pin[0]};
}

// ---- loop 2: the one-pass scheme with the scalars on the host -------------------------------------------------------------------
// (with or without a ring, product recomputed or stored, residual stored or rebuilt)
static CgResult cg_loop_host_scalars(CgCall& c, const CgPlan& p) {
  HipBpcg* s = c.s; BpcgBlocks& k = s->blk; hipStream_t st = c.st;
  const int n = c.n, nrhs = c.nrhs, R = p.R, J = R - 1;   // J: pending directions before x is brought up to date
  std::vector<double> wTw(nrhs), bet(nrhs), bprev_host(nrhs, 0.0), newrho(nrhs);
  std::vector<double> ahist((size_t)(J > 0 ? J : 1) * nrhs, 0.0);   // the coefficients of the pending x updates, one row per direction
  CgPending w;
  auto flush_x = [&]() {
    if (w.npend == 0) return;
    double* d_ahist = gcge_hip_partial_ws((size_t)J * nrhs);
    GCGE_HIP_CHECK(hipMemcpyAsync(d_ahist, ahist.data(), (size_t)w.npend * nrhs * sizeof(double), hipMemcpyHostToDevice, st));
    cg_flush_x(c, p, w, d_ahist);
    GCGE_HIP_CHECK(hipStreamSynchronize(st));   // ahist (pageable) and the partial workspace are reused right away
  };
  int niter = 0;
  while (niter < s->max_iter && c.nact > 0) {
    s->col_iters += nrhs; s->active_col_iters += c.nact;
    int alo = 0, ahi = nrhs;
    if (R == 1) {   // (with a ring every column takes part in every step: the slots must stay complete)
      while (alo < nrhs && !c.active[alo]) ++alo;
      while (ahi > alo && !c.active[ahi - 1]) --ahi;
    }
    int aw = ahi - alo;
    if (((alo & 1) || (aw & 1))) { alo &= ~1; ahi = (ahi + 1) & ~1; aw = ahi - alo; }   // keep 16-byte column pairs
    void** pcur = p.slots[w.cur];
    if (p.recompute) {
      if (gcge_hip_cg_pass1_mv(c.mat, pcur, alo, aw, c.pTw.data() + alo, wTw.data() + alo) != 0) {
        fprintf(stderr, "HIP_BlockPCG: first CG pass refused operands it had accepted\n"); abort();
      }
    } else c.apply(pcur, alo, k.mv_ws[2], alo, aw, c.pTw.data() + alo, wTw.data() + alo);
    s->spmm_calls++; s->spmm_cols += aw;
    {   // one all-reduce for both sums
      std::vector<double> both(2 * (size_t)aw);
      memcpy(both.data(), c.pTw.data() + alo, aw * sizeof(double)); memcpy(both.data() + aw, wTw.data() + alo, aw * sizeof(double));
      reduce_over_ranks(both.data(), 2 * aw);
      memcpy(c.pTw.data() + alo, both.data(), aw * sizeof(double)); memcpy(wTw.data() + alo, both.data() + aw, aw * sizeof(double));
    }
    for (int j = alo; j < ahi; ++j) {
      c.flag[j] = c.active[j]; c.coef[j] = 0.0; bet[j] = 0.0;
      if (!c.active[j]) continue;
      const double al = c.rho2[j] / c.pTw[j];
      double rho_pred = al * al * wTw[j] - c.rho2[j];
      if (!(rho_pred > 0.0) || !std::isfinite(rho_pred)) rho_pred = 0.0;   // cancellation: restart this column from r
      c.coef[j] = al; bet[j] = rho_pred / c.rho2[j];
    }
    c.upload(alo, aw, bet.data(), c.coef.data(), c.flag.data());   // d_coef = [beta | alpha]
    const double* d_alpha = s->d_coef + s->cap; const double* d_beta = s->d_coef;
    if (R > 1)   // this iteration's row of the pending x update
      for (int j = 0; j < nrhs; ++j) ahist[(size_t)w.npend * nrhs + j] = (j >= alo && j < ahi && c.active[j]) ? c.coef[j] : 0.0;
    if (p.recompute) {
      if (gcge_hip_cg_pass2_mv(c.mat, pcur, k.mv_ws[0], p.slots[(w.cur + 1) % R], alo, aw, d_alpha, d_beta, s->d_flag, newrho.data()) != 0) {
        fprintf(stderr, "HIP_BlockPCG: second CG pass refused operands it had accepted\n"); abort();
      }
      ++s->recompute_iters;
      reduce_over_ranks(newrho.data(), aw);
    } else {
      double* part = gcge_hip_partial_ws((size_t)c.grid.nb * aw + aw + (size_t)(J > 0 ? J : 0) * nrhs);
      if (R > 1) {
        long ldq;
        const double* pold = gcge_hip_mv_device_ptr(p.slots[w.cur], &ldq);
        double* pnew = gcge_hip_mv_device_ptr(p.slots[(w.cur + 1) % R], &ldq);
        if (p.implicit_r) {   // r is not stored: rebuilt from p_k and p_{k-1} (beta_{k-1} of the previous step, 0 at the start)
          const double* pprev = gcge_hip_mv_device_ptr(p.slots[(w.cur + R - 1) % R], &ldq);
          double* d_bprev = part + (size_t)c.grid.nb * aw + aw;   // (behind the partial sums and their total; J * nrhs doubles are reserved there)
          GCGE_HIP_CHECK(hipStreamSynchronize(st));        // the pinned staging below may still feed the upload() above
          memcpy(s->h_pin, bprev_host.data() + alo, aw * sizeof(double));
          GCGE_HIP_CHECK(hipMemcpyAsync(d_bprev, s->h_pin, aw * sizeof(double), hipMemcpyHostToDevice, st));
          hipLaunchKernelGGL(cg_update_p_implicit<4>, dim3((unsigned)c.grid.nb), dim3(256), 0, st, (long)n, c.dw + alo, c.ldw,
                             (niter == 0 ? pold : pprev) + alo, pold + alo, pnew + alo, c.ldp, aw, d_alpha, d_beta,
                             (const double*)d_bprev, s->d_flag, part, cg_tpr(aw));
          for (int j = alo; j < ahi; ++j) bprev_host[j] = c.active[j] ? bet[j] : 0.0;
          ++s->implicit_r_iters;
        } else
          hipLaunchKernelGGL(cg_update_rp<4>, dim3((unsigned)c.grid.nb), dim3(256), 0, st, (long)n, c.dw + alo, c.ldw, c.dr + alo, c.ldr,
                             pold + alo, pnew + alo, c.ldp, aw, d_alpha, d_beta, s->d_flag, part, cg_tpr(aw));
      } else {
        hipLaunchKernelGGL(cg_update_all<4>, dim3((unsigned)c.grid.nb), dim3(256), 0, st, (long)n, c.dw + alo, c.ldw, c.dr + alo, c.ldr,
                           c.dp + alo, c.ldp, c.dx + alo, c.ldx, aw, d_alpha, d_beta, s->d_flag, part, cg_tpr(aw));
      }
      c.partial_sums_to_host(part, aw, newrho.data());
    }
    if (R > 1) { ++w.npend; w.cur = (w.cur + 1) % R; }
    c.retire_columns(alo, ahi, newrho.data());
    ++niter;
    if (w.npend == J && J > 0) flush_x();
  }
  flush_x();
  return {niter, c.last_res[0]};
}

// ---- loop 3: two sweeps, for blocks that cannot be walked with 16-byte lanes ------------------------------------------------------
static CgResult cg_loop_two_sweeps(CgCall& c) {
  HipBpcg* s = c.s; BpcgBlocks& k = s->blk; hipStream_t st = c.st;
  const int n = c.n, nrhs = c.nrhs;
  std::vector<double> aprev(nrhs, 0.0);
  std::vector<int> pend(nrhs, 0);           // x update of the last step still to be applied
  // d_coef holds [beta | aprev/alpha] (2*cap doubles), d_flag the per-column flags
  int niter = 0;
  while (niter < s->max_iter && c.nact > 0) {
    // contiguous column window covering every active column and every pending x update
    int lo = 0, hi = nrhs;
    while (lo < nrhs && !c.active[lo] && !pend[lo]) ++lo;
    while (hi > lo && !c.active[hi - 1] && !pend[hi - 1]) --hi;
    int mw = hi - lo;
    // x += alpha' p (deferred) ; p = r + beta p
    for (int j = lo; j < hi; ++j) {
      c.flag[j] = (c.active[j] ? (niter == 0 ? 2 : 1) : 0) | (pend[j] ? 4 : 0);
      c.coef[j] = (c.active[j] && niter > 0) ? c.rho2[j] / c.rho1[j] : 0.0;
    }
    c.upload(lo, mw, c.coef.data(), aprev.data(), c.flag.data());
    launch_update_xp((long)n, c.dr + lo, c.ldr, c.dp + lo, c.ldp, c.dx + lo, c.ldx, mw, s->d_coef, s->d_coef + s->cap, s->d_flag, st);
    for (int j = lo; j < hi; ++j) pend[j] = 0;
    // w = A p and pTw on the window of ACTIVE columns
    int alo = lo, ahi = hi;
    while (alo < hi && !c.active[alo]) ++alo;
    while (ahi > alo && !c.active[ahi - 1]) --ahi;
    const int aw = ahi - alo;
    c.apply(k.mv_ws[1], alo, k.mv_ws[2], alo, aw, c.pTw.data() + alo);
    s->spmm_calls++; s->spmm_cols += aw;
    reduce_over_ranks(c.pTw.data() + alo, aw);
    // r -= alpha w ; rho2 = diag(r^T r)
    for (int j = alo; j < ahi; ++j) {
      c.coef[j] = c.active[j] ? c.rho2[j] / c.pTw[j] : 0.0; c.flag[j] = c.active[j];
      if (c.active[j]) { aprev[j] = c.coef[j]; pend[j] = 1; }
    }
    c.upload(alo, aw, c.coef.data(), c.coef.data(), c.flag.data());
    double* part = gcge_hip_partial_ws((size_t)c.grid.nb * aw + aw);
    hipLaunchKernelGGL(cg_update_r, dim3((unsigned)c.grid.nb), dim3(256), 0, st, (long)n, c.dw + alo, c.ldw, c.dr + alo, c.ldr, aw,
                       s->d_coef, s->d_flag, part, c.grid.rpb);
    std::vector<double> newrho(aw);
    c.partial_sums_to_host(part, aw, newrho.data());
    c.retire_columns(alo, ahi, newrho.data());
    ++niter;
  }
  {   // flush the x updates still pending
    int lo = 0, hi = nrhs;
    while (lo < nrhs && !pend[lo]) ++lo;
    while (hi > lo && !pend[hi - 1]) --hi;
    if (hi > lo) {
      const int mw = hi - lo;
      for (int j = lo; j < hi; ++j) { c.flag[j] = pend[j] ? 4 : 0; c.coef[j] = 0.0; }
      c.upload(lo, mw, c.coef.data(), aprev.data(), c.flag.data());
      launch_update_xp((long)n, c.dr + lo, c.ldr, c.dp + lo, c.ldp, c.dx + lo, c.ldx, mw, s->d_coef, s->d_coef + s->cap, s->d_flag, st);
    }
  }
  return {niter, c.last_res[0]};
}

// checks, shape, plan, start, one of the three loops, result
static void HIP_BlockPCG_run(void* mat, void** mv_b, void** mv_x, int* start_bx, int* end_bx, struct OPS_* ops) {
  HipBpcg* s = (HipBpcg*)ops->multi_linear_solver_workspace;
  const int nrhs = end_bx[0] - start_bx[0];
  assert(nrhs == end_bx[1] - start_bx[1]);
  if (nrhs <= 0) { s->niter = 0; return; }
  const int n = gcge_hip_mv_nrows(mv_x);
  if (gcge_hip_mv_nrows(mv_b) != n) { fprintf(stderr, "HIP_BlockPCG: b and x have different row counts\n"); abort(); }
  bpcg_shape(s, n, nrhs, mv_x, ops);
  BpcgBlocks& k = s->blk;
  CgCall c = {s, ops, (hipStream_t)gcge_hip_stream(), mat, mv_b, mv_x, start_bx[0], start_bx[1], n, nrhs, *GCGE_GetLinearSolverArgs(), cg_switches()};
  if (c.args.sigma != 0.0 && c.args.matB != nullptr && k.mv_ws[3] == nullptr) ops->MultiVecCreateByMultiVec(&k.mv_ws[3], k.ws_cols, mv_x, ops);
  if (s->cap < nrhs) {
    if (s->d_coef) { hipFree(s->d_coef); hipFree(s->d_flag); hipHostFree(s->h_pin); }
    s->cap = nrhs + 64;
    GCGE_HIP_CHECK(hipMalloc(&s->d_coef, 2 * s->cap * sizeof(double)));
    GCGE_HIP_CHECK(hipMalloc(&s->d_flag, s->cap * sizeof(int)));
    GCGE_HIP_CHECK(hipHostMalloc(&s->h_pin, 3 * s->cap * sizeof(double)));
  }
  c.dx = gcge_hip_mv_device_ptr(mv_x, &c.ldx) + c.xc0;
  c.dr = gcge_hip_mv_device_ptr(k.mv_ws[0], &c.ldr);
  c.dp = gcge_hip_mv_device_ptr(k.mv_ws[1], &c.ldp);
  c.dw = gcge_hip_mv_device_ptr(k.mv_ws[2], &c.ldw);
  c.dxs = c.dx; c.ldxs = c.ldx;
  c.one_pass = nrhs <= 512 && cg_vec_ok(nrhs, {c.dw, c.dr, c.dp, c.dx}, {c.ldw, c.ldr, c.ldp, c.ldx});
  c.grid = cg_grid(n);
  for (std::vector<double>* v : {&c.norm_b, &c.rho1, &c.rho2, &c.pTw, &c.init_res, &c.last_res, &c.coef}) v->assign(nrhs, 0.0);
  c.active.assign(nrhs, 0); c.flag.assign(nrhs, 0);

  // One plan per call.  Planning sizes the direction ring, and a new ring is sized by the memory that is free at that moment, so
  // the call plans where the ring has always been sized: ahead of the start where the start's form depends on the plan (pattern
  // matrix, no shift — the only calls whose start may leave r out), behind it for every other call.
  const bool plan_first = c.args.sigma == 0.0 && gcge_hip_cg_recompute_pays(mat);
  CgPlan plan = {};
  if (plan_first) plan = cg_plan(c);
  const bool p0_done = cg_start(c, plan_first && plan.start_without_r, plan_first && plan.recompute);
  if (!plan_first) plan = cg_plan(c);
  s->spmm_calls++; s->spmm_cols += nrhs;
  c.nact = 0;
  for (int i = 0; i < nrhs; ++i) {
    c.init_res[i] = sqrt(c.rho2[i]); c.last_res[i] = c.init_res[i];
    c.active[i] = c.init_res[i] > s->tol * c.norm_b[i];
    c.nact += c.active[i];
  }
  CgResult res = {0, c.last_res[0]};   // (no active column: no iteration)
  if (c.nact > 0) {
    if (plan.loop != CG_TWO_SWEEPS && !p0_done) {   // p0 = r0  (slot 0 is mv_ws[1]; the two-sweep loop's first sweep copies it)
      int st2[2] = {0, 0}, en2[2] = {nrhs, nrhs};
      ops->MultiVecAxpby(1.0, k.mv_ws[0], 0.0, k.mv_ws[1], st2, en2, ops);
    }
    res = plan.loop == CG_DEVICE_SCALARS ? cg_loop_device_scalars(c, plan)
        : plan.loop == CG_HOST_SCALARS   ? cg_loop_host_scalars(c, plan) : cg_loop_two_sweeps(c);
  }
  if (c.dxs != c.dx) { CgPending none; cg_flush_x(c, plan, none, s->d_coef); }   // no iteration ran: x = the initial guess
  s->niter = res.niter;
  s->residual = res.residual;
}
static void HIP_BlockPCG(void* mat, void** mv_b, void** mv_x, int* start_bx, int* end_bx, struct OPS_* ops) {
  HipBpcg* s = (HipBpcg*)ops->multi_linear_solver_workspace;
  const double t0 = ops->GetWtime ? ops->GetWtime() : 0.0;
  HIP_BlockPCG_run(mat, mv_b, mv_x, start_bx, end_bx, ops);
  s->total_iters += s->niter;
  if (ops->GetWtime) s->total_seconds += ops->GetWtime() - t0;
  static const bool trace = getenv("GCGE_CG_TRACE") != nullptr;   // one line per call on stderr (tuning aid)
  if (trace && ops->GetWtime)
    fprintf(stderr, "HIP_BlockPCG: %d columns (b at %d, x at %d), %d iterations, ring of %d, %.1f ms\n", end_bx[0] - start_bx[0], start_bx[0],
            start_bx[1], s->niter, s->blk.ring_len, 1e3 * (ops->GetWtime() - t0));
}

// C-ABI: install the fused solver (GCG: pass flag = 1 to the harness / -gcge_user_defined_multi_lin_sol 1)
extern "C" void gcge_hip_bpcg_setup(struct OPS_* ops, int max_iter, double rate, double tol, const char* tol_type) {
  // "user": the column scales BlockPCG finds in its scalar scratch (src/ops_lin_sol.c:186-192) are read from
  // GCGE_LINSOL_ARGS.user_scale at solve time (the GCG driver publishes lambda_j + sigma there); anything else is refused
  if (tol_type != nullptr && strcmp(tol_type, "abs") != 0 && strcmp(tol_type, "rel") != 0 && strcmp(tol_type, "user") != 0) {
    fprintf(stderr, "gcge_hip_bpcg_setup: tol_type \"%s\" is not one of \"abs\", \"rel\", \"user\"\n", tol_type);
    abort();
  }
  g_bpcg.max_iter = max_iter; g_bpcg.rate = rate; g_bpcg.tol = tol;
  strncpy(g_bpcg.tol_type, tol_type ? tol_type : "abs", 7); g_bpcg.tol_type[7] = 0;
  ops->multi_linear_solver_workspace = (void*)&g_bpcg;
  ops->MultiLinearSolver = HIP_BlockPCG;
}
// Optional: create the solver's blocks (r, p, w and the ring of direction slots) NOW, for systems with the rows of `mv_like` and up
// to `ncols` right-hand sides, instead of inside the first solve.  The counterpart of the reference's EigenSolverCreateWorkspace /
// MultiLinearSolverSetup_BlockPCG (src/ops_lin_sol.c:439-465), which take the CG's blocks from the caller before any timer
// starts: a ring of 15 slots at BASELINE config 2's shape is 129 GB of fresh device memory, which the driver clears on first
// use (4 s in a new process — otherwise spent inside the first call).  Collective when a communicator exists.
extern "C" int gcge_hip_bpcg_prepare(struct OPS_* ops, void* mat, void** mv_like, int ncols) {
  if (ops == nullptr || ops->MultiLinearSolver != HIP_BlockPCG || mv_like == nullptr || ncols <= 0) return -1;
  HipBpcg* s = (HipBpcg*)ops->multi_linear_solver_workspace;
  bpcg_shape(s, gcge_hip_mv_nrows(mv_like), ncols, mv_like, ops);
  bpcg_ring(s, mat, mv_like, GCGE_GetLinearSolverArgs()->sigma, ops);
  GCGE_HIP_CHECK(hipStreamSynchronize((hipStream_t)gcge_hip_stream()));
  return s->blk.ring_len;
}
extern "C" void gcge_hip_bpcg_stats(long* spmm_calls, long* spmm_cols, int* last_niter) {
  if (spmm_calls) *spmm_calls = g_bpcg.spmm_calls;
  if (spmm_cols) *spmm_cols = g_bpcg.spmm_cols;
  if (last_niter) *last_niter = g_bpcg.niter;
}
extern "C" long gcge_hip_bpcg_recompute_iters(void) { return g_bpcg.recompute_iters; }
extern "C" long gcge_hip_bpcg_device_scalar_iters(void) { return g_bpcg.dev_scalar_iters; }
extern "C" long gcge_hip_bpcg_implicit_r_iters(void) { return g_bpcg.implicit_r_iters; }
extern "C" long gcge_hip_bpcg_stored_dev_iters(void) { return g_bpcg.stored_dev_iters; }
extern "C" long gcge_hip_bpcg_fused_starts(void) { return g_bpcg.fused_starts; }
extern "C" void gcge_hip_bpcg_time_stats(long* iters, double* seconds, int reset) {
  if (iters) *iters = g_bpcg.total_iters;
  if (seconds) *seconds = g_bpcg.total_seconds;
  if (reset) { g_bpcg.total_iters = 0; g_bpcg.total_seconds = 0.0; }
}
extern "C" void gcge_hip_bpcg_column_stats(long* col_iters, long* active_col_iters) {
  if (col_iters) *col_iters = g_bpcg.col_iters;
  if (active_col_iters) *active_col_iters = g_bpcg.active_col_iters;
}
extern "C" long gcge_hip_bpcg_surplus_iters(void) { return g_bpcg.surplus_iters; }
extern "C" long gcge_hip_bpcg_trimmed_iters(void) { return g_bpcg.trimmed_iters; }
extern "C" long gcge_hip_bpcg_legacy_start_sums(void) { return g_bpcg.legacy_start_sums; }
extern "C" long gcge_hip_bpcg_start_in_place_stats(long* declined) { if (declined) *declined = g_bpcg.starts_materialised; return g_bpcg.starts_in_place; }
extern "C" double gcge_hip_bpcg_last_residual(void) { return g_bpcg.residual; }   // what the last call reported (column 0)
// the fused CG as the smoother of BlockAMG for the HIP table: same stopping rules as MultiLinearSolverSetup_BlockPCG, its own
// blocks per level (parked sets above)
static void amg_smoother_setup(int max_iter, double rate, double tol, const char* tol_type, struct OPS_* ops) {
  gcge_hip_bpcg_setup(ops, max_iter, rate, tol, tol_type);
}
static double amg_smoother_residual(struct OPS_* ops) { (void)ops; return g_bpcg.residual; }
// this file's part of the HIP table's back-end record (OPS_HIP_Set): the smoother above, and the solver itself as the one that
// takes b = x diag(scale) unformed (see cg_start)
extern "C" void gcge_hip_bpcg_backend(GCGE_BACKEND* be) {
  be->amg_smoother_setup = amg_smoother_setup;
  be->amg_smoother_residual = amg_smoother_residual;
  be->scaled_rhs_solver = HIP_BlockPCG;
  be->amg_final_cols = 1;
  be->start_in_place = 1;               // HIP_BlockPCG accepts an initial guess elsewhere (GCGE_LINSOL_ARGS.x_src: cg_start_elsewhere)
}
extern "C" void gcge_hip_bpcg_release(struct OPS_* ops) {
  for (int i = 0; i < g_nparked; ++i) bpcg_destroy_set(&g_parked[i], ops);
  g_nparked = 0;
  bpcg_destroy_set(&g_bpcg.blk, ops);
}
