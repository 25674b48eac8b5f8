// New values for a live handle with a star or a dense form (the second half of gcge_hip_mat_update_values_device, mat_values.hip): such a
// handle stores its values behind its builders — the star's diagonal, the remainder the split leaves (entries MINUS a coefficient at star
// positions), block values in MFMA fragment order over up to 4 layers, a pad-8 remainder — and an update replays, on the device, the
// provenance those builders recorded when gcge_hip_mat_keep_value_maps was on at creation (value_maps.h: the rule, shared with the host):
//   check    k_vm_check, one thread per CSR entry, BEFORE the first store: an entry the star carries (pinned) must keep its coefficient's
//            bits — the coefficients are fixed for the life of the handle —, the diagonal must not be NaN (the split refuses those);
//            (an update allocates nothing after the handle's first: the flag word and the scratch stay with the maps)
//   write    d_diag[r]   = new value of the row's diagonal entry (0.0: none stored)               k_vm_gather over the rows
//            scratch[e]  = new value minus coefficient, for every entry e of the star's remainder  k_vm_star_rem (rem nnz doubles)
//            d_vals[s], d_pval[s] = scratch[map[s]] (without a star: new values[map[s]]), pads 0.0  k_vm_gather over the slots
// Every kernel is one thread per DESTINATION slot: a wave stores 512 contiguous bytes and reads 256 contiguous bytes of map; the gathered
// side is as local as the builders left it (a block row's entries are runs of a CSR row).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>

#include "gcge_hip.h"
#include "gcge_hip_internal.h"
#include "star_split.h"
#include "value_maps.h"

using namespace gcge;

extern "C" void gcge_hip_spmm_dense_mode(int mode);
extern "C" int gcge_hip_spmm_dense_mode_get(void);
static inline uint64_t vm_bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

struct GcgeStarMaps {
  long nnz, nrows, rem_nnz;
  int* d_diag_src; unsigned char* d_pin;            // [row], [CSR entry]
  int* d_rem_src; unsigned char* d_rem_code;        // [entry of the star's remainder]
  double* d_coef;                                   // [code]: the star's coefficients, GCGE_VM_NCODE doubles
  // what an update works in, allocated by the first one and kept (not maps: not counted in gcge_hip_star_maps_bytes)
  int* d_flag; double* d_rem;                       // the flag word; the star's remainder under the new values, rem_nnz doubles
};

static GcgeVmCoef vm_coef(const StarCoef& c) {
  GcgeVmCoef o;
  memset(&o, 0, sizeof o);
  for (int k = 1; k <= STAR_R; ++k) { o.c[gcge_vm_code(0, k)] = c.cx[k]; o.c[gcge_vm_code(1, k)] = c.cy[k]; o.c[gcge_vm_code(2, k)] = c.cz[k]; }
  return o;
}
template <class T>
static T* vm_to_device(const std::vector<T>& v) {
  T* d = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&d, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) GCGE_HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}
extern "C" GcgeStarMaps* gcge_hip_star_maps_create(const void* star_host, long nnz) {
  const StarHost* H = (const StarHost*)star_host;
  if (H == nullptr || !H->keep_maps || (long)H->pin.size() != nnz || H->rem_src.size() != H->rem_col.size()) return nullptr;
  GcgeStarMaps* M = new GcgeStarMaps();
  M->nnz = nnz; M->nrows = (long)H->diag_src.size(); M->rem_nnz = (long)H->rem_src.size();
  M->d_diag_src = vm_to_device(H->diag_src); M->d_pin = vm_to_device(H->pin);
  M->d_rem_src = vm_to_device(H->rem_src); M->d_rem_code = vm_to_device(H->rem_code);
  const GcgeVmCoef coef = vm_coef(H->c);
  M->d_coef = vm_to_device(std::vector<double>(coef.c, coef.c + GCGE_VM_NCODE));
  M->d_flag = nullptr; M->d_rem = nullptr;
  return M;
}
extern "C" void gcge_hip_star_maps_free(GcgeStarMaps* M) {
  if (M == nullptr) return;
  hipFree(M->d_diag_src); hipFree(M->d_pin); hipFree(M->d_rem_src); hipFree(M->d_rem_code); hipFree(M->d_coef);
  if (M->d_flag != nullptr) hipFree(M->d_flag);
  if (M->d_rem != nullptr) hipFree(M->d_rem);
  delete M;
}
extern "C" long gcge_hip_star_maps_bytes(const GcgeStarMaps* M) {
  return M == nullptr ? 0 : M->nnz + 4 * M->nrows + 5 * M->rem_nnz;
}

static long g_vm_stats[4] = {0, 0, 0, 0};
extern "C" void gcge_hip_mat_update_form_stats(long out[4]) { for (int i = 0; i < 4; ++i) out[i] = g_vm_stats[i]; }

#define VM_BS 256
static unsigned vm_blocks(long n) { return (unsigned)((n + VM_BS - 1) / VM_BS); }

// flag bits: 1 a pinned entry left its coefficient, 2 a NaN on the diagonal
__global__ __launch_bounds__(VM_BS) void k_vm_check(long nnz, const double* __restrict__ nv, const unsigned char* __restrict__ pin,
                                                    const double* __restrict__ coef, int* __restrict__ flag) {
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nnz) return;
  const int p = pin[q];
  if (p == 0) return;
  const int bad = gcge_vm_check(nv[q], p < GCGE_VM_NCODE || p == GCGE_VM_PIN_DIAG ? p : 0, coef);
  if (bad != 0 && (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bad) != bad) atomicOr(flag, bad);
}
// dst[s] = src[map[s]], 0.0 where the map names no source; nsrc bounds the gather (a map is the builder's: an entry outside reads nothing)
__global__ __launch_bounds__(VM_BS) void k_vm_gather(long n, const int* __restrict__ map, const double* __restrict__ src, long nsrc, double* __restrict__ dst) {
  const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int m = map[s];
  dst[s] = gcge_vm_gather(src, m < nsrc ? m : -1);
}
// the star's remainder under the new values: out[e] = nv[src[e]] - coef[code[e]]
__global__ __launch_bounds__(VM_BS) void k_vm_star_rem(long n, const int* __restrict__ src, const unsigned char* __restrict__ code, const double* __restrict__ nv,
                                                       long nnz, const double* __restrict__ coef, double* __restrict__ out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int m = src[e], c = code[e];
  out[e] = gcge_vm_replay(nv, m < nnz ? m : -1, c < GCGE_VM_NCODE ? c : 0, coef);
}

// 1: the handle has a star or a dense form (mat_values.hip then takes the two calls below instead of its pattern path)
extern "C" int gcge_hip_mat_has_value_form(const GCGE_HIP_MAT* A) { return A->star != nullptr || A->star_rem != nullptr || A->dense != nullptr; }

// 1: the handle holds the maps an update needs — decided from their presence, not their size (a star whose rows are all clean has a
// block form without a single slot)
static bool vm_dense_maps(const void* DM, const int** d_vmap, double** d_vals, long* nvals, const int** d_pmap, double** d_pval, long* npval, long* nsrc) {
  const int* vm = nullptr;
  if (DM == nullptr) return false;
  gcge_hip_dense_value_maps(DM, &vm, d_vals, nvals, d_pmap, d_pval, npval, nsrc);
  if (d_vmap) *d_vmap = vm;
  return vm != nullptr;
}
extern "C" int gcge_hip_mat_holds_value_maps(const GCGE_HIP_MAT* A) {
  const void* DM = A->star != nullptr ? A->star_rem : A->dense;
  if (A->star != nullptr && A->star_maps == nullptr) return 0;
  return vm_dense_maps(DM, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ? 1 : 0;
}
// The check: everything that can stop an update, before the first store.  0: go on and write; 1: declined (nothing was written).
// *d2h: bytes copied device to host are added.
extern "C" int gcge_hip_mat_forms_check(GCGE_HIP_MAT* A, const double* d_val, long* d2h) {
  const void* DM = A->star != nullptr ? A->star_rem : A->dense;
  // declined from the handle alone: no maps, a tiled remainder
  long nsrc = 0;
  if (!gcge_hip_mat_holds_value_maps(A) || gcge_hip_dense_remainder_is_tiled(DM)) return 1;
  vm_dense_maps(DM, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nsrc);
  if (A->star == nullptr) {                       // blocks + remainder of the values themselves: every entry is free
    GCGE_REQUIRE(nsrc == A->nnz, "value maps: the block form was built from the CSR values");
    return 0;
  }
  GcgeStarMaps* M = A->star_maps;
  GCGE_REQUIRE(nsrc == M->rem_nnz, "value maps: the block form was built from the star's remainder");
  if (M->nnz != A->nnz || M->nrows != A->nrows) return 1;
  hipStream_t st = (hipStream_t)gcge_hip_stream();
  if (M->d_flag == nullptr) {
    GCGE_HIP_CHECK(hipMalloc(&M->d_flag, sizeof(int)));
    GCGE_HIP_CHECK(hipMalloc(&M->d_rem, (size_t)(M->rem_nnz ? M->rem_nnz : 1) * sizeof(double)));
  }
  GCGE_HIP_CHECK(hipMemsetAsync(M->d_flag, 0, sizeof(int), st));
  if (M->nnz > 0) k_vm_check<<<vm_blocks(M->nnz), VM_BS, 0, st>>>(M->nnz, d_val, M->d_pin, M->d_coef, M->d_flag);
  GCGE_HIP_CHECK(hipGetLastError());
  int flag = 0;
  GCGE_HIP_CHECK(hipMemcpyAsync(&flag, M->d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  if (d2h) *d2h += (long)sizeof(int);
  if (flag & 1) g_vm_stats[2] += 1;
  if (flag & 2) g_vm_stats[3] += 1;
  return flag != 0 ? 1 : 0;
}
// The write, after the check passed and behind k_mv_values on the same stream (the caller synchronises it): launches only.
extern "C" void gcge_hip_mat_forms_write(GCGE_HIP_MAT* A, const double* d_val) {
  hipStream_t st = (hipStream_t)gcge_hip_stream();
  void* DM = A->star != nullptr ? A->star_rem : A->dense;
  const int *d_vmap = nullptr, *d_pmap = nullptr; double *d_vals = nullptr, *d_pval = nullptr; long nvals = 0, npval = 0, nsrc = 0;
  vm_dense_maps(DM, &d_vmap, &d_vals, &nvals, &d_pmap, &d_pval, &npval, &nsrc);
  const double* src = d_val;
  if (A->star != nullptr) {
    const GcgeStarMaps* M = A->star_maps;
    if (M->nrows > 0) k_vm_gather<<<vm_blocks(M->nrows), VM_BS, 0, st>>>(M->nrows, M->d_diag_src, d_val, M->nnz, gcge_hip_star_diag(A->star));
    if (M->rem_nnz > 0) k_vm_star_rem<<<vm_blocks(M->rem_nnz), VM_BS, 0, st>>>(M->rem_nnz, M->d_rem_src, M->d_rem_code, d_val, M->nnz, M->d_coef, M->d_rem);
    src = M->d_rem;
    g_vm_stats[0] += 1;
  } else {
    g_vm_stats[1] += 1;
  }
  if (nvals > 0) k_vm_gather<<<vm_blocks(nvals), VM_BS, 0, st>>>(nvals, d_vmap, src, nsrc, d_vals);
  if (npval > 0) k_vm_gather<<<vm_blocks(npval), VM_BS, 0, st>>>(npval, d_pmap, src, nsrc, d_pval);
  GCGE_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ host self-check (no device)
// spmm_dense.hip: the block form of (rowptr, colidx, val) with its maps, replayed on src, expanded into per-row (column, value) lists
long gcge_dense_maps_expand(int nrows, int ncols_local, const int* rowptr, const int* colidx, const double* val, const unsigned char* not_listed,
                            const double* src, std::vector<std::vector<std::pair<int, double>>>& got, long* out);

// The forms and their maps built from val0, the maps replayed on val1 through value_maps.h, star + diagonal + blocks + remainder expanded
// back into per-row sums per column and compared with the CSR rows of val1: exact where one stored value makes the entry, to the one
// rounding of "entry minus coefficient" where the star and the remainder share it (the bound of gcge_hip_star_selfcheck).  A geometry
// (nx > 0, box_of_row) is the masked grid of gcge_hip_mat_create_grid; without one the grid is read off the rows as the upload does.
// Returns the number of differing entries — (row, column) pairs — (0: equal), -1: neither a star nor a dense form, -2: the update would be declined (a pinned entry
// moved, a NaN on the diagonal).  out[0] forms found (1 star, 2 dense, 3 both), out[1] layers of blocks, out[2] pinned entries, out[3]
// bytes of maps.
static long value_maps_selfcheck(int nrows, const int* rowptr, const int* colidx, const double* val0, const double* val1, int dense_mode,
                                 int nx, int ny, int nz, const int* box_of_row, long* out) {
  const long nnz = rowptr[nrows];
  const int saved_mode = gcge_hip_spmm_dense_mode_get();
  gcge_hip_spmm_dense_mode(dense_mode);
  struct Restore { int m; ~Restore() { gcge_hip_spmm_dense_mode(m); } } restore{saved_mode};
  StarHost H;
  H.keep_maps = true;
  StarRows M = {nrows, nrows, 0, nrows, nullptr, rowptr, colidx, val0};
  if (box_of_row != nullptr && nx > 0 && ny > 0 && nz > 0) { M.box = box_of_row; M.bnx = nx; M.bny = ny; M.bnz = nz; M.nglobal = (long)nx * ny * nz; }
  bool star = star_build_host(M, &H);
  if (!star && M.box == nullptr) {
    H = StarHost(); H.keep_maps = true;
    int* od = H.own_dims;
    if (star_infer_box(nrows, rowptr, colidx, &H.own_box, &od[0], &od[1], &od[2])) {
      M.box = H.own_box.data(); M.bnx = od[0]; M.bny = od[1]; M.bnz = od[2]; M.nglobal = (long)od[0] * od[1] * od[2];
      star = star_build_host(M, &H);
    }
  }
  std::vector<std::vector<std::pair<int, double>>> got((size_t)nrows);
  long dout[2] = {0, 0}, pinned = 0, bytes = 0;
  int forms = 0;
  if (star) {
    // the remainder under val1 (what the update forms in its scratch), then the blocks of the remainder as built from val0
    const GcgeVmCoef coef = vm_coef(H.c);
    std::vector<double> rem1(H.rem_val.size());
    for (size_t e = 0; e < rem1.size(); ++e) {
      if (H.rem_src[e] < -1 || H.rem_src[e] >= nnz || H.rem_code[e] >= GCGE_VM_NCODE) return nrows + 1;
      rem1[e] = gcge_vm_replay(val1, H.rem_src[e], H.rem_code[e], coef.c);
    }
    const long bad = gcge_dense_maps_expand(nrows, nrows, H.rem_rowptr.data(), H.rem_col.data(), H.rem_val.data(), (const unsigned char*)H.clean.data(),
                                            rem1.data(), got, dout);
    if (bad != 0) star = false;                  // (-1: no block form under the star — the upload drops the star then; > 0 cannot happen)
    else {
      forms = 1 | (dout[0] > 0 ? 2 : 0); bytes = nnz + 4L * nrows + 5L * (long)rem1.size() + dout[1];
      for (long q = 0; q < nnz; ++q) {           // the update's check
        const int p = H.pin[(size_t)q];
        pinned += p != 0 && p != GCGE_VM_PIN_DIAG;
        if (gcge_vm_check(val1[q], p, coef.c) != 0) return -2;
      }
    }
  }
  if (!star) {
    for (auto& g : got) g.clear();
    const long bad = gcge_dense_maps_expand(nrows, nrows, rowptr, colidx, val0, nullptr, val1, got, dout);
    if (bad < 0) return -1;
    if (bad > 0) return nrows + 1;
    forms = 2; bytes = dout[1]; pinned = 0;
  }
  if (out) { out[0] = forms; out[1] = dout[0]; out[2] = pinned; out[3] = bytes; }
  // the star and the diagonal, as gcge_hip_star_selfcheck lays them out
  const StarGeom& g = H.g;
  const long sy = g.nx, sz = (long)g.nx * g.ny;
  auto xrow = [&](long gq) -> long { return M.box != nullptr ? (long)H.inv[(size_t)gq] : gq; };
  auto there = [&](long gq) -> bool { return M.box == nullptr || H.inv[(size_t)gq] >= 0; };
  long bad = 0;
  std::vector<std::pair<long, double>> want, have;
  for (int r = 0; r < nrows; ++r) {
    want.clear(); have.clear();
    for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) want.emplace_back((long)colidx[q], val1[q]);
    if (star) {
      if (H.diag_src[(size_t)r] >= 0) have.emplace_back((long)r, gcge_vm_gather(val1, H.diag_src[(size_t)r]));
      const long gr = M.gpos(r);
      const int gz = (int)(gr / sz), gy = (int)((gr - (long)gz * sz) / sy), gx = (int)(gr - (long)gz * sz - (long)gy * sy);
      for (int k = 1; k <= STAR_R; ++k) {
        if (vm_bits(H.c.cx[k])) { if (gx - k >= 0 && there(gr - k)) have.emplace_back(xrow(gr - k), H.c.cx[k]); if (gx + k < g.nx && there(gr + k)) have.emplace_back(xrow(gr + k), H.c.cx[k]); }
        if (vm_bits(H.c.cy[k])) { if (gy - k >= 0 && there(gr - k * sy)) have.emplace_back(xrow(gr - k * sy), H.c.cy[k]); if (gy + k < g.ny && there(gr + k * sy)) have.emplace_back(xrow(gr + k * sy), H.c.cy[k]); }
        if (vm_bits(H.c.cz[k])) { if (gz - k >= 0 && there(gr - k * sz)) have.emplace_back(xrow(gr - k * sz), H.c.cz[k]); if (gz + k < g.nz && there(gr + k * sz)) have.emplace_back(xrow(gr + k * sz), H.c.cz[k]); }
      }
    }
    for (auto& e : got[(size_t)r]) have.emplace_back((long)e.first, e.second);
    auto less = [](const std::pair<long, double>& p, const std::pair<long, double>& q) { return p.first < q.first; };
    std::stable_sort(want.begin(), want.end(), less); std::stable_sort(have.begin(), have.end(), less);
    size_t i = 0, j = 0;
    while (i < want.size() || j < have.size()) {
      const long c = (j >= have.size() || (i < want.size() && want[i].first <= have[j].first)) ? want[i].first : have[j].first;
      double wv = 0.0, hv = 0.0, mag = 0.0; int nw = 0, nh = 0;
      while (i < want.size() && want[i].first == c) { wv += want[i].second; ++i; ++nw; }
      while (j < have.size() && have[j].first == c) { hv += have[j].second; mag = std::max(mag, std::abs(have[j].second)); ++j; ++nh; }
      if (nw == 0 || nh <= 1) { if (vm_bits(wv + 0.0) != vm_bits(hv + 0.0) && !(wv == 0.0 && hv == 0.0)) ++bad; }
      else if (std::abs(wv - hv) > 4.0 * 2.220446049250313e-16 * std::max(mag, std::abs(wv))) ++bad;
    }
  }
  return bad;
}
// The same question for a ROW SLAB (local columns, halo columns >= nrows behind `ghost`; box_of_local_col != NULL: a slab of a masked
// grid, the box index of every local column), asked of the stored values themselves: the split and the block form built from val0 with
// their maps, the maps replayed on val1 — diagonal, the star's remainder, every block slot and pad-8 slot — against the split and the
// block form built directly from val1, value for value as bits, structure for structure.  Returns the number of differing stored
// values (0: the update in place leaves what a creation from val1 stores), -1: neither a star nor a dense form, -2: the update would
// be declined (a pinned entry moved, a NaN on the diagonal).  out[0] forms found (1 star, 2 dense, 3 both), out[1] layers of blocks,
// out[2] pinned entries, out[3] halo columns among the star's remainder (a slab's maps must reach them).
extern "C" long gcge_hip_value_maps_selfcheck_slab(int nrows, int ncols_local, long row_begin, long nglobal, const int* ghost, const int* rowptr,
                                                   const int* colidx, const double* val0, const double* val1, int dense_mode, int nx, int ny,
                                                   int nz, const int* box_of_local_col, long* out) {
  const long nnz = rowptr[nrows];
  const int saved_mode = gcge_hip_spmm_dense_mode_get();
  gcge_hip_spmm_dense_mode(dense_mode);
  struct Restore { int m; ~Restore() { gcge_hip_spmm_dense_mode(m); } } restore{saved_mode};
  typedef std::vector<std::vector<std::pair<int, double>>> Rows;
  auto differing = [&](const Rows& a, const Rows& b) -> long {
    long bad = 0;
    for (int r = 0; r < nrows; ++r) {
      const auto &x = a[(size_t)r], &y = b[(size_t)r];
      if (x.size() != y.size()) { bad += (long)std::max(x.size(), y.size()); continue; }
      for (size_t i = 0; i < x.size(); ++i) bad += x[i].first != y[i].first || vm_bits(x[i].second) != vm_bits(y[i].second);
    }
    return bad;
  };
  StarHost H0, H1;
  H0.keep_maps = true;
  StarRows M0 = {nrows, ncols_local, row_begin, nglobal, ghost, rowptr, colidx, val0};
  if (box_of_local_col != nullptr && nx > 0 && ny > 0 && nz > 0) {
    M0.box = box_of_local_col; M0.bnx = nx; M0.bny = ny; M0.bnz = nz; M0.nglobal = (long)nx * ny * nz; M0.box_cols = ncols_local != nrows;
  }
  StarRows M1 = M0;
  M1.val = val1;
  Rows got0((size_t)nrows), got1((size_t)nrows);
  long d0[2] = {0, 0}, d1[2] = {0, 0}, bad = 0, pinned = 0, halo = 0;
  if (star_build_host(M0, &H0)) {
    const GcgeVmCoef coef = vm_coef(H0.c);
    for (long q = 0; q < nnz; ++q) {                    // the update's check
      const int p = H0.pin[(size_t)q];
      pinned += p != 0 && p != GCGE_VM_PIN_DIAG;
      if (gcge_vm_check(val1[q], p, coef.c) != 0) return -2;
    }
    if (!star_build_host(M1, &H1)) return nrows + 1;
    if (memcmp(&H0.c, &H1.c, sizeof H0.c) != 0 || H0.rem_rowptr != H1.rem_rowptr || H0.rem_col != H1.rem_col || H0.clean != H1.clean) return nrows + 2;
    for (int r = 0; r < nrows; ++r) bad += vm_bits(gcge_vm_gather(val1, H0.diag_src[(size_t)r])) != vm_bits(H1.diag[(size_t)r]);
    std::vector<double> rem1(H0.rem_val.size());
    for (size_t e = 0; e < rem1.size(); ++e) {
      if (H0.rem_src[e] < -1 || H0.rem_src[e] >= nnz || H0.rem_code[e] >= GCGE_VM_NCODE) return nrows + 1;
      rem1[e] = gcge_vm_replay(val1, H0.rem_src[e], H0.rem_code[e], coef.c);
      bad += vm_bits(rem1[e]) != vm_bits(H1.rem_val[e]);
      halo += H0.rem_col[e] >= nrows;
    }
    const long b0 = gcge_dense_maps_expand(nrows, ncols_local, H0.rem_rowptr.data(), H0.rem_col.data(), H0.rem_val.data(), (const unsigned char*)H0.clean.data(),
                                           rem1.data(), got0, d0);
    const long b1 = gcge_dense_maps_expand(nrows, ncols_local, H1.rem_rowptr.data(), H1.rem_col.data(), H1.rem_val.data(), (const unsigned char*)H1.clean.data(),
                                           H1.rem_val.data(), got1, d1);
    if (b0 == 0 && b1 == 0) {
      if (out) { out[0] = 1 | (d0[0] > 0 ? 2 : 0); out[1] = d0[0]; out[2] = pinned; out[3] = halo; }
      return bad + differing(got0, got1);
    }
    if (b0 > 0 || b1 > 0) return nrows + 1;
    for (auto& g : got0) g.clear();                     // (no block form under the star: the upload drops the star then)
    for (auto& g : got1) g.clear();
  }
  const long b0 = gcge_dense_maps_expand(nrows, ncols_local, rowptr, colidx, val0, nullptr, val1, got0, d0);
  const long b1 = gcge_dense_maps_expand(nrows, ncols_local, rowptr, colidx, val1, nullptr, val1, got1, d1);
  if (b0 < 0 || b1 < 0) return -1;
  if (b0 > 0 || b1 > 0) return nrows + 1;
  if (out) { out[0] = 2; out[1] = d0[0]; out[2] = 0; out[3] = 0; }
  return differing(got0, got1);
}
extern "C" long gcge_hip_value_maps_selfcheck(int nrows, const int* rowptr, const int* colidx, const double* val0, const double* val1, int dense_mode,
                                              long* out) {
  return value_maps_selfcheck(nrows, rowptr, colidx, val0, val1, dense_mode, 0, 0, 0, nullptr, out);
}
extern "C" long gcge_hip_value_maps_selfcheck_grid(int nrows, const int* rowptr, const int* colidx, const double* val0, const double* val1, int dense_mode,
                                                   int nx, int ny, int nz, const int* box_of_row, long* out) {
  return value_maps_selfcheck(nrows, rowptr, colidx, val0, val1, dense_mode, nx, ny, nz, box_of_row, out);
}
