// Matrices from DEVICE-resident CSR arrays (gcge_hip_mat_create_device, include/gcge_hip.h) and blocks of vectors out to and in from
// device memory (gcge_hip_mv_to_device, gcge_hip_mv_from_device): the ways in and out of the back-end that never touch the host with
// O(n) data.
//
// The constructor checks its input on the device (rowptr alone first, then the columns by position: nothing is addressed through a
// value that has not been checked), copies the CSR, builds the pad-8 copy (hipcub scan of (len + 7) / 8 + a fill kernel, pads
// (own row, 0.0) as in mat_upload.hip) and searches for a pattern table.  build_patterns (mat_upload.hip) is split in two:
//   (a) "every row gets the id of its class, ids by first occurrence" — here by kernels: a 64-bit hash per row (the host's mixer), a
//       small open-addressing table in global memory (64-bit atomicCAS on the keys, atomicMin on the first row), a verify pass that
//       compares every row with the first row of its class entry by entry, as bits (a mismatch is a hash collision: give up), ids
//       from the ascending first rows, a pid pass with a histogram;
//   (b) the table itself — pattern_table.h, the SAME host code for both paths, fed with the class representatives (at most 64 KB),
//       the histogram, and for the chain layout the distinct 64-bit row keys in order of first occurrence, which a second run of the
//       same class machinery finds (keys are exact there: nothing to verify).
// Only a RUN HEAD — a row whose key differs from row r - 1's — touches the table: the interior rows of a stencil matrix share one
// class and an atomic per row on one address would serialise the chip; the first row of a class is always a run head, so the
// atomicMin over run heads is still the first occurrence.  Integer atomics only, no kernel waits for another, and which slot a key
// lands in is the only thing scheduling decides: ids come from the first rows.  Probing is bounded: more classes than a table holds
// (a counter) is "not a pattern matrix".
// Equality: two rows are one class when their lengths and every (column - row, value bits) agree; see gcge_hip.h for the one case in
// which the host's comparison with the previous row's pattern merges more.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "gcge_hip.h"
#include "gcge_hip_internal.h"
#include "pattern_table.h"

static long g_md_stats[4] = {0, 0, 0, 0};
static int g_md_hash_bits = 64;
extern "C" void gcge_hip_mat_device_stats(long out[4]) { for (int i = 0; i < 4; ++i) out[i] = g_md_stats[i]; }
extern "C" void gcge_hip_mat_device_hash_bits(int bits) { g_md_hash_bits = bits < 0 ? 0 : bits > 64 ? 64 : bits; }

static hipStream_t md_stream() { return (hipStream_t)gcge_hip_stream(); }
static unsigned md_blocks(long n, int bs) { return (unsigned)((n + bs - 1) / bs); }
static void md_download(void* dst, const void* src, size_t bytes) {   // (synchronises the stream first: the kernels before it are done)
  GCGE_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, md_stream()));
  GCGE_HIP_CHECK(hipStreamSynchronize(md_stream()));
  g_md_stats[3] += (long)bytes;
}
template <class T> static T* md_alloc(size_t count) { T* p = nullptr; GCGE_HIP_CHECK(hipMalloc(&p, (count ? count : 1) * sizeof(T))); return p; }

#define MD_EMPTY 0xFFFFFFFFFFFFFFFFull
#define MD_BS 256
#define MD_MAXPAT 1024          // bins of the pid pass's LDS histogram (a table of width 7 holds 585 patterns)

// ------------------------------------------------------------------------------------------------------------------- input checks
// flag bits: 1 rowptr[0] != 0, 2 a decreasing pair, 4 rowptr[nrows] != nnz, 8 a column out of range.  out[0] = flags, out[1] = the
// longest row (meaningful when the flags stay 0).  Reads rowptr[0 .. nrows] only.
__global__ void k_md_check_rowptr(int n, long nnz, const int* __restrict__ rp, int* __restrict__ out) {
  __shared__ int smax;
  if (threadIdx.x == 0) smax = 0;
  __syncthreads();
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) {
    const int a = rp[i];
    int bad = 0;
    if (i == 0 && a != 0) bad |= 1;
    if (i == n && (long)a != nnz) bad |= 4;
    if (i < n) {
      const int b = rp[i + 1];
      if (b < a) bad |= 2; else { const long len = (long)b - a; atomicMax(&smax, len > INT_MAX ? INT_MAX : (int)len); }
    }
    if (bad) atomicOr(&out[0], bad);
  }
  __syncthreads();
  if (threadIdx.x == 0 && smax > 0) atomicMax(&out[1], smax);
}
// reads colidx[0 .. nnz) by position
__global__ void k_md_check_cols(long nnz, int n, const int* __restrict__ ci, int* __restrict__ out) {
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  const int c = ci[k];
  if (c < 0 || c >= n) atomicOr(&out[0], 8);
}

// ------------------------------------------------------------------------------------------------------------------- pad-8 copy
__global__ void k_md_octets(int n, const int* __restrict__ rp, int* __restrict__ octs) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  octs[i] = i < n ? (rp[i + 1] - rp[i] + 7) / 8 : 0;
}
__global__ void k_md_pad8_fill(int n, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ va,
                               const int* __restrict__ orp, int* __restrict__ pc, double* __restrict__ pv) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  size_t o = (size_t)orp[r] * 8;
  const size_t end = (size_t)orp[r + 1] * 8;
  for (int k = rp[r]; k < rp[r + 1]; ++k, ++o) { pc[o] = ci[k]; pv[o] = va[k]; }
  for (; o < end; ++o) { pc[o] = (int)r; pv[o] = 0.0; }
}

// ------------------------------------------------------------------------------------------------------------------- (a) row classes
// the host's row hash (build_patterns), cut to its low bits; MD_EMPTY marks a free slot of the table and is never a key
__global__ void k_md_row_hash(int n, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ va, uint64_t mask,
                              uint64_t* __restrict__ key) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int q0 = rp[r], q1 = rp[r + 1];
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)(q1 - q0);
  for (int q = q0; q < q1; ++q) {
    const uint64_t vb = (uint64_t)__double_as_longlong(va[q]);
    h = (h ^ (uint64_t)((long)ci[q] - r)) * 0xBF58476D1CE4E5B9ull; h ^= h >> 29;
    h = (h ^ vb) * 0x94D049BB133111EBull; h ^= h >> 32;
  }
  h &= mask;
  key[r] = h == MD_EMPTY ? MD_EMPTY - 1 : h;
}
// the chain layout's key of every row (gcge_pat_row_key, pattern_table.h)
struct MdSlots { long s[16]; };
__global__ void k_md_chain_key(int n, const unsigned short* __restrict__ pid, long S, int nslot_used, MdSlots slots, uint64_t* __restrict__ key) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  unsigned mask = 0;
  for (int q = 0; q < nslot_used; ++q) { const long c = r + slots.s[q]; if (c < 0 || c >= n) mask |= 1u << q; }
  const unsigned head = r < S, tail = r + S >= n;
  key[r] = ((uint64_t)pid[r] << 32) | ((uint64_t)head << 31) | ((uint64_t)tail << 30) | mask;
}

__global__ void k_md_table_init(int T, uint64_t* __restrict__ tkey, int* __restrict__ tfirst) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < T) { tkey[s] = MD_EMPTY; tfirst[s] = INT_MAX; }
}
static __device__ __forceinline__ unsigned md_home(uint64_t k, int shift) { return (unsigned)((k * 0x9E3779B97F4A7C15ull) >> shift); }
// run heads enter their key; count[0] = distinct keys so far.  Once it passes maxpat the answer is "too many" whatever else happens,
// so every thread may stop: at most T probes per run head, and none once the counter is over.
__global__ void k_md_insert(int n, const uint64_t* __restrict__ key, int T, int shift, uint64_t* __restrict__ tkey, int* __restrict__ tfirst,
                            int* __restrict__ count, int maxpat) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint64_t k = key[r];
  if (r > 0 && key[r - 1] == k) return;
  unsigned s = md_home(k, shift);
  for (int probe = 0; probe < T; ++probe, s = (s + 1) & (unsigned)(T - 1)) {
    if (__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > maxpat) return;
    const unsigned long long old = atomicCAS((unsigned long long*)&tkey[s], (unsigned long long)MD_EMPTY, (unsigned long long)k);
    if (old == MD_EMPTY) atomicAdd(count, 1);
    if (old == MD_EMPTY || old == k) { atomicMin(&tfirst[s], (int)r); return; }
  }
  atomicMax(count, maxpat + 1);       // (a full table: cannot happen while the counter is at most maxpat < T)
}
// ids from the ascending first rows: slot_id[s] = how many classes start before this one (-1: a free slot), rep_first[id] = its first row
__global__ void k_md_rank(int T, const uint64_t* __restrict__ tkey, const int* __restrict__ tfirst, int* __restrict__ slot_id, int* __restrict__ rep_first) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= T) return;
  if (tkey[s] == MD_EMPTY) { slot_id[s] = -1; return; }
  const int f = tfirst[s];
  int id = 0;
  for (int q = 0; q < T; ++q) id += (tkey[q] != MD_EMPTY && tfirst[q] < f) ? 1 : 0;
  slot_id[s] = id; rep_first[id] = f;
}
// every row: the id of its key's class; verify != 0: the row against the first row of the class, as bits (flag |= 1: a collision);
// freq != NULL: rows per id (an LDS histogram per block, one global atomic per block and id that occurs in it).  flag |= 2: a key
// that is not in the table (cannot happen: every key's first row is a run head).
__global__ void k_md_pid(int n, const uint64_t* __restrict__ key, int T, int shift, const uint64_t* __restrict__ tkey, const int* __restrict__ slot_id,
                         const int* __restrict__ rep_first, int verify, const int* __restrict__ rp, const int* __restrict__ ci,
                         const double* __restrict__ va, unsigned short* __restrict__ pid, unsigned long long* __restrict__ freq, int npat,
                         int* __restrict__ flag) {
  __shared__ unsigned hist[MD_MAXPAT];
  if (freq != nullptr) { for (int b = threadIdx.x; b < npat; b += blockDim.x) hist[b] = 0; __syncthreads(); }
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) {
    const uint64_t k = key[r];
    unsigned s = md_home(k, shift);
    int id = -1;
    for (int probe = 0; probe < T; ++probe, s = (s + 1) & (unsigned)(T - 1)) {
      const uint64_t t = tkey[s];
      if (t == k) { id = slot_id[s]; break; }
      if (t == MD_EMPTY) break;
    }
    if (id < 0 || id >= npat) { atomicOr(flag, 2); id = 0; }
    else if (verify) {
      const int f = rep_first[id];
      if (f != (int)r) {
        const int q0 = rp[r], len = rp[r + 1] - q0, g0 = rp[f];
        bool same = len == rp[f + 1] - g0;
        for (int e = 0; same && e < len; ++e)
          same = ((long)ci[q0 + e] - r == (long)ci[g0 + e] - f) && __double_as_longlong(va[q0 + e]) == __double_as_longlong(va[g0 + e]);
        if (!same && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(flag, 1);
      }
    }
    pid[r] = (unsigned short)id;
    if (freq != nullptr) atomicAdd(&hist[id], 1u);
  }
  if (freq != nullptr) {
    __syncthreads();
    for (int b = threadIdx.x; b < npat; b += blockDim.x) if (hist[b] != 0) atomicAdd(&freq[b], (unsigned long long)hist[b]);
  }
}
// the class representatives as table rows of lt entries {value, column - row}, padded with {0.0, 0}
__global__ void k_md_reps(int npat, int lt, const int* __restrict__ rep_first, const int* __restrict__ rp, const int* __restrict__ ci,
                          const double* __restrict__ va, GcgePatEntry* __restrict__ tab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npat * lt) return;
  const int p = i / lt, k = i % lt, f = rep_first[p], q = rp[f] + k;
  GcgePatEntry e = {0.0, 0};
  if (q < rp[f + 1]) { e.val = va[q]; e.off = (long)ci[q] - f; }
  tab[i] = e;
}
__global__ void k_md_rep_keys(int npat, const int* __restrict__ rep_first, const uint64_t* __restrict__ key, uint64_t* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < npat) out[p] = key[rep_first[p]];
}

// The classes of d_key[0 .. n): ids by first occurrence into d_pid, *npat_out of them, their first rows in d_rep_first (maxpat ints).
// 0: done, 1: more than maxpat classes, 2: a row differs from the first row of its class (verify).
struct MdTable { int T, shift; uint64_t* tkey; int *tfirst, *slot_id, *count; };
static int md_classes(int n, const uint64_t* d_key, int maxpat, const MdTable& tb, int verify, const int* rp, const int* ci, const double* va,
                      unsigned short* d_pid, unsigned long long* d_freq, int* d_rep_first, int* npat_out) {
  hipStream_t st = md_stream();
  GCGE_HIP_CHECK(hipMemsetAsync(tb.count, 0, 2 * sizeof(int), st));      // count[0]: classes, count[1]: flags of the pid pass
  k_md_table_init<<<md_blocks(tb.T, MD_BS), MD_BS, 0, st>>>(tb.T, tb.tkey, tb.tfirst);
  k_md_insert<<<md_blocks(n, MD_BS), MD_BS, 0, st>>>(n, d_key, tb.T, tb.shift, tb.tkey, tb.tfirst, tb.count, maxpat);
  int npat = 0;
  md_download(&npat, tb.count, sizeof(int));
  if (npat > maxpat) return 1;
  k_md_rank<<<md_blocks(tb.T, MD_BS), MD_BS, 0, st>>>(tb.T, tb.tkey, tb.tfirst, tb.slot_id, d_rep_first);
  if (d_freq != nullptr) GCGE_HIP_CHECK(hipMemsetAsync(d_freq, 0, (size_t)npat * sizeof(unsigned long long), st));
  k_md_pid<<<md_blocks(n, MD_BS), MD_BS, 0, st>>>(n, d_key, tb.T, tb.shift, tb.tkey, tb.slot_id, d_rep_first, verify, rp, ci, va, d_pid, d_freq, npat,
                                                  tb.count + 1);
  int flag = 0;
  md_download(&flag, tb.count + 1, sizeof(int));
  GCGE_REQUIRE((flag & 2) == 0, "device pattern search: every row key is in the table");
  *npat_out = npat;
  return (flag & 1) ? 2 : 0;
}

// The pattern search on device arrays that passed the checks.  true: *pid_out (nrows ids, hipMalloc'd) and tab / spans as
// build_patterns would leave them; false: no pattern form from here (*collision: because of a hash collision).
struct MdPattern { unsigned short* d_pid; std::vector<GcgePatEntry> tab; int npat, lt; long span, span2, near; };
static bool md_pattern_search(int n, const int* rp, const int* ci, const double* va, int lt, MdPattern& out, bool* collision) {
  hipStream_t st = md_stream();
  const int maxpat = gcge_pat_max_patterns(lt);
  if (maxpat > MD_MAXPAT) return false;
  MdTable tb;
  tb.T = 1; int lg = 0;
  while (tb.T < 4 * maxpat) { tb.T *= 2; ++lg; }
  tb.shift = 64 - lg;
  tb.tkey = md_alloc<uint64_t>((size_t)tb.T); tb.tfirst = md_alloc<int>((size_t)tb.T); tb.slot_id = md_alloc<int>((size_t)tb.T);
  tb.count = md_alloc<int>(2);
  uint64_t* d_key = md_alloc<uint64_t>((size_t)n);
  unsigned short *d_pid = md_alloc<unsigned short>((size_t)n), *d_cpid = nullptr;
  unsigned long long* d_freq = md_alloc<unsigned long long>((size_t)maxpat);
  int* d_rep = md_alloc<int>((size_t)maxpat);
  GcgePatEntry* d_tab = md_alloc<GcgePatEntry>((size_t)maxpat * lt);
  uint64_t* d_keys_out = md_alloc<uint64_t>((size_t)maxpat);
  bool ok = false;
  do {
    const uint64_t mask = g_md_hash_bits >= 64 ? ~0ull : ((1ull << g_md_hash_bits) - 1ull);
    k_md_row_hash<<<md_blocks(n, MD_BS), MD_BS, 0, st>>>(n, rp, ci, va, mask, d_key);
    int npat = 0;
    const int rc = md_classes(n, d_key, maxpat, tb, 1, rp, ci, va, d_pid, d_freq, d_rep, &npat);
    if (rc != 0) { *collision = rc == 2; break; }
    k_md_reps<<<md_blocks((long)npat * lt, MD_BS), MD_BS, 0, st>>>(npat, lt, d_rep, rp, ci, va, d_tab);
    out.tab.resize((size_t)npat * lt);
    std::vector<unsigned long long> fq((size_t)npat);
    GCGE_HIP_CHECK(hipMemcpyAsync(fq.data(), d_freq, fq.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    g_md_stats[3] += (long)(fq.size() * sizeof(unsigned long long));
    md_download(out.tab.data(), d_tab, out.tab.size() * sizeof(GcgePatEntry));
    // (b): the host code of build_patterns
    std::vector<long> freq(fq.begin(), fq.end());
    GcgePatPlan plan;
    gcge_pat_plan(out.tab, freq, lt, plan);
    out.npat = npat; out.lt = lt; out.span = plan.span; out.span2 = plan.span2; out.near = 0;
    if (plan.chain) {
      MdSlots sl;
      for (int q = 0; q < 16; ++q) sl.s[q] = q < lt ? plan.slot[q] : 0;
      k_md_chain_key<<<md_blocks(n, MD_BS), MD_BS, 0, st>>>(n, d_pid, plan.S, plan.nslot_used, sl, d_key);
      d_cpid = md_alloc<unsigned short>((size_t)n);
      int nkey = 0;
      if (md_classes(n, d_key, maxpat, tb, 0, rp, ci, va, d_cpid, nullptr, d_rep, &nkey) == 0) {
        k_md_rep_keys<<<md_blocks(nkey, MD_BS), MD_BS, 0, st>>>(nkey, d_rep, d_key, d_keys_out);
        std::vector<uint64_t> keys((size_t)nkey);
        md_download(keys.data(), d_keys_out, keys.size() * sizeof(uint64_t));
        std::vector<GcgePatEntry> ctab;
        if (gcge_pat_chain_table(plan, keys, ctab)) {
          out.tab.swap(ctab); std::swap(d_pid, d_cpid);
          out.npat = nkey;
          gcge_pat_chain_spans(plan, out.tab, &out.span2, &out.near);
        }
      }
    }
    ok = true;
  } while (0);
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  hipFree(tb.tkey); hipFree(tb.tfirst); hipFree(tb.slot_id); hipFree(tb.count);
  hipFree(d_key); hipFree(d_freq); hipFree(d_rep); hipFree(d_tab); hipFree(d_keys_out);
  if (d_cpid != nullptr) hipFree(d_cpid);
  if (ok) out.d_pid = d_pid; else hipFree(d_pid);
  return ok;
}

// ------------------------------------------------------------------------------------------------------------------- the constructor
// (the checks have vouched for rowptr[0] == 0 and rowptr[nrows] == nnz: the entries between them come back)
static GCGE_HIP_MAT* md_fall_back(int nrows, long nnz, const int* d_rp, const int* d_ci, const double* d_va, bool as_given) {
  std::vector<int> rp((size_t)nrows + 1), ci((size_t)(nnz ? nnz : 1));
  std::vector<double> va((size_t)(nnz ? nnz : 1));
  rp[0] = 0; rp[(size_t)nrows] = (int)nnz;
  if (nrows > 1) GCGE_HIP_CHECK(hipMemcpyAsync(rp.data() + 1, d_rp + 1, ((size_t)nrows - 1) * sizeof(int), hipMemcpyDeviceToHost, md_stream()));
  if (nnz > 0) {
    GCGE_HIP_CHECK(hipMemcpyAsync(ci.data(), d_ci, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost, md_stream()));
    GCGE_HIP_CHECK(hipMemcpyAsync(va.data(), d_va, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost, md_stream()));
  }
  GCGE_HIP_CHECK(hipStreamSynchronize(md_stream()));
  g_md_stats[1] += 1;
  g_md_stats[3] += (long)(((size_t)nrows - 1) * sizeof(int) + (size_t)nnz * (sizeof(int) + sizeof(double)));
  return as_given ? gcge_hip_mat_create_as_given(nrows, rp.data(), ci.data(), va.data())
                  : gcge_hip_mat_create(nrows, nrows, 0, rp.data(), ci.data(), va.data());
}

static GCGE_HIP_MAT* md_create(int nrows, long nnz, const int* d_rp, const int* d_ci, const double* d_va, bool as_given) {
  const char* who = as_given ? "gcge_hip_mat_create_device_as_given" : "gcge_hip_mat_create_device";
  if (!gcge_mat_device_args_ok(nrows, nnz, d_rp, d_ci, d_va)) {
    fprintf(stderr, "%s: refused: nrows >= 1, 0 <= nnz < 2^31 and device arrays are required\n", who);
    return nullptr;
  }
  if (gcge_hip_init(-1) != 0) return nullptr;
  hipStream_t st = md_stream();
  // the checks: rowptr by itself (rowptr[0 .. nrows] only), the columns by position (colidx[0 .. nnz) only); reported in that order
  int* d_chk = md_alloc<int>(2);
  int chk[2] = {0, 0};
  GCGE_HIP_CHECK(hipMemsetAsync(d_chk, 0, 2 * sizeof(int), st));
  k_md_check_rowptr<<<md_blocks((long)nrows + 1, MD_BS), MD_BS, 0, st>>>(nrows, nnz, d_rp, d_chk);
  if (nnz > 0) k_md_check_cols<<<md_blocks(nnz, MD_BS), MD_BS, 0, st>>>(nnz, nrows, d_ci, d_chk);   // (by position: independent of rowptr)
  md_download(chk, d_chk, 2 * sizeof(int));
  hipFree(d_chk);
  if (chk[0] != 0) {
    fprintf(stderr, "%s: refused: %s\n", who, (chk[0] & 1) ? "rowptr[0] is not 0" : (chk[0] & 2) ? "rowptr decreases" :
            (chk[0] & 4) ? "rowptr[nrows] is not nnz" : "a column index is outside [0, nrows)");
    return nullptr;
  }
  const int maxlen = chk[1];
  // a re-ordered matrix of this size is live: the new one has to adopt its order, which the host path does
  if (!as_given) { const GcgePerm* P = gcge_hip_perm_live(nrows); if (P != nullptr && !P->identity) return md_fall_back(nrows, nnz, d_rp, d_ci, d_va, false); }
  const int lt = gcge_hip_pattern_width(maxlen);
  MdPattern pat; pat.d_pid = nullptr;
  bool collision = false;
  if (lt == 0 || gcge_hip_spmm_tile_mode_get() == 2 || !md_pattern_search(nrows, d_rp, d_ci, d_va, lt, pat, &collision)) {
    if (collision) g_md_stats[2] += 1;
    return md_fall_back(nrows, nnz, d_rp, d_ci, d_va, as_given);
  }
  // the handle gcge_hip_mat_create_as_given makes of a pattern matrix: CSR and pad-8 copies, pid + table, the identity order
  GCGE_HIP_MAT* A = (GCGE_HIP_MAT*)calloc(1, sizeof(GCGE_HIP_MAT));
  A->nrows = nrows; A->nglobal = nrows; A->row_begin = 0; A->nnz = nnz; A->nghost = 0;
  A->d_rowptr = md_alloc<int>((size_t)nrows + 1); A->d_colidx = md_alloc<int>((size_t)nnz); A->d_val = md_alloc<double>((size_t)nnz);
  GCGE_HIP_CHECK(hipMemcpyAsync(A->d_rowptr, d_rp, ((size_t)nrows + 1) * sizeof(int), hipMemcpyDeviceToDevice, st));
  if (nnz > 0) {
    GCGE_HIP_CHECK(hipMemcpyAsync(A->d_colidx, d_ci, (size_t)nnz * sizeof(int), hipMemcpyDeviceToDevice, st));
    GCGE_HIP_CHECK(hipMemcpyAsync(A->d_val, d_va, (size_t)nnz * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  int* d_octs = md_alloc<int>((size_t)nrows + 1);
  A->d_orp = md_alloc<int>((size_t)nrows + 1);
  k_md_octets<<<md_blocks((long)nrows + 1, MD_BS), MD_BS, 0, st>>>(nrows, d_rp, d_octs);
  size_t bytes = 0;
  GCGE_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_octs, A->d_orp, nrows + 1, st));
  void* tmp = nullptr;
  GCGE_HIP_CHECK(hipMalloc(&tmp, bytes ? bytes : 8));
  GCGE_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, d_octs, A->d_orp, nrows + 1, st));
  int noct = 0;
  md_download(&noct, A->d_orp + nrows, sizeof(int));
  hipFree(tmp); hipFree(d_octs);
  A->noct = noct;
  A->d_pcol = md_alloc<int>((size_t)noct * 8); A->d_pval = md_alloc<double>((size_t)noct * 8);
  k_md_pad8_fill<<<md_blocks(nrows, MD_BS), MD_BS, 0, st>>>(nrows, d_rp, d_ci, d_va, A->d_orp, A->d_pcol, A->d_pval);
  A->d_pid = pat.d_pid; A->npat = pat.npat; A->pat_lt = pat.lt; A->pat_span = pat.span; A->pat_span2 = pat.span2; A->pat_near = pat.near;
  GCGE_HIP_CHECK(hipMalloc(&A->d_tab, pat.tab.size() * sizeof(GcgePatEntry)));
  GCGE_HIP_CHECK(hipMemcpyAsync(A->d_tab, pat.tab.data(), pat.tab.size() * sizeof(GcgePatEntry), hipMemcpyHostToDevice, st));
  GCGE_HIP_CHECK(hipStreamSynchronize(st));
  A->ov_lo = 0; A->ov_hi = nrows;
  if (GcgePerm* P = gcge_hip_perm_identity(nrows)) A->perm = gcge_hip_perm_acquire(P);
  g_md_stats[0] += 1;
  return A;
}
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_device(int nrows, long nnz, const int* d_rowptr, const int* d_colidx, const double* d_val) {
  return md_create(nrows, nnz, d_rowptr, d_colidx, d_val, false);
}
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_device_as_given(int nrows, long nnz, const int* d_rowptr, const int* d_colidx, const double* d_val) {
  return md_create(nrows, nnz, d_rowptr, d_colidx, d_val, true);
}

extern "C" long gcge_hip_mat_pattern_table(const GCGE_HIP_MAT* A, unsigned short* pid_out, void* tab_out) {
  if (A == nullptr || A->d_pid == nullptr) return 0;
  const size_t nt = (size_t)A->npat * A->pat_lt;
  GCGE_HIP_CHECK(hipStreamSynchronize(md_stream()));
  if (pid_out != nullptr) GCGE_HIP_CHECK(hipMemcpy(pid_out, A->d_pid, (size_t)A->nrows * sizeof(unsigned short), hipMemcpyDeviceToHost));
  if (tab_out != nullptr) GCGE_HIP_CHECK(hipMemcpy(tab_out, A->d_tab, nt * sizeof(GcgePatEntry), hipMemcpyDeviceToHost));
  return (long)nt;
}

// ------------------------------------------------------------------------------------------------------------------- blocks out
// d_out[row(i) * ldo + j] = block[i * ld + c0 + j]; row(i) = perm[i] for a block that lives in the back-end's own order
__global__ void k_md_mv_gather(int n, int m, const double* __restrict__ src, long ld, const int* __restrict__ perm, double* __restrict__ out, long ldo) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n * m) return;
  const long i = t / m; const int j = (int)(t % m);
  const long r = perm != nullptr ? perm[i] : i;
  out[r * ldo + j] = src[i * ld + j];
}
// the block's row order on the device for one call (NULL: the caller's order); freed by the caller after its kernel is done
static int* md_perm_upload(const GcgePerm* P, int n) {
  if (P == nullptr) return nullptr;
  int* d_perm = md_alloc<int>((size_t)n);
  GCGE_HIP_CHECK(hipMemcpyAsync(d_perm, P->perm, (size_t)n * sizeof(int), hipMemcpyHostToDevice, md_stream()));
  return d_perm;
}
extern "C" void gcge_hip_mv_to_device(void** mv, int c0, int c1, double* d_out, long ldo) {
  gcge_hip_apply_pending();
  GcgeHipMV* v = (GcgeHipMV*)mv;
  const int n = v->nrows, m = c1 - c0;
  GCGE_REQUIRE(c0 >= 0 && c1 <= v->ncols && m >= 0 && ldo >= m && d_out != nullptr, "gcge_hip_mv_to_device: ranges");
  if (m == 0 || n == 0) return;
  int* d_perm = md_perm_upload(real_perm(v->perm), n);
  k_md_mv_gather<<<md_blocks((long)n * m, MD_BS), MD_BS, 0, md_stream()>>>(n, m, v->d + c0, v->ld, d_perm, d_out, ldo);
  GCGE_HIP_CHECK(hipStreamSynchronize(md_stream()));
  if (d_perm != nullptr) hipFree(d_perm);
}

// ------------------------------------------------------------------------------------------------------------------- blocks in
// block[i * ld + c0 + j] = d_in[row(i) * row_stride + j * col_stride]; row(i) = perm[i] for a block that lives in the back-end's own
// order (the direction of gcge_hip_mv_from_host, the inverse of k_md_mv_gather).  Three forms:
//   rows contiguous (col_stride == 1): k_md_rows_in, the row-slab form of the block-stream kernels in vec_kernels.hip — tpr lanes walk
//     a row, a block owns a contiguous slab of rows, four rows are in flight per lane, no division on a flattened index; a lane
//     moves 16 bytes where source and destination columns are both 16-byte aligned (one 8-byte head lane in front of an odd first
//     column, one behind an odd last one) and 8 bytes where their parities differ; the source row is read through perm[i], the
//     destination rows stay in order;
//   columns contiguous (row_stride == 1), no permutation: the padded 32 x 32 LDS transpose of the host path
//     (gcge_hip_colmajor_to_rowmajor), both sides coalesced;
//   everything else: k_md_elems_in, one element per thread by 2-D indexing — coalesced on the destination only.
typedef double v2d_md __attribute__((ext_vector_type(2)));
#define MD_IN_COLS 256           // columns per launch of the row form (one lane per column at most: tpr <= 256)
__global__ __launch_bounds__(256) void k_md_rows_in(long n, int m, const double* __restrict__ src, long lds, const int* __restrict__ perm,
                                                    double* __restrict__ dst, long ldd, int head, int wide, int nl, int tpr) {
  const int tx = threadIdx.x % tpr, ty = threadIdx.x / tpr, rpb = 256 / tpr;
  if (tx >= nl) return;
  int j, w;
  if (!wide) { j = tx; w = 1; }
  else if (tx < head) { j = 0; w = 1; }
  else { j = head + 2 * (tx - head); w = min(2, m - j); }
  const long slab = (((n + gridDim.x - 1) / gridDim.x) + rpb - 1) / rpb * rpb;
  const long rend = min(n, ((long)blockIdx.x + 1) * slab);
  long row = (long)blockIdx.x * slab + ty;
  if (w == 2) {
    for (; row + 3L * rpb < rend; row += 4L * rpb) {
      long sr[4]; v2d_md a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const long r = row + (long)u * rpb; sr[u] = perm != nullptr ? (long)perm[r] : r; }
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d_md*>(src + sr[u] * lds + j));
#pragma unroll
      for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(a[u], reinterpret_cast<v2d_md*>(dst + (row + (long)u * rpb) * ldd + j));
    }
    for (; row < rend; row += rpb) {
      const long s = perm != nullptr ? (long)perm[row] : row;
      *reinterpret_cast<v2d_md*>(dst + row * ldd + j) = *reinterpret_cast<const v2d_md*>(src + s * lds + j);
    }
  } else {
    for (; row + 3L * rpb < rend; row += 4L * rpb) {
      long sr[4]; double a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const long r = row + (long)u * rpb; sr[u] = perm != nullptr ? (long)perm[r] : r; }
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = __builtin_nontemporal_load(src + sr[u] * lds + j);
#pragma unroll
      for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(a[u], dst + (row + (long)u * rpb) * ldd + j);
    }
    for (; row < rend; row += rpb) {
      const long s = perm != nullptr ? (long)perm[row] : row;
      dst[row * ldd + j] = src[s * lds + j];
    }
  }
}
// the slow form: 16 x 16 threads, columns along x
__global__ __launch_bounds__(256) void k_md_elems_in(long n, int m, const double* __restrict__ src, long rs, long cs, const int* __restrict__ perm,
                                                     double* __restrict__ dst, long ldd) {
  const long i = (long)blockIdx.x * 16 + threadIdx.y;
  if (i >= n) return;
  const long s = perm != nullptr ? (long)perm[i] : i;
  for (int j = threadIdx.x; j < m; j += 16) dst[i * ldd + j] = src[s * rs + (long)j * cs];
}
static void md_rows_in(int n, int m, const double* src, long lds, const int* d_perm, double* dst, long ldd) {
  // 16-byte lanes need even strides and the same parity of the two first columns (the block itself is 16-byte aligned)
  const int pd = (((uintptr_t)dst & 15) == 8) ? 1 : 0, ps = (((uintptr_t)src & 15) == 8) ? 1 : 0;
  const int wide = (lds % 2 == 0 && ldd % 2 == 0 && pd == ps && m - pd >= 2) ? 1 : 0;
  const int head = wide ? pd : 0;
  const int nl = wide ? head + (m - head + 1) / 2 : m;
  int tpr = 1;
  while (tpr < nl) tpr *= 2;
  const int rpb = 256 / tpr;
  const long want = ((long)n + 4L * rpb - 1) / (4L * rpb);
  const unsigned grid = (unsigned)(want < 1 ? 1 : want > 8192 ? 8192 : want);
  k_md_rows_in<<<grid, 256, 0, md_stream()>>>((long)n, m, src, lds, d_perm, dst, ldd, head, wide, nl, tpr);
}
extern "C" void gcge_hip_mv_from_device(void** mv, int c0, int c1, const double* d_in, long row_stride, long col_stride) {
  gcge_hip_apply_pending();              // a held-back scaling is applied first and then overwritten, never applied to the new data
  GcgeHipMV* v = (GcgeHipMV*)mv;
  const int n = v->nrows, m = c1 - c0;
  GCGE_REQUIRE(c0 >= 0 && c0 <= c1 && c1 <= v->ncols, "gcge_hip_mv_from_device: column range");
  if (m == 0 || n == 0) return;
  GCGE_REQUIRE(d_in != nullptr && ((uintptr_t)d_in & 7) == 0 && row_stride >= 1 && col_stride >= 1, "gcge_hip_mv_from_device: source and strides");
  GCGE_REQUIRE((col_stride == 1 && row_stride >= m) || (row_stride == 1 && col_stride >= n) ||
               row_stride / col_stride >= m || col_stride / row_stride >= n, "gcge_hip_mv_from_device: no two entries of the source alias");
  GCGE_REQUIRE(row_stride <= (LONG_MAX / 16) / n && col_stride <= (LONG_MAX / 16) / m, "gcge_hip_mv_from_device: the source's extent");
  const uintptr_t s0 = (uintptr_t)d_in, s1 = s0 + (size_t)(((long)(n - 1) * row_stride + (long)(m - 1) * col_stride + 1) * (long)sizeof(double));
  const uintptr_t b0 = (uintptr_t)v->d, b1 = b0 + v->bytes;
  GCGE_REQUIRE(s1 <= b0 || b1 <= s0, "gcge_hip_mv_from_device: the source does not overlap the block");
  int* d_perm = md_perm_upload(real_perm(v->perm), n);
  double* dst = v->d + c0;
  if (col_stride == 1) {
    for (int c = 0; c < m; c += MD_IN_COLS) md_rows_in(n, m - c < MD_IN_COLS ? m - c : MD_IN_COLS, d_in + c, row_stride, d_perm, dst + c, v->ld);
  } else if (row_stride == 1 && d_perm == nullptr) {
    GCGE_REQUIRE(gcge_hip_colmajor_to_rowmajor(n, m, d_in, col_stride, dst, v->ld, md_stream()) == 0, "gcge_hip_mv_from_device: kernel launch");
  } else {
    k_md_elems_in<<<md_blocks(n, 16), dim3(16, 16), 0, md_stream()>>>((long)n, m, d_in, row_stride, col_stride, d_perm, dst, v->ld);
  }
  GCGE_HIP_CHECK(hipGetLastError());
  GCGE_HIP_CHECK(hipStreamSynchronize(md_stream()));
  if (d_perm != nullptr) hipFree(d_perm);
}
