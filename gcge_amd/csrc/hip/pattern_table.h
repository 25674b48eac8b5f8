// The table side of the pattern format (spmm_pattern.hip): host code that needs no HIP, so it also compiles alone under a sanitizer
// (the one piece kernels share, the slot rule below, is __host__ __device__ only when hipcc compiles it).
// A pattern search has two parts:
//   (a) every row gets the id of its class (rows equal as {(column - row, value bits)}), ids by first occurrence — done over all
//       rows, by build_patterns on the host arrays (mat_upload.hip) or by the kernels of mat_device.hip on device arrays;
//   (b) everything that works on the small table — the most frequent class and its spans, the canonical slots of the chain layout,
//       the per-class slot values and extras, the chain table from the distinct (class, head, tail, mask) keys — done HERE, by the
//       same code for both, from the class representatives (npat * lt entries), a histogram of ids, and the distinct row keys in
//       order of first occurrence.  What (b) makes of equal inputs is equal bit for bit by construction.
#ifndef GCGE_PATTERN_TABLE_H
#define GCGE_PATTERN_TABLE_H
#include <stdint.h>
#include <algorithm>
#include <vector>

struct GcgePatEntry { double val; long off; };

#if defined(__HIPCC__)
#define GCGE_PAT_HD __host__ __device__
#else
#define GCGE_PAT_HD
#endif
// The slot rule of the per-row values (d_rowval[8 r + slot], build_patterns in mat_upload.hip): the table slot that takes the entry
// with column offset `off` of a row whose table row is e[0 .. lt).  The diagonal sits in slot 1 of a chain-layout table (where slots
// whose address would leave the block also read offset 0); every other entry takes the first slot not used by an earlier entry of
// its row that carries its offset and a non-zero table value.  -1: no such slot, or slot 1 taken twice.  *used: the slots taken so far.
// Shared by the kernels of mat_values.hip and the host check in tools/pattern_values_check.cpp; build_patterns keeps its own copy.
static inline GCGE_PAT_HD int gcge_pat_value_slot(const GcgePatEntry* e, int lt, bool chain_layout, long off, unsigned* used) {
  int slot = -1;
  if (chain_layout && off == 0) slot = 1;
  else for (int k = 0; k < lt; ++k) if (!(*used >> k & 1) && e[k].off == off && e[k].val != 0.0) { slot = k; break; }
  if (slot < 0 || slot >= lt || (*used >> slot & 1)) return -1;
  *used |= 1u << slot;
  return slot;
}
// how many slots of a table row are present (table value != 0.0): a row of the matrix whose length differs stores a +-0.0
static inline GCGE_PAT_HD int gcge_pat_present_slots(const GcgePatEntry* e, int lt) {
  int c = 0;
  for (int k = 0; k < lt; ++k) c += e[k].val != 0.0 ? 1 : 0;
  return c;
}

// gcge_hip_mat_create_device's check of its arguments before anything is launched: a positive row count, 0 <= nnz < 2^31 (the
// pad-8 copy's octets, at most (nnz + 7 nrows) / 8, then fit an int as well), arrays that are there
static inline bool gcge_mat_device_args_ok(long nrows, long nnz, const void* rowptr, const void* colidx, const void* val) {
  const long imax = 2147483647L;
  if (nrows < 1 || nrows > imax || nnz < 0 || nnz > imax || rowptr == nullptr) return false;
  return nnz == 0 || (colidx != nullptr && val != nullptr);
}

// most patterns a table of width lt may hold (64 KB of table, ids in 16 bits)
static inline int gcge_pat_max_patterns(int lt) { return std::min(65535, (int)(64 * 1024 / (lt * sizeof(GcgePatEntry)))); }

struct GcgePatPlan {
  int lt = 0, npat = 0, common = 0;
  long span = 0, span2 = 0;              // longest and second longest |offset| of the most frequent pattern
  bool chain = false;                    // the chain layout has its slots: the rewrite goes on with the rows' keys
  long S = 0, Lline = 0;
  int nslot_used = 0;
  std::vector<long> slot;                // lt canonical offsets: [-S, 0, +S, (-L, +L,) the others ascending, 0 ...]
  std::vector<double> pval;              // npat * lt: every generic pattern's value on every canonical slot
  std::vector<std::vector<GcgePatEntry>> extras;   // per generic pattern: the entries that fit no slot (at most 2)
};

// (b), first half.  tab: npat * lt entries, freq: rows per pattern.
static inline void gcge_pat_plan(const std::vector<GcgePatEntry>& tab, const std::vector<long>& freq, int lt, GcgePatPlan& P) {
  P = GcgePatPlan();
  P.lt = lt; P.npat = (int)(tab.size() / lt);
  // reuse distance that matters for the launch geometry: the longest offset of the MOST FREQUENT pattern
  // (interior rows); boundary and halo patterns may reach much further
  const int common = P.common = (int)(std::max_element(freq.begin(), freq.end()) - freq.begin());
  for (int k = 0; k < lt; ++k) {
    const long o = tab[(size_t)common * lt + k].off;
    P.span = std::max(P.span, o < 0 ? -o : o);
  }
  for (int k = 0; k < lt; ++k) {
    const long o = tab[(size_t)common * lt + k].off, ao = o < 0 ? -o : o;
    if (ao < P.span) P.span2 = std::max(P.span2, ao);
  }
  // Chain layout (spmm_pattern_chain_kernel): possible when the interior stencil reaches -S, 0 and +S with S a
  // multiple of 32 rows and all patterns together use at most lt distinct offsets.  Every pattern is then rewritten
  // on the same slots [-S, 0, +S, the other offsets ascending]: entries a row does not have get value 0 but keep
  // their offset as long as the address stays inside the block of vectors (patterns are split by that validity),
  // so what a lane loads through a slot depends on its position only, never on its pattern.
  const long S = P.span;
  if (lt < 4 || S <= 0 || S % 32 != 0) return;
  // canonical slots: the offsets of the interior stencil, chain first
  std::vector<long> offs;
  { bool m = false, c = false, q = false;
    for (int k = 0; k < lt; ++k) {
      const GcgePatEntry& e = tab[(size_t)common * lt + k];
      if (e.val == 0.0 && e.off == 0) continue;
      offs.push_back(e.off); m |= e.off == -S; c |= e.off == 0; q |= e.off == S;
    }
    if (!(m && c && q)) return; }
  std::vector<long>& slot = P.slot;
  slot = {-S, 0, S};
  std::sort(offs.begin(), offs.end());
  // second longest offset L with both signs present: slots 3,4 (line exchange of spmm_pattern_chain2_kernel)
  long Lline = 0;
  for (long o : offs) { const long ao = o < 0 ? -o : o; if (ao < S && ao > Lline && std::binary_search(offs.begin(), offs.end(), -o)) Lline = ao; }
  if (Lline >= 8 && Lline % 8 == 0 && lt >= 5) { slot.push_back(-Lline); slot.push_back(Lline); } else Lline = 0;
  for (long o : offs) if (o != -S && o != 0 && o != S && !(Lline && (o == -Lline || o == Lline))) slot.push_back(o);
  const int nslot_used = (int)slot.size();
  if (nslot_used > lt) return;
  while ((int)slot.size() < lt) slot.push_back(0);            // unused slots: own row, value 0
  // per generic pattern: value on every canonical slot + the entries that fit no slot ("extras": halo columns of
  // a row slab).  An extra may ride in slot 0 of a row of the first S rows (no predecessor in the chain: slot 0 is
  // loaded explicitly when a wave starts) or in slot 2 of a row of the last S rows (no successor reads it).
  const int np = P.npat;
  P.pval.assign((size_t)np * lt, 0.0);
  P.extras.assign((size_t)np, std::vector<GcgePatEntry>());
  for (int p = 0; p < np; ++p)
    for (int k = 0; k < lt; ++k) {
      const GcgePatEntry& e = tab[(size_t)p * lt + k];
      if (e.val == 0.0 && e.off == 0) continue;
      int sidx = -1;
      for (int q = 0; q < nslot_used; ++q) if (slot[q] == e.off) { sidx = q; break; }
      if (sidx >= 0) P.pval[(size_t)p * lt + sidx] += e.val;
      else { P.extras[p].push_back(e); if (P.extras[p].size() > 2) return; }
    }
  P.S = S; P.Lline = Lline; P.nslot_used = nslot_used; P.chain = true;
}

// The key of row r in the chain layout: its generic pattern, whether it is one of the first / last S rows, and the slots whose
// canonical address leaves the block of vectors.  (mat_device.hip computes the same value in a kernel.)
static inline uint64_t gcge_pat_row_key(const GcgePatPlan& P, unsigned pid, long r, long nrows, long ncols_local) {
  unsigned mask = 0;
  for (int q = 0; q < P.nslot_used; ++q) { const long c = r + P.slot[q]; if (c < 0 || c >= ncols_local) mask |= 1u << q; }
  const unsigned head = r < P.S, tail = r + P.S >= nrows;
  return ((uint64_t)pid << 32) | ((uint64_t)head << 31) | ((uint64_t)tail << 30) | mask;
}

// (b), second half: the chain table from the distinct row keys in order of first occurrence (the new ids).  false: the rewrite
// does not apply (too many keys, an entry that would point outside the block, an extra without a free slot) — the plain table stays.
static inline bool gcge_pat_chain_table(const GcgePatPlan& P, const std::vector<uint64_t>& keys, std::vector<GcgePatEntry>& ctab) {
  const int lt = P.lt;
  ctab.clear();
  if (!P.chain || (int)keys.size() > gcge_pat_max_patterns(lt)) return false;
  bool ok = true;
  std::vector<GcgePatEntry> row((size_t)lt);
  for (const uint64_t key : keys) {
    const size_t pid = (size_t)(key >> 32);
    const unsigned head = (unsigned)(key >> 31) & 1u, tail = (unsigned)(key >> 30) & 1u, mask = (unsigned)(key & 0x3FFFFFFFu);
    if (pid >= (size_t)P.npat) return false;
    for (int q = 0; q < lt; ++q) {
      row[q].val = P.pval[pid * lt + q];
      row[q].off = (q < P.nslot_used && !(mask >> q & 1)) ? P.slot[q] : 0;
      if (mask >> q & 1) { if (row[q].val != 0.0) ok = false; row[q].val = 0.0; }   // an entry cannot point outside
    }
    for (const GcgePatEntry& e : P.extras[pid]) {
      if (head && row[0].val == 0.0) row[0] = e;
      else if (tail && row[2].val == 0.0) row[2] = e;
      else ok = false;
    }
    for (int q = 0; q < lt; ++q) ctab.push_back(row[q]);
  }
  return ok;
}
// what the handle records of a chain table: pat_span2 (-L, or -1 without the line slots) and pat_near (the ring table's reach)
static inline void gcge_pat_chain_spans(const GcgePatPlan& P, const std::vector<GcgePatEntry>& ctab, long* span2, long* near) {
  *span2 = P.Lline ? -P.Lline : -1;
  *near = 0;
  if (P.Lline && P.lt == 7 && P.nslot_used == 7 && P.slot[5] == -1 && P.slot[6] == 1)
    for (const GcgePatEntry& e : ctab) *near = std::max(*near, e.off < 0 ? -e.off : e.off);
}
#endif
