// Stand-alone host check of the slot rule of the per-row values (gcge_pat_value_slot, csrc/hip/pattern_table.h), which the kernels of
// csrc/hip/mat_values.hip (gcge_hip_mat_update_values_device) share with this file.  Build and run under the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Igcge_amd/csrc/hip tools/pattern_values_check.cpp -o /tmp/pvc && /tmp/pvc
// For the 7-point stencil on 8^3 (chain + line layout) and 5^3 (plain table) and the 15-point stencil on 8^3 (table width 16) it
// builds pid, table and chain table through pattern_table.h — a VALUE table (classes by offsets and values) and, for tables of at
// most 8 slots, an OFFSETS-ONLY table (classes by offsets, 1.0 on every present slot: build_patterns' by_offsets form) — then gives
// the matrix new values of three kinds:
//   U  every value doubled                               (the classes of a value table stay uniform)
//   V  diag[r] += (7 r) % 5                              (an SCF step: another diagonal in every row)
//   W  a_ij = -(1 + (i + j) % 3), a_ii = 20 + i % 4      (symmetric, everything varies)
// and checks, for every row: each entry finds a slot; the slot carries the entry's offset; the table's offsets with the per-row
// values reproduce the row's new entries exactly and address nothing outside the block; under U the value table rewritten from the
// first row of every class reproduces every row by itself.  Last: an explicitly stored 0.0 / -0.0 is flagged (the count of present
// slots differs from the row's length, and off the diagonal the entry finds no slot).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>
#include "pattern_table.h"

struct Row { std::vector<GcgePatEntry> e; };
static bool g_by_offsets = false;
static bool operator<(const Row& a, const Row& b) {
  if (a.e.size() != b.e.size()) return a.e.size() < b.e.size();
  for (size_t i = 0; i < a.e.size(); ++i) {
    if (a.e[i].off != b.e[i].off) return a.e[i].off < b.e[i].off;
    if (!g_by_offsets && memcmp(&a.e[i].val, &b.e[i].val, 8) != 0) return memcmp(&a.e[i].val, &b.e[i].val, 8) < 0;
  }
  return false;
}
static std::vector<Row> stencil(int N, bool diag15) {
  std::vector<Row> rows((size_t)N * N * N);
  for (int z = 0; z < N; ++z) for (int y = 0; y < N; ++y) for (int x = 0; x < N; ++x) {
    const long r = x + (long)N * (y + (long)N * z);
    std::map<long, double> m;
    m[0] = diag15 ? 14.0 : 6.0;
    for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
      const int k = abs(dx) + abs(dy) + abs(dz);
      if (!(k == 1 || (diag15 && k == 3))) continue;
      if (x + dx < 0 || x + dx >= N || y + dy < 0 || y + dy >= N || z + dz < 0 || z + dz >= N) continue;
      m[dx + (long)N * (dy + (long)N * dz)] = k == 1 ? -2.0 : -1.0;
    }
    for (auto& kv : m) rows[(size_t)r].e.push_back(GcgePatEntry{kv.second, kv.first});
  }
  return rows;
}
static std::vector<Row> new_values(const std::vector<Row>& rows, char kind) {
  std::vector<Row> out(rows);
  for (size_t r = 0; r < out.size(); ++r)
    for (GcgePatEntry& e : out[r].e) {
      const long c = (long)r + e.off;
      if (kind == 'U') e.val *= 2.0;
      if (kind == 'V' && e.off == 0) e.val += (double)((7 * r) % 5);
      if (kind == 'W') e.val = e.off == 0 ? 20.0 + (double)(r % 4) : -(1.0 + (double)(((long)r + c) % 3));
    }
  return out;
}
struct Table { int lt; bool chain_layout; std::vector<int> pid; std::vector<GcgePatEntry> tab; };
// pid and table as build_patterns / the device search leave them (by_offsets: 1.0 on every present slot)
static Table build(const std::vector<Row>& rows, int lt, bool by_offsets) {
  const long n = (long)rows.size();
  Table T; T.lt = lt; T.chain_layout = false;
  g_by_offsets = by_offsets;
  std::map<Row, int> id_of; std::vector<int> pid((size_t)n); std::vector<GcgePatEntry> tab; std::vector<long> freq;
  for (long r = 0; r < n; ++r) {
    auto it = id_of.find(rows[(size_t)r]);
    if (it == id_of.end()) {
      it = id_of.emplace(rows[(size_t)r], (int)freq.size()).first; freq.push_back(0);
      for (int k = 0; k < lt; ++k) {
        GcgePatEntry e = k < (int)rows[(size_t)r].e.size() ? rows[(size_t)r].e[(size_t)k] : GcgePatEntry{0.0, 0};
        if (by_offsets && k < (int)rows[(size_t)r].e.size()) e.val = 1.0;
        tab.push_back(e);
      }
    }
    pid[(size_t)r] = it->second; ++freq[(size_t)it->second];
  }
  g_by_offsets = false;
  GcgePatPlan plan;
  gcge_pat_plan(tab, freq, lt, plan);
  long span2 = plan.span2, near = 0;
  if (plan.chain) {
    std::map<uint64_t, int> kid; std::vector<uint64_t> keys; std::vector<int> cpid((size_t)n);
    for (long r = 0; r < n; ++r) {
      const uint64_t key = gcge_pat_row_key(plan, (unsigned)pid[(size_t)r], r, n, n);
      auto it = kid.find(key);
      if (it == kid.end()) { it = kid.emplace(key, (int)keys.size()).first; keys.push_back(key); }
      cpid[(size_t)r] = it->second;
    }
    std::vector<GcgePatEntry> ctab;
    if (gcge_pat_chain_table(plan, keys, ctab)) { tab.swap(ctab); pid.swap(cpid); gcge_pat_chain_spans(plan, tab, &span2, &near); }
  }
  T.chain_layout = span2 <= -1;          // (mat_upload.hip: A->pat_span2 <= -1)
  T.pid = pid; T.tab = tab;
  return T;
}
// the per-row values of `rows` in the slots of T by the shared rule; false: an entry without a slot, or a slot with another offset
static bool scatter(const Table& T, const std::vector<Row>& rows, std::vector<double>& rv, long* bad_row) {
  const int lt = T.lt;
  rv.assign(rows.size() * (size_t)lt, 0.0);
  for (size_t r = 0; r < rows.size(); ++r) {
    const GcgePatEntry* e = &T.tab[(size_t)T.pid[r] * lt];
    unsigned used = 0;
    for (const GcgePatEntry& a : rows[r].e) {
      const int s = gcge_pat_value_slot(e, lt, T.chain_layout, a.off, &used);
      if (s < 0 || s >= lt || e[s].off != a.off) { *bad_row = (long)r; return false; }
      rv[r * lt + (size_t)s] = a.val;
    }
  }
  return true;
}
// sum over slots of val[slot] at (row + offset) == the row's entries, nothing addressed outside [0, n)
static bool reproduces(const Table& T, const std::vector<Row>& rows, const std::vector<double>* rv, long* bad_row) {
  const int lt = T.lt; const long n = (long)rows.size();
  for (long r = 0; r < n; ++r) {
    std::map<long, double> got, want;
    for (int k = 0; k < lt; ++k) {
      const GcgePatEntry& e = T.tab[(size_t)T.pid[(size_t)r] * lt + k];
      if (r + e.off < 0 || r + e.off >= n) { *bad_row = r; return false; }
      const double v = rv != nullptr ? (*rv)[(size_t)r * lt + k] : e.val;
      if (v != 0.0) got[e.off] += v;
    }
    for (const GcgePatEntry& a : rows[(size_t)r].e) want[a.off] += a.val;
    if (got != want) { *bad_row = r; return false; }
  }
  return true;
}
static int check(int N, bool diag15, int lt, int want_chain_layout) {
  const std::vector<Row> rows = stencil(N, diag15);
  int bad = 0;
  for (int by_offsets = 0; by_offsets <= (lt <= 8 ? 1 : 0); ++by_offsets) {
    const Table T = build(rows, lt, by_offsets != 0);
    if ((int)T.chain_layout != want_chain_layout) { fprintf(stderr, "N %d lt %d: chain layout %d, expected %d\n", N, lt, (int)T.chain_layout, want_chain_layout); return 1; }
    for (size_t r = 0; r < rows.size(); ++r)
      if (gcge_pat_present_slots(&T.tab[(size_t)T.pid[r] * lt], lt) != (int)rows[r].e.size()) { fprintf(stderr, "N %d lt %d: row %zu: present slots\n", N, lt, r); return 1; }
    for (const char kind : {'U', 'V', 'W', 'O'}) {          // O: the values the table was built from
      const std::vector<Row> nv = kind == 'O' ? rows : new_values(rows, kind);
      std::vector<double> rv; long where = -1;
      if (!scatter(T, nv, rv, &where)) { fprintf(stderr, "N %d lt %d %c by_offsets %d: row %ld: an entry without a slot\n", N, lt, kind, by_offsets, where); bad = 1; continue; }
      if (!reproduces(T, nv, &rv, &where)) { fprintf(stderr, "N %d lt %d %c by_offsets %d: row %ld is not reproduced by table + row values\n", N, lt, kind, by_offsets, where); bad = 1; }
      if (!by_offsets && (kind == 'U' || kind == 'O')) {    // the table rewrite: every present slot from the first row of its class
        Table R = T;
        std::vector<long> first(T.tab.size() / lt, -1);
        for (size_t r = 0; r < rows.size(); ++r) if (first[(size_t)T.pid[r]] < 0) first[(size_t)T.pid[r]] = (long)r;
        for (size_t p = 0; p < first.size(); ++p)
          for (int k = 0; k < lt; ++k) if (T.tab[p * lt + k].val != 0.0) R.tab[p * lt + k].val = rv[(size_t)first[p] * lt + k];
        if (!reproduces(R, nv, nullptr, &where)) { fprintf(stderr, "N %d lt %d %c: row %ld is not reproduced by the rewritten table\n", N, lt, kind, where); bad = 1; }
      }
    }
    printf("N %d, %s, %s table: %zu table rows, chain layout %d: U V W reproduced\n", N, diag15 ? "15-point" : "7-point", by_offsets ? "offsets-only" : "value",
           T.tab.size() / lt, (int)T.chain_layout);
  }
  return bad;
}
// an explicitly stored zero: the class's table row has a slot without a value, so the count differs and the entry finds no slot
static int check_stored_zero(int N, int lt, double zero, long off_of_zero) {
  std::vector<Row> rows = stencil(N, false);
  const long r = 2 + (long)N * (2 + (long)N * 2);           // an interior row
  bool hit = false;
  for (GcgePatEntry& e : rows[(size_t)r].e) if (e.off == off_of_zero) { e.val = zero; hit = true; }
  if (!hit) { fprintf(stderr, "stored zero: no entry at offset %ld\n", off_of_zero); return 1; }
  const Table T = build(rows, lt, false);
  const GcgePatEntry* e = &T.tab[(size_t)T.pid[(size_t)r] * lt];
  if (gcge_pat_present_slots(e, lt) == (int)rows[(size_t)r].e.size()) { fprintf(stderr, "stored zero at offset %ld: the slot count does not show it\n", off_of_zero); return 1; }
  unsigned used = 0; int noslot = 0;
  for (const GcgePatEntry& a : rows[(size_t)r].e) if (gcge_pat_value_slot(e, lt, T.chain_layout, a.off, &used) < 0) ++noslot;
  const bool diag_of_chain = T.chain_layout && off_of_zero == 0;   // (the diagonal's slot is fixed: only the count shows the zero)
  if (noslot != (diag_of_chain ? 0 : 1)) { fprintf(stderr, "stored zero at offset %ld: %d entries without a slot\n", off_of_zero, noslot); return 1; }
  // every other row is untouched by it
  for (size_t q = 0; q < rows.size(); ++q)
    if ((long)q != r && gcge_pat_present_slots(&T.tab[(size_t)T.pid[q] * lt], lt) != (int)rows[q].e.size()) { fprintf(stderr, "stored zero: row %zu flagged\n", q); return 1; }
  return 0;
}
int main() {
  int bad = 0;
  bad |= check(8, false, 7, 1);
  bad |= check(5, false, 7, 0);
  bad |= check(8, true, 16, 0);
  bad |= check_stored_zero(6, 7, 0.0, 36);
  bad |= check_stored_zero(6, 7, -0.0, 1);
  bad |= check_stored_zero(8, 7, 0.0, 64);
  bad |= check_stored_zero(8, 7, -0.0, 0);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
