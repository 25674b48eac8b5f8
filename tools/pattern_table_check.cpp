// Stand-alone host check of csrc/hip/pattern_table.h (the table side of the pattern search, shared by the host and the device path) and
// of the device constructor's argument check.  Build and run under the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Igcge_amd/csrc/hip tools/pattern_table_check.cpp -o /tmp/ptc && /tmp/ptc
// It feeds the representative rows of a 7-point stencil (8^3 grid: S = 64, L = 8, chain + line layout; 5^3: no chain layout) and of a
// 15-point stencil (table width 16) through gcge_pat_plan / gcge_pat_row_key / gcge_pat_chain_table and checks that the table
// reproduces the matrix: sum over slots of value at (row + offset) == the row's entries.
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <vector>
#include "pattern_table.h"

struct Row { std::vector<GcgePatEntry> e; };
static bool operator<(const Row& a, const Row& b) {
  if (a.e.size() != b.e.size()) return a.e.size() < b.e.size();
  for (size_t i = 0; i < a.e.size(); ++i) { if (a.e[i].off != b.e[i].off) return a.e[i].off < b.e[i].off; if (a.e[i].val != b.e[i].val) return a.e[i].val < b.e[i].val; }
  return false;
}
// rows of a stencil on an N^3 grid, ascending columns: the 7-point star, or with diag15 the star plus the 8 cube diagonals
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
      m[dx + (long)N * (dy + (long)N * dz)] = k == 1 ? -1.0 : -0.5;
    }
    for (auto& kv : m) rows[(size_t)r].e.push_back(GcgePatEntry{kv.second, kv.first});
  }
  return rows;
}
static int check(int N, bool diag15, int lt, int want_chain) {
  const std::vector<Row> rows = stencil(N, diag15);
  const long n = (long)rows.size();
  // (a): ids by first occurrence
  std::map<Row, int> id_of; std::vector<int> pid((size_t)n); std::vector<GcgePatEntry> tab; std::vector<long> freq;
  for (long r = 0; r < n; ++r) {
    auto it = id_of.find(rows[(size_t)r]);
    if (it == id_of.end()) {
      it = id_of.emplace(rows[(size_t)r], (int)freq.size()).first; freq.push_back(0);
      for (int k = 0; k < lt; ++k) tab.push_back(k < (int)rows[(size_t)r].e.size() ? rows[(size_t)r].e[(size_t)k] : GcgePatEntry{0.0, 0});
    }
    pid[(size_t)r] = it->second; ++freq[(size_t)it->second];
  }
  // (b)
  GcgePatPlan plan;
  gcge_pat_plan(tab, freq, lt, plan);
  std::vector<int> fpid(pid);
  long span2 = plan.span2, near = 0;
  int chain = 0;
  if (plan.chain) {
    std::map<uint64_t, int> kid; std::vector<uint64_t> keys; std::vector<int> cpid((size_t)n);
    for (long r = 0; r < n; ++r) {
      const uint64_t key = gcge_pat_row_key(plan, (unsigned)pid[(size_t)r], r, n, n);
      auto it = kid.find(key);
      if (it == kid.end()) { it = kid.emplace(key, (int)keys.size()).first; keys.push_back(key); }
      cpid[(size_t)r] = it->second;
    }
    std::vector<GcgePatEntry> ctab;
    if (gcge_pat_chain_table(plan, keys, ctab)) { tab.swap(ctab); fpid.swap(cpid); gcge_pat_chain_spans(plan, tab, &span2, &near); chain = span2 <= -8 ? 2 : 1; }
    std::vector<uint64_t> many((size_t)gcge_pat_max_patterns(lt) + 1, keys[0]);
    if (gcge_pat_chain_table(plan, many, ctab)) { fprintf(stderr, "too many keys were accepted\n"); return 1; }
  }
  if (chain != want_chain) { fprintf(stderr, "N %d lt %d: chain layout %d, expected %d\n", N, lt, chain, want_chain); return 1; }
  // the table reproduces every row
  for (long r = 0; r < n; ++r) {
    std::map<long, double> got, want;
    for (int k = 0; k < lt; ++k) { const GcgePatEntry& e = tab[(size_t)fpid[(size_t)r] * lt + k]; if (r + e.off < 0 || r + e.off >= n) { fprintf(stderr, "row %ld: slot %d leaves the block\n", r, k); return 1; } if (e.val != 0.0) got[e.off] += e.val; }
    for (const GcgePatEntry& e : rows[(size_t)r].e) want[e.off] += e.val;
    if (got != want) { fprintf(stderr, "N %d lt %d: row %ld is not reproduced\n", N, lt, r); return 1; }
  }
  printf("N %d, %s: %zu classes -> %zu table rows, span %ld span2 %ld near %ld, chain %d\n", N, diag15 ? "15-point" : "7-point", freq.size(), tab.size() / lt, plan.span, span2, near, chain);
  return 0;
}
int main() {
  int bad = 0;
  bad |= check(8, false, 7, 2);
  bad |= check(5, false, 7, 0);
  bad |= check(16, false, 7, 2);
  bad |= check(8, true, 16, 0);
  bad |= check(12, true, 16, 0);
  int dummy = 0;
  const bool a = gcge_mat_device_args_ok(5, 7, &dummy, &dummy, &dummy), b = gcge_mat_device_args_ok(0, 0, &dummy, nullptr, nullptr),
             c = gcge_mat_device_args_ok(5, -1, &dummy, &dummy, &dummy), d = gcge_mat_device_args_ok(5, 2147483648L, &dummy, &dummy, &dummy),
             e = gcge_mat_device_args_ok(5, 7, nullptr, &dummy, &dummy), f = gcge_mat_device_args_ok(5, 7, &dummy, nullptr, &dummy),
             g = gcge_mat_device_args_ok(2147483647L, 2147483647L, &dummy, &dummy, &dummy), h = gcge_mat_device_args_ok(1, 0, &dummy, nullptr, nullptr);
  if (!(a && !b && !c && !d && !e && !f && g && h)) { fprintf(stderr, "argument check\n"); bad = 1; }
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
