// K1 (grid path) — the upload-time analysis behind the plane sweep of spmm_star.hip, host code only: the grid the rows of a CSR matrix live on (read off the
// column offsets most rows share, or recovered from the rows' couplings), the star's coefficients, the split A = S + D + R the sweep and its followers multiply by.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <unordered_map>
#include "star_split.h"
#include "value_maps.h"

namespace gcge {
static_assert(GCGE_VM_ARM == STAR_R, "value_maps.h codes the coefficients of a star of arm length STAR_R");

static inline uint64_t star_bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

// The offsets (global column - global row) of a star on a lexicographic grid: |o| in {1..Rx} u {sy, 2 sy, .., Ry sy} u {sz, .., Rz sz},
// each carried (as + o or - o: rows next to a face of the grid, or of a slab at the end of the grid, have only one of the two)
// by at least half of the sampled rows.  false: the frequent offsets are not such a set.
static bool star_offsets(const StarRows& M, int* Rx_, int* Ry_, int* Rz_, long* sy_, long* sz_) {
  const int nrows = M.nrows;
  if (nrows < 2048) return false;
  const int nsamp = std::min(nrows, 8192);
  std::unordered_map<long, int> hist;
  std::vector<long> seen;
  for (int t = 0; t < nsamp; ++t) {
    const int r = (int)((long)t * nrows / nsamp);
    seen.clear();
    for (int q = M.rowptr[r]; q < M.rowptr[r + 1]; ++q) { const long o = M.gcol(M.colidx[q]) - M.gpos(r); if (o != 0) seen.push_back(o < 0 ? -o : o); }
    std::sort(seen.begin(), seen.end());
    seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
    for (long o : seen) ++hist[o];
  }
  std::vector<long> offs;
  for (auto& kv : hist) if (kv.second * 2 >= nsamp) offs.push_back(kv.first);
  std::sort(offs.begin(), offs.end());
  if (offs.empty() || offs[0] != 1) return false;
  // runs: 1 .. Rx, then sy, 2 sy, .. Ry sy, then sz, 2 sz, .. Rz sz
  size_t i = 0; int Rx = 0, Ry = 0, Rz = 0; long sy = 0, sz = 0;
  while (i < offs.size() && offs[i] == Rx + 1) { ++Rx; ++i; }
  if (i >= offs.size()) return false;
  sy = offs[i];
  while (i < offs.size() && offs[i] == (long)(Ry + 1) * sy) { ++Ry; ++i; }
  if (i >= offs.size()) return false;
  sz = offs[i];
  while (i < offs.size() && offs[i] == (long)(Rz + 1) * sz) { ++Rz; ++i; }
  if (i != offs.size()) return false;                                  // a frequent offset that is not part of a star
  if (sz % sy != 0 || M.nglobal % sz != 0) return false;
  *Rx_ = Rx; *Ry_ = Ry; *Rz_ = Rz; *sy_ = sy; *sz_ = sz;
  return true;
}

// grid strides and the star's coefficients from the offsets (global column - global row) most rows share; false: no star on a grid here
static bool star_detect(const StarRows& M, StarHost* H) {
  const int nrows = M.nrows; const int* rowptr = M.rowptr; const int* colidx = M.colidx; const double* val = M.val;
  int Rx = 0, Ry = 0, Rz = 0; long sy = 0, sz = 0;
  if (!star_offsets(M, &Rx, &Ry, &Rz, &sy, &sz)) return false;
  const int nsamp = std::min(nrows, 8192);
  const int R = std::max(Rx, std::max(Ry, Rz));
  if (R > STAR_R || sy <= 2L * STAR_R || sz % sy != 0 || sz / sy <= 2L * STAR_R || M.nglobal % sz != 0 || M.nglobal / sz < 2) return false;
  StarGeom& g = H->g;
  g.nx = (int)sy; g.ny = (int)(sz / sy); g.nz = (int)(M.nglobal / sz); H->R = R;
  if (M.box != nullptr) {            // a masked domain: the box is the grid, the rows are found through the map / the line table
    if (g.nx != M.bnx || g.ny != M.bny || g.nz != M.bnz || (M.ncols_local != nrows && !M.box_cols)) return false;
    g.zs = 0; g.ze = g.nz;
    if (M.box_cols) { g.zs = (int)(M.box[0] / sz); g.ze = (int)(M.box[nrows - 1] / sz) + 1; }   // a slab: the planes its own rows touch
  } else {
    // the slab must be whole planes (a partition cut inside a plane keeps the other forms: gcge_amd.dist.partition_by_nnz(align=))
    if (M.row_begin % sz != 0 || (long)nrows % sz != 0) return false;
    g.zs = (int)(M.row_begin / sz); g.ze = g.zs + (int)((long)nrows / sz);
  }
  if (g.ze > g.nz) return false;
  g.zmin = std::max(0, g.zs - R); g.zmax = std::min(g.nz, g.ze + R);
  g.mid_off = -sz * g.zs; g.lo_off = g.hi_off = 0;
  // the planes below and above among the halo rows: whole and contiguous (every point of them is some row's neighbour)
  const int ng = M.ncols_local - nrows;
  auto run = [&](long first, long count, long* off) -> bool {       // halo rows first .. first + count - 1 -> *off + global = row of X
    if (count == 0) return true;
    if (M.ghost == nullptr) return false;
    const int* lo = std::lower_bound(M.ghost, M.ghost + ng, (int)first);
    const long idx = lo - M.ghost;
    if (idx + count > ng) return false;
    if (M.ghost[idx] != first || M.ghost[idx + count - 1] != first + count - 1) return false;   // (ascending and unique: the run is gap-free)
    *off = (long)nrows + idx - first;
    return true;
  };
  if (M.box == nullptr) {             // (a masked grid finds its halo rows through the line table, line by line)
    if (!run((long)g.zmin * sz, (long)(g.zs - g.zmin) * sz, &g.lo_off)) return false;
    if (!run((long)g.ze * sz, (long)(g.zmax - g.ze) * sz, &g.hi_off)) return false;
  }
  // coefficients: the most frequent value of every offset among the sampled rows; the star must be symmetric
  memset(&H->c, 0, sizeof(H->c));
  for (int axis = 0; axis < 3; ++axis) {
    const int Ra = axis == 0 ? Rx : axis == 1 ? Ry : Rz;
    const long stride = axis == 0 ? 1 : axis == 1 ? sy : sz;
    double* dst = axis == 0 ? H->c.cx : axis == 1 ? H->c.cy : H->c.cz;
    for (int k = 1; k <= Ra; ++k) {
      std::unordered_map<uint64_t, int> vals[2];
      for (int t = 0; t < nsamp; ++t) {
        const int r = (int)((long)t * nrows / nsamp);
        for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) {
          const long o = M.gcol(colidx[q]) - M.gpos(r);
          if (o == k * stride) ++vals[0][star_bits(val[q])];
          else if (o == -k * stride) ++vals[1][star_bits(val[q])];
        }
      }
      uint64_t best[2] = {0, 0}; int bcnt[2] = {-1, -1};
      for (int sgn = 0; sgn < 2; ++sgn) for (auto& kv : vals[sgn]) if (kv.second > bcnt[sgn]) { bcnt[sgn] = kv.second; best[sgn] = kv.first; }
      if (bcnt[0] < 0 && bcnt[1] < 0) return false;
      if (bcnt[0] >= 0 && bcnt[1] >= 0 && best[0] != best[1]) return false;   // (a slab at the end of the grid may see one direction only)
      memcpy(&dst[k], &best[bcnt[0] >= 0 ? 0 : 1], 8);
    }
  }
  return true;
}

// Split A = S + D + R: S the star (the same coefficients in every row, truncated at the faces of the grid), D the diagonal, R the
// remainder.  EVERY row takes S + D from the sweep; a row is "clean" when its R is empty (its off-diagonal entries are exactly the
// star, bit for bit).  In the other rows — inside atom blocks, next to anything irregular — R holds: every entry that is not at a
// star position as it is; at a star position the entry MINUS the star's coefficient (nothing when they are equal; minus the
// coefficient where the row has no entry there), rounded once.  R is added to what the sweep wrote by the kernels that follow it
// (dense blocks + listed rows, spmm_dense.hip).  So the sweep needs no per-row decision and the listed rows carry only what really
// differs from the star: on the SiO2-like matrix two thirds of the non-zeros the listed rows held before were plain star entries.
bool star_build_host(const StarRows& M, StarHost* H) {
  const int nrows = M.nrows; const int* rowptr = M.rowptr; const int* colidx = M.colidx; const double* val = M.val;
  if (M.ncols_local != nrows && M.ghost == nullptr && !M.box_cols) return false;     // halo columns of unknown origin: the other forms
  if (!star_detect(M, H)) return false;
  const StarGeom& gm = H->g;
  const int nx = gm.nx, ny = gm.ny, nz = gm.nz;
  const long sy = nx, sz = (long)nx * ny;
  H->diag.assign((size_t)nrows, 0.0);
  H->rem_rowptr.assign((size_t)nrows + 1, 0);
  const bool maps = H->keep_maps;
  if (maps) { H->diag_src.assign((size_t)nrows, -1); H->pin.assign((size_t)rowptr[nrows], 0); }
  uint64_t cb[3][STAR_R + 1]; double cv[3][STAR_R + 1];
  for (int k = 0; k <= STAR_R; ++k) {
    cv[0][k] = H->c.cx[k]; cv[1][k] = H->c.cy[k]; cv[2][k] = H->c.cz[k];
    for (int a = 0; a < 3; ++a) cb[a][k] = star_bits(cv[a][k]);
  }
  const long stride[3] = {1, sy, sz};
  // masked domains: grid point -> row (-1: not a row)
  std::vector<int>& inv = H->inv;
  inv.clear();
  if (M.box != nullptr) {
    inv.assign((size_t)M.nglobal, -1);
    const int ncl = M.box_cols ? M.ncols_local : nrows;               // (a slab: the halo rows too — ascending among themselves)
    for (int r = 0; r < ncl; ++r) {
      if (M.box[r] < 0 || M.box[r] >= M.nglobal || inv[M.box[r]] != -1 || (r > 0 && r != nrows && M.box[r] <= M.box[r - 1])) return false;   // (scan order, no point twice)
      inv[M.box[r]] = r;
    }
  }
  // local column (= row of X) of grid point gq: own rows, or the halo planes below / above as the sweep addresses them
  auto xcol = [&](long gq) -> long {
    if (M.box != nullptr) return inv[gq];
    const int zz = (int)(gq / sz);
    return (zz < gm.zs ? gm.lo_off : zz >= gm.ze ? gm.hi_off : gm.mid_off) + gq;
  };
  std::vector<char>& clean = H->clean;
  clean.assign((size_t)nrows, 0);
  // rows are independent: contiguous chunks, one thread each, every chunk with its own remainder arrays (joined in order below)
  const int nt = gcge_upload_threads();
  std::vector<std::vector<int>> crc((size_t)nt); std::vector<std::vector<double>> crv((size_t)nt);
  std::vector<std::vector<int>> crs((size_t)nt); std::vector<std::vector<unsigned char>> crk((size_t)nt);   // (maps: source and code of every remainder entry)
  std::vector<long> cclean((size_t)nt, 0); std::vector<int> cfail((size_t)nt, 0);
  std::vector<int>& rcnt = H->rem_rowptr;                             // [r + 1] = entries of row r for now, prefix-summed below
  gcge_parallel_chunks(nrows, nt, [&](int chunk, long rb, long re) {
  struct RemEntry { int first; double second; int src; int code; };   // column, value; where the value came from (value_maps.h): it rides through the sort
  std::vector<RemEntry> rem;                                           // remainder of the row being looked at
  std::vector<int>& rc = crc[chunk]; std::vector<double>& rv = crv[chunk];
  std::vector<int>& rs = crs[chunk]; std::vector<unsigned char>& rk = crk[chunk];
  long nclean = 0;
  for (int r = (int)rb; r < (int)re; ++r) {
    const long gr = M.gpos(r);
    const int gz = (int)(gr / sz), gy = (int)((gr - (long)gz * sz) / sy), gx = (int)(gr - (long)gz * sz - (long)gy * sy);
    const int g[3] = {gx, gy, gz}, dim[3] = {nx, ny, nz};
    // the neighbour k steps along axis a (sgn 0: down, 1: up) is a point of the domain
    auto exists = [&](int a, int sgn, int k) -> bool {
      if (!(sgn ? g[a] + k < dim[a] : g[a] - k >= 0)) return false;
      return M.box == nullptr || inv[gr + (sgn ? 1 : -1) * k * stride[a]] >= 0;
    };
    bool seen[3][2][STAR_R + 1] = {};
    rem.clear();
    bool have_diag = false; double dv = 0.0; int dq = -1;
    for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) {
      const long o = M.gcol(colidx[q]) - gr;
      if (o == 0 && !have_diag) { have_diag = true; dv = val[q]; dq = q; continue; }
      const long ao = o < 0 ? -o : o; const int sgn = o < 0 ? 0 : 1;
      int a = -1, k = 0;
      if (ao >= 1 && ao <= STAR_R) { a = 0; k = (int)ao; }
      else if (ao % sz == 0 && ao / sz >= 1 && ao / sz <= STAR_R) { a = 2; k = (int)(ao / sz); }
      else if (ao % sy == 0 && ao / sy >= 1 && ao / sy <= STAR_R) { a = 1; k = (int)(ao / sy); }
      // a star position: the neighbour k steps along axis a exists in the grid and the star reaches that far
      const bool star_pos = a >= 0 && cb[a][k] != 0 && !seen[a][sgn][k] && exists(a, sgn, k);
      if (!star_pos) { rem.push_back(RemEntry{colidx[q], val[q], q, 0}); continue; }
      seen[a][sgn][k] = true;
      if (star_bits(val[q]) != cb[a][k]) rem.push_back(RemEntry{colidx[q], val[q] - cv[a][k], q, gcge_vm_code(a, k)});
      else if (maps) H->pin[q] = (unsigned char)gcge_vm_code(a, k);   // the star carries this entry: new values must keep it
    }
    for (int a = 0; a < 3; ++a)
      for (int k = 1; k <= STAR_R; ++k) {
        if (cb[a][k] == 0) continue;
        for (int sgn = 0; sgn < 2; ++sgn) {
          if (!exists(a, sgn, k) || seen[a][sgn][k]) continue;
          // the sweep adds coefficient x neighbour here, the row has no such entry: the remainder takes it back
          const long gq = gr + (sgn ? 1 : -1) * k * stride[a];
          const int zz = (int)(gq / sz);
          if (zz < gm.zmin || zz >= gm.zmax) { cfail[chunk] = 1; return; }   // (cannot happen: zmin / zmax cover the star's reach)
          rem.push_back(RemEntry{(int)xcol(gq), -cv[a][k], -1, gcge_vm_code(a, k)});
        }
      }
    if (dv != dv) { cfail[chunk] = 1; return; }                        // a NaN on the diagonal: not for this form
    H->diag[r] = dv;
    if (maps && dq >= 0) { H->diag_src[r] = dq; H->pin[dq] = GCGE_VM_PIN_DIAG; }
    if (rem.empty()) { clean[r] = 1; ++nclean; }
    else {
      std::sort(rem.begin(), rem.end(), [](const RemEntry& p, const RemEntry& q) { return p.first < q.first; });
      for (auto& e : rem) { rc.push_back(e.first); rv.push_back(e.second); }
      if (maps) for (auto& e : rem) { rs.push_back(e.src); rk.push_back((unsigned char)e.code); }
    }
    rcnt[r + 1] = (int)rem.size();
  }
  cclean[chunk] = nclean;
  });
  long nclean = 0;
  for (int c = 0; c < nt; ++c) { if (cfail[c]) return false; nclean += cclean[c]; }
  for (int r = 0; r < nrows; ++r) rcnt[r + 1] += rcnt[r];
  std::vector<int>& rc = H->rem_col; std::vector<double>& rv = H->rem_val;
  rc.resize((size_t)rcnt[nrows]); rv.resize((size_t)rcnt[nrows]);
  {
    size_t off = 0;
    for (int c = 0; c < nt; ++c) {
      if (!crc[c].empty()) { memcpy(rc.data() + off, crc[c].data(), crc[c].size() * sizeof(int)); memcpy(rv.data() + off, crv[c].data(), crv[c].size() * sizeof(double)); }
      off += crc[c].size();
      std::vector<int>().swap(crc[c]); std::vector<double>().swap(crv[c]);
    }
    if (off != rc.size()) return false;
  }
  if (maps) {
    H->rem_src.clear(); H->rem_code.clear();
    H->rem_src.reserve(rc.size()); H->rem_code.reserve(rc.size());
    for (int c = 0; c < nt; ++c) { H->rem_src.insert(H->rem_src.end(), crs[c].begin(), crs[c].end()); H->rem_code.insert(H->rem_code.end(), crk[c].begin(), crk[c].end()); }
    if (H->rem_src.size() != rc.size()) return false;
  }
  H->nclean = nclean;
  if (2 * nclean < nrows) return false;
  return true;
}

// Geometry of a MASKED grid recovered from the rows alone (one rank; a matrix that arrives as a file, e.g. Matrix Market, names
// no grid): the rows are the points of a convex domain inside a box in scan order (x fastest), every row couples to its
// neighbours along the three axes (a star of any arm length) and to anything else (atom blocks).  Then
//   * rows r and r + 1 lie on one x LINE exactly when the entry (r, r + 1) is there;
//   * consecutive lines l, l + 1 of one PLANE (y and y + 1) are coupled through the + y neighbours: every star row of l has ONE
//     entry among the rows of l + 1, and all of them agree on the shift between where the two lines begin in x — the shift most
//     rows vote for; lines without such a vote (the last line of a plane and the first of the next one share no neighbour) end a plane;
//   * consecutive planes are coupled through the + z neighbours in the same way: a vote on the (x, y) shift between their frames.
// Votes come from the rows that are no longer than the median row (the star rows), from all rows of a line only when none of
// its rows is that short.  box[r] = x + nx (y + ny z) in the bounding box of what was found.  A wrong guess costs speed, never
// the result: the split of star_build_host is exact for any one-to-one ascending map (the remainder takes every difference),
// and the form is refused when fewer than half of the rows come out clean.  false: the rows do not look like this.
bool star_infer_box(int nrows, const int* rowptr, const int* colidx, std::vector<int>* box_, int* nx_, int* ny_, int* nz_) {
  if (nrows < 2048) return false;
  // lines
  std::vector<int> lstart;                                             // first row of every line (+ nrows at the end)
  std::vector<int> lineof((size_t)nrows);
  long linked = 0;
  lstart.push_back(0);
  for (int r = 0; r < nrows; ++r) {
    lineof[r] = (int)lstart.size() - 1;
    if (r + 1 == nrows) break;
    bool next = false;
    for (int q = rowptr[r]; q < rowptr[r + 1] && !next; ++q) next = colidx[q] == r + 1;
    if (next) ++linked; else lstart.push_back(r + 1);
  }
  const int nl = (int)lstart.size();
  lstart.push_back(nrows);
  if (2 * linked < nrows || nl < 16) return false;
  // the median row length: rows up to it vote
  int med;
  {
    std::vector<int> len((size_t)nrows);
    for (int r = 0; r < nrows; ++r) len[r] = rowptr[r + 1] - rowptr[r];
    std::nth_element(len.begin(), len.begin() + nrows / 2, len.end());
    med = len[nrows / 2];
  }
  // planes: shift of line l + 1 against line l, or a break
  std::vector<int> xoff((size_t)nl, 0), pstart;                        // x of a line's first row in its plane's frame; first line of every plane
  std::vector<int> votes;
  pstart.push_back(0);
  for (int l = 0; l + 1 < nl; ++l) {
    const int a0 = lstart[l], a1 = lstart[l + 1], b0 = a1, b1 = lstart[l + 2];
    const int span = (a1 - a0) + (b1 - b0);
    const int need = std::min(a1 - a0, b1 - b0);
    int best = 0, bestn = 0;
    // (the + y neighbour of a star row is its only entry in the next line: the vote of a true pair of lines is nearly unanimous;
    //  pass 1 — every row of the line votes — where the short rows alone do not carry it)
    for (int pass = 0; pass < 2 && 2 * bestn < need; ++pass) {
      votes.assign((size_t)span + 1, 0);
      for (int r = a0; r < a1; ++r) {
        if (pass == 0 && rowptr[r + 1] - rowptr[r] > med) continue;
        for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) {
          const int c = colidx[q];
          if (c >= b0 && c < b1) ++votes[(size_t)((r - a0) - (c - b0) + (b1 - b0))];
        }
      }
      bestn = 0;
      for (int k = 0; k <= span; ++k) if (votes[k] > bestn) { bestn = votes[k]; best = k - (b1 - b0); }
    }
    if (bestn > 0 && 2 * bestn >= need) xoff[l + 1] = xoff[l] + best;
    else { pstart.push_back(l + 1); xoff[l + 1] = 0; }
  }
  const int np = (int)pstart.size();
  pstart.push_back(nl);
  if (getenv("GCGE_STAR_INFER_DEBUG")) fprintf(stderr, "star_infer_box: %d rows, %d lines, %d planes, median row %d\n", nrows, nl, np, med);
  if (np < 2 * STAR_R + 2) return false;
  // frames: (x, y) shift of plane p + 1 against plane p
  std::vector<int> px((size_t)np, 0), py((size_t)np, 0);
  std::unordered_map<long, int> pv;
  for (int p = 0; p + 1 < np; ++p) {
    const int r0 = lstart[pstart[p]], r1 = lstart[pstart[p + 1]], s1 = lstart[pstart[p + 2]];
    const long need = std::min(r1 - r0, s1 - r1);
    int bestn = 0; long bestk = 0;
    for (int pass = 0; pass < 2 && 4L * bestn < need; ++pass) {
      pv.clear();
      for (int r = r0; r < r1; ++r) {
        if (pass == 0 && rowptr[r + 1] - rowptr[r] > med) continue;
        const int l = lineof[r], x = xoff[l] + (r - lstart[l]), y = l - pstart[p];
        for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) {
          const int c = colidx[q];
          if (c < r1 || c >= s1) continue;
          const int lc = lineof[c], xc = xoff[lc] + (c - lstart[lc]), yc = lc - pstart[p + 1];
          if (x - xc <= -(1 << 20) || x - xc >= (1 << 20) || y - yc <= -(1 << 20) || y - yc >= (1 << 20)) return false;   // (the key packs two 22-bit fields)
          ++pv[(long)(x - xc + (1 << 20)) * (1L << 22) + (y - yc + (1 << 20))];
        }
      }
      bestn = 0;
      for (auto& kv : pv) if (kv.second > bestn) { bestn = kv.second; bestk = kv.first; }
    }
    if (getenv("GCGE_STAR_INFER_DEBUG")) fprintf(stderr, "plane %d rows %d..%d lines %d votes %d need %ld\n", p, r0, r1, pstart[p + 1] - pstart[p], bestn, need);
    if (bestn == 0 || 4L * bestn < std::min(r1 - r0, s1 - r1)) return false;   // two planes that share no column of points: not such a domain
    px[p + 1] = px[p] + (int)(bestk >> 22) - (1 << 20);
    py[p + 1] = py[p] + (int)(bestk & ((1L << 22) - 1)) - (1 << 20);
  }
  // the bounding box
  long xmin = 0, xmax = 0, ymin = 0, ymax = 0; bool first = true;
  for (int p = 0; p < np; ++p)
    for (int l = pstart[p]; l < pstart[p + 1]; ++l) {
      const long x0 = (long)px[p] + xoff[l], x1 = x0 + (lstart[l + 1] - lstart[l]) - 1, y = (long)py[p] + (l - pstart[p]);
      if (first) { xmin = x0; xmax = x1; ymin = ymax = y; first = false; }
      xmin = std::min(xmin, x0); xmax = std::max(xmax, x1); ymin = std::min(ymin, y); ymax = std::max(ymax, y);
    }
  const long nx = xmax - xmin + 1, ny = ymax - ymin + 1, nz = np;
  // a box far larger than the domain: the lines did not line up (a ball fills 52 % of its box, a thin slab of one more: 8 x the rows is
  // ample — and bounds the point-wise map of the box, 4 bytes per box point on the host and on the device, by 32 bytes per row)
  if (nx * ny * nz >= (1L << 31) || nx * ny * nz > 8L * nrows) return false;
  box_->resize((size_t)nrows);
  for (int p = 0; p < np; ++p)
    for (int l = pstart[p]; l < pstart[p + 1]; ++l) {
      const long x0 = (long)px[p] + xoff[l] - xmin, y = (long)py[p] + (l - pstart[p]) - ymin;
      for (int r = lstart[l]; r < lstart[l + 1]; ++r) (*box_)[r] = (int)(x0 + (r - lstart[l]) + nx * (y + ny * p));
    }
  for (int r = 1; r < nrows; ++r) if ((*box_)[r] <= (*box_)[r - 1]) return false;   // (scan order must have come out)
  *nx_ = (int)nx; *ny_ = (int)ny; *nz_ = (int)nz;
  return true;
}

}  // namespace gcge

using namespace gcge;

// Grid of a matrix whose rows are (mostly) star stencils, from a slab of its rows with GLOBAL column indices (host only; what a
// partitioner needs to put its cuts on plane boundaries: gcge_amd.dist.partition_by_nnz(align = nx * ny)).  out[0..3] = nx, ny,
// nz, arm length.  1: found, 0: no such grid.
extern "C" int gcge_hip_star_grid(int nrows, long row_begin, long nglobal, const int* rowptr, const int* colidx_global, const double* val, long* out) {
  StarRows M = {nrows, nrows, row_begin, nglobal, nullptr, rowptr, colidx_global, val};
  M.global_cols = true;
  int Rx = 0, Ry = 0, Rz = 0; long sy = 0, sz = 0;
  if (!star_offsets(M, &Rx, &Ry, &Rz, &sy, &sz)) return 0;
  if (out) { out[0] = sy; out[1] = sz / sy; out[2] = nglobal / sz; out[3] = std::max(Rx, std::max(Ry, Rz)); }
  return 1;
}

// Structural self-check of the split (host only; tests): every clean row is rebuilt from the star, its diagonal and the grid and
// compared with the CSR row, bit for bit; every other row must sit in the remainder unchanged.  0: identical; > 0: differences;
// -1: the matrix does not take this form.  out[0..4] = nx, ny, nz, arm length, clean rows; out[5..10] (slabs) = first / last + 1
// plane of the slab, first / last + 1 plane the sweep may load, rows of X where the planes below / above begin (-1: none).
static long star_selfcheck(const StarRows& M, long* out) {
  StarHost H;
  const int nrows = M.nrows; const long row_begin = M.row_begin; const int* rowptr = M.rowptr; const int* colidx = M.colidx; const double* val = M.val;
  if (!star_build_host(M, &H)) return -1;
  const StarGeom& g = H.g;
  const long sy = g.nx, sz = (long)g.nx * g.ny;
  if (out) {
    out[0] = g.nx; out[1] = g.ny; out[2] = g.nz; out[3] = H.R; out[4] = H.nclean;
    out[5] = g.zs; out[6] = g.ze; out[7] = g.zmin; out[8] = g.zmax;
    out[9] = g.zmin < g.zs ? g.lo_off + sz * g.zmin : -1; out[10] = g.ze < g.zmax ? g.hi_off + sz * g.ze : -1;
  }
  if (out) out[11] = H.rem_rowptr[nrows];
  long bad = 0;
  // where the sweep finds grid point (global row gq): the row of X, as the kernel computes it
  auto xrow = [&](long gq) -> long {
    if (M.box != nullptr) return H.inv[gq];
    const int zz = (int)(gq / sz); return (zz < g.zs ? g.lo_off : zz >= g.ze ? g.hi_off : g.mid_off) + gq;
  };
  auto there = [&](long gq) -> bool { return M.box == nullptr || H.inv[gq] >= 0; };   // a point of the domain
  // every row rebuilt as star + diagonal + remainder (per column, in the order the kernels add them) against the CSR row: clean
  // rows bit for bit; the others to the one rounding of "entry minus coefficient" at the star positions; a position the row
  // has no entry at must cancel exactly
  std::vector<std::pair<long, double>> want, got;
  for (int r = 0; r < nrows; ++r) {
    want.clear(); got.clear();
    for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) want.emplace_back((long)colidx[q], val[q]);   // local columns = rows of X
    const long gr = M.gpos(r);
    const int gz = (int)(gr / sz), gy = (int)((gr - (long)gz * sz) / sy), gx = (int)(gr - (long)gz * sz - (long)gy * sy);
    const bool is_clean = H.clean[r] != 0;
    if (is_clean != (H.rem_rowptr[r + 1] == H.rem_rowptr[r])) ++bad;
    bool stored_diag = false;
    for (auto& w : want) stored_diag |= w.first == r;
    if (stored_diag || H.diag[r] != 0.0) got.emplace_back((long)r, H.diag[r]);
    for (int k = 1; k <= STAR_R; ++k) {
      if (star_bits(H.c.cx[k])) { if (gx - k >= 0 && there(gr - k)) got.emplace_back(xrow(gr - k), H.c.cx[k]); if (gx + k < g.nx && there(gr + k)) got.emplace_back(xrow(gr + k), H.c.cx[k]); }
      if (star_bits(H.c.cy[k])) { if (gy - k >= 0 && there(gr - k * sy)) got.emplace_back(xrow(gr - k * sy), H.c.cy[k]); if (gy + k < g.ny && there(gr + k * sy)) got.emplace_back(xrow(gr + k * sy), H.c.cy[k]); }
      if (star_bits(H.c.cz[k])) {
        if (gz - k >= 0 && there(gr - k * sz)) { if (gz - k < g.zmin) ++bad; got.emplace_back(xrow(gr - k * sz), H.c.cz[k]); }
        if (gz + k < g.nz && there(gr + k * sz)) { if (gz + k >= g.zmax) ++bad; got.emplace_back(xrow(gr + k * sz), H.c.cz[k]); }
      }
    }
    const size_t nstar = got.size();
    for (int q = H.rem_rowptr[r]; q < H.rem_rowptr[r + 1]; ++q) got.emplace_back((long)H.rem_col[q], H.rem_val[q]);
    auto less = [](const std::pair<long, double>& p, const std::pair<long, double>& q) { return p.first < q.first; };
    std::stable_sort(want.begin(), want.end(), less); std::stable_sort(got.begin(), got.end(), less);   // (stable: star part before remainder)
    (void)nstar;
    size_t i = 0, j = 0;
    bool ok = true;
    while (i < want.size() || j < got.size()) {
      const long c = (j >= got.size() || (i < want.size() && want[i].first <= got[j].first)) ? want[i].first : got[j].first;
      double wv = 0.0, gv = 0.0, mag = 0.0; int nw = 0, ng = 0;
      while (i < want.size() && want[i].first == c) { wv += want[i].second; ++i; ++nw; }
      while (j < got.size() && got[j].first == c) { gv += got[j].second; mag = std::max(mag, fabs(got[j].second)); ++j; ++ng; }
      if (is_clean || nw == 0 || ng <= 1) { if (star_bits(wv + 0.0) != star_bits(gv + 0.0) && !(wv == 0.0 && gv == 0.0)) ok = false; }
      else if (fabs(wv - gv) > 4.0 * 2.220446049250313e-16 * std::max(mag, fabs(wv))) ok = false;
    }
    if (!ok) ++bad;
  }
  return bad;
}
extern "C" long gcge_hip_star_selfcheck_slab(int nrows, int ncols_local, long row_begin, long nglobal, const int* ghost, const int* rowptr,
                                             const int* colidx, const double* val, long* out) {
  const StarRows M = {nrows, ncols_local, row_begin, nglobal, ghost, rowptr, colidx, val};
  return star_selfcheck(M, out);
}
// the same for a matrix on a MASKED grid: row r is grid point box_of_row[r] = x + nx (y + ny z) (ascending: scan order); out as above
extern "C" long gcge_hip_star_selfcheck_grid(int nrows, const int* rowptr, const int* colidx, const double* val, int nx, int ny, int nz,
                                             const int* box_of_row, long* out) {
  StarRows M = {nrows, nrows, 0, (long)nx * ny * nz, nullptr, rowptr, colidx, val};
  M.box = box_of_row; M.bnx = nx; M.bny = ny; M.bnz = nz;
  return star_selfcheck(M, out);
}
// The geometry star_infer_box recovers (host only; tests, tools): dims[0..2] = nx, ny, nz of the bounding box, box_of_row[r] = x + nx
// (y + ny z).  1: found, 0: the rows are not the points of a masked grid in scan order.
extern "C" int gcge_hip_star_infer_grid(int nrows, const int* rowptr, const int* colidx, int* dims, int* box_of_row) {
  std::vector<int> box; int nx = 0, ny = 0, nz = 0;
  if (!star_infer_box(nrows, rowptr, colidx, &box, &nx, &ny, &nz)) return 0;
  dims[0] = nx; dims[1] = ny; dims[2] = nz;
  memcpy(box_of_row, box.data(), (size_t)nrows * sizeof(int));
  return 1;
}
extern "C" long gcge_hip_star_selfcheck(int nrows, int ncols_local, const int* rowptr, const int* colidx, const double* val, long* out) {
  if (ncols_local != nrows) return -1;
  long o[12];
  const long bad = gcge_hip_star_selfcheck_slab(nrows, ncols_local, 0, nrows, nullptr, rowptr, colidx, val, o);
  if (out && bad >= 0) for (int i = 0; i < 5; ++i) out[i] = o[i];
  return bad;
}
