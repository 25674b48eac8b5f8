// K1 (grid path) — what the upload-time analysis of a matrix with star rows (star_split.hip), the plane sweep built on its result
// (spmm_star.hip) and the upload that owns that result (mat_upload.hip) share.
#ifndef GCGE_STAR_SPLIT_H
#define GCGE_STAR_SPLIT_H
#include "gcge_hip_internal.h"
namespace gcge {
constexpr int STAR_R = 6;                       // arm length the kernel is built for (shorter stars: zero coefficients)
struct StarCoef { double cx[STAR_R + 1], cy[STAR_R + 1], cz[STAR_R + 1]; };   // [k]: coefficient of the neighbours k steps away ([0] unused)
// Where the planes of the grid live in a block of vectors.  One rank: the slab is the grid.  A row slab of a partitioned matrix
// (planes [zs, ze) of nz; cuts on plane boundaries) finds the planes below and above among its halo rows: the halo rows are
// ascending by global index, so the up to R whole planes on either side are two contiguous runs of them — row of grid point
// (in-plane offset i, plane zz) = off + plane_rows * zz + i with off = mid_off inside the slab, lo_off below, hi_off above;
// planes outside [zmin, zmax) are outside the grid (Dirichlet: zero) or beyond the star's arms (coefficient zero): never loaded.
struct StarGeom { int nx, ny, nz, zs, ze, zmin, zmax; long lo_off, mid_off, hi_off; };
struct StarHost {
  StarGeom g; int R = 0; StarCoef c; long nclean = 0;
  std::vector<double> diag;                                           // NaN: row stays in the remainder
  std::vector<char> clean;                                            // 1: star row
  std::vector<int> inv;                                               // masked domains: grid point -> row (-1: none)
  std::vector<int> own_box; int own_dims[3] = {0, 0, 0};              // masked domains whose geometry was recovered here (star_infer_box): box index of every row; nx, ny, nz
  std::vector<int> rem_rowptr, rem_col; std::vector<double> rem_val;  // every entry of the rows that are not clean (local columns)
  // value maps (value_maps.h), built only when keep_maps is set before star_build_host: where diag / rem_val came from in the CSR values
  bool keep_maps = false;
  std::vector<int> diag_src;                                          // [row] CSR index of the stored diagonal entry, -1: none
  std::vector<int> rem_src; std::vector<unsigned char> rem_code;      // [remainder entry] CSR index (-1: taken back), coefficient code
  std::vector<unsigned char> pin;                                     // [CSR entry] see value_maps.h
};

// The rows of one slab: local rows [0, nrows) are global rows row_begin + r; local column c < nrows is global column row_begin + c,
// c >= nrows is halo row c - nrows = global column ghost[c - nrows] (ascending).  One rank: row_begin = 0, no halo columns.
// With a geometry (box != NULL; one rank, no halo columns): row r is grid point box[r] = x + bnx (y + bny z) of a bnx x bny x bnz
// box of which only some points are rows (a masked domain: the grid points inside a sphere, say) — "global index" then means
// the box index, and nglobal the size of the box.
struct StarRows {
  int nrows, ncols_local; long row_begin, nglobal; const int* ghost; const int *rowptr, *colidx; const double* val;
  bool global_cols = false;                                           // colidx holds global columns already (partitioners)
  const int* box = nullptr; int bnx = 0, bny = 0, bnz = 0;
  bool box_cols = false;                                              // box[] covers every LOCAL column (a row slab of a masked grid: own rows, then halo rows)
  long gcol(int c) const { return box != nullptr ? (long)box[c] : global_cols ? (long)c : c < nrows ? row_begin + c : (long)ghost[c - nrows]; }
  long gpos(int r) const { return box != nullptr ? (long)box[r] : row_begin + r; }
};
bool star_build_host(const StarRows& M, StarHost* H);
bool star_infer_box(int nrows, const int* rowptr, const int* colidx, std::vector<int>* box_, int* nx_, int* ny_, int* nz_);
}  // namespace gcge
// spmm_star.hip: the sweep's device object (NULL: none) and, through *host, the split behind it — the caller's to read and delete
extern "C" void* gcge_hip_star_build(int nrows, int ncols_local, long row_begin, long nglobal, const int* ghost, const int* rowptr, const int* colidx,
                                     const double* val, const GcgeGridGeom* geom, gcge::StarHost** host, int keep_maps);
#endif
