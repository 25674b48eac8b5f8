// The multigrid hierarchy of the HIP back-end: ops->MultiGridCreate / MultiGridDestroy (reference slots src/ops.h:134-139).
//
// The reference's BlockAMG (src/ops_lin_sol.c:466-715; ours: csrc/host/lin_sol.c) takes A_0 = A, A_{l+1}, P_l from the back-end:
// app/app_slepc.c:648-728 extracts them from PETSc GAMG, app/app_hypre.c from BoomerAMG, app/app_lapack.c:863-929 builds a 1-D toy.
// Here: the aggregation hierarchy of include/gcge_multigrid.h (2 x 2 x 2 cells of a detected grid or of a masked grid's box, greedy
// aggregates otherwise; A_{l+1} = scale P^T A_l P), built from the device-resident CSR of A one level after the other
// (multigrid_create_device: aggregates, Galerkin products and P / P^T on the device, mg_device.hip) or, in mode 1 and when a level
// is out of the kernels' reach, by the host builders on the downloaded CSR (multigrid_create_host).  Either way every coarse level
// goes up through gcge_hip_mat_create (gcge_hip_mat_create_grid on a masked grid) — so a coarse Laplacian gets the pattern kernels,
// a coarse real-space Hamiltonian its blocks, exactly like a matrix the caller uploads.  A matrix without a grid under
// gcge_mg_set_graph_method (1) is aggregated by MIS-2 on the device (mg_aggregate.hip) and its coarse levels go up through
// gcge_hip_mat_create_as_given: their rows keep the hierarchy's numbering whatever the row order search would do.  The prolongations are rectangular matrices
// (GCGE_HIP_MAT_::rect_ncols): CSR of P for MatDotMultiVec, CSR of P^T for MatTransDotMultiVec, both through the generic CSR
// kernel (spmm.hip) — one non-zero per fine row, every fine row of the block read or written exactly once.
// Row slabs (one rank per GPU): a slab of whole planes coarsens by itself (every rank pairs its own planes) — local prolongations, coarse slabs
// through the slab constructor (gcge_hip_mat_create_slab over RCCL, or a registered factory: the tests' torch.distributed transport).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <array>
#include <vector>

#include "gcge_hip.h"
#include "gcge_solver.h"
#include "gcge_multigrid.h"
#include "gcge_hip_internal.h"

static double mg_now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_rect(int nrows, int ncols, const int* rowptr, const int* colidx, const double* val,
                                                  const int* t_rowptr, const int* t_colidx, const double* t_val) {
  if (gcge_hip_init(-1) != 0) return nullptr;
  GCGE_HIP_MAT* P = (GCGE_HIP_MAT*)calloc(1, sizeof(GCGE_HIP_MAT));
  const size_t nnz = (size_t)rowptr[nrows];
  GCGE_REQUIRE(nrows > 0 && ncols > 0 && (size_t)t_rowptr[ncols] == nnz, "gcge_hip_mat_create_rect: the two triples hold the same entries");
  for (size_t k = 0; k < nnz; ++k) GCGE_REQUIRE(colidx[k] >= 0 && colidx[k] < ncols && t_colidx[k] >= 0 && t_colidx[k] < nrows, "gcge_hip_mat_create_rect: index in range");
  P->nrows = nrows; P->nglobal = nrows; P->nnz = (long)nnz; P->rect_ncols = ncols;
  P->rect_one_per_row = nnz == (size_t)nrows;
  for (int r = 0; r < nrows && P->rect_one_per_row; ++r) P->rect_one_per_row = rowptr[r + 1] - rowptr[r] == 1;
  auto up = [](const void* h, size_t bytes) { void* d = nullptr; GCGE_HIP_CHECK(hipMalloc(&d, bytes ? bytes : 8)); GCGE_HIP_CHECK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); return d; };
  P->d_rowptr = (int*)up(rowptr, ((size_t)nrows + 1) * sizeof(int));
  P->d_colidx = (int*)up(colidx, nnz * sizeof(int));
  P->d_val = (double*)up(val, nnz * sizeof(double));
  P->d_t_rowptr = (int*)up(t_rowptr, ((size_t)ncols + 1) * sizeof(int));
  P->d_t_colidx = (int*)up(t_colidx, nnz * sizeof(int));
  P->d_t_val = (double*)up(t_val, nnz * sizeof(double));
  return P;
}

// the same from the CSR triple of P alone (the transpose by counting, ascending columns)
extern "C" GCGE_HIP_MAT* gcge_hip_mat_create_rect_csr(const GCGE_CSR* P) {
  const int nr = P->nrows, nc = P->ncols;
  const size_t nnz = (size_t)P->rowptr[nr];
  std::vector<int> tp((size_t)nc + 1, 0), tc(nnz ? nnz : 1); std::vector<double> tv(nnz ? nnz : 1);
  for (size_t k = 0; k < nnz; ++k) { GCGE_REQUIRE(P->colidx[k] >= 0 && P->colidx[k] < nc, "gcge_hip_mat_create_rect_csr: column in range"); ++tp[(size_t)P->colidx[k] + 1]; }
  for (int c = 0; c < nc; ++c) tp[c + 1] += tp[c];
  std::vector<int> fill(tp.begin(), tp.end() - 1);
  for (int r = 0; r < nr; ++r)
    for (int k = P->rowptr[r]; k < P->rowptr[r + 1]; ++k) { const int q = fill[P->colidx[k]]++; tc[q] = r; tv[q] = P->val[k]; }
  return gcge_hip_mat_create_rect(nr, nc, P->rowptr, P->colidx, P->val, tp.data(), tc.data(), tv.data());
}


// one hierarchy per MultiGridCreate call; found again through the A_array pointer MultiGridDestroy hands back
// (scale, slab: what gcge_hip_multigrid_refresh needs to know of the build — the factor of its Galerkin products, and whether the levels
// are row slabs; of a slab hierarchy also, per level l < num_levels - 1, colagg[l]: a device array of nrows_l + nghost_l ints, the LOCAL
// column of level l + 1 every local column of level l aggregates into (gcge_mg_slab_colagg), and nlo[l]: the halo columns of level l + 1
// that lie below its slab.  Empty: the halo rows of some level were not named, the hierarchy cannot be refreshed.  Freed with it.)
struct MgHold {
  void** A_array; std::vector<GCGE_HIP_MAT*> owned; int num_levels = 0; double scale = 0.5; bool slab = false;
  std::vector<int*> colagg; std::vector<int> nlo;
};
static std::vector<MgHold> g_mg;
static double g_mg_seconds = 0.0;
extern "C" double gcge_hip_multigrid_seconds(void) { return g_mg_seconds; }   // host + upload time of the last MultiGridCreate

static void download_csr(const GCGE_HIP_MAT_* A, GCGE_CSR* out, std::vector<int>& rp, std::vector<int>& ci, std::vector<double>& va) {
  rp.resize((size_t)A->nrows + 1); ci.resize((size_t)(A->nnz ? A->nnz : 1)); va.resize((size_t)(A->nnz ? A->nnz : 1));
  GCGE_HIP_CHECK(hipStreamSynchronize((hipStream_t)gcge_hip_stream()));
  GCGE_HIP_CHECK(hipMemcpy(rp.data(), A->d_rowptr, ((size_t)A->nrows + 1) * sizeof(int), hipMemcpyDeviceToHost));
  GCGE_HIP_CHECK(hipMemcpy(ci.data(), A->d_colidx, (size_t)A->nnz * sizeof(int), hipMemcpyDeviceToHost));
  GCGE_HIP_CHECK(hipMemcpy(va.data(), A->d_val, (size_t)A->nnz * sizeof(double), hipMemcpyDeviceToHost));
  memset(out, 0, sizeof *out);
  out->nrows = A->nrows; out->ncols = A->nrows; out->row_begin = 0; out->nnz = A->nnz;
  out->rowptr = rp.data(); out->colidx = ci.data(); out->val = va.data();
}

// the last MultiGridCreate: seconds per phase and bytes copied device to host
enum { MG_DETECT, MG_AGGREGATE, MG_GALERKIN, MG_TRANSFER, MG_COARSE, MG_OTHER, MG_NPHASE };
static double g_mg_phase[MG_NPHASE]; static long g_mg_d2h = 0;
static int g_mg_mode = 0;
extern "C" void gcge_hip_multigrid_mode(int mode) { g_mg_mode = mode; }
extern "C" int gcge_hip_multigrid_get_mode(void) { return g_mg_mode; }
extern "C" void gcge_hip_multigrid_stats(double* seconds6, long* d2h_bytes) {
  if (seconds6 != nullptr) for (int i = 0; i < MG_NPHASE; ++i) seconds6[i] = g_mg_phase[i];
  if (d2h_bytes != nullptr) *d2h_bytes = g_mg_d2h;
}
static long csr_bytes(long nrows, long nnz) { return (nrows + 1) * (long)sizeof(int) + nnz * (long)(sizeof(int) + sizeof(double)); }

static gcge_hip_slab_factory_fn g_slab_factory = nullptr; static void* g_slab_factory_ctx = nullptr;
extern "C" void gcge_hip_set_slab_factory(gcge_hip_slab_factory_fn fn, void* ctx) { g_slab_factory = fn; g_slab_factory_ctx = ctx; }

// ------------------------------------------------------------------------------------------------------------ what every build ends in
// the arguments of the MultiGridCreate slot, and what a build hands over: the coarse handles in hierarchy order (As / Bs: levels 1 ..,
// Bs empty without a B to coarsen), the grid or box of every level (zeros: aggregated over the graph) and what the trace says of it
struct MgSlot { void*** A_array; void*** B_array; void*** P_array; int* num_levels; void* A; void* B; };
struct MgBuilt {
  std::vector<GCGE_HIP_MAT*> As, Bs, Ps;
  std::vector<std::array<int, 3>> dims;
  bool masked = false; const char* how = "";       // how: " (device build)", " (host build)" or nothing
  int rank = 0, world = 0; std::vector<long> global_rows;       // a row slab: the rows of all ranks, level by level
  std::vector<int*> colagg; std::vector<int> nlo;               // ... and what MgHold keeps for a refresh
};

static void mg_install(const MgSlot& s, const MgBuilt& b) {
  const int L = (int)b.As.size() + 1;
  MgHold h;
  *s.A_array = (void**)calloc(L, sizeof(void*));
  *s.P_array = (void**)calloc(L > 1 ? L - 1 : 1, sizeof(void*));
  if (s.B_array != nullptr) *s.B_array = (void**)calloc(L, sizeof(void*));
  (*s.A_array)[0] = s.A;
  if (s.B_array != nullptr) (*s.B_array)[0] = s.B;
  for (int l = 1; l < L; ++l) {
    (*s.A_array)[l] = b.As[l - 1]; h.owned.push_back(b.As[l - 1]);
    if (!b.Bs.empty()) { (*s.B_array)[l] = b.Bs[l - 1]; h.owned.push_back(b.Bs[l - 1]); }
  }
  for (int l = 0; l + 1 < L; ++l) { (*s.P_array)[l] = b.Ps[l]; h.owned.push_back(b.Ps[l]); }
  if (getenv("GCGE_MG_TRACE") != nullptr)
    for (int l = 0; l < L; ++l) {
      const GCGE_HIP_MAT* m = (const GCGE_HIP_MAT*)(*s.A_array)[l];
      const int* d = b.dims[l].data();
      if (b.world > 0)
        fprintf(stderr, "MultiGridCreate: rank %d of %d, level %d: %d of %ld rows, %ld non-zeros, grid %d x %d x %d, K1 form %s\n", b.rank, b.world, l, m->nrows,
                b.global_rows[l], m->nnz, d[0], d[1], d[2], gcge_hip_mat_spmm_form(m));
      else if (b.masked)
        fprintf(stderr, "MultiGridCreate: level %d: %d rows, %ld non-zeros, masked grid in the box %d x %d x %d (%.1f%% of it), K1 form %s%s\n", l, m->nrows,
                m->nnz, d[0], d[1], d[2], 100.0 * m->nrows / ((double)d[0] * d[1] * d[2]), gcge_hip_mat_spmm_form(m), b.how);
      else
        fprintf(stderr, "MultiGridCreate: level %d: %d rows, %ld non-zeros, grid %d x %d x %d, K1 form %s%s\n", l, m->nrows, m->nnz, d[0], d[1], d[2],
                gcge_hip_mat_spmm_form(m), b.how);
    }
  h.A_array = *s.A_array; h.num_levels = L; h.slab = b.world > 0; h.colagg = b.colagg; h.nlo = b.nlo;
  gcge_mg_get_defaults(&h.scale, nullptr, nullptr);       // (every build takes the defaults in force when it runs)
  g_mg.push_back(h);
  *s.num_levels = L;
}

// a finished host hierarchy as handles: all A_l / B_l level by level through make(l, csr), then all P_l
template <class Make> static void mg_load_host(const GCGE_MG& mg, bool withB, MgBuilt& out, Make make) {
  for (int l = 1; l < mg.num_levels; ++l) {
    GCGE_HIP_MAT* a = make(l, mg.A[l]);
    GCGE_REQUIRE(a != nullptr, "MultiGridCreate: upload of a coarse matrix");
    out.As.push_back(a);
    if (withB) {
      GCGE_HIP_MAT* b = make(l, mg.B[l]);
      GCGE_REQUIRE(b != nullptr, "MultiGridCreate: upload of a coarse B");
      out.Bs.push_back(b);
    }
  }
  for (int l = 0; l + 1 < mg.num_levels; ++l) {
    GCGE_HIP_MAT* p = gcge_hip_mat_create_rect(mg.P[l].nrows, mg.P[l].ncols, mg.P[l].rowptr, mg.P[l].colidx, mg.P[l].val,
                                               mg.PT[l].rowptr, mg.PT[l].colidx, mg.PT[l].val);
    GCGE_REQUIRE(p != nullptr, "MultiGridCreate: upload of a prolongation");
    out.Ps.push_back(p);
  }
  for (int l = 0; l < mg.num_levels; ++l) out.dims.push_back({mg.dims[l][0], mg.dims[l][1], mg.dims[l][2]});
}

// ------------------------------------------------------------------------------------------------------------ row slabs
// a row slab (one rank per GPU): whole planes of a detected grid, cut on any plane boundary — every rank coarsens its own slab
// (gcge_mg_build_slab), the coarse slabs go through the slab constructor (ghost list, halo plan: collective); no B below level 0
static void multigrid_create_slab(const MgSlot& s, const GCGE_HIP_MAT_* mA) {
  GCGE_REQUIRE(mA->h_part != nullptr && mA->part_world >= 1, "MultiGridCreate on a row slab: the partition of all ranks (gcge_hip_mat_create_slab / gcge_hip_mat_set_partition)");
  GCGE_REQUIRE(mA->nghost == 0 || mA->h_ghost_global != nullptr, "MultiGridCreate on a row slab: the global rows behind the halo columns (gcge_hip_mat_create_local_ghosts)");
  const int world = mA->part_world;
  int rank = -1;
  for (int r = 0; r < world; ++r) if (mA->h_part[r] == mA->row_begin && mA->h_part[r + 1] == (long)mA->row_begin + mA->nrows) rank = r;
  GCGE_REQUIRE(rank >= 0, "MultiGridCreate on a row slab: the slab is one of the partition's");
  GCGE_CSR cA; std::vector<int> rp, ci; std::vector<double> va;
  download_csr(mA, &cA, rp, ci, va);
  for (size_t k = 0; k < (size_t)mA->nnz; ++k) ci[k] = ci[k] < mA->nrows ? mA->row_begin + ci[k] : mA->h_ghost_global[ci[k] - mA->nrows];   // local -> GLOBAL columns
  cA.row_begin = mA->row_begin; cA.ncols = (int)mA->h_part[world];
  int dims[3] = {0, 0, 0};
  if (!gcge_mg_detect_grid(&cA, dims, nullptr) || (long)dims[0] * dims[1] * dims[2] != mA->h_part[world]) {
    fprintf(stderr, "MultiGridCreate (HIP back-end): a row slab is coarsened along a detected grid only; this matrix shows none\n");
    abort();
  }
  GCGE_MG mg; long* parts = nullptr;
  const int rc = gcge_mg_build_slab(&cA, dims, mA->h_part, rank, world, *s.num_levels, 0.0, &mg, &parts);
  if (rc != 0) { fprintf(stderr, "MultiGridCreate (HIP back-end): gcge_mg_build_slab failed (%d) — slabs must be whole planes of the %d x %d x %d grid\n", rc, dims[0], dims[1], dims[2]); abort(); }
  MgBuilt built;
  built.rank = rank; built.world = world;
  for (int l = 0; l < mg.num_levels; ++l) built.global_rows.push_back(parts[(size_t)l * (world + 1) + world]);
  const int buf_cols = mA->buf_cols > 0 ? mA->buf_cols : 128;
  mg_load_host(mg, false, built, [&](int l, const GCGE_CSR& c) {
    const long* pl = parts + (size_t)l * (world + 1);
    GCGE_HIP_MAT* a = g_slab_factory != nullptr ? g_slab_factory(pl, world, rank, c.rowptr, c.colidx, c.val, buf_cols, g_slab_factory_ctx)
                                                : gcge_hip_mat_create_slab(pl, c.rowptr, c.colidx, c.val, buf_cols);
    GCGE_REQUIRE(a != nullptr, "MultiGridCreate: construction of a coarse slab");
    if (a->h_part == nullptr) gcge_hip_mat_set_partition(a, pl, world);
    return a;
  });
  // what a refresh in place needs of the neighbours, while the host still knows it: where every local column of a level — the halo
  // columns through their owners' pairing and the coarse slab's halo list — lands among the local columns of the next one
  bool named = true;
  for (int l = 0; l + 1 < mg.num_levels && named; ++l) {
    const GCGE_HIP_MAT_* f = l == 0 ? mA : built.As[(size_t)l - 1];
    const GCGE_HIP_MAT_* c = built.As[(size_t)l];
    if ((f->nghost > 0 && f->h_ghost_global == nullptr) || (c->nghost > 0 && c->h_ghost_global == nullptr)) { named = false; break; }
    std::vector<int> colagg((size_t)f->nrows + f->nghost + 1);
    int nlo = 0;
    if (gcge_mg_slab_colagg(mg.dims[l], parts + (size_t)l * (world + 1), rank, world, f->h_ghost_global, f->nghost, c->h_ghost_global, c->nghost,
                            colagg.data(), &nlo) != 0) { named = false; break; }
    for (int k = 0; k < f->nrows + f->nghost; ++k) GCGE_REQUIRE(colagg[(size_t)k] >= 0 && colagg[(size_t)k] < c->nrows + c->nghost, "MultiGridCreate on a row slab: a local column of the coarse slab");
    int* d = nullptr;
    GCGE_HIP_CHECK(hipMalloc(&d, colagg.size() * sizeof(int)));
    GCGE_HIP_CHECK(hipMemcpy(d, colagg.data(), colagg.size() * sizeof(int), hipMemcpyHostToDevice));
    built.colagg.push_back(d); built.nlo.push_back(nlo);
  }
  if (!named) { for (int* d : built.colagg) hipFree(d); built.colagg.clear(); built.nlo.clear(); }
  gcge_mg_free(&mg);
  free(parts);
  mg_install(s, built);
}

// ------------------------------------------------------------------------------------------------------------ the host builds
// mode 1, and whatever the device build gives up on: gcge_mg_build on the downloaded CSR of A (and B) — gcge_mg_build_masked with the
// handle's geometry on a masked grid, whose levels go up through gcge_hip_mat_create_grid with THEIR geometry (see below)
static void multigrid_create_host(const MgSlot& s, const GCGE_HIP_MAT_* mA, const GCGE_HIP_MAT_* mB, bool masked) {
  double t = mg_now();
  GCGE_CSR cA, cB; std::vector<int> rpA, ciA, rpB, ciB; std::vector<double> vaA, vaB;
  download_csr(mA, &cA, rpA, ciA, vaA);
  if (mB != nullptr) download_csr(mB, &cB, rpB, ciB, vaB);
  g_mg_d2h += csr_bytes(mA->nrows, mA->nnz) + (mB != nullptr ? csr_bytes(mB->nrows, mB->nnz) : 0);
  g_mg_phase[MG_TRANSFER] += mg_now() - t; t = mg_now();
  GCGE_MG mg;
  MgBuilt built;
  built.masked = masked;
  if (masked) {
    const int rc = gcge_mg_build_masked(&cA, mB != nullptr ? &cB : nullptr, mA->geom_dims, mA->h_box, *s.num_levels, 0, 0.0, &mg);
    if (rc != 0) { fprintf(stderr, "MultiGridCreate: gcge_mg_build_masked failed (%d)\n", rc); abort(); }
    built.how = " (host build)";
  } else if (gcge_mg_build(&cA, mB != nullptr ? &cB : nullptr, *s.num_levels, 0, 0.0, &mg) != 0) { fprintf(stderr, "MultiGridCreate: out of host memory\n"); abort(); }
  g_mg_phase[masked ? MG_AGGREGATE : MG_OTHER] += mg_now() - t; t = mg_now();       // (all of the host builder, whatever it did)
  const bool as_given = !masked && gcge_mg_get_graph_method() == 1;       // (MIS-2 levels: rows as given; a level on a grid has dims)
  mg_load_host(mg, s.B_array != nullptr && mB != nullptr, built, [&](int l, const GCGE_CSR& c) {
    const int* d = mg.dims[l];
    if (masked) return gcge_hip_mat_create_grid(c.nrows, c.rowptr, c.colidx, c.val, d[0], d[1], d[2], gcge_mg_level_box(&mg, l));
    if (as_given && d[0] == 0) return gcge_hip_mat_create_as_given(c.nrows, c.rowptr, c.colidx, c.val);
    return gcge_hip_mat_create(c.nrows, c.nrows, 0, c.rowptr, c.colidx, c.val);
  });
  g_mg_phase[MG_COARSE] += mg_now() - t;
  gcge_mg_free(&mg);
  mg_install(s, built);
}

// ------------------------------------------------------------------------------------------------------------ the device build
// The host builders' hierarchy (same stopping rules, same defaults) from the device-resident CSR of A (and B), one level after the
// other: aggregate, Galerkin products (mg_device.hip), P / P^T from the device arrays, then the coarse level is downloaded (8 x smaller
// than its parent on a grid) and uploaded again through the constructor that analyses it exactly as in the host build; the next level
// is coarsened from the Galerkin output, in hierarchy order — never from the coarse handle, whose rows gcge_hip_mat_create may
// re-order.  Only the aggregation differs between the three kinds of coarsening:
//   grid    2 x 2 x 2 cells of the grid detected from the sampled rows, and their members, in closed form on the device;
//   graph   method 0: the unchanged greedy host aggregation on that level's CSR (downloaded once, then the coarse download of the
//           level before), coarse levels through gcge_hip_mat_create — whose row order search may re-order a level of 65 536 rows or
//           more inside its handle while P / P^T keep the hierarchy's numbering: open for this method;
//           method 1 (gcge_mg_set_graph_method): MIS-2 aggregation on the level's device CSR (mg_aggregate.hip; host-driven rounds, one
//           int per round comes back, the level itself does not), coarse levels through gcge_hip_mat_create_as_given: rows as given,
//           so P / P^T, the blocks of MultiVecCreateByMat and the smoother's parked blocks agree by construction.  Rounds that reach
//           their cap hand the level to the host routine on a downloaded CSR;
//   masked  a handle that carries the geometry of a masked grid (gcge_hip_mat_geometry: the grid points inside a sphere in scan order,
//           the PARSEC matrices): the occupied 2 x 2 x 2 cells of its bounding box, in scan order of the coarse box a masked grid
//           again, from the device-resident box array (counts, two sums, members by binary search); the coarse box array comes back
//           with the level, which goes up through gcge_hip_mat_create_grid with ITS geometry: the rows stay as given (P / P^T match
//           by construction) and the level carries its geometry like a matrix the caller named one for.
// Grid and MIS-2 levels skip that round trip by default (gcge_hip_multigrid_device_levels): the Galerkin output goes to
// gcge_hip_mat_create_device (MIS-2: its as-given variant), which analyses it on the device with the host constructors' result and
// downloads a level only to fall back to them; masked levels need gcge_hip_mat_create_grid and greedy-graph levels are wanted on the
// host by the next aggregation anyway, so both keep the round trip.
// Returns false with nothing left behind when a level is out of the kernels' reach (a coarse row of more than 512 distinct columns,
// 2^31 entries): the caller then builds on the host.
static int g_mg_masked_cells = 1;
extern "C" void gcge_hip_multigrid_masked_cells(int on) { g_mg_masked_cells = on != 0; }
extern "C" int gcge_hip_multigrid_get_masked_cells(void) { return g_mg_masked_cells; }
// grid and MIS-2 hierarchies: the coarse levels go from the Galerkin output into gcge_hip_mat_create_device (1, default) or are
// downloaded for the host constructors (0); the same hierarchy either way
static int g_mg_device_levels = 1;
extern "C" void gcge_hip_multigrid_device_levels(int on) { g_mg_device_levels = on != 0; }
extern "C" int gcge_hip_multigrid_get_device_levels(void) { return g_mg_device_levels; }
static bool mg_is_masked_grid(const GCGE_HIP_MAT_* m) {
  return g_mg_masked_cells && m->geom_kind != 0 && m->d_box != nullptr && (long)m->geom_dims[0] * m->geom_dims[1] * m->geom_dims[2] != (long)m->nrows;
}

struct DevCsr { int n; long nnz; int* rp; int* ci; double* va; bool owned; };
static void devcsr_free(DevCsr& c) { if (c.owned) { hipFree(c.rp); hipFree(c.ci); hipFree(c.va); } c = DevCsr{0, 0, nullptr, nullptr, nullptr, false}; }
enum MgKind { MG_GRID, MG_GRAPH, MG_MASKED };

static bool multigrid_create_device(const MgSlot& s, const GCGE_HIP_MAT_* mA, const GCGE_HIP_MAT_* mB, bool masked) {
  double scale = 0.5, theta = 0.25; int min_rows = 64;
  gcge_mg_get_defaults(&scale, &min_rows, &theta);
  const int max_levels = *s.num_levels;
  GCGE_HIP_CHECK(hipStreamSynchronize((hipStream_t)gcge_hip_stream()));
  double t = mg_now();
  int dims[3] = {0, 0, 0};
  MgKind kind = MG_MASKED;
  if (masked) memcpy(dims, mA->geom_dims, sizeof dims);
  else {
    kind = gcge_hip_mg_detect_grid_device(mA->nrows, mA->d_rowptr, mA->d_colidx, dims, &g_mg_d2h) ? MG_GRID : MG_GRAPH;
    if (kind == MG_GRAPH) dims[0] = dims[1] = dims[2] = 0;
    g_mg_phase[MG_DETECT] += mg_now() - t;
  }
  MgBuilt built;
  built.masked = masked; built.how = " (device build)";
  DevCsr fa{mA->nrows, mA->nnz, mA->d_rowptr, mA->d_colidx, mA->d_val, false};
  DevCsr fb{0, 0, nullptr, nullptr, nullptr, false};
  if (mB != nullptr) fb = DevCsr{mB->nrows, mB->nnz, mB->d_rowptr, mB->d_colidx, mB->d_val, false};
  GCGE_CSR hostA; memset(&hostA, 0, sizeof hostA);       // the level's CSR on the host once it is there (what a graph level aggregates)
  int* d_box = mA->d_box; bool own_box = false;          // masked: the level's box array (level 0: the handle's)
  bool ok = true;
  const bool mis2 = kind == MG_GRAPH && gcge_mg_get_graph_method() == 1, trace = getenv("GCGE_MG_TRACE") != nullptr;
  for (int l = 0; l + 1 < max_levels; ++l) {
    const int nf = fa.n;
    if (nf <= min_rows) break;
    t = mg_now();
    int nc = 0, cdims[3] = {0, 0, 0};
    int *d_agg = nullptr, *d_ptr = nullptr, *d_mem = nullptr, *d_cbox = nullptr;
    GCGE_HIP_CHECK(hipMalloc(&d_agg, (size_t)nf * sizeof(int)));
    GCGE_HIP_CHECK(hipMalloc(&d_mem, (size_t)nf * sizeof(int)));
    if (kind == MG_MASKED) {
      nc = gcge_hip_mg_agg_masked_device(dims, d_box, nf, d_agg, d_mem, &d_ptr, &d_cbox, cdims, &g_mg_d2h);
      g_mg_phase[MG_AGGREGATE] += mg_now() - t;
    } else if (kind == MG_GRID) {
      nc = ((dims[0] + 1) / 2) * ((dims[1] + 1) / 2) * ((dims[2] + 1) / 2);
      GCGE_HIP_CHECK(hipMalloc(&d_ptr, ((size_t)nc + 1) * sizeof(int)));
      gcge_hip_mg_agg_grid_device(dims, d_agg, d_ptr, d_mem, cdims);
      g_mg_phase[MG_AGGREGATE] += mg_now() - t;
    } else if (mis2 && (nc = gcge_hip_mg_agg_graph_device(nf, fa.rp, fa.ci, fa.va, theta, d_agg, d_mem, &d_ptr, &g_mg_d2h)) >= 0) {
      g_mg_phase[MG_AGGREGATE] += mg_now() - t;
      if (trace) fprintf(stderr, "MultiGridCreate: level %d: %d rows aggregated on the device in %d rounds: %d aggregates\n", l, nf, gcge_hip_mg_graph_rounds(), nc);
    } else {
      if (mis2) {
        g_mg_phase[MG_AGGREGATE] += mg_now() - t; t = mg_now();
        if (trace) fprintf(stderr, "MultiGridCreate: level %d: the device aggregation gave up after %d rounds; aggregated on the host\n", l, gcge_hip_mg_graph_rounds());
      }
      if (hostA.rowptr == nullptr) {
        if (gcge_hip_mg_download_csr(nf, nf, fa.nnz, fa.rp, fa.ci, fa.va, &hostA, &g_mg_d2h) != 0) { fprintf(stderr, "MultiGridCreate: out of host memory\n"); abort(); }
        g_mg_phase[MG_TRANSFER] += mg_now() - t; t = mg_now();
      }
      std::vector<int> agg((size_t)nf), ptr, mem;
      nc = mis2 ? gcge_mg_aggregate_mis2(&hostA, theta, agg.data()) : gcge_mg_aggregate_graph(&hostA, theta, agg.data());
      if (nc >= 1) gcge_hip_mg_members_host(agg.data(), nf, nc, ptr, mem);
      g_mg_phase[MG_AGGREGATE] += mg_now() - t; t = mg_now();
      if (nc >= 1) {
        GCGE_HIP_CHECK(hipMalloc(&d_ptr, ((size_t)nc + 1) * sizeof(int)));
        GCGE_HIP_CHECK(hipMemcpy(d_agg, agg.data(), (size_t)nf * sizeof(int), hipMemcpyHostToDevice));
        GCGE_HIP_CHECK(hipMemcpy(d_ptr, ptr.data(), ((size_t)nc + 1) * sizeof(int), hipMemcpyHostToDevice));
        GCGE_HIP_CHECK(hipMemcpy(d_mem, mem.data(), (size_t)nf * sizeof(int), hipMemcpyHostToDevice));
      }
      g_mg_phase[MG_TRANSFER] += mg_now() - t;
    }
    auto free_agg = [&] { hipFree(d_agg); hipFree(d_ptr); hipFree(d_mem); };
    if (nc < 1 || (long)nc * 3 > (long)nf * 2) { free_agg(); hipFree(d_cbox); break; }     // coarsening stalled
    t = mg_now();
    DevCsr ca{nc, 0, nullptr, nullptr, nullptr, true}, cb{0, 0, nullptr, nullptr, nullptr, false};
    int rc = gcge_hip_mg_galerkin_device(nf, fa.rp, fa.ci, fa.va, d_agg, nc, d_ptr, d_mem, scale, &ca.rp, &ca.ci, &ca.va, &ca.nnz, &g_mg_d2h);
    if (rc == 0 && mB != nullptr) {
      cb = DevCsr{nc, 0, nullptr, nullptr, nullptr, true};
      rc = gcge_hip_mg_galerkin_device(nf, fb.rp, fb.ci, fb.va, d_agg, nc, d_ptr, d_mem, 1.0, &cb.rp, &cb.ci, &cb.va, &cb.nnz, &g_mg_d2h);
      if (rc != 0) cb.owned = false;
    }
    if (rc != 0) ca.owned = ca.rp != nullptr;
    g_mg_phase[MG_GALERKIN] += mg_now() - t;
    if (rc != 0) { devcsr_free(ca); devcsr_free(cb); free_agg(); hipFree(d_cbox); ok = false; break; }
    t = mg_now();
    GCGE_HIP_MAT* p = gcge_hip_mat_create_rect_device(nf, nc, d_agg, d_ptr, d_mem);
    GCGE_REQUIRE(p != nullptr, "MultiGridCreate: a prolongation from device arrays");
    built.Ps.push_back(p);
    free_agg();
    g_mg_phase[MG_OTHER] += mg_now() - t; t = mg_now();
    GCGE_CSR hc, hb; memset(&hc, 0, sizeof hc); memset(&hb, 0, sizeof hb);
    if (g_mg_device_levels && (kind == MG_GRID || mis2)) {
      // the coarse level never leaves the device: the constructor for device arrays analyses the Galerkin output where it is, and
      // downloads it only to fall back to the host constructor named below (its bytes are booked here)
      auto ingest = [&](const DevCsr& c) {
        long s0[4], s1[4];
        gcge_hip_mat_device_stats(s0);
        GCGE_HIP_MAT* m = mis2 ? gcge_hip_mat_create_device_as_given(nc, c.nnz, c.rp, c.ci, c.va) : gcge_hip_mat_create_device(nc, c.nnz, c.rp, c.ci, c.va);
        gcge_hip_mat_device_stats(s1);
        g_mg_d2h += s1[3] - s0[3];
        return m;
      };
      GCGE_HIP_MAT* a = ingest(ca);
      GCGE_REQUIRE(a != nullptr, "MultiGridCreate: a coarse matrix from device arrays");
      built.As.push_back(a);
      if (s.B_array != nullptr && mB != nullptr) {
        GCGE_HIP_MAT* b = ingest(cb);
        GCGE_REQUIRE(b != nullptr, "MultiGridCreate: a coarse B from device arrays");
        built.Bs.push_back(b);
      }
      g_mg_phase[MG_COARSE] += mg_now() - t;
      gcge_csr_free(&hostA); memset(&hostA, 0, sizeof hostA);       // (a level the host has to aggregate is downloaded when it is needed)
    } else {
      std::vector<int> cbox(masked ? (size_t)nc : 0);
      if (gcge_hip_mg_download_csr(nc, nc, ca.nnz, ca.rp, ca.ci, ca.va, &hc, &g_mg_d2h) != 0 ||
          (mB != nullptr && gcge_hip_mg_download_csr(nc, nc, cb.nnz, cb.rp, cb.ci, cb.va, &hb, &g_mg_d2h) != 0)) { fprintf(stderr, "MultiGridCreate: out of host memory\n"); abort(); }
      if (masked) {
        GCGE_HIP_CHECK(hipMemcpy(cbox.data(), d_cbox, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost));
        g_mg_d2h += (long)((size_t)nc * sizeof(int));
      }
      g_mg_phase[MG_TRANSFER] += mg_now() - t; t = mg_now();
      auto upload = [&](const GCGE_CSR& c) {
        if (masked) return gcge_hip_mat_create_grid(nc, c.rowptr, c.colidx, c.val, cdims[0], cdims[1], cdims[2], cbox.data());
        if (mis2) return gcge_hip_mat_create_as_given(nc, c.rowptr, c.colidx, c.val);
        return gcge_hip_mat_create(nc, nc, 0, c.rowptr, c.colidx, c.val);
      };
      GCGE_HIP_MAT* a = upload(hc);
      GCGE_REQUIRE(a != nullptr, "MultiGridCreate: upload of a coarse matrix");
      built.As.push_back(a);
      if (s.B_array != nullptr && mB != nullptr) {
        GCGE_HIP_MAT* b = upload(hb);
        GCGE_REQUIRE(b != nullptr, "MultiGridCreate: upload of a coarse B");
        built.Bs.push_back(b);
      }
      g_mg_phase[MG_COARSE] += mg_now() - t;
      gcge_csr_free(&hb);
      gcge_csr_free(&hostA); hostA = hc;
    }
    devcsr_free(fa); fa = ca;
    devcsr_free(fb); fb = cb;
    if (own_box) hipFree(d_box);
    d_box = d_cbox; own_box = masked;
    built.dims.push_back({dims[0], dims[1], dims[2]});
    if (kind != MG_GRAPH) { dims[0] = cdims[0]; dims[1] = cdims[1]; dims[2] = cdims[2]; }
  }
  t = mg_now();
  devcsr_free(fa); devcsr_free(fb);
  gcge_csr_free(&hostA);
  if (own_box) hipFree(d_box);
  if (!ok) {
    for (GCGE_HIP_MAT* m : built.As) gcge_hip_mat_destroy(m);
    for (GCGE_HIP_MAT* m : built.Bs) gcge_hip_mat_destroy(m);
    for (GCGE_HIP_MAT* m : built.Ps) gcge_hip_mat_destroy(m);
    if (getenv("GCGE_MG_TRACE") != nullptr) fprintf(stderr, "MultiGridCreate: a level is out of the device path's reach; built on the host\n");
    return false;
  }
  built.dims.push_back({dims[0], dims[1], dims[2]});
  mg_install(s, built);
  g_mg_phase[MG_OTHER] += mg_now() - t;
  return true;
}

static void mg_report(double t0) {
  if (getenv("GCGE_MG_TRACE") == nullptr) return;
  fprintf(stderr, "MultiGridCreate (%s path): %.3f s = detect %.3f + aggregate %.3f + Galerkin %.3f + transfers %.3f + coarse upload %.3f + other %.3f; "
          "%ld bytes device to host\n", g_mg_mode == 0 ? "device" : "host", mg_now() - t0, g_mg_phase[MG_DETECT], g_mg_phase[MG_AGGREGATE],
          g_mg_phase[MG_GALERKIN], g_mg_phase[MG_TRANSFER], g_mg_phase[MG_COARSE], g_mg_phase[MG_OTHER], g_mg_d2h);
}

extern "C" void gcge_hip_multigrid_create(void*** A_array, void*** B_array, void*** P_array, int* num_levels, void* A, void* B, struct OPS_* ops) {
  const GCGE_HIP_MAT_* mA = (const GCGE_HIP_MAT_*)A; const GCGE_HIP_MAT_* mB = (const GCGE_HIP_MAT_*)B;
  const double t0 = mg_now();
  GCGE_REQUIRE(mA != nullptr && mA->rect_ncols == 0 && num_levels != nullptr && *num_levels >= 1, "MultiGridCreate: a square matrix and a level count");
  for (int i = 0; i < MG_NPHASE; ++i) g_mg_phase[i] = 0.0;
  g_mg_d2h = 0;
  const MgSlot s{A_array, B_array, P_array, num_levels, A, B};
  const bool slab = mA->nghost > 0 || mA->part_world > 1;
  if (slab) multigrid_create_slab(s, mA);
  else {
    const bool masked = mg_is_masked_grid(mA);         // a masked grid: the cells of its box at every level, on the device or on the host
    if (g_mg_mode != 0 || !multigrid_create_device(s, mA, mB, masked)) multigrid_create_host(s, mA, mB, masked);
  }
  g_mg_seconds = mg_now() - t0;
  if (!slab) mg_report(t0);
}

extern "C" void gcge_hip_multigrid_destroy(void*** A_array, void*** B_array, void*** P_array, int* num_levels, struct OPS_* ops) {
  GCGE_HIP_CHECK(hipStreamSynchronize((hipStream_t)gcge_hip_stream()));
  for (size_t i = 0; i < g_mg.size(); ++i) {
    if (g_mg[i].A_array != *A_array) continue;
    for (GCGE_HIP_MAT* m : g_mg[i].owned) gcge_hip_mat_destroy(m);
    for (int* d : g_mg[i].colagg) hipFree(d);
    g_mg.erase(g_mg.begin() + (long)i);
    break;
  }
  free(*A_array); *A_array = nullptr;
  free(*P_array); *P_array = nullptr;
  if (B_array != nullptr && *B_array != nullptr) { free(*B_array); *B_array = nullptr; }
}

// ------------------------------------------------------------------------------------------------------------ refresh in place
// A live hierarchy after level 0 took new values (gcge_hip_mat_update_values_device): level by level the values of A_{l+1} = scale P_l^T
// A_l P_l — the numeric half of the Galerkin product (k_mg_galerkin_values, mg_device.hip) on what the handles hold: level l's CSR, the
// aggregates P_l keeps (agg = its columns, ptr / mem = its transpose) and level l + 1's own structure — into a block of the pool, then
// through the in-place update of the coarse handle, which re-derives every stored copy of the values (pad-8, table or row values, star
// diagonal, blocks).  The structure of a Galerkin product does not depend on the values and the sums are those of the build, so a
// refreshed hierarchy is the fresh one bit for bit.  Nothing is all-or-nothing across levels: the first level that declines ends the
// call, and the hierarchy is then stale from that level on (see include/gcge_hip.h).
static long g_mr_stats[4] = {0, 0, 0, 0};
extern "C" void gcge_hip_multigrid_refresh_stats(long out[4]) { for (int i = 0; i < 4; ++i) out[i] = g_mr_stats[i]; }

// Level 0 may live in a row order of the back-end's own (mat_upload.hip "row orders"): the hierarchy was built from the handle's CSR, in
// the handle's order, and P_0's rows are numbered like it.  A re-ordered coarse level would contradict its prolongation.
// A hierarchy of row slabs (multigrid_create_slab) is refreshed like one of whole matrices, every rank its own levels: each coarse row of a
// slab level is scale x the sum over fine rows the rank owns (aggregates never cross a cut), its halo columns only have to know which
// coarse column they fall into (MgHold::colagg), and the coarse slab takes its values through the same in-place update.  Nothing here is
// collective — the ranks agree on the outcome in GCGE_AMGRefresh (csrc/host/harness.c).  No B below level 0 on slabs: A's levels only.
static bool mr_level_ok(const GCGE_HIP_MAT_* m, int level) {
  return m != nullptr && m->rect_ncols == 0 && (level == 0 || real_perm(m->perm) == nullptr) && m->d_rowptr != nullptr;
}
// 0: level l + 1 of `arr` now holds scale P^T (level l) P; 1: declined, the level is as it was
static int mr_level(const MgHold* h, void** arr, int l, const GCGE_HIP_MAT_* P, double scale) {
  const GCGE_HIP_MAT_* f = (const GCGE_HIP_MAT_*)arr[l];
  GCGE_HIP_MAT_* c = (GCGE_HIP_MAT_*)arr[l + 1];
  const size_t bytes = (size_t)(c->nnz > 0 ? c->nnz : 1) * sizeof(double);
  double* work = (double*)gcge_hip_pool_alloc(bytes);
  long u0[6], u1[6];
  gcge_hip_mat_update_stats(u0);
  int rc = h->slab ? gcge_hip_mg_galerkin_values_slab_into(f->nrows + f->nghost, f->d_rowptr, f->d_colidx, f->d_val, h->colagg[(size_t)l], P->rect_ncols,
                                                           P->d_t_rowptr, P->d_t_colidx, scale, c->d_rowptr, c->d_colidx, work, h->nlo[(size_t)l], &g_mr_stats[3])
                   : gcge_hip_mg_galerkin_values_into(f->nrows, f->d_rowptr, f->d_colidx, f->d_val, P->d_colidx, P->rect_ncols, P->d_t_rowptr, P->d_t_colidx,
                                                      scale, c->d_rowptr, c->d_colidx, work, &g_mr_stats[3]);
  if (rc == 0) rc = gcge_hip_mat_update_values_device(c, c->nnz, work) != 0;
  gcge_hip_mat_update_stats(u1);
  g_mr_stats[3] += u1[5] - u0[5];
  gcge_hip_pool_free(work, bytes);
  if (rc == 0) g_mr_stats[2] += 1;
  return rc;
}
static const MgHold* mr_hold(void** A_array) {
  for (const MgHold& k : g_mg) if (k.A_array == A_array) return &k;
  return nullptr;
}
// what a refresh decides from the handles alone, before anything is written: 0 go on, -1 (GCGE_BACKEND.multigrid_refresh_check)
extern "C" int gcge_hip_multigrid_refresh_check(void** A_array, void** B_array, void** P_array, int num_levels) {
  const MgHold* h = mr_hold(A_array);
  if (h == nullptr || A_array == nullptr || P_array == nullptr || num_levels != h->num_levels) return -1;
  if (h->slab && num_levels > 1 && ((int)h->colagg.size() != num_levels - 1 || (int)h->nlo.size() != num_levels - 1)) return -1;
  const bool withB = !h->slab && B_array != nullptr && B_array[0] != nullptr;
  for (int l = 0; l < num_levels; ++l) {
    const GCGE_HIP_MAT_* a = (const GCGE_HIP_MAT_*)A_array[l];
    if (!mr_level_ok(a, l) || (withB && !mr_level_ok((const GCGE_HIP_MAT_*)B_array[l], l))) return -1;
    if (!h->slab && (a->nghost != 0 || a->row_begin != 0)) return -1;       // (a level with halo columns outside a slab hierarchy: no colagg)
    if (withB && ((const GCGE_HIP_MAT_*)B_array[l])->nrows != a->nrows) return -1;
    if (l == 0) continue;
    const GCGE_HIP_MAT_* P = (const GCGE_HIP_MAT_*)P_array[l - 1];
    if (P == nullptr || !P->rect_one_per_row || P->d_t_rowptr == nullptr || P->nrows != ((const GCGE_HIP_MAT_*)A_array[l - 1])->nrows ||
        P->rect_ncols != a->nrows) return -1;
  }
  return 0;
}
extern "C" int gcge_hip_multigrid_refresh(void** A_array, void** B_array, void** P_array, int num_levels) {
  if (gcge_hip_multigrid_refresh_check(A_array, B_array, P_array, num_levels) != 0) return -1;
  const MgHold* h = mr_hold(A_array);
  const bool withB = !h->slab && B_array != nullptr && B_array[0] != nullptr;
  GCGE_HIP_CHECK(hipStreamSynchronize((hipStream_t)gcge_hip_stream()));
  for (int l = 0; l + 1 < num_levels; ++l) {
    const GCGE_HIP_MAT_* P = (const GCGE_HIP_MAT_*)P_array[l];
    if (mr_level(h, A_array, l, P, h->scale) != 0 || (withB && mr_level(h, B_array, l, P, 1.0) != 0)) { g_mr_stats[1] += 1; return l + 1; }
  }
  g_mr_stats[0] += 1;
  return 0;
}
