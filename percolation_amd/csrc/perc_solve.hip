// perc_solve.hip -- the conductance solve of libperc (gfx950): lattice and
// matrix buffers, the solver-format choice, and the fused Jacobi-PCG that
// follows linbcg's operation order (Square/bondc.f:750-838): the register
// march (default), the resident cooperative solve, the one-workgroup solve,
// the literal dot order; plus the SpMV and roofline probes.  All
// floating-point elementwise work is written out in the reference's order
// and compiled with -ffp-contract=off, so every per-row value is bitwise what
// bondc.f computes; only the global dot products are re-associated
// (deterministically: fixed grid, fixed tree), unless the literal dot order
// is asked for.
#include "perc_march.h"
#include "perc_resident.h"

#include <cstring>

namespace perc {
namespace {

// ---------------------------------------------------------------------------
// Lattice build
__global__ void k_forward_count(Geom g, int* fc /* t+2 */) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s > g.t + 1) return;
  fc[s] = (s >= 1 && s <= g.t - 1) ? forward_count(g, (int)s) : 0;
}

__global__ void k_row_count(Geom g, int N, int* rc /* N+1 */) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > N) return;
  if (i == N) { rc[N] = 0; return; }
  const int s = i + g.m + 1;
  int nbr[6];
  const int c = sorted_neighbours(g, s, nbr);
  int cnt = 0;
  for (int j = 0; j < c; ++j) cnt += (nbr[j] > g.m && nbr[j] <= g.t - g.m);
  rc[i] = cnt;
}

__global__ void k_fill_col(Geom g, int N, const int* rowptr, int* col) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int s = i + g.m + 1;
  int nbr[6];
  const int c = sorted_neighbours(g, s, nbr);
  int k = rowptr[i];
  for (int j = 0; j < c; ++j)
    if (nbr[j] > g.m && nbr[j] <= g.t - g.m) col[k++] = nbr[j] - g.m - 1;
}


// Kernel-timing events: no system-scope fence when they are recorded (the
// hipEventDisableSystemFence contract: elapsed times only, read after a
// stream synchronize).  With the default fence the launches that carry the
// start / stop events pay an L2 write-back + invalidate the other launches
// do not, and read ~1 % above rocprofv3's durations of the same kernels
// (profiles/r3_8_*, r3_9_ab_event_fence_L4096.log).
hipError_t timing_event_create(hipEvent_t* ev) {
  return hipEventCreateWithFlags(ev, hipEventDisableSystemFence);
}

// launch a CG kernel; when kernel timing armed h->ev_next, the launch
// records them at the kernel's own start and end (hipExtLaunchKernel: the
// dispatch packet's timestamps, no separate event packets around it)
template <typename K>
void klaunch(perc_ctx* h, K kern, dim3 g, dim3 b, hipStream_t st, const CGArgs& a) {
  if (h->ev_next[0]) {
    hipExtLaunchKernelGGL(kern, g, b, 0, st, h->ev_next[0], h->ev_next[1], 0, a);
    h->ev_next[0] = h->ev_next[1] = nullptr;
  } else {
    kern<<<g, b, 0, st>>>(a);
  }
}

// every k_cg_march this library compiles (the list: perc_march.h)
constexpr MarchVariant kMarchTable[] = {PERC_MARCH_VARIANTS(PERC_MARCH_ROW)};
constexpr MarchKey kMarchOcc = {PERC_MARCH_OCC};

MarchKernel find_march(const MarchKey& k) {
  for (const MarchVariant& v : kMarchTable)
    if (v.key == k) return v.fn;
  return nullptr;
}

// (the open-square path of the strip-major nibble kernels: not in a slab solve)
bool march_open(const CGArgs& a) { return a.sm && a.nib != nullptr && !a.T.pbc && !a.slab; }

// launch the selected march kernel on its grid (the slot-weighted bands' or
// the static split's).  A key the table lacks is a programming error: it is
// reported, never launched as another variant.
hipError_t launch_march(perc_ctx* h, int mode, hipStream_t st, const CGArgs& a) {
  const MarchSel sel = {h->plan.qfree, a.sm != 0,          a.lit != nullptr, a.nib != nullptr, a.mgran != nullptr,
                        a.mtrace != nullptr, a.mes != 0, a.rm_pnib != 0,   march_open(a)};
  const MarchKey k = select_march(mode, sel);
  const MarchKernel fn = find_march(k);
  if (!fn) {
    fprintf(stderr, "[perc] march variant {%d, %d, %d, %d, %d, %d, %d, %d, %d, %d} is not compiled\n", k.mode, k.sm,
            k.d, k.paux, k.tr, k.tag, k.pk, k.lit, k.esr, k.open);
    return hipErrorInvalidConfiguration;
  }
  klaunch(h, fn, k.sm && a.wslots > 0 ? h->wm_grid : h->march_grid, 64 * kMarchWaves, st, a);
  return hipSuccess;
}

// S(k), or the fused P(k)+S(k) of the tiled stencil kernel
hipError_t launch_cg_spmv(perc_ctx* h, const CGArgs& a, int G) {
  if (h->plan.fused) {
    const int th = h->tile_h;
    const dim3 G2(h->tile_grid), B2(tile_threads(th));
    hipStream_t st = h->stream;
    if (h->plan.march) return launch_march(h, kMarchP, st, a);
    if (h->g.scn == 4) {
      if (th == 32) klaunch(h, k_cg_ps<4, true, 32>, G2, B2, st, a);
      else if (th == 16) klaunch(h, k_cg_ps<4, true, 16>, G2, B2, st, a);
      else klaunch(h, k_cg_ps<4, true, 8>, G2, B2, st, a);
    } else {
      if (th == 32) klaunch(h, k_cg_ps<6, true, 32>, G2, B2, st, a);
      else if (th == 16) klaunch(h, k_cg_ps<6, true, 16>, G2, B2, st, a);
      else klaunch(h, k_cg_ps<6, true, 8>, G2, B2, st, a);
    }
  } else if (!h->plan.stencil) {
    // CSR: one row per thread (k_spmv's row) and the q.p partials
    const int ns = csr_slots(a.A.maxrow), GR = h->row_grid;
    if (ns == 4 && a.A.ecol) klaunch(h, k_cg_spmv_row<-1>, GR, kBlock, h->stream, a);
    else if (ns == 4) klaunch(h, k_cg_spmv_row<4>, GR, kBlock, h->stream, a);
    else if (ns == kMaxNnzRow) klaunch(h, k_cg_spmv_row<kMaxNnzRow>, GR, kBlock, h->stream, a);
    else klaunch(h, k_cg_spmv_row<0>, GR, kBlock, h->stream, a);
  }
  else if (h->g.scn == 4) klaunch(h, k_cg_spmv<4>, G, kBlock, h->stream, a);
  else klaunch(h, k_cg_spmv<6>, G, kBlock, h->stream, a);
  return hipSuccess;
}

// B(k) (streaming; the fused format walks its chunks in reverse)
hipError_t launch_cg_b(perc_ctx* h, const CGArgs& a, int G) {
  // fused formats: b_grid (set with the lattice, see dev_build_lattice)
  if (h->plan.fused && h->b_grid > 0) G = h->b_grid;
  if (h->plan.march && h->plan.qfree) {
    return launch_march(h, kMarchB, h->stream, a);
  } else if (h->plan.stencil) {
    // x on every row with the march's x-in-B (fused, row-major): XF
    if (a.bx && a.xrows == 0 && !a.sm) klaunch(h, k_cg_b<true, true>, G, kBlock, h->stream, a);
    else klaunch(h, k_cg_b<true>, G, kBlock, h->stream, a);
  } else {
    klaunch(h, k_cg_b<false>, G, kBlock, h->stream, a);
  }
  return hipSuccess;
}

void launch_spmv(perc_ctx* h, const CGArgs& a, const double* x, double* y) {
  if (!h->plan.stencil) spmv_launch(h, a.A, x, y, h->stream);
  else if (h->g.scn == 4) k_spmv_st<4><<<h->grid, kBlock, 0, h->stream>>>(a.St, x, y);
  else k_spmv_st<6><<<h->grid, kBlock, 0, h->stream>>>(a.St, x, y);
}

// The nibble-code march kernels build the interior form's four terms from
// kSqRasterMask at compile time (march_step): nibble codes only where that
// form (bits 11.. of the interior column class) is regular with exactly this
// mask; any other lattice keeps the u16 codes and their run-time mask.
bool sq_nibble_form(const perc_ctx* h) {
  const int f = h->ncls[0] >> 11;
  return f >= 0 && f < h->forms.nforms && h->forms.regular[f] && h->forms.rmask[f] == kSqRasterMask;
}

// nibble codes (PERC_MARCH_NIBBLE): the u16 row codes packed two sites per
// byte into d.nib_sm, strip-major (SM) or row-major; a takes them where every
// row's upper code bits are its column class's (h->nib_used), else it keeps
// the u16 codes
template <bool SM>
hipError_t pack_nibbles(perc_ctx* h, CGArgs& a) {
  DeviceBuffers& d = h->d;
  hipStream_t st = h->stream;
  const long long n = (long long)a.T.nrows * a.T.m;
  if (!d.nib_sm) HIP_TRY(dmalloc(&d.nib_sm, (size_t)h->N / 2 + 16));
  HIP_TRY(hipMemsetAsync(d.sflag + 3, 0, sizeof(int), st));
  k_pack_nib<SM><<<blocks_for(n / 2), kBlock, 0, st>>>(a.T, d.code, d.nib_sm, h->ncls[0], h->ncls[1], h->ncls[2],
                                                       d.sflag + 3);
  HIP_TRY(dbg_sync(st, "k_pack_nib"));
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, d.sflag + 3, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (!bad) {
    a.nib = d.nib_sm;
    for (int c = 0; c < 3; ++c) a.ncls[c] = h->ncls[c];
  }
  h->nib_used = !bad;
  return hipSuccess;
}

// edge {p, z} pairs per strip side and row (the march P's halo columns; its B
// stores them), the first P's from r0 in a's layout
hipError_t init_edges(perc_ctx* h, CGArgs& a) {
  const long long ne = 2ll * (a.T.m / kMarchW) * a.T.nrows;
  if (!h->d.ez) HIP_TRY(dmalloc(&h->d.ez, 2 * (size_t)ne + 8));
  a.ez = h->d.ez;
  k_edge_init<<<blocks_for(ne), kBlock, 0, h->stream>>>(a);
  return dbg_sync(h->stream, "k_edge_init");
}

// the row-major march's nibble codes (vectors past the Infinity Cache, the
// open square lattice, PERC_MARCH_NIBBLE): 0.5 instead of 2 bytes of row
// code per element in P and B (24.5 + 48m / N instead of 26 B per row; B
// 0.297 vs 0.304 ms at L = 8192); a row whose upper code bits are not its
// column class's keeps the u16 codes.  (pbc lattices keep the u16 codes: the
// row-major nibble kernels compile the open-square path only)
hipError_t to_nib_rows(perc_ctx* h, CGArgs& a) {
  h->nib_used = false;
  a.rm_pnib = h->knobs.rm_pu16 ? 0 : 1;
  if (!h->nib_ok || !sq_nibble_form(h) || h->g.pbc || !(h->march_mode & PERC_MARCH_NIBBLE) ||
      !h->plan.march || !h->plan.qfree || a.sm)
    return hipSuccess;
  HIP_TRY(pack_nibbles<false>(h, a));
  if (h->nib_used) {
    // the row-major nibble march's P takes its halo columns from the edge
    // {p, z} pairs its B stores (as the strip-major march)
    HIP_TRY(init_edges(h, a));
    a.mes = a.T.bh <= kEdgeRowsRm && !h->knobs.edge_step ? 1 : 0;  // (B's bands: march_h rows)
  }
  return hipSuccess;
}

// tagged-granule reductions of the strip-major q-free march (a.sm): a P and
// a B region, each sized for the largest grid either kernel runs; a new
// solve epoch, so no granule of an earlier solve carries a valid tag
hipError_t setup_granules(perc_ctx* h, CGArgs& a, int itmax) {
  if (!h->plan.march_tag || !a.sm || itmax > kTagMaxIter) return hipSuccess;
  const int GM = std::max(red_grid(h), h->wm_grid);
  const size_t region = (size_t)2 * 2 * ((size_t)GM + red_groups(GM));  // NV <= 2, 16-B granules
  const size_t need = 2 * region;
  if (h->d.mgran_n < need) {
    if (h->d.mgran) HIP_TRY(hipFree(h->d.mgran));
    h->d.mgran = nullptr;
    HIP_TRY(dmalloc(&h->d.mgran, need));
    HIP_TRY(hipMemsetAsync(h->d.mgran, 0, need * sizeof(double), h->stream));  // tag 0: never a launch's
    h->d.mgran_n = need;
  }
  a.mgran = h->d.mgran;
  a.mgran_b = h->d.mgran + region;
  a.merr = &h->d.scal->pad[1];
  ++h->solve_epoch;
  return hipSuccess;
}

}  // namespace

// ===========================================================================
hipError_t dev_build_lattice(perc_ctx* h) {
  const Geom& g = h->g;
  const int t = g.t, N = h->N;
  hipStream_t st = h->stream;
  DeviceBuffers& d = h->d;
  // bond_first
  DevBuf<int> fc, rc;
  HIP_TRY(fc.alloc(t + 2));
  HIP_TRY(dmalloc(&d.bond_first, t + 2));
  k_forward_count<<<blocks_for(t + 2), kBlock, 0, st>>>(g, fc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(exclusive_scan(fc, d.bond_first, t + 2, st));
  fc.reset();
  h->h_bond_first.resize(t + 2);
  HIP_TRY(hipMemcpy(h->h_bond_first.data(), d.bond_first, sizeof(int) * (t + 2),
                    hipMemcpyDeviceToHost));
  h->bf_closed = g.lattice == kSquare && g.n >= 2;
  for (int r = 0; r + 2 <= g.n && h->bf_closed; ++r)
    for (int c = 0; c < g.m; ++c)
      if (h->h_bond_first[(size_t)r * g.m + c + 1] != bf_square(g, r, c)) {
        h->bf_closed = false;
        break;
      }
  // the open lattice's top row too (bf_open_square: the labeling wave tiles)
  h->bf_open_sq = h->bf_closed && !g.pbc;
  for (int c = 0; c + 1 < g.m && h->bf_open_sq; ++c)
    if (h->h_bond_first[(size_t)(g.n - 1) * g.m + c + 1] != (g.n - 1) * (2 * g.m - 1) + c) h->bf_open_sq = false;
  // CSR pattern of the interior block
  HIP_TRY(rc.alloc(N + 1));
  HIP_TRY(dmalloc(&d.rowptr, N + 1));
  k_row_count<<<blocks_for(N + 1), kBlock, 0, st>>>(g, N, rc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(exclusive_scan(rc, d.rowptr, N + 1, st));
  rc.reset();
  int nnz = 0;
  HIP_TRY(hipMemcpy(&nnz, d.rowptr + N, sizeof(int), hipMemcpyDeviceToHost));
  h->nnz = nnz;
  // a lattice row has at most scn off-diagonals (square 4, triangular 6):
  // the CSR kernels' entry slots per row (k_spmv<4> / k_cg_spmv_row<4> on
  // the square lattice; the default 6 loaded two dead slots per row there)
  h->csr_maxrow = g.scn;
  HIP_TRY(dmalloc(&d.col, (size_t)nnz + 8));
  HIP_TRY(dmalloc(&d.val, (size_t)nnz + 8));
  k_fill_col<<<blocks_for(N), kBlock, 0, st>>>(g, N, d.rowptr, d.col);
  HIP_TRY(hipGetLastError());
  HIP_TRY(dmalloc(&d.diag, N + 2));
  HIP_TRY(dmalloc(&d.rhs, N + 2));
  HIP_TRY(dmalloc(&d.dtab, kDiagTab));  // double2 entries
  h->forms = stencil_forms(g);
  HIP_TRY(dmalloc(&d.forms_dev, 1));
  HIP_TRY(hipMemcpy(d.forms_dev, &h->forms, sizeof(StencilForms), hipMemcpyHostToDevice));
  HIP_TRY(dmalloc(&d.sflag, 4));
  // occupancy + labeling
  HIP_TRY(dmalloc(&d.bocc, (size_t)h->nb + 8));
  HIP_TRY(dmalloc(&d.socc, t + 8));
  HIP_TRY(dmalloc(&d.order, (size_t)std::max<long long>(h->nb, t) + 8));
  HIP_TRY(dmalloc(&d.parent, t + 8));
  HIP_TRY(dmalloc(&d.member, t + 8));
  HIP_TRY(dmalloc(&d.top, t + 8));
  HIP_TRY(dmalloc(&d.counters, 8 + kMaxSpanList));
  // CG vectors (padded to even length for the 16 B paths) and the row codes.
  // One hipMalloc per array: a single arena with the arrays at staggered
  // offsets (0 / 256 B .. 64 KB per array) measured no better (march P+S
  // 0.104-0.117 ms either way, profiles/r2_4_march_depth.log)
  {
    const size_t nv = (size_t)N + 2;
    HIP_TRY(dmalloc(&d.r, nv));
    HIP_TRY(dmalloc(&d.p0, nv));
    HIP_TRY(dmalloc(&d.p1, nv));
    HIP_TRY(dmalloc(&d.q, nv));
    HIP_TRY(dmalloc(&d.x, nv));
    HIP_TRY(dmalloc(&d.code, (size_t)N + 8));
  }
  h->grid = cg_grid(N);
  h->row_grid = cdiv(N, kBlock);
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess)
    cus = 0;
  h->tile_h = kTileHMax;
  while (h->tile_h > 8 && cdiv(std::max(g.n - 2, 0), h->tile_h) * cdiv(g.m, kTileW) < kMinTiles)
    h->tile_h /= 2;
  h->tile_grid = cdiv(std::max(g.n - 2, 0), h->tile_h) * cdiv(g.m, kTileW);
  // register-march kernel (full 128-column strips): reduction buffers for
  // its largest grid (band height 1)
  h->march_grid_max = g.m % kMarchW == 0 && g.n > 2 ? march_grid_for(g.m / kMarchW, g.n - 2, 1) : 0;
  march_geometry(h);
  res_geometry(h);
  // grid of the streaming B in the fused formats.  Vectors that fit the
  // 256 MB Infinity Cache (L <= 4096): two long-lived workgroups per CU
  // (L = 4096: 0.063 vs 0.069 ms for 8192 short ones; 256 .. 2048 long
  // ones 0.069-0.079).  Larger vectors: short workgroups of 2 pairs per
  // thread, dispatched in address order, so the accesses in flight stay
  // in a narrow window of the arrays (L = 8192: 0.312 ms vs 0.361 with
  // 512, 0.334 with 16384); the partials buffer bounds the grid
  if ((size_t)N * sizeof(double) > kLargeVector)
    h->b_grid = std::min<long long>(cdiv((long long)N, 4ll * kBlock), red_grid(h));
  else
    h->b_grid = std::min(2 * cus, h->grid);
  if (h->res_G > 0) {
    HIP_TRY(dmalloc(&d.res_xch, (size_t)2 * h->res_G * 2 * 2 * g.m));
    HIP_TRY(dmalloc(&d.res_bar, 9 * kTicketStride));
    HIP_TRY(dmalloc(&d.res_gran, (size_t)2 * (3 * h->res_G + kResLitGran)));
    HIP_TRY(dmalloc(&d.res_reg, 9 * kTicketStride));
    HIP_TRY(dmalloc(&d.res_xg, kResXgDoubles));
  }
  HIP_TRY(dmalloc(&d.partials, kRedSlots * red_partials_size(red_grid(h))));
  HIP_TRY(dmalloc(&d.tickets, kRedSlots * red_tickets_size(red_grid(h))));
  HIP_TRY(hipMemset(d.tickets, 0, kRedSlots * red_tickets_size(red_grid(h)) * sizeof(unsigned)));
  HIP_TRY(dmalloc(&d.scal, 1));
  HIP_TRY(dmalloc(&d.iout, 2 * (size_t)g.m));
  HIP_TRY(hipMemset(d.bocc, 0, (size_t)h->nb + 8));
  HIP_TRY(hipMemset(d.socc, 0, t + 8));
  return hipStreamSynchronize(st);
}

hipError_t dev_alloc_matrix(perc_ctx* h, int N, long long nnz) {
  DeviceBuffers& d = h->d;
  h->N = N;
  h->nnz = nnz;
  HIP_TRY(dmalloc(&d.rowptr, N + 1));
  HIP_TRY(dmalloc(&d.col, (size_t)nnz + 8));
  HIP_TRY(dmalloc(&d.val, (size_t)nnz + 8));
  HIP_TRY(dmalloc(&d.diag, N + 2));
  HIP_TRY(dmalloc(&d.rhs, N + 2));
  const size_t nv = (size_t)N + 2;
  HIP_TRY(dmalloc(&d.x, nv));
  HIP_TRY(dmalloc(&d.r, nv));
  HIP_TRY(dmalloc(&d.p0, nv));
  HIP_TRY(dmalloc(&d.p1, nv));
  HIP_TRY(dmalloc(&d.q, nv));
  h->grid = cg_grid(N);
  h->row_grid = cdiv(N, kBlock);
  h->tile_grid = 0;
  h->march_grid = h->march_grid_max = 0;
  HIP_TRY(dmalloc(&d.partials, kRedSlots * red_partials_size(red_grid(h))));
  HIP_TRY(dmalloc(&d.tickets, kRedSlots * red_tickets_size(red_grid(h))));
  HIP_TRY(hipMemset(d.tickets, 0, kRedSlots * red_tickets_size(red_grid(h)) * sizeof(unsigned)));
  HIP_TRY(dmalloc(&d.scal, 1));
  return hipSuccess;
}

void dev_free_all(perc_ctx* h) {
  DeviceBuffers& d = h->d;
  void* ptrs[] = {d.bond_first, d.rowptr, d.col, d.val, d.diag, d.rhs, d.code, d.dtab, d.sflag, d.bocc, d.socc,
                  d.order, d.parent, d.member, d.top, d.counters, d.x, d.r,
                  d.p0, d.p1, d.q, d.partials, d.tickets, d.scal, d.err_hist, d.iout,
                  d.res_xch, d.res_bar, d.bw, d.code_sm, d.csize, d.res_gran, (void*)d.nib_sm,
                  d.sel_hist, d.sel_cand, d.mgran, d.forms_dev, d.lit, d.ccpart, d.ell_col, d.ell_val,
                  d.ell_cnt, d.res_reg, d.res_xg, d.ez};
  for (void* p : ptrs)
    if (p) hipFree(p);
  d = DeviceBuffers{};
  h->N = 0;
  h->nnz = 0;
}

// CUs of the device, and the workgroups a CU holds of the kernel that sizes
// the bands (PERC_MARCH_OCC)
void march_occupancy(const perc_ctx* h, int* cus, int* per_cu) {
  hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, h->device);
  hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, find_march(kMarchOcc), 64 * kMarchWaves, 0);
}

// band height and grid of the register-march kernel, and the slot-weighted
// bands where the device allows them (the policy: perc_solve_plan.h)
void march_geometry(perc_ctx* h) {
  const Geom& g = h->g;
  h->march_grid = 0;
  h->wm_slots = 0;
  h->wm_grid = 0;
  if (g.m % kMarchW != 0 || g.n <= 2) return;
  const int nrows = g.n - 2;
  int cus = 0, per_cu = 0;
  march_occupancy(h, &cus, &per_cu);
  h->march_h = march_rows_for(g.m, nrows, cus, per_cu, h->march_mode, h->march_rows_req);
  h->march_grid = march_grid_for(g.m / kMarchW, nrows, h->march_h);
  const SlotGeometry s = slot_geometry(g.m, nrows, cus, per_cu, h->slot_w_set ? h->slot_w : kSlotW);
  h->wm_slots = s.slots;
  h->wm_grid = s.grid;
  std::memcpy(h->wm_cum, s.cum, sizeof(s.cum));
}

// resident solve: m a multiple of 1024 (MT = m / 1024 columns per thread
// and row), or m < 1024 with m threads per workgroup rounded up to whole
// waves (one column each: mid-size lattices, whose launched kernels are
// latency-bound), the
// band height H of ceil(nrows / CUs) rows within the LDS and register
// budget, one workgroup per CU
void res_geometry(perc_ctx* h) {
  const Geom& g = h->g;
  h->res_G = 0;
  h->res_uneven = false;
  const bool narrow = g.m < kResThreads;
  if ((g.m % kResThreads != 0 && !narrow) || g.n <= 2) return;
  int cus = 0, coop = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess ||
      hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, h->device) != hipSuccess ||
      !coop || cus <= 0)
    return;
  h->res_NT = narrow ? (g.m + 63) / 64 * 64 : kResThreads;  // whole waves
  const int nrows = g.n - 2, MT = narrow ? 1 : g.m / kResThreads;
  const int H = cdiv(nrows, cus);
  // m = 1024: at most 4 rows per CU (r, q, code of 4 elements per thread
  // in registers, 97 VGPRs); m = 2048: at most 8 rows per CU, q formed
  // twice instead of kept (16 elements per thread: r and code only)
  if (!((MT == 1 && H <= 4) || (MT == 2 && H <= 8)) || (long long)H * g.m > kResLdsRows) return;
  for (int f = 0; f < h->forms.nforms; ++f)
    if (!h->forms.regular[f]) return;  // wrapped columns (pbc): slot order is not raster order
  h->res_MT = MT;
  h->res_H = H;
  h->res_G = cdiv(nrows, H);
}

// solver kernels for the requested format and what the assembly allows
void select_format(perc_ctx* h) {
  const SolveRequest req = {h->fmt_req, h->march_mode, h->dot_order, h->march_rows_req};
  const SolveFacts facts = {h->N,     h->stencil_ok, h->tiled_ok,           h->march_ok,
                            h->res_G, h->wm_slots,   h->d.rowptr != nullptr};
  h->plan = solve_plan(req, facts);
}

// strip-major copies of r (into the q buffer: r and q swap roles for the
// solve) and of the row codes; a switches to them
hipError_t to_strips(perc_ctx* h, CGArgs& a) {
  DeviceBuffers& d = h->d;
  hipStream_t st = h->stream;
  if (!d.code_sm) HIP_TRY(dmalloc(&d.code_sm, (size_t)h->N + 8));
  const long long n = (long long)a.T.nrows * a.T.m;
  k_to_strips<uint16_t><<<blocks_for(n), kBlock, 0, st>>>(a.T, d.code, d.code_sm);
  k_to_strips<double><<<blocks_for(n), kBlock, 0, st>>>(a.T, d.r, d.q);
  HIP_TRY(dbg_sync(st, "k_to_strips"));
  a.r = d.q;
  a.q = d.r;
  a.St.code = d.code_sm;
  a.sm = 1;
  a.bx = 1;  // x (row-major) is updated in the q-free march B
  HIP_TRY(init_edges(h, a));  // (from the strip-major r and codes: a.sm set)
  // nibble codes (PERC_MARCH_NIBBLE, square lattice): 0.5 instead of 2
  // bytes of row code per element in both march kernels
  h->nib_used = false;
  if (h->nib_ok && sq_nibble_form(h) && (h->march_mode & PERC_MARCH_NIBBLE)) HIP_TRY(pack_nibbles<true>(h, a));
  if (h->plan.march_slots) {
    a.wslots = h->wm_slots;
    for (int i = 0; i <= h->wm_slots; ++i) {
      a.wcum[0][i] = h->wm_cum[0][i];
      a.wcum[1][i] = h->wm_cum[1][i];
    }
  }
  // B stages its edge pairs in LDS where every band of B holds <= kEdgeRows
  // rows (the bands as k_cg_march forms them, perc_bands.h: the staging has
  // no other bound; MarchKnobs::edge_step: the per-step stores)
  const int ns = a.wslots;
  const int hmax =
      ns > 0 ? tallest_slot_band(a.T.nrows, h->wm_grid / ns * kMarchWaves / (a.T.m / kMarchW), ns, a.wcum[1]) : a.T.bh;
  a.mes = hmax <= kEdgeRows && !h->knobs.edge_step ? 1 : 0;
  return hipSuccess;
}

// The resident solve's synchronisation floor (perc_bench_kernel 6): the
// same cooperative grid running only what an iteration of k_cg_res does to
// synchronise -- the two block sums and the two grid-wide reductions
// (res_allreduce_x, or res_gather where the placement falls back) -- on dummy
// values, `iters` times.  The time per iteration is what the resident solve
// cannot go below whatever its memory traffic.
__global__ __launch_bounds__(1024) void k_res_sync_probe(ResArgs a, int iters) {
  __shared__ double s_red[32];
  __shared__ double s_res[8];
  __shared__ int s_flag[2];
  const ResXcd X = res_register(a, s_flag);
  unsigned epoch = 0;
  double v1[1] = {(double)X.w}, tot1[1], acc2[2], tot2[2];
  for (int k = 0; k < iters && s_flag[1]; ++k) {
    double w1[1] = {v1[0] + (double)threadIdx.x};
    if (X.ok) {
      if (!res_allreduce_x<1>(a, epoch, 0, X, w1, tot1, s_red, s_res)) break;
    } else {
      block_sum<1>(w1, s_red);
      if (!res_gather<1>(a, epoch, a.gran, w1, tot1, s_red)) break;
    }
    acc2[0] = tot1[0] * 1e-30 + (double)threadIdx.x;
    acc2[1] = (double)k;
    if (X.ok) {
      if (!res_allreduce_x<2>(a, epoch, 1, X, acc2, tot2, s_red, s_res)) break;
    } else {
      block_sum<2>(acc2, s_red);
      if (!res_gather<2>(a, epoch, a.gran + 2 * (size_t)a.G, acc2, tot2, s_red)) break;
    }
    v1[0] = tot2[0] * 1e-30;
  }
}

// the resident kernel for m = 1024 (MT = 1) / 2048, square-lattice
// positions only (sq) or all eight
// (NT threads per workgroup, m of them for m <= 1024: with one column per
// thread the template's NT is only the launch bound, so widths up to 512
// share the 512-bound instantiation -- 125-142 VGPRs, no spills)
template <bool LIT, bool XG>
const void* res_kernel_t(int MT, bool sq, int NT) {
  if (MT == 1 && NT <= 512)
    return sq ? (const void*)k_cg_res<1, 4, true, kResSquareMask, 512, LIT, XG>
              : (const void*)k_cg_res<1, 4, true, 0xFFu, 512, LIT, XG>;
  if (MT == 1)
    return sq ? (const void*)k_cg_res<1, 4, true, kResSquareMask, kResThreads, LIT, XG>
              : (const void*)k_cg_res<1, 4, true, 0xFFu, kResThreads, LIT, XG>;
  return sq ? (const void*)k_cg_res<2, 8, false, kResSquareMask, kResThreads, LIT, XG>
            : (const void*)k_cg_res<2, 8, false, 0xFFu, kResThreads, LIT, XG>;
}
// (lit: the literal dot order's instantiation, LIT = true, whose reductions
// are serial folds; xg: the fast order's XCD-grouped reductions)
const void* res_kernel(int MT, bool sq, int NT, bool lit, bool xg) {
  if (lit) return res_kernel_t<true, false>(MT, sq, NT);
  return xg && kResXcdGather ? res_kernel_t<false, true>(MT, sq, NT) : res_kernel_t<false, false>(MT, sq, NT);
}

// one cooperative launch runs the whole iteration loop (k_cg_res)
hipError_t dev_solve_resident(perc_ctx* h, const CGArgs& ca, int* iter, double* err) {
  DeviceBuffers& d = h->d;
  hipStream_t st = h->stream;
  ResArgs a;
  a.St = ca.St;
  a.m = h->g.m;
  a.nrows = h->g.n - 2;
  a.pbc = h->g.pbc;
  a.G = h->res_G;
  a.H = h->res_H;
  a.xrows = ca.xrows;
  a.r0 = d.r;
  a.x = d.x;
  a.S = d.scal;
  a.err_hist = d.err_hist;
  a.err_hist_cap = d.err_hist_cap;
  a.xch = d.res_xch;
  a.bar = d.res_bar;
  a.gran = d.res_gran;
  a.lit = ca.lit;
  a.reg = d.res_reg;
  a.xg = d.res_xg;
  HIP_TRY(hipMemsetAsync(d.res_bar, 0, 9 * kTicketStride * sizeof(unsigned), st));
  HIP_TRY(hipMemsetAsync(d.res_reg, 0, 9 * kTicketStride * sizeof(unsigned), st));
  HIP_TRY(hipMemsetAsync(d.res_xg, 0, kResXgDoubles * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(d.res_gran, 0, (size_t)2 * (3 * h->res_G + kResLitGran) * sizeof(double), st));
  void* args[] = {&a};
  // reductions by tagged-granule all-gather (res_gather): L = 1024 15.5 vs
  // 16.6 us per iteration against a counter barrier + partial reads, L =
  // 2048 33.7 vs 34.65 (profiles/r2_10_resident_gather_ab.log)
  const bool sq = (h->forms.umask & ~kResSquareMask) == 0;
  // (PERC_RES_FLAT=1 in the environment: the flat all-gather instantiation,
  // for tests of that fallback)
  // The grouped reductions need G / 8 workgroups on every XCD: a grid that
  // cannot be placed so (G % 8 != 0, or more than kResXcdMax per XCD) takes
  // the flat instantiation from the host, and so does a context whose grouped
  // launch once found the placement uneven (h->res_uneven, reset with the
  // lattice), instead of paying a cooperative launch that leaves at once
  const bool xg = !h->knobs.res_flat && a.G % 8 == 0 && a.G / 8 <= kResXcdMax && !h->res_uneven;
  const void* fn = res_kernel(h->res_MT, sq, h->res_NT, a.lit != nullptr, xg);
  KernelTiming& T = h->timing;
  if (T.enabled) {
    if (T.ev.size() < 2) T.ev.resize(2, nullptr);
    for (int i = 0; i < 2; ++i)
      if (!T.ev[i]) HIP_TRY(timing_event_create(&T.ev[i]));
    HIP_TRY(hipEventRecord(T.ev[0], st));
  }
  HIP_TRY(hipLaunchCooperativeKernel(fn, dim3(a.G), dim3(h->res_NT), args, 0, st));
  HIP_TRY(dbg_sync(st, "k_cg_res"));
  if (T.enabled) HIP_TRY(hipEventRecord(T.ev[1], st));
  CGScalars hs{};
  HIP_TRY(hipMemcpyAsync(&hs, d.scal, sizeof(hs), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  bool grouped = xg && a.lit == nullptr && kResXcdGather;
  if (hs.pad[kResPadUneven] != 0) {
    // the grouped launch found the workgroups spread unevenly over the XCDs
    // and left at once (no state touched): the flat all-gather instantiation
    // runs the solve.  Its flag words are cleared first -- pad[1] is also the
    // tagged march's error word -- and the context remembers the placement
    h->res_uneven = true;
    grouped = false;
    HIP_TRY(hipMemsetAsync(d.scal->pad, 0, 2 * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(d.res_bar, 0, 9 * kTicketStride * sizeof(unsigned), st));
    fn = res_kernel(h->res_MT, sq, h->res_NT, a.lit != nullptr, false);
    HIP_TRY(hipLaunchCooperativeKernel(fn, dim3(a.G), dim3(h->res_NT), args, 0, st));
    HIP_TRY(dbg_sync(st, "k_cg_res"));
    if (T.enabled) HIP_TRY(hipEventRecord(T.ev[1], st));
    HIP_TRY(hipMemcpyAsync(&hs, d.scal, sizeof(hs), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (hs.pad[0] != 0) {
    fprintf(stderr, "[perc] k_cg_res: grid barrier timed out\n");
    return hipErrorLaunchTimeOut;
  }
  if (grouped) h->last_flags |= PERC_RAN_XCD_GROUPED;
  if (T.enabled && hs.iter > 0) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, T.ev[0], T.ev[1]));
    T.spmv_ms += ms;  // whole iterations: P+S and B together
    T.spmv_n += hs.iter;
  }
  *iter = hs.iter;
  *err = hs.err;
  return hipSuccess;
}


namespace {
hipError_t dev_solve_impl(perc_ctx* h, int itol, double tol, int itmax, bool x0_zero, bool full_x,
                          int* iter, double* err);

// the solver's environment knobs (MarchKnobs, perc_internal.h): every value
// from the environment as it is now, but time_every, which a process reads once
MarchKnobs read_march_knobs() {
  auto num = [](const char* name, int unset) {
    const char* v = std::getenv(name);
    return v ? std::atoi(v) : unset;
  };
  auto flag = [](const char* name) {
    const char* v = std::getenv(name);
    return v && v[0] == '1';
  };
  static const int time_every = num("PERC_TIME_EVERY", 0);
  MarchKnobs k;
  k.rm_pu16 = flag("PERC_MARCH_RM_PU16");
  k.edge_step = flag("PERC_MARCH_EDGE_STEP");
  k.xafter = flag("PERC_MARCH_XAFTER");
  k.res_flat = flag("PERC_RES_FLAT");
  if (const char* v = std::getenv("PERC_MARCH_FRONT")) k.front = v[0] != '0';
  if (time_every > 0) k.time_every = time_every;  // (else the default)
  k.trace = std::getenv("PERC_MARCH_TRACE");
  k.trace_it = num("PERC_MARCH_TRACE_IT", 1000);
  return k;
}

// What a march solve needs before its first launch: the layout (strip-major
// copies, or the row-major march's nibble codes), the tagged granules, how x
// is carried, and what perc_last_solve reports.  probe: perc_bench_kernel's
// steady-state launches of the same kernels (no solve: last_flags stays).
hipError_t prepare_march(perc_ctx* h, CGArgs& a, int itmax, bool probe) {
  if (h->plan.strips) HIP_TRY(to_strips(h, a));
  else HIP_TRY(to_nib_rows(h, a));
  HIP_TRY(setup_granules(h, a, itmax));
  // x on the electrode-side rows, each iteration's update applied by the
  // next B at its start (k_cg_march, kXin), the last by k_march_xpend
  // (MarchKnobs::xafter: the update after each B's walk; the probe times the
  // production path whatever the knob)
  a.mxin = a.sm && !a.lit && !a.slab && a.xrows == h->g.m && !(h->knobs.xafter && !probe) ? 1 : 0;
  if (probe) return hipSuccess;
  const bool host_fold = a.lit && h->dot_order == PERC_DOT_LITERAL_HOST;
  h->last_flags = (h->dot_order != PERC_DOT_FAST ? PERC_RAN_LITERAL : 0) | (a.lit ? PERC_RAN_LIT_TERMS : 0) |
                  (h->plan.march && h->plan.qfree ? PERC_RAN_QFREE : 0) | (a.sm ? PERC_RAN_STRIPS : 0) |
                  (a.nib ? PERC_RAN_NIBBLE : 0) | (a.mgran ? PERC_RAN_TAG : 0) |
                  (host_fold ? PERC_RAN_HOST_FOLD : 0) | (h->plan.march && h->plan.qfree && march_open(a) ? PERC_RAN_OPEN : 0);
  return hipSuccess;
}
}  // namespace

hipError_t dev_solve(perc_ctx* h, int itol, double tol, int itmax, bool x0_zero, bool full_x,
                     int* iter, double* err) {
  h->knobs = read_march_knobs();
  h->last_kernel = h->last_flags = h->last_front = 0;
  h->last_iter = -1;
  const hipError_t e = dev_solve_impl(h, itol, tol, itmax, x0_zero, full_x, iter, err);
  if (e == hipSuccess) h->last_iter = *iter;
  return e;
}

namespace {
// PERC_DOT_LITERAL_HOST: k_fold_qp's and k_fold_b's sums and epilogues on the
// host CPU, from the terms the march kernels stored (a.lit): the same IEEE
// adds in the same ascending-j order (host code is compiled with
// -ffp-contract=off and no reassociation), the same divisions and sqrt
// (correctly rounded on both sides), so every scalar is PERC_DOT_LITERAL's
// bitwise.  One host round trip per fold; the serial chain runs at the
// CPU's add latency instead of a GPU wave's (~17 cycles per dependent fp64
// add, tools/fold_bench.hip).
struct HostFold {
  PinnedBuf<double> t;  // 3 N
};
hipError_t host_fold_qp(perc_ctx* h, const CGArgs& a, HostFold& hf) {
  const int N = h->N;
  hipStream_t st = h->stream;
  CGScalars s{};
  HIP_TRY(hipMemcpyAsync(&s, h->d.scal, sizeof(s), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hf.t, a.lit, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (s.done) return hipSuccess;
  const double* __restrict__ t = hf.t.get();
  double acc = 0.0;
  for (int j = 0; j < N; ++j) acc = acc + t[j];  // akden, bondc.f:803-805
  s.akden = acc;
  s.ak = s.bknum / acc;
  s.bkden = s.bknum;
  s.pad[2] = 1;
  HIP_TRY(hipMemcpyAsync(h->d.scal, &s, sizeof(s), hipMemcpyHostToDevice, st));
  return hipStreamSynchronize(st);
}
hipError_t host_fold_b(perc_ctx* h, const CGArgs& a, HostFold& hf) {
  const int N = h->N;
  hipStream_t st = h->stream;
  CGScalars s{};
  HIP_TRY(hipMemcpyAsync(&s, h->d.scal, sizeof(s), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hf.t + N, a.lit + N, sizeof(double) * 2 * (size_t)N, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (s.pad[2] == 0) return hipSuccess;  // no iteration ran since the last fold
  const double* __restrict__ t1 = hf.t + N;
  const double* __restrict__ t2 = hf.t + 2 * (size_t)N;
  double a0 = 0.0, a1 = 0.0;
  for (int j = 0; j < N; ++j) {  // bknum :785-787, snrm :872-875
    a0 = a0 + t1[j];
    a1 = a1 + t2[j];
  }
  const int k = s.iter;
  const double err = std::sqrt(a1) / s.bnrm;
  s.bk = a0 / s.bkden;
  s.bknum = a0;
  s.err = err;
  if (k - 1 < a.err_hist_cap)
    HIP_TRY(hipMemcpyAsync(a.err_hist + (k - 1), &err, sizeof(double), hipMemcpyHostToDevice, st));
  s.done = !(err > s.tol) || k >= s.itmax + 1 ? 1 : 0;
  s.pad[2] = 0;
  HIP_TRY(hipMemcpyAsync(h->d.scal, &s, sizeof(s), hipMemcpyHostToDevice, st));
  return hipStreamSynchronize(st);
}

// linbcg with itol 3 or 4 (bondc.f:771-775, 816-832): the stopping test is
// NR's step-size estimate |z| / |z(k-1) - z| * |ak| |p| / |x| in the L2
// (itol 3) or max (itol 4) norm, so every iteration needs |z|, |p| and |x|
// besides the two dots.  The reference only calls itol 2 (its drivers) and
// this mode is for linbcg_'s other callers: plain row-major kernels on the
// CSR operator, three launches per iteration (p update; q = A p with p.q;
// x, r update with z.r and the three norms), block partials summed on the
// host in block order each iteration -- not the march's single-pass design.
// kX34Grid blocks stride over the rows.
constexpr int kX34Grid = 1024;

template <bool MAXN>
__device__ __forceinline__ double x34_norm(double acc, double v) {
  return MAXN ? fmax(acc, fabs(v)) : acc + v * v;
}
// v[0] summed, v[1..K-1] norm-combined, over the block; thread 0 writes
// out[blockIdx.x * 4 + k]
template <int K, bool MAXN>
__device__ __forceinline__ void x34_block(double (&v)[K], double* out) {
  __shared__ double s[K][kBlock / 64];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double x = v[k];
    for (int o = 32; o > 0; o >>= 1) {
      const double y = __shfl_xor(x, o);
      x = (k == 0 || !MAXN) ? x + y : fmax(x, y);
    }
    if ((threadIdx.x & 63) == 0) s[k][threadIdx.x >> 6] = x;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    double x = s[k][0];
    for (int w = 1; w < kBlock / 64; ++w) x = (k == 0 || !MAXN) ? x + s[k][w] : fmax(x, s[k][w]);
    out[blockIdx.x * 4 + k] = x;
  }
}
__device__ __forceinline__ double x34_row(const CsrView& A, const double* __restrict__ x, int i) {
  double ax = A.diag[i] * x[i];
  for (int j = A.rowptr[i]; j < A.rowptr[i + 1]; ++j) ax = ax + A.val[j] * x[A.col[j]];
  return ax;
}
// r = b - A x; {z.r, |D^-1 b|, |D^-1 r|}
template <bool MAXN>
__global__ __launch_bounds__(kBlock) void k_x34_init(CsrView A, const double* __restrict__ b,
                                                     const double* __restrict__ x,
                                                     double* __restrict__ r, double* out) {
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < A.N; i += gridDim.x * kBlock) {
    const double di = A.diag[i], ri = b[i] - x34_row(A, x, i);
    r[i] = ri;
    v[0] = v[0] + (ri / di) * ri;
    v[1] = x34_norm<MAXN>(v[1], b[i] / di);
    v[2] = x34_norm<MAXN>(v[2], ri / di);
  }
  x34_block<3, MAXN>(v, out);
}
// p = z (first) or bk p + z, z = r / d (bondc.f:789-797)
__global__ __launch_bounds__(kBlock) void k_x34_p(CsrView A, const double* __restrict__ r,
                                                  double* __restrict__ p, double bk, int first) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < A.N; i += gridDim.x * kBlock) {
    const double z = r[i] / A.diag[i];
    p[i] = first ? z : bk * p[i] + z;
  }
}
// q = A p; {p.q} (bondc.f:799-805)
__global__ __launch_bounds__(kBlock) void k_x34_qp(CsrView A, const double* __restrict__ p,
                                                   double* __restrict__ q, double* out) {
  double v[1] = {0.0};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < A.N; i += gridDim.x * kBlock) {
    const double qi = x34_row(A, p, i);
    q[i] = qi;
    v[0] = v[0] + qi * p[i];
  }
  x34_block<1, false>(v, out);
}
// x += ak p, r -= ak q (bondc.f:808-812); {z.r, |z|, |p|, |x|}
template <bool MAXN>
__global__ __launch_bounds__(kBlock) void k_x34_upd(CsrView A, double* __restrict__ x,
                                                    double* __restrict__ r,
                                                    const double* __restrict__ p,
                                                    const double* __restrict__ q, double ak,
                                                    double* out) {
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < A.N; i += gridDim.x * kBlock) {
    const double xi = x[i] + ak * p[i], ri = r[i] - ak * q[i], z = ri / A.diag[i];
    x[i] = xi;
    r[i] = ri;
    v[0] = v[0] + z * ri;
    v[1] = x34_norm<MAXN>(v[1], z);
    v[2] = x34_norm<MAXN>(v[2], p[i]);
    v[3] = x34_norm<MAXN>(v[3], xi);
  }
  x34_block<4, MAXN>(v, out);
}

hipError_t dev_solve_x34(perc_ctx* h, int itol, double tol, int itmax, int* iter, double* err) {
  HIP_TRY(ensure_csr(h));
  if (!h->csr_ok) {
    set_error("linbcg itol 3/4: no CSR copy of the system");
    return hipErrorInvalidValue;
  }
  const int N = h->N;
  const bool MX = itol == 4;
  hipStream_t st = h->stream;
  const CsrView A = make_cg_args(h).A;
  const int G = std::max(1, std::min(kX34Grid, cdiv(N, kBlock)));
  struct {
    DevBuf<double> r, p, q, part;
  } w;
  HIP_TRY(w.r.alloc((size_t)N));
  HIP_TRY(w.p.alloc((size_t)N));
  HIP_TRY(w.q.alloc((size_t)N));
  HIP_TRY(w.part.alloc((size_t)4 * G));
  std::vector<double> part(4 * (size_t)G);
  double sum[4];
  // the literal dot orders (perc_set_dot_order, linbcg_'s default): the
  // vectors come to the host and every sum and norm is formed there in
  // ascending j as bondc.f:785-787, 803-805, 867-884 form them (host code
  // has no contraction or reassociation; the device's elementwise x, r, p,
  // q, z are the reference's expressions, so the iterates are its bitwise)
  const bool lit = h->dot_order != PERC_DOT_FAST;
  std::vector<double> hd, hv[3];
  if (lit) {
    hd.resize(N);
    for (auto& v : hv) v.resize(N);
    HIP_TRY(hipMemcpyAsync(hd.data(), A.diag, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  }
  auto snrm = [&](const double* v, bool div) {  // snrm of v (or of v / d)
    if (!MX) {
      double a = 0.0;
      for (int j = 0; j < N; ++j) {
        const double t = div ? v[j] / hd[j] : v[j];
        a = a + t * t;
      }
      return std::sqrt(a);
    }
    double a = std::fabs(div ? v[0] / hd[0] : v[0]);
    for (int j = 1; j < N; ++j) a = std::max(a, std::fabs(div ? v[j] / hd[j] : v[j]));
    return a;
  };
  auto zdot = [&](const double* r) {  // sum z(j) rr(j), z = r / d
    double a = 0.0;
    for (int j = 0; j < N; ++j) a = a + (r[j] / hd[j]) * r[j];
    return a;
  };
  auto get = [&](int k, const double* dv) {
    return hipMemcpyAsync(hv[k].data(), dv, sizeof(double) * N, hipMemcpyDeviceToHost, st);
  };
  auto fold = [&](int K) -> hipError_t {  // block partials in block order
    HIP_TRY(hipMemcpyAsync(part.data(), w.part, sizeof(double) * 4 * G, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < K; ++k) {
      double v = part[k];
      for (int g = 1; g < G; ++g) v = (k == 0 || !MX) ? v + part[4 * g + k] : std::max(v, part[4 * g + k]);
      sum[k] = (k == 0 || MX) ? v : std::sqrt(v);
    }
    return hipSuccess;
  };
  h->last_kernel = 0;  // (other launched kernels)
  if (MX) k_x34_init<true><<<G, kBlock, 0, st>>>(A, h->d.rhs, h->d.x, w.r, w.part);
  else k_x34_init<false><<<G, kBlock, 0, st>>>(A, h->d.rhs, h->d.x, w.r, w.part);
  HIP_TRY(hipGetLastError());
  HIP_TRY(fold(3));
  if (lit) {  // bondc.f:772-775 and the first bknum
    HIP_TRY(get(0, h->d.rhs));
    HIP_TRY(get(1, w.r));
    HIP_TRY(hipStreamSynchronize(st));
    sum[1] = snrm(hv[0].data(), true);
    sum[2] = snrm(hv[1].data(), true);
    sum[0] = zdot(hv[1].data());
  }
  constexpr double kEps = 1.00e-14;  // bondc.f:753
  double bknum = sum[0], bnrm = sum[1], znrm = sum[2], bkden = 1.0, e = 0.0;
  std::vector<double> hist;
  int k = 0;
  while (k <= itmax) {  // bondc.f:780
    ++k;
    const double zm1nrm = znrm;
    k_x34_p<<<G, kBlock, 0, st>>>(A, w.r, w.p, k == 1 ? 0.0 : bknum / bkden, k == 1);
    bkden = bknum;
    k_x34_qp<<<G, kBlock, 0, st>>>(A, w.p, w.q, w.part);
    HIP_TRY(hipGetLastError());
    HIP_TRY(fold(1));
    if (lit) {
      HIP_TRY(get(0, w.p));
      HIP_TRY(get(1, w.q));
      HIP_TRY(hipStreamSynchronize(st));
      double a = 0.0;
      for (int j = 0; j < N; ++j) a = a + hv[1][j] * hv[0][j];
      sum[0] = a;
    }
    const double ak = bknum / sum[0];
    if (MX) k_x34_upd<true><<<G, kBlock, 0, st>>>(A, h->d.x, w.r, w.p, w.q, ak, w.part);
    else k_x34_upd<false><<<G, kBlock, 0, st>>>(A, h->d.x, w.r, w.p, w.q, ak, w.part);
    HIP_TRY(hipGetLastError());
    HIP_TRY(fold(4));
    if (lit) {  // (hv[0] still holds this iteration's p)
      HIP_TRY(get(1, w.r));
      HIP_TRY(get(2, h->d.x));
      HIP_TRY(hipStreamSynchronize(st));
      sum[0] = zdot(hv[1].data());
      sum[1] = snrm(hv[1].data(), true);
      sum[2] = snrm(hv[0].data(), false);
      sum[3] = snrm(hv[2].data(), false);
    }
    bknum = sum[0];
    znrm = sum[1];
    bool test = false;
    if (std::fabs(zm1nrm - znrm) > kEps * znrm) {
      e = znrm / std::fabs(zm1nrm - znrm) * (std::fabs(ak) * sum[2]);
      if (e <= 0.50 * sum[3]) {
        e = e / sum[3];
        test = true;
      } else {
        e = znrm / bnrm;  // goto 100: no tolerance test this iteration
      }
    } else {
      e = znrm / bnrm;
    }
    hist.push_back(e);
    if (test && !(e > tol)) break;
  }
  if (h->d.err_hist && h->d.err_hist_cap > 0 && !hist.empty())
    HIP_TRY(hipMemcpyAsync(h->d.err_hist, hist.data(),
                           sizeof(double) * std::min<size_t>(hist.size(), h->d.err_hist_cap),
                           hipMemcpyHostToDevice, st));
  CGScalars hs{};  // (perc_err_history reads the count from the scalars)
  hs.iter = k;
  hs.err = e;
  hs.tol = tol;
  hs.itmax = itmax;
  hs.done = 1;
  HIP_TRY(hipMemcpyAsync(h->d.scal, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  *iter = k;
  *err = e;
  return hipSuccess;
}

// The Krylov front of a launched march solve that starts from x0 = 0.
//
// r(0) = b is nonzero on the lattice rows [lo, hi] only (the driven row next
// to the Va electrode; k_cg_init records them, CGScalars::rlo / rhi).  The
// Jacobi preconditioner is diagonal and the operator couples a row to rows
// within `reach` = 1 of it (the forms table's row offsets), so by induction
// over linbcg's recurrences
//   p(1) = z(0)                 is nonzero within 0 rows of [lo, hi],
//   q(k) = A p(k), r(k) = r(k-1) - ak q(k)   within one row more than p(k),
//   p(k+1) = bk p(k) + r(k) / d              within as many rows as r(k):
// p(k) reaches k - 1 rows, q(k), r(k), z(k) and B's edge pairs k rows, and
// the x update B(k) applies (ak(k-1) p(k-1)) k - 2 rows.  Every other row of
// them is an exact zero, and so are its terms of q.p, z.r and r.r: a band
// that misses [lo - k, hi + k] loads zeros, forms zeros and stores zeros in
// launch k, and what it would store is already there -- the first chunk's
// launches walk every band, so both p buffers, r, the edge pairs and the
// literal order's term buffer hold the parent's own zeros on every row the
// front has not reached, and no kernel of the solve writes them again before
// the front arrives.  (Zeros added to x, a partial or a literal fold leave it
// bitwise what it was; a skipped band's own partial is +0.0 either way.)
//
// Launch k gets [lo - (k + 1), hi + (k + 1)], one row more than the bound.
// The row is deliberate: k is the host's count of launches, the device's
// iteration is S->iter + 1, and the two agree only while the solve runs; a
// bound that is tight to the row would turn any slip of one between them (a
// launch re-ordered in a later change, p's reach counted from 1) into wrong
// numbers, where the margin costs one band one iteration early.
//
// On only when x0 = 0, one slab, the launched q-free march, the operator's
// row reach 1 and no phase trace; PERC_MARCH_FRONT=0 turns it off.
struct MarchFront {
  bool on = false;     // the conditions hold
  bool known = false;  // rows [lo, hi] read back and some band still dead
  int lo = 0, hi = -1;
  int last_dead = 0;   // the last iteration launched with a dead band
};

int forms_row_reach(const StencilForms& F) {
  int reach = 0;
  for (int f = 0; f < F.nforms; ++f)
    for (int j = 0; j < F.cnt[f]; ++j) reach = std::max(reach, std::abs(F.dr[f][j]));
  return reach;
}

bool front_allowed(const perc_ctx* h, const CGArgs& a, bool x0_zero) {
  return x0_zero && h->knobs.front && !h->knobs.trace && h->nslab <= 1 && !a.slab && h->plan.stencil && h->plan.march &&
         h->plan.qfree && a.T.m > 0 && a.T.nrows > 0 && (long long)a.T.m * a.T.nrows == h->N &&
         forms_row_reach(h->forms) == 1;
}

// does some band of the march P (which = 0) or B (1) miss a's live rows?  (the
// bands as k_cg_march forms them, perc_bands.h)
bool front_dead_band(const perc_ctx* h, const CGArgs& a, int which) {
  const int nrows = a.T.nrows;
  auto dead = [&](const BandRows& b) { return b.r0 < b.rend && !(b.r0 < a.fhi && b.rend > a.flo); };
  if (a.wslots > 0) {
    const int ns = a.wslots, Q = h->wm_grid / ns * kMarchWaves / (a.T.m / kMarchW);
    for (int q = 0; q < Q; ++q)
      for (int sl = 0; sl < ns; ++sl)
        if (dead(slot_band(nrows, Q, q, ns, sl, a.wcum[which]))) return true;
    return false;
  }
  for (int band = 0; band * a.T.bh < nrows; ++band)
    if (dead(static_band(nrows, a.T.bh, band))) return true;
  return false;
}

// the live rows of launch a.kiter
void front_rows(const perc_ctx* h, MarchFront& F, CGArgs& a) {
  a.flo = kFrontAllLo;
  a.fhi = kFrontAllHi;
  if (!F.known) return;
  const int k = a.kiter, lo = F.lo - (k + 1), hi = F.hi + (k + 1);
  if (lo <= 0 && hi >= a.T.nrows - 1) {  // the front has crossed the lattice
    F.known = false;
    return;
  }
  a.flo = std::max(lo, 0);
  a.fhi = std::min(hi + 1, a.T.nrows);
  if (front_dead_band(h, a, 0) || front_dead_band(h, a, 1)) F.last_dead = k;
}

// Kernel timing of the launch loop: per timed iteration the start / stop
// events of P, S and B, recorded by the kernels' own dispatch packets
// (klaunch).  Every `every`-th iteration of a chunk is sampled: 64 (a timed
// launch's event packets open a dispatch gap of several us: every 8th
// iteration timed cost ~1 us per iteration on average,
// profiles/r6_43_march_gaps.txt; MarchKnobs::time_every overrides)
struct IterTiming {
  enum Phase { kP = 0, kS = 1, kB = 2 };
  static constexpr int kEv = 6;  // events per iteration slot of a chunk
  perc_ctx* h;
  KernelTiming& T;
  const int every;
  explicit IterTiming(perc_ctx* ctx) : h(ctx), T(ctx->timing), every(ctx->knobs.time_every) {}
  hipError_t init() {  // events for the longest chunk
    if (!T.enabled || T.ev.size() >= kEv * (size_t)ChunkSchedule::kMax) return hipSuccess;
    const size_t have = T.ev.size();
    T.ev.resize(kEv * (size_t)ChunkSchedule::kMax);
    for (size_t i = have; i < T.ev.size(); ++i) HIP_TRY(timing_event_create(&T.ev[i]));
    return hipSuccess;
  }
  // the next CG launch is iteration slot j's `phase`: it carries the events if j is sampled
  void arm(int j, Phase phase) {
    if (!T.enabled || j % every != 0) return;
    h->ev_next[0] = T.ev[kEv * j + 2 * phase];
    h->ev_next[1] = T.ev[kEv * j + 2 * phase + 1];
  }
  void disarm() { h->ev_next[0] = h->ev_next[1] = nullptr; }
  // after the chunk's synchronize: the sampled launches among its first
  // `real` iterations (the launches of this chunk that did work)
  void collect(int real) {
    if (!T.enabled) return;
    int nt = 0;
    for (int j = 0; j < real; j += every, ++nt) {
      float tp = 0.f, ts = 0.f, tb = 0.f;
      if (!h->plan.fused) hipEventElapsedTime(&tp, T.ev[kEv * j], T.ev[kEv * j + 1]);
      hipEventElapsedTime(&ts, T.ev[kEv * j + 2], T.ev[kEv * j + 3]);
      hipEventElapsedTime(&tb, T.ev[kEv * j + 4], T.ev[kEv * j + 5]);
      T.p_ms += tp;
      T.spmv_ms += ts;
      T.update_ms += tb;
    }
    T.spmv_n += nt;
    T.update_n += nt;
    T.p_n += nt;
  }
};

// Phase probe of the strip-major march (MarchKnobs::trace): per-wave stamps
// (4 words) of the P and B launches of iterations first_it (default 1000) ..
// +3, appended to the CSV at `path` after the solve
struct MarchTrace {
  static constexpr int kIters = 4;  // traced iterations
  DevBuf<unsigned long long> buf;
  const char* path = nullptr;
  int first_it = 0;
  size_t waves = 0;
  size_t words() const { return (size_t)2 * kIters * 4 * waves; }
  hipError_t alloc(const perc_ctx* h) {
    path = h->knobs.trace;
    first_it = h->knobs.trace_it;
    waves = (size_t)std::max(h->march_grid, h->wm_grid) * kMarchWaves;
    HIP_TRY(buf.alloc(words()));
    return hipMemsetAsync(buf, 0, words() * 8, h->stream);
  }
  // the stamps of launch kiter's P (kb = 0) or B (1); null outside the traced iterations
  unsigned long long* slot(int kiter, int kb) const {
    const int it = kiter - first_it;
    return buf && it >= 0 && it < kIters ? buf + (size_t)(2 * it + kb) * 4 * waves : nullptr;
  }
  hipError_t dump(const perc_ctx* h) const {
    if (!buf) return hipSuccess;
    std::vector<unsigned long long> tr(words());
    HIP_TRY(hipMemcpy(tr.data(), buf, tr.size() * 8, hipMemcpyDeviceToHost));
    if (FILE* fo = fopen(path, "a")) {
      fprintf(fo, "# m=%d nrows=%d band_rows=%d grid=%d waves=%zu (wall clock ticks, 100 MHz)\n"
                  "iter,kernel,wave,t_entry,t_walk_end,t_exit,xcc,hw_id\n",
              h->g.m, h->g.n - 2, h->march_h, h->march_grid, waves);
      for (int it = 0; it < kIters; ++it)
        for (int kb = 0; kb < 2; ++kb)
          for (size_t wv = 0; wv < waves; ++wv) {
            const unsigned long long* v = &tr[((size_t)(2 * it + kb) * waves + wv) * 4];
            fprintf(fo, "%d,%s,%zu,%llu,%llu,%llu,%llu,%llu\n", first_it + it, kb ? "B" : "P", wv, v[0],
                    v[1], v[2], v[3] >> 32, v[3] & 0xffffffffull);
          }
      fclose(fo);
    }
    return hipSuccess;
  }
};

// the solve's scalars, tickets and error history; x = 0 when it starts there
hipError_t reset_scalars(perc_ctx* h, double tol, int itmax, bool x0_zero) {
  DeviceBuffers& d = h->d;
  hipStream_t st = h->stream;
  if (!h->plan.stencil) HIP_TRY(ensure_csr(h));
  if (d.err_hist_cap < itmax + 2) {
    if (d.err_hist) HIP_TRY(hipFree(d.err_hist));
    d.err_hist_cap = itmax + 2;
    HIP_TRY(dmalloc(&d.err_hist, d.err_hist_cap));
  }
  CGScalars hs{};
  hs.tol = tol;
  hs.itmax = itmax;
  hs.bkden = 1.0;
  hs.rlo = INT_MAX;  // (k_cg_init's atomic min / max)
  hs.rhi = -1;
  HIP_TRY(hipMemcpyAsync(d.scal, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d.tickets, 0, kRedSlots * red_tickets_size(red_grid(h)) * sizeof(unsigned),
                         st));
  if (x0_zero) {
    k_zero<<<blocks_for(h->N + 2), kBlock, 0, st>>>(d.x, h->N + 2);
  }
  return hipSuccess;
}

// r(0), bnrm and the first bknum (k_cg_init; the literal order: in ascending
// j), and where the literal order's production kernels store their terms
hipError_t solve_prologue(perc_ctx* h, CGArgs& a, int itol, bool x0_zero) {
  DeviceBuffers& d = h->d;
  hipStream_t st = h->stream;
  const bool literal = h->dot_order != PERC_DOT_FAST, ST = h->plan.stencil;
  if (ST) k_cg_init<true><<<h->grid, kBlock, 0, st>>>(a, itol, x0_zero ? 1 : 0);
  else k_cg_init<false><<<h->grid, kBlock, 0, st>>>(a, itol, x0_zero ? 1 : 0);
  HIP_TRY(dbg_sync(st, "k_cg_init"));
  if (literal) {  // bnrm and the first bknum in ascending j
    if (ST) k_fold_init<true><<<1, 64, 0, st>>>(a, itol);
    else k_fold_init<false><<<1, 64, 0, st>>>(a, itol);
    HIP_TRY(dbg_sync(st, "k_fold_init"));
  }
  // the production kernels in the literal order store their terms (a.lit):
  // the q-free march and the resident solve
  if (literal && !h->plan.small && (h->plan.resident || (h->plan.march && h->plan.qfree))) {
    if (!d.lit) HIP_TRY(dmalloc(&d.lit, (size_t)3 * h->N + 8));
    a.lit = d.lit;
  }
  return hipSuccess;
}

// The solves that are one kernel: the one-workgroup solve (k_cg_small) and the
// resident cooperative solve.  *done stays false where neither applies, or the
// resident launch was refused and the launched kernels take over.
hipError_t solve_one_kernel(perc_ctx* h, const CGArgs& a, int* iter, double* err, bool* done) {
  hipStream_t st = h->stream;
  const bool literal = h->dot_order != PERC_DOT_FAST, ST = h->plan.stencil;
  *done = false;
  if (!h->plan.small && !h->plan.resident) return hipSuccess;
  // (the one-kernel solves' flags; the launched kernels': prepare_march)
  h->last_flags = (literal ? PERC_RAN_LITERAL : 0) | (a.lit ? PERC_RAN_LIT_TERMS : 0);
  if (h->plan.small) {  // one workgroup runs the whole loop (k_cg_small)
    // (x is kept on every row here: the operator is the CSR one and N small)
    if (ST) {
      if (literal) k_cg_small<true, true><<<1, kSmallThreads, 0, st>>>(a);
      else k_cg_small<true, false><<<1, kSmallThreads, 0, st>>>(a);
    } else {
      if (literal) k_cg_small<false, true><<<1, kSmallThreads, 0, st>>>(a);
      else k_cg_small<false, false><<<1, kSmallThreads, 0, st>>>(a);
    }
    HIP_TRY(dbg_sync(st, "k_cg_small"));
    CGScalars hs{};
    HIP_TRY(hipMemcpyAsync(&hs, h->d.scal, sizeof(hs), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *iter = hs.iter;
    *err = hs.err;
    *done = true;
    return hipSuccess;
  }
  const hipError_t e = dev_solve_resident(h, a, iter, err);
  // the cooperative launch can be refused when the grid cannot be
  // co-resident (e.g. CUs taken by another context): nothing ran, r and
  // the scalars are as k_cg_init left them, so the launched kernels take
  // over for this solve
  if (e != hipErrorCooperativeLaunchTooLarge && e != hipErrorInvalidConfiguration) {
    *done = true;
    return e;
  }
  (void)hipGetLastError();
  fprintf(stderr, "[perc] resident solve not launchable (%s): launched kernels\n",
          hipGetErrorString(e));
  h->plan.resident = false;
  h->last_kernel = h->plan.family();
  return hipSuccess;
}

// the x updates the loop left pending (a solve that ran an iteration)
hipError_t finish_x(perc_ctx* h, const CGArgs& a) {
  hipStream_t st = h->stream;
  if (!a.bx) {
    k_cg_xfinal<<<h->grid, kBlock, 0, st>>>(a);
    HIP_TRY(dbg_sync(st, "k_cg_xfinal"));
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (a.mxin) {  // the last B's x update
    k_march_xpend<<<cdiv(2 * h->g.m, kBlock), kBlock, 0, st>>>(a);
    HIP_TRY(dbg_sync(st, "k_march_xpend"));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return hipSuccess;
}

// The launched kernels: iterations in chunks (ChunkSchedule); the device flag
// makes the launches past the stop no-ops
hipError_t solve_launched(perc_ctx* h, CGArgs& a, int itmax, bool x0_zero, int* iter, double* err) {
  hipStream_t st = h->stream;
  const bool literal = h->dot_order != PERC_DOT_FAST, ST = h->plan.stencil;
  const int G = h->grid;
  if (!(h->plan.march && h->plan.qfree)) a.lit = nullptr;  // (the other kernels store no terms)
  HIP_TRY(prepare_march(h, a, itmax, false));
  MarchFront front;
  front.on = front_allowed(h, a, x0_zero);
  if (front.on) h->last_flags |= PERC_RAN_FRONT;
  HostFold hf;
  const bool host_fold = (h->last_flags & PERC_RAN_HOST_FOLD) != 0;
  if (host_fold) HIP_TRY(hf.t.alloc(3 * (size_t)h->N));
  PinnedBuf<CGScalars> hsp;
  HIP_TRY(hsp.alloc(1));
  IterTiming timing(h);
  HIP_TRY(timing.init());
  MarchTrace trace;
  if (h->knobs.trace && h->plan.march && a.sm && h->plan.qfree) HIP_TRY(trace.alloc(h));
  ChunkSchedule cs;
  int done_iters = 0;
  while (true) {
    for (int j = 0; j < cs.chunk; ++j) {
      a.kiter = cs.kiter(j);
      front_rows(h, front, a);
      // (tag: exact in a double while solve_epoch < 2^29)
      a.mtag = (double)(((unsigned long long)h->solve_epoch << 24) | (unsigned long long)a.kiter);
      a.mtrace = trace.slot(a.kiter, 0);
      if (!h->plan.fused) {
        timing.arm(j, IterTiming::kP);
        if (ST) klaunch(h, k_cg_p<true>, G, kBlock, st, a);
        else klaunch(h, k_cg_p<false>, G, kBlock, st, a);
        HIP_TRY(dbg_sync(st, "k_cg_p"));
      }
      timing.arm(j, IterTiming::kS);
      HIP_TRY(launch_cg_spmv(h, a, G));
      HIP_TRY(dbg_sync(st, "k_cg_spmv"));
      if (host_fold) {  // akden in ascending j, then ak (on the host)
        HIP_TRY(host_fold_qp(h, a, hf));
      } else if (literal) {  // akden in ascending j, then ak
        k_fold_qp<<<1, 64, 0, st>>>(a);
        HIP_TRY(dbg_sync(st, "k_fold_qp"));
      }
      timing.arm(j, IterTiming::kB);
      a.mtrace = trace.slot(a.kiter, 1);
      HIP_TRY(launch_cg_b(h, a, G));
      a.mtrace = nullptr;
      HIP_TRY(dbg_sync(st, "k_cg_b"));
      timing.disarm();
      if (host_fold) {  // z.r and r.r in ascending j: bk, err, the stop test (host)
        HIP_TRY(host_fold_b(h, a, hf));
      } else if (literal) {  // z.r and r.r in ascending j: bk, err, the stop test
        if (ST) k_fold_b<true><<<1, 64, 0, st>>>(a);
        else k_fold_b<false><<<1, 64, 0, st>>>(a);
        HIP_TRY(dbg_sync(st, "k_fold_b"));
      }
    }
    cs.chunk_done();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hsp, h->d.scal, sizeof(CGScalars), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    timing.collect(std::min(cs.chunk, hsp->iter - done_iters));
    done_iters = hsp->iter;
    if (hsp->done) break;
    // the first chunk walked every band; its read-back brings the source rows
    if (front.on && cs.first_done() && hsp->rhi >= hsp->rlo) {
      front.lo = hsp->rlo / a.T.m;
      front.hi = hsp->rhi / a.T.m;
      front.known = front.hi < a.T.nrows;
    }
    if (cs.overrun(itmax)) break;
    cs.grow();
  }
  if (hsp->iter > 0) HIP_TRY(finish_x(h, a));
  HIP_TRY(trace.dump(h));
  *iter = hsp->iter;
  *err = hsp->err;
  // iterations that ran with a dead band (the launches past the stop did nothing)
  h->last_front = std::max(0, std::min(hsp->iter, front.last_dead) - ChunkSchedule::kFirst);
  if (a.mgran && hsp->pad[1] != 0) {
    fprintf(stderr, "[perc] k_cg_march: reduction granule not seen within the poll limit\n");
    return hipErrorLaunchTimeOut;
  }
  return hipSuccess;
}

hipError_t dev_solve_impl(perc_ctx* h, int itol, double tol, int itmax, bool x0_zero, bool full_x,
                          int* iter, double* err) {
  if (h->dot_order != PERC_DOT_FAST && h->nslab > 1) {
    set_error("the literal dot order sums over the whole system: one slab only");
    return hipErrorInvalidValue;
  }
  HIP_TRY(reset_scalars(h, tol, itmax, x0_zero));
  if (itol >= 3) return dev_solve_x34(h, itol, tol, itmax, iter, err);
  // row slabs (perc_set_slabs; the prologue starts from x = 0, as linbcg's
  // callers do)
  if (h->nslab > 1 && x0_zero) {
    h->last_kernel = PERC_RAN_SLABS;
    return dev_solve_slabs(h, h->nslab, itol, tol, itmax, full_x, iter, err);
  }
  CGArgs a = make_cg_args(h);
  // linbcg never reads x inside the iteration (r is recursive), and the
  // terminal currents read it only on the interior rows next to the
  // electrodes (bondc.f:554-592): unless the caller wants every voltage, x
  // is carried on the first and last lattice rows only -- bitwise the same
  // values there, 16 B/row/iteration less traffic
  a.xrows = full_x || h->g.m <= 0 ? 0 : h->g.m;
  HIP_TRY(solve_prologue(h, a, itol, x0_zero));
  h->last_kernel = h->plan.family();
  bool done = false;
  HIP_TRY(solve_one_kernel(h, a, iter, err, &done));
  if (done) return hipSuccess;
  return solve_launched(h, a, itmax, x0_zero, iter, err);
}
}  // namespace

hipError_t dev_spmv(perc_ctx* h, const double* x, double* y) {
  if (!h->plan.stencil) HIP_TRY(ensure_csr(h));
  DeviceBuffers& d = h->d;
  hipStream_t st = h->stream;
  const size_t bytes = sizeof(double) * h->N;
  HIP_TRY(hipMemcpyAsync(d.p0, x, bytes, hipMemcpyHostToDevice, st));
  CGArgs a = make_cg_args(h);
  launch_spmv(h, a, d.p0, d.q);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(y, d.q, bytes, hipMemcpyDeviceToHost, st));
  return hipStreamSynchronize(st);
}

hipError_t dev_selftest_division(long long n, unsigned long long seed, unsigned long long* out3) {
  unsigned long long* d = nullptr;
  HIP_TRY(dmalloc(&d, 3));
  HIP_TRY(hipMemset(d, 0, 3 * sizeof(unsigned long long)));
  k_selftest_div<<<4096, kBlock>>>(n, seed, d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out3, d, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return hipFree(d);
}

hipError_t dev_bench(perc_ctx* h, int which, int reps, double* ms) {
  h->knobs = read_march_knobs();
  HIP_TRY(ensure_csr(h));  // the probes run every format
  DeviceBuffers& d = h->d;
  hipStream_t st = h->stream;
  CGArgs a = make_cg_args(h);
  const bool ST = h->plan.stencil;
  // scalars for a steady-state iteration (iter = 1 -> general p update)
  CGScalars hs{};
  hs.bknum = 1.0;
  hs.bkden = 2.0;
  hs.bk = 0.5;
  hs.ak = 0.5;
  hs.bnrm = 1.0;
  hs.tol = -1.0;
  hs.itmax = 1 << 30;
  hs.iter = 1;
  a.kiter = 2;
  // the solve's layout and reductions for the CG kernels (the plain SpMV
  // probe stays row-major): strip-major copies, tagged granules
  if (which == 1 || which == 2 || which == 5) HIP_TRY(prepare_march(h, a, hs.itmax, true));
  HIP_TRY(hipMemcpyAsync(d.scal, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d.tickets, 0, kRedSlots * red_tickets_size(red_grid(h)) * sizeof(unsigned),
                         st));
  if (which == 6 && h->res_G <= 0) return hipErrorInvalidConfiguration;  // no resident grid
  // STREAM copy: 512 MB -> 512 MB, well past the 256 MB Infinity Cache
  DevBuf<double> cp_src, cp_dst;
  const size_t cp_n = (size_t)64 << 20;
  if (which == 4) {
    HIP_TRY(cp_src.alloc(cp_n));
    HIP_TRY(cp_dst.alloc(cp_n));
    HIP_TRY(hipMemsetAsync(cp_src, 0, cp_n * sizeof(double), st));
  }
  hipError_t lerr = hipSuccess;
  auto keep = [&](hipError_t le) {  // the first failed launch
    if (le != hipSuccess && lerr == hipSuccess) lerr = le;
  };
  auto launch = [&]() {
    const int G = h->grid;
    if (which == 0) {
      launch_spmv(h, a, d.p0, d.q);
    } else if (which == 1) {
      keep(launch_cg_spmv(h, a, G));
    } else if (which == 2) {
      keep(launch_cg_b(h, a, G));
    } else if (which == 3) {
      if (ST) k_cg_p<true><<<G, kBlock, 0, st>>>(a);
      else k_cg_p<false><<<G, kBlock, 0, st>>>(a);
    } else if (which == 6) {  // resident sync floor: 16 iterations per launch
      ResArgs ra{};
      ra.G = h->res_G;
      ra.gran = d.res_gran;
      ra.reg = d.res_reg;
      ra.xg = d.res_xg;
      ra.S = d.scal;
      int iters = 16;
      void* args[] = {&ra, &iters};
      (void)hipMemsetAsync(d.res_gran, 0, (size_t)2 * 3 * h->res_G * sizeof(double), st);
      (void)hipMemsetAsync(d.res_reg, 0, 9 * kTicketStride * sizeof(unsigned), st);
      (void)hipMemsetAsync(d.res_xg, 0, kResXgDoubles * sizeof(double), st);
      // a refused grid (CUs taken) must not time an empty stream
      keep(hipLaunchCooperativeKernel((const void*)k_res_sync_probe, dim3(ra.G), dim3(h->res_NT), args, 0, st));
    } else if (which == 5) {  // one whole iteration
      if (!h->plan.fused) {
        if (ST) k_cg_p<true><<<G, kBlock, 0, st>>>(a);
        else k_cg_p<false><<<G, kBlock, 0, st>>>(a);
      }
      keep(launch_cg_spmv(h, a, G));
      keep(launch_cg_b(h, a, G));
    } else {
      k_copy<<<cdiv(cp_n / 2, kBlock), kBlock, 0, st>>>(cp_src.get(), cp_dst.get(), (int)cp_n);
    }
  };
  // the B kernel advances iter (tol < 0 keeps it running); values are
  // irrelevant for timing
  for (int i = 0; i < 3; ++i) launch();
  HIP_TRY(lerr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(h->ev[0], st));
  for (int i = 0; i < reps; ++i) launch();
  HIP_TRY(hipEventRecord(h->ev[1], st));
  HIP_TRY(hipEventSynchronize(h->ev[1]));
  HIP_TRY(lerr);
  float t = 0.f;
  HIP_TRY(hipEventElapsedTime(&t, h->ev[0], h->ev[1]));
  *ms = (double)t / reps / (which == 6 ? 16 : 1);
  return hipSuccess;
}

}  // namespace perc
