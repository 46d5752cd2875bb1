// perc_batch.h -- the batch path of libperc: many independent small
// realisations (bond, site or mixed) in one launch, one workgroup per
// (trial, counts) item.  Who owns what: perc_batch.hip the context's rank
// store (below), the conductance path's device buffers, dev_batch_run and
// k_batch_cond; perc_batch_large.hip and perc_batch_weighted.hip their kernel
// and its launch; perc_batch_item.h the device code the three kernels share
// (the item's front end, the workgroup sums, the electrode rows' currents);
// perc_batch_currents.h the bond-current epilogue of k_batch_cond's FIELDS
// instantiations; perc_batch_scan.hip, perc_batch_clusters.hip and
// perc_batch_shuffle.hip their kernels and per-launch buffers (ranks in device
// memory in, results out); perc_batch_plan.h the host-only plan (the orders'
// inverse permutations, the item checks, the cut of a call into runs);
// perc_batch_host.cpp the C-ABI, the LDS plans and the one front door of the
// conductance, scan and cluster calls.
#pragma once
#include <cmath>
#include <type_traits>

#include "perc_internal.h"

namespace perc {

// rows of the largest interior system one workgroup solves (= k_cg_small's
// kSmallRows: 8 rows per thread at 1024 threads)
constexpr int kBatchRows = 8192;
constexpr int kBatchEPT = 8;  // rows per thread, at most

// what the kernel leaves per item (the host adds Gtop / Gbot from iout)
struct BatchOut {
  double err;
  int iter, status;
  int nclusters, nspan, span_root, span_sites;
  int fallback, pad;
};

// What every conductance kernel takes (dev_batch_run fills it once): the
// lattice, the trials' rank arrays, the items, the outputs and the solve's
// parameters.  A kernel's argument block is this plus its own LDS plan.
struct BatchItemArgs {
  Geom g;
  int N, nb;
  const int* bond_first;
  const StencilForms* forms;
  const int* rank;    // ntrials x nb (bond and mixed kinds)
  const int* rank_s;  // ntrials x t (site and mixed kinds)
  const int* item_trial;
  const int* item_count;   // occupied entries of the bond order (bond and mixed kinds)
  const int* item_nsites;  // ... of the site order (site and mixed kinds)
  BatchOut* out;
  double* iout;  // nitems x 2m
  int* sflag;
  int fast, fl, fr, bf_closed;
  int solve, itol, itmax, cur_rule;
  double Va, g0, leak, tol;
};

// The run-time (kind, literal) pair as compile-time constants:
// f(std::bool_constant<LIT>, std::integral_constant<int, KIND>)
template <class F>
hipError_t dispatch_kind_order(int kind, bool literal, F&& f) {
  auto of = [&](auto lit) {
    if (kind == PERC_BOND) return f(lit, std::integral_constant<int, PERC_BOND>{});
    if (kind == PERC_SITE) return f(lit, std::integral_constant<int, PERC_SITE>{});
    return f(lit, std::integral_constant<int, PERC_SITEBOND>{});
  };
  return literal ? of(std::true_type{}) : of(std::false_type{});
}
// ... and a workgroup size of 256 / 512 / 1024 with its slot 0 / 1 / 2:
// f(std::integral_constant<int, NT>, slot)
template <class F>
hipError_t dispatch_threads(int nt, F&& f) {
  if (nt == 256) return f(std::integral_constant<int, 256>{}, 0);
  if (nt == 512) return f(std::integral_constant<int, 512>{}, 1);
  return f(std::integral_constant<int, 1024>{}, 2);
}

// The labeling view every conductance kernel's arena starts with (byte
// offsets, multiples of 16): parent (int, t + 1) at 0, the bond occupancy
// (nb + 1 bytes), the member flags (t + 1), the spanning flags (m + 1) and,
// for the site and mixed kinds, one byte per site (socc, t + 1; the bond
// kind's layout has none: oSocc = 0, unused).  label_end: its size.
struct BatchLabelView {
  int oBocc, oMem, oFlag, oSocc, label_end;
};
BatchLabelView batch_label_view(const Geom& g, int kind);

// Byte offsets of the workgroup's LDS arena (every offset a multiple of 16).
// The solver's p and q (8 N bytes each) start the arena; the labeling view
// (batch_label_view) aliases them: its arrays are dead once the row codes,
// the top row's rhs and the electrode rows' current codes are formed, before
// the first iteration writes p.  The row codes follow whichever view ends
// later.
struct BatchLds {
  int oQ, oBocc, oMem, oFlag, oSocc, oC, oRed, oOff, oF, oRhs, oCur, oInt, total;
};
BatchLds batch_lds(const Geom& g, int kind = PERC_BOND);
constexpr int kBatchLdsStatic = 2048;  // fold_chunk's term rows (static __shared__)
constexpr int kBatchLdsMax = 160 * 1024;

// threads per workgroup for an N-row system: the fewest of 256 / 512 / 1024
// that keep kBatchEPT rows per thread (PERC_BATCH_THREADS overrides it where
// it still fits: the geometry A/B of tools/cond_workers.py)
int batch_threads(int N);

// host-only checks of perc_batch_supported / perc_batch_cond_supported (the
// kind's own LDS layout)
bool batch_supported(const Geom& g, int kind = PERC_BOND);

// ---- the rank store (perc_batch.hip) -------------------------------------
// One per context: for each list (PERC_BOND: ntrials x nb, PERC_SITE: ntrials
// x t) the trials' rank arrays in device memory -- rank[tr * N + id - 1] =
// position of id in trial tr's order (INT_MAX: not in it) -- and one pinned
// host row to form them in.  Every batch kernel reads its ranks from here.
// The contract: every C-ABI batch call leaves the store holding the trials of
// its last run, numbered as that run numbered them, so nothing may rely on
// ranks surviving across C-ABI calls.  The one user of several launches over
// one filling is the ensemble's batched trial loop, which makes no C-ABI call
// in between: batch_upload_orders -> batch_run_items -> batch_scan_uploaded
// -> batch_run_items.
// stage: the list's pinned row sized for ntrials trials (the contents are not
// kept); commit: the row's first ntrials trials copied up on the context's
// stream and marked as held (the row is the store's until the next stage)
hipError_t dev_batch_stage(perc_ctx* h, int list, int ntrials, int** row);
hipError_t dev_batch_commit(perc_ctx* h, int list, int ntrials);
// the list's device buffer sized for ntrials trials and marked as holding
// them, for a kernel to fill (the device shuffle)
hipError_t dev_batch_reserve(perc_ctx* h, int list, int ntrials, int** d_rank);
// the list's ranks in device memory and the trials they hold (NULL, 0: none)
const int* dev_batch_ranks(perc_ctx* h, int list, int* ntrials);
// ---- conductance (perc_batch.hip: dev_batch_run) -------------------------
// the solve's parameters, as perc_batch_cond takes them; literal: the dot order
struct BatchSolve {
  int solve = 1, cur_rule = PERC_CUR_FORTRAN;
  double Va = 1.0, g0 = 1.0, leak = 0.0;
  int itol = 2;
  double tol = 0.0;
  int itmax = 0;
  bool literal = false;
};
// One launch over nitems items of the trials the store holds: out[nitems];
// iout[nitems * 2m] (solve != 0 only).  It reads the rank arrays its kind
// needs (item_nsites / item_count may be NULL where the kind does not read
// them) and refuses an item whose trial lies outside them.  wts (optional):
// the items' per-bond weights -- the launch is k_batch_cond_w's, whatever
// `large` says.  fld (optional): the launch is k_batch_cond's FIELDS
// instantiation, whatever `large` says; it solves every item.
struct BatchWeights;
struct BatchFields;
hipError_t dev_batch_run(perc_ctx* h, int kind, const BatchSolve& sv, int nitems, const int* item_trial,
                         const int* item_nsites, const int* item_count, BatchOut* out, double* iout,
                         bool large = false, const BatchWeights* wts = nullptr,
                         const BatchFields* fld = nullptr);
void dev_batch_free(perc_ctx* h);
// host side (perc_batch_host.cpp).  Where a call's ranks come from: order
// lists (ntrials x (t + 1) / ntrials x (nb + 1)) or, seeded, one seed per
// trial for the device shuffle; a list the kind does not read may be NULL.
// held: the store already holds the call's trials under the caller's numbers
// (batch_upload_orders), nothing is staged or shuffled.  replay: run the
// items several clusters span through the single path (false: leave them with
// fallback = 1 and the kernel's nspan -- enough for the bisection of the first
// spanning count); a replayed item's order is the caller's trial's, or,
// seeded, regenerated with perc_shuffle_seeded.
struct BatchSources {
  bool seeded = false;
  const int* site_src = nullptr;
  const int* bond_src = nullptr;
  bool held = false;
  bool replay = true;
};
// The items of a conductance call of any kind in runs of bounded size: per
// run, the ranks of the trials it names into the store (unless held), one
// launch, the fold of the terminal currents, the replays.  wts (optional):
// the call's per-bond weights (perc_batch_cond_weighted) -- k_batch_cond_w's
// launches, and a replayed item's weights set on the context after its
// labeling and cleared after it.
int batch_run_items_kind(perc_ctx* h, int kind, int ntrials, const BatchSources& src, int nitems,
                         const int* item_trial, const int* item_nsites, const int* item_nbonds,
                         const BatchSolve& sv, perc_batch_item* out, const BatchWeights* wts = nullptr,
                         const BatchFields* fld = nullptr);
// perc_batch_bondc's two halves, so the ensemble fills the store with a
// group's orders once and launches over them many times (the bond kind under
// PERC_CUR_FORTRAN, the store held)
int batch_upload_orders(perc_ctx* h, int ntrials, const int* orders);
int batch_run_items(perc_ctx* h, const int* orders, int nitems, const int* item_trial,
                    const int* item_count, int solve, bool replay, double Va, double g0, double leak,
                    int itol, double tol, int itmax, perc_batch_item* out);
// ---- bond currents (perc_batch_currents.h: k_batch_cond's FIELDS epilogue) --
// What perc_batch_cond_currents asks beside the conductances (host arrays, the
// items' entries at the chunk's offset): the records (cur, one per item) and
// the interior voltages (vint: items x N doubles, or NULL).  The default
// kernel only: the large one keeps x on 2m rows, the weighted one has other
// bond values.
struct BatchFields {
  double cut = 0.0;
  perc_batch_currents* cur = nullptr;
  double* vint = nullptr;
};
// octave of |i| below g0 Va (e0 = ilogb(g0 Va)): the record's histogram bin;
// 63 for a zero current and for everything 63 octaves down or more
__host__ __device__ inline int current_bin(int e0, double a) {
  if (a == 0.0) return 63;
  const long long b = (long long)e0 - (long long)ilogb(a);
  return b < 0 ? 0 : (b > 63 ? 63 : (int)b);
}
// ---- lattices up to 128 x 128 (perc_batch_large.hip: k_batch_cond_large) --
// One workgroup of 1024 threads, at most kBatchLargeEPT rows per thread: p
// alone in LDS, every thread's row codes and r in its registers, q held in
// registers (fast order) or rebuilt from p where r needs it (literal order),
// x on the 2m electrode-adjacent rows only.  Taken
// only while perc_set_batch_large is on (perc_ctx::batch_large).
constexpr int kBatchLargeSites = 16384;  // 128 x 128
constexpr int kBatchLargeThreads = 1024;
constexpr int kBatchLargeEPT = 16;  // rows per thread, at most
// Byte offsets of its LDS arena (every offset a multiple of 16).  Solver
// view: p (8 N) at 0, x of the first and last m rows (16 m), the literal
// order's staging row (two sums x 1024 terms).  The labeling view
// (batch_label_view) aliases it and is dead after the barrier that follows
// the assembly.  The reduction scratch, the
// form table, the current codes and the counters follow whichever view ends
// later.
struct BatchLargeLds {
  int oX, oStage, oBocc, oMem, oFlag, oSocc, oRed, oOff, oF, oCur, oInt, total;
};
BatchLargeLds batch_large_lds(const Geom& g, int kind);
// host-only check of perc_batch_large_supported
bool batch_large_supported(const Geom& g, int kind);
// one launch of k_batch_cond_large<literal, kind> over nitems items on the
// context's stream
hipError_t dev_batch_large_launch(perc_ctx* h, int kind, bool literal, const BatchItemArgs& c, int nitems);
// ---- per-bond weights (perc_batch_weighted.hip: k_batch_cond_w) ---------
// k_batch_cond_large's scheme (p alone of the N-sized solver arrays in LDS,
// r, the diagonal, q and the form / count of a thread's own rows in its
// registers, x on the 2m electrode-adjacent rows) with the rows' slot values
// themselves in LDS, one array of N doubles per slot, where the other two
// kernels rebuild them from a two-value code.  256 / 512 / 1024 threads, at
// most kBatchWEPT rows per thread.
constexpr int kBatchWEPT = 4;
constexpr int kBatchWRows = 1024 * kBatchWEPT;
// threads per workgroup: the fewest of 256 / 512 / 1024 that keep kBatchWEPT
// rows per thread
int batch_w_threads(int N);
// Byte offsets of its LDS arena (every offset a multiple of 16).  Solver
// view: p (8 N) at 0, x of the first and last m rows (16 m), the literal
// order's staging row (two sums x NT terms).  The labeling view
// (batch_label_view) aliases it.  After whichever view ends later, outside both: the slot values
// (scn arrays of 8 N bytes; the assembly writes them while it still reads
// parent and bocc), the electrode rows' slot values (2m sites x 6 doubles),
// the reduction scratch, the form table and 32 counters.
struct BatchWLds {
  int oX, oStage, oBocc, oMem, oFlag, oSocc, oVal, oEl, oRed, oOff, oF, oInt, total;
};
BatchWLds batch_w_lds(const Geom& g, int kind);
// host-only check of perc_batch_weighted_supported
bool batch_w_supported(const Geom& g, int kind);
// The weights of one perc_batch_cond_weighted call (host arrays, the items'
// entries at the chunk's offset): explicit rows (weights: nwsets x nb,
// item_wset) or ConductCalc seeds (item_wseed), never both.
struct BatchWeights {
  int nwsets = 0;
  const double* weights = nullptr;
  const int* item_wset = nullptr;
  const unsigned* item_wseed = nullptr;
};
// what dev_batch_run hands the weighted kernel beside the common block: per
// item either its weight row (wrows + item_wset[i] * nb) or its draws
// (u + i * nb, from k_twister_stream) and its row of the launch's scratch
// (wscratch + i * wstride; wstride = nb rounded up to 16 doubles, so that no
// two workgroups write one 128-byte line)
struct BatchWItems {
  const int* item_wset = nullptr;  // explicit mode, else NULL
  const double* wrows = nullptr;
  const double* u = nullptr;       // ConductCalc mode
  double* wscratch = nullptr;
  int wstride = 0;
};
// one launch of k_batch_cond_w<threads, literal, kind> over nitems items on
// the context's stream
hipError_t dev_batch_w_launch(perc_ctx* h, int kind, bool literal, const BatchItemArgs& c,
                              const BatchWItems& w, int nitems);
// k_twister_stream: n genrand_res53 doubles per seed (d_seeds, d_out: device)
hipError_t dev_twister_launch(perc_ctx* h, int nseeds, const unsigned* d_seeds, long long n, double* d_out);
// perc_batch_twister: seeds and out on the host, through the batch buffers
hipError_t dev_batch_twister(perc_ctx* h, int nseeds, const unsigned* seeds, long long n, double* out);
// ---- threshold scans (perc_batch_scan.hip: k_batch_scan) ----------------
// sites of the largest lattice one workgroup scans (128 x 128)
constexpr int kScanSites = 16384;
constexpr int kScanSPT = 16;  // sites per thread, at most
// Byte offsets of k_batch_scan's LDS arena (every offset a multiple of 16):
// parent (int, t + 1) at 0, the per-root sizes (int, t + 1; the site
// occupancy while the links of a labeling are formed), one link byte per site
// (bit k: the forward bond to nearestn slot k connects; bit 7: member site),
// the spanning flags (m + 1 bytes), 16 ints.
struct ScanLds {
  int oSize, oLink, oFlag, oInt, total;
};
ScanLds scan_lds(const Geom& g);
constexpr int kScanLdsStatic = 256;  // the compiler's own static LDS of k_batch_scan (resource usage)
// threads per workgroup for t sites: the fewest of 256 / 512 / 1024 that keep
// kScanSPT sites per thread
int scan_threads(int t);
// host-only check of perc_scan_supported
bool scan_supported(const Geom& g);
// device side.  Scan of ntrials trials from rank arrays in device memory
// (the store's: d_rank_b ntrials x nb, d_rank_s ntrials x t; either may be
// NULL where the kind does not read it); fixed (host, ntrials, mixed kinds
// only); out (host, ntrials).  kind PERC_BOND / PERC_SITE / PERC_SITEBOND,
// scan PERC_BOND / PERC_SITE (mixed only).
hipError_t dev_scan_run(perc_ctx* h, int kind, int scan, int ntrials, const int* d_rank_s,
                        const int* d_rank_b, const int* fixed, perc_scan_item* out);
void dev_scan_free(perc_ctx* h);
// ---- cluster statistics (perc_batch_clusters.hip: k_batch_clusters) -----
// the exact part of an item's histogram row: sizes 1..nexact, nexact at most
constexpr int kClusterExactMax = 1024;
// Byte offsets of k_batch_clusters' LDS arena (every offset a multiple of
// 16): the scan's arena (scan_lds: parent, the per-root sizes, the link
// bytes, the spanning flags, 16 ints), then the histogram row (nexact + 32
// ints) and the waves' partial sums (16 waves x 9 words of 8 bytes).
struct ClusterLds {
  int oSize, oLink, oFlag, oInt, oHist, oRed, total;
};
ClusterLds cluster_lds(const Geom& g, int nexact);
constexpr int kClusterLdsStatic = 256;  // the compiler's own static LDS of k_batch_clusters (resource usage)
// host-only check of perc_batch_clusters_supported: the scan's lattices, and
// 0 <= nexact <= kClusterExactMax
bool clusters_supported(const Geom& g, int nexact);
// The geometry instantiations' arena (k_batch_clusters<.., GEOM = true>):
// cluster_lds, then kGeomWords words of 8 bytes at *oGeo -- the 3 x 32 octave
// sums of an item's rows, 12 workgroup sums, the largest cluster's key and the
// spanning root.
constexpr int kGeomRowWords = 96;
constexpr int kGeomWords = kGeomRowWords + 16;
ClusterLds cluster_geom_lds(const Geom& g, int nexact, int* oGeo);
// host-only check of perc_batch_geometry_supported: clusters_supported, pbc == 0
bool geometry_supported(const Geom& g, int nexact);
// device side.  nitems items over rank arrays in device memory (d_rank_b:
// ntrials x nb, d_rank_s: ntrials x t; either may be NULL where the kind does
// not read it; every item_trial lies inside them: the caller's check); the
// item lists, out (nitems) and hist (nitems x (nexact + 32), or NULL) on the
// host.  Threads per workgroup: scan_threads(t).  geom (nitems, host): the
// launch is the GEOM instantiation's, which also fills rows (nitems x
// kGeomRowWords, or NULL).
hipError_t dev_clusters_run(perc_ctx* h, int kind, int nitems, const int* d_rank_s, const int* d_rank_b,
                            const int* item_trial, const int* item_nsites, const int* item_nbonds,
                            int nexact, perc_cluster_item* out, int* hist, perc_cluster_geom* geom = nullptr,
                            long long* rows = nullptr);
void dev_clusters_free(perc_ctx* h);
// ---- device shuffle (perc_batch_shuffle.hip: k_shuffle_ranks) -----------
// Byte offsets of k_shuffle_ranks' LDS arena (every offset a multiple of 16):
// the order (16-bit ids, N + 1) at 0, the swap targets of 64 steps (int).
struct ShuffleLds {
  int oJ, total;
};
ShuffleLds shuffle_lds(int N);
// host-only check of perc_shuffle_device_supported: every id of 1..N and the
// spill slot in 16 bits, the arena within a workgroup's LDS
bool shuffle_supported(int N);
// ntrials trials of a list (PERC_BOND / PERC_SITE) shuffled by seeds (host)
// into the rank store (dev_batch_reserve); orders_out (host, ntrials x
// (N + 1)) and ranks_out (host, ntrials x N) may be NULL.  list kShuffleFree:
// a list of nfree ids that is no list of the lattice, its ranks in a buffer of
// the shuffle's own (the rank store stays as it is).
constexpr int kShuffleFree = -1;
hipError_t dev_shuffle_run(perc_ctx* h, int list, int ntrials, const int* seeds, int* orders_out,
                           int* ranks_out, int nfree = 0);
void dev_shuffle_free(perc_ctx* h);
// host side (perc_batch_host.cpp): the first spanning bond count of every
// trial of the group batch_upload_orders left in the store (bond kind), one
// launch
int batch_scan_uploaded(perc_ctx* h, int ntrials, perc_scan_item* out);
// the closed-form rows' forms of the square lattice (perc_assemble.hip)
void asm_closed_forms(perc_ctx* h, int* fast_out, int* fl_out, int* fr_out);

}  // namespace perc
