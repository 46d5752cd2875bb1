// perc_batch.h -- the batch path of libperc: many independent small bond
// realisations in one launch, one workgroup per (trial, bond count) item
// (perc_batch.hip: k_batch_bondc; perc_batch_host.cpp: the C-ABI and the
// ensemble's batched trial loop).
#pragma once
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

// Byte offsets of the workgroup's LDS arena (every offset a multiple of 16).
// The solver's p and q (8 N bytes each) start the arena; the labeling's
// arrays -- parent (int, t + 1), the bond occupancy (nb + 1 bytes), the
// member and spanning flags -- alias them: they are dead once the row codes,
// the top row's rhs and the electrode rows' current codes are formed, before
// the first iteration writes p.  The row codes follow whichever ends later.
struct BatchLds {
  int oQ, oBocc, oMem, oFlag, oC, oRed, oOff, oF, oRhs, oCur, oInt, total;
};
BatchLds batch_lds(const Geom& g);
constexpr int kBatchLdsStatic = 2048;  // fold_chunk's term rows (static __shared__)
constexpr int kBatchLdsMax = 160 * 1024;

// threads per workgroup for an N-row system: the fewest of 256 / 512 / 1024
// that keep kBatchEPT rows per thread (PERC_BATCH_THREADS overrides it where
// it still fits: the geometry A/B of tools/cond_workers.py)
int batch_threads(int N);

// host-only checks of perc_batch_supported
bool batch_supported(const Geom& g);

// device side (perc_batch.hip).  The orders' inverse permutations, once per
// group of trials: rank[tr * nb + id - 1] = position of bond id in trial
// tr's order (INT_MAX: not in it); then any number of launches over items of
// those trials.  out[nitems]; iout[nitems * 2m] (solve != 0 only).
hipError_t dev_batch_upload(perc_ctx* h, int ntrials, const int* rank);
hipError_t dev_batch_run(perc_ctx* h, int nitems, const int* item_trial, const int* item_count,
                         int solve, double Va, double g0, double leak, int itol, double tol,
                         int itmax, bool literal, BatchOut* out, double* iout);
void dev_batch_free(perc_ctx* h);
// host side (perc_batch_host.cpp): perc_batch_bondc's two halves, so the
// ensemble uploads a group's orders once and launches over them many times.
// replay: run the items several clusters span through the single path
// (false: leave them with fallback = 1 and the kernel's nspan -- enough for
// the bisection of the first spanning count)
int batch_upload_orders(perc_ctx* h, int ntrials, const int* orders);
int batch_run_items(perc_ctx* h, const int* orders, int nitems, const int* item_trial,
                    const int* item_count, int solve, bool replay, double Va, double g0, double leak,
                    int itol, double tol, int itmax, perc_batch_item* out);
// the closed-form rows' forms of the square lattice (perc_assemble.hip)
void asm_closed_forms(perc_ctx* h, int* fast_out, int* fl_out, int* fr_out);

}  // namespace perc
