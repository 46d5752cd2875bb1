// perc_batch_host.cpp -- host side of the batch path (include/perc.h:
// perc_batch_supported, perc_batch_bondc, perc_batch_cond_supported,
// perc_batch_cond, perc_batch_large_supported, perc_set_batch_large,
// perc_scan_supported, perc_batch_scan and the seeded forms
// perc_batch_shuffle, perc_batch_scan_seeded, perc_batch_cond_seeded, and the
// weighted perc_batch_weighted_supported, perc_batch_cond_weighted,
// perc_batch_twister, and the cluster tables' perc_batch_clusters_supported,
// perc_batch_clusters, perc_batch_clusters_seeded, the cluster geometry's
// perc_batch_geometry_supported, perc_batch_clusters_geom,
// perc_batch_clusters_geom_seeded, and the current
// distributions' perc_batch_currents_supported, perc_batch_cond_currents,
// perc_batch_cond_currents_seeded, perc_current_stats_host):
// the launch geometry and LDS layouts, then the calls.  Who owns what: every
// entry point keeps the checks of its own path (rule pairing, cut, nexact,
// fixed, its *_supported and that message) and shares perc_batch_plan.h's
// check_items and ItemRuns and, per run, provide_ranks -- the one place that
// turns order lists or seed lists into rank arrays in the context's rank
// store (perc_batch.h).  batch_cond_impl is the front door of every
// conductance call, perc_batch_bondc included; batch_run_items_kind its run
// loop: one launch per run, the fold of the terminal currents and the
// single-path replay of the items several clusters span.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "perc_batch.h"
#include "perc_batch_plan.h"

namespace perc {

// x rounded up to a multiple of 16 (the arenas' offsets)
static int up16(long long x) { return (int)((x + 15) & ~15LL); }

BatchLabelView batch_label_view(const Geom& g, int kind) {
  BatchLabelView V{};
  V.oBocc = up16(4 * ((long long)g.t + 1));
  V.oMem = V.oBocc + up16(nbonds(g) + 1);
  V.oFlag = V.oMem + up16(g.t + 1);
  V.label_end = V.oFlag + up16(g.m + 1);
  if (kind != PERC_BOND) {  // the site occupancy, one byte per site
    V.oSocc = V.label_end;
    V.label_end = V.oSocc + up16((long long)g.t + 1);
  }
  return V;
}

// the lattices every one-workgroup conductance kernel takes: three rows and
// columns at least, an even m on the triangular lattice (perc_ctx_create, H7)
static bool batch_geom_ok(const Geom& g) {
  return g.n >= 3 && g.m >= 3 && !(g.lattice == kTriangular && (g.m % 2) == 1);
}

BatchLds batch_lds(const Geom& g, int kind) {
  const long long N = (long long)g.t - 2 * g.m;
  BatchLds L{};
  L.oQ = up16(8 * N);
  const int solver_end = L.oQ + up16(8 * N);
  const BatchLabelView V = batch_label_view(g, kind);
  L.oBocc = V.oBocc, L.oMem = V.oMem, L.oFlag = V.oFlag, L.oSocc = V.oSocc;
  L.oC = std::max(solver_end, V.label_end);
  L.oRed = L.oC + up16(2 * N);
  L.oOff = L.oRed + up16(48 * sizeof(double));
  L.oF = L.oOff + up16(kMaxForms * kMaxSlots * sizeof(int));
  L.oRhs = L.oF + up16(sizeof(StencilForms));
  L.oCur = L.oRhs + up16(8LL * g.m);
  L.oInt = L.oCur + up16(4LL * g.m);
  L.total = L.oInt + 64;
  return L;
}

int batch_threads(int N) {
  int nt = N <= 256 * kBatchEPT ? 256 : (N <= 512 * kBatchEPT ? 512 : 1024);
  if (const char* e = std::getenv("PERC_BATCH_THREADS")) {
    const int v = std::atoi(e);
    if ((v == 256 || v == 512 || v == 1024) && (long long)v * kBatchEPT >= N) nt = v;
  }
  return nt;
}

// every interior row one of the stencil forms, every stencil bond present
// (k_assemble's sflag bits 1 and 2)
static bool stencil_rows_ok(const Geom& g) {
  const StencilForms F = stencil_forms(g);
  if (F.nforms <= 0) return false;
  for (int s = g.m + 1; s <= g.t - g.m; ++s) {
    int nb[6];
    const int cnt = sorted_neighbours(g, s, nb);
    bool form = false;
    for (int f = 0; f < F.nforms && !form; ++f) {
      bool same = F.cnt[f] == cnt;
      for (int j = 0; j < cnt && same; ++j) same = F.off[f][j] == nb[j] - s;
      form = same;
    }
    if (!form) return false;
    for (int j = 0; j < cnt; ++j) {
      const int lo = std::min(s, nb[j]), hi = std::max(s, nb[j]);
      int nn[6];
      nearestn(g, lo, nn);
      bool bond = false;
      for (int k = 0; k < g.scn; ++k) bond |= nn[k] == hi;
      if (!bond) return false;
    }
  }
  return true;
}

bool batch_supported(const Geom& g, int kind) {
  if (!batch_geom_ok(g)) return false;
  const long long N = (long long)(g.n - 2) * g.m;
  if (N > kBatchRows) return false;
  if (!stencil_rows_ok(g)) return false;
  const BatchLds L = batch_lds(g, kind);
  return L.total + kBatchLdsStatic <= kBatchLdsMax;
}

BatchLargeLds batch_large_lds(const Geom& g, int kind) {
  const long long N = (long long)g.t - 2 * g.m;
  BatchLargeLds L{};
  L.oX = up16(8 * N);
  L.oStage = L.oX + up16(16LL * g.m);
  const int solver_end = L.oStage + 2 * kBatchLargeThreads * (int)sizeof(double);
  const BatchLabelView V = batch_label_view(g, kind);
  L.oBocc = V.oBocc, L.oMem = V.oMem, L.oFlag = V.oFlag, L.oSocc = V.oSocc;
  // x and the staging row lie in what the labeling view overhangs of p, or
  // past it; what the labeling and the assembly read follows both views
  L.oRed = std::max(solver_end, V.label_end);
  L.oOff = L.oRed + up16(48 * sizeof(double));
  L.oF = L.oOff + up16(kMaxForms * kMaxSlots * sizeof(int));
  L.oCur = L.oF + up16(sizeof(StencilForms));
  L.oInt = L.oCur + up16(4LL * g.m);
  L.total = L.oInt + 64;
  return L;
}

bool batch_large_supported(const Geom& g, int kind) {
  if (!batch_geom_ok(g)) return false;
  if ((long long)g.m * g.n > kBatchLargeSites) return false;
  if (!stencil_rows_ok(g)) return false;
  const BatchLargeLds L = batch_large_lds(g, kind);
  return L.total + kBatchLdsStatic <= kBatchLdsMax;
}

int batch_w_threads(int N) { return N <= 256 * kBatchWEPT ? 256 : (N <= 512 * kBatchWEPT ? 512 : 1024); }

BatchWLds batch_w_lds(const Geom& g, int kind) {
  const long long N = (long long)g.t - 2 * g.m;
  const int nt = batch_w_threads((int)std::min<long long>(N, kBatchWRows));
  BatchWLds L{};
  L.oX = up16(8 * N);
  L.oStage = L.oX + up16(16LL * g.m);
  const int solver_end = L.oStage + 2 * nt * (int)sizeof(double);
  const BatchLabelView V = batch_label_view(g, kind);
  L.oBocc = V.oBocc, L.oMem = V.oMem, L.oFlag = V.oFlag, L.oSocc = V.oSocc;
  // the slot values are written while the labeling view is still read and
  // read while the solver view is live: past both
  L.oVal = std::max(solver_end, V.label_end);
  L.oEl = L.oVal + up16(8LL * g.scn * N);
  L.oRed = L.oEl + up16(8LL * 6 * 2 * g.m);
  L.oOff = L.oRed + up16(48 * sizeof(double));
  L.oF = L.oOff + up16(kMaxForms * kMaxSlots * sizeof(int));
  L.oInt = L.oF + up16(sizeof(StencilForms));
  L.total = L.oInt + 128;
  return L;
}

bool batch_w_supported(const Geom& g, int kind) {
  if (!batch_geom_ok(g)) return false;
  const long long N = (long long)(g.n - 2) * g.m;
  if (N > kBatchWRows) return false;  // kBatchWEPT rows per thread at 1024 threads
  if (!batch_large_supported(g, kind)) return false;  // (its checks, stencil_rows_ok among them)
  const BatchWLds L = batch_w_lds(g, kind);
  return (long long)L.total + kBatchLdsStatic <= kBatchLdsMax;
}

ScanLds scan_lds(const Geom& g) {
  ScanLds L{};
  L.oSize = up16(4 * ((long long)g.t + 1));
  L.oLink = L.oSize + up16(4 * ((long long)g.t + 1));
  L.oFlag = L.oLink + up16((long long)g.t + 1);
  L.oInt = L.oFlag + up16((long long)g.m + 1);
  L.total = L.oInt + 64;
  return L;
}

int scan_threads(int t) { return t <= 256 * kScanSPT ? 256 : (t <= 512 * kScanSPT ? 512 : 1024); }

bool scan_supported(const Geom& g) {
  if (g.n < 3 || g.m < 3 || (long long)g.m * g.n > kScanSites) return false;
  return scan_lds(g).total + kScanLdsStatic <= kBatchLdsMax;
}

ClusterLds cluster_lds(const Geom& g, int nexact) {
  const ScanLds S = scan_lds(g);
  ClusterLds L{};
  L.oSize = S.oSize, L.oLink = S.oLink, L.oFlag = S.oFlag, L.oInt = S.oInt;
  L.oHist = S.total;
  L.oRed = L.oHist + up16(4 * ((long long)nexact + 32));
  L.total = L.oRed + 16 * 9 * 8;
  return L;
}

bool clusters_supported(const Geom& g, int nexact) {
  if (nexact < 0 || nexact > kClusterExactMax || !scan_supported(g)) return false;
  return cluster_lds(g, nexact).total + kClusterLdsStatic <= kBatchLdsMax;
}

ClusterLds cluster_geom_lds(const Geom& g, int nexact, int* oGeo) {
  ClusterLds L = cluster_lds(g, nexact);
  *oGeo = L.total;
  L.total += up16(8LL * kGeomWords);
  return L;
}

bool geometry_supported(const Geom& g, int nexact) {
  if (g.pbc != 0 || !clusters_supported(g, nexact)) return false;
  int oGeo = 0;
  return cluster_geom_lds(g, nexact, &oGeo).total + kClusterLdsStatic <= kBatchLdsMax;
}

ShuffleLds shuffle_lds(int N) {
  ShuffleLds L{};
  L.oJ = up16(2 * ((long long)N + 1));
  L.total = L.oJ + 64 * (int)sizeof(int);
  return L;
}

bool shuffle_supported(int N) {
  if (N < 1 || N > 0xFFFF - 1) return false;  // ids 1..N and the target N + 1 in 16 bits
  return shuffle_lds(N).total <= kBatchLdsMax;
}

// One list's ranks of a run into the rank store: the run's trial j is the
// call's trial used[j] (used NULL: first + j).  Orders: their inverse
// permutations formed in the store's pinned row, then committed; seeds: the
// device shuffle, which fills the store itself.
static hipError_t provide_list(perc_ctx* h, int list, const BatchSources& src, int first, const int* used, int k,
                               std::vector<int>* seeds) {
  const int N = list == PERC_BOND ? (int)h->nb : h->g.t;
  const int* from = list == PERC_BOND ? src.bond_src : src.site_src;
  auto trial = [&](int j) { return (size_t)(used ? used[j] : first + j); };
  if (src.seeded) {
    seeds->resize((size_t)k);
    for (int j = 0; j < k; ++j) (*seeds)[j] = from[trial(j)];
    return dev_shuffle_run(h, list, k, seeds->data(), nullptr, nullptr);
  }
  int* row = nullptr;
  const hipError_t e = dev_batch_stage(h, list, k, &row);
  if (e != hipSuccess) return e;
  for (int j = 0; j < k; ++j) order_ranks(1, N, from + trial(j) * (N + 1), row + (size_t)j * N);
  return dev_batch_commit(h, list, k);
}

// ... of the lists the kind reads: the one orders-or-seeds switch of the
// conductance, scan and cluster calls.  d_s / d_b (optional): the store's
// ranks of the lists the kind reads, for a launch that takes them as pointers
static hipError_t provide_ranks(perc_ctx* h, int kind, const BatchSources& src, int first, const int* used,
                                int k, const int** d_s = nullptr, const int** d_b = nullptr) {
  std::vector<int> seeds;
  hipError_t e = hipSuccess;
  int held = 0;
  if (kind != PERC_BOND) e = provide_list(h, PERC_SITE, src, first, used, k, &seeds);
  if (e == hipSuccess && kind != PERC_SITE) e = provide_list(h, PERC_BOND, src, first, used, k, &seeds);
  if (d_s) *d_s = kind != PERC_BOND ? dev_batch_ranks(h, PERC_SITE, &held) : nullptr;
  if (d_b) *d_b = kind != PERC_SITE ? dev_batch_ranks(h, PERC_BOND, &held) : nullptr;
  return e;
}

// the most trials of the lists the kind reads whose rank arrays stay under
// 64 MB of device memory per run
static long long rank_run_cap(perc_ctx* h, int kind) {
  return (64LL << 20) / (4LL * ((kind != PERC_BOND ? h->g.t : 0) + (kind != PERC_SITE ? h->nb : 0)));
}

int batch_upload_orders(perc_ctx* h, int ntrials, const int* orders) {
  hipSetDevice(h->device);
  BatchSources src;
  src.bond_src = orders;
  return hip_status(provide_ranks(h, PERC_BOND, src, 0, nullptr, ntrials), "perc_batch_bondc/upload");
}

int batch_run_items_kind(perc_ctx* h, int kind, int ntrials, const BatchSources& src, int nitems,
                         const int* item_trial, const int* item_nsites, const int* item_nbonds,
                         const BatchSolve& sv_in, perc_batch_item* out, const BatchWeights* wts,
                         const BatchFields* fld) {
  const int nb = (int)h->nb, m = h->g.m, t = h->g.t;
  const size_t N = (size_t)h->N;
  const int rule = kind;  // (PERC_RULE_* of a kind has the kind's number)
  const bool need_s = kind != PERC_BOND, need_b = kind != PERC_SITE;
  BatchSolve sv = sv_in;
  sv.literal = h->dot_order != PERC_DOT_FAST;
  const int solve = sv.solve, cur_rule = sv.cur_rule;
  const double Va = sv.Va;
  const char* who = kind == PERC_BOND && cur_rule == PERC_CUR_FORTRAN ? "perc_batch_bondc" : "perc_batch_cond";
  hipSetDevice(h->device);
  hipError_t e;
  // launches of bounded size (the iout rows: 16 m bytes per item)
  int chunk = std::max(1, std::min(16384, (int)((64LL << 20) / (16LL * m))));
  // ... and the weighted kernel's rows (its draws, its scratch: 8 nb bytes per item each)
  if (wts) chunk = std::max(1, std::min(chunk, (int)((64LL << 20) / (8LL * (nb + 16)))));
  // ... and the interior voltages (8 N bytes per item)
  if (fld && fld->vint) chunk = std::max(1, std::min(chunk, (int)((64LL << 20) / (16LL * m + 8LL * (long long)N))));
  // ... and the rank arrays of the trials a run names (at most one per item)
  if (!src.held) chunk = (int)std::max(1LL, std::min<long long>(chunk, rank_run_cap(h, kind)));
  std::vector<BatchOut> bo((size_t)std::min(nitems, chunk));
  // a fallback item's record on the host: the bond list, the mask, the voltages
  std::vector<int> fb1, fb2, canon;
  std::vector<unsigned char> focc_s, focc_b, fmask;
  std::vector<double> fvint;
  std::vector<double> iout(solve ? bo.size() * 2 * (size_t)m : 0);
  std::vector<int> slist, blist, sregen, bregen;
  ItemRuns runs(src.held ? nullptr : item_trial, nitems, ntrials, chunk);
  while (runs.next()) {
    const int i0 = runs.i0, n = runs.n;
    if (!src.held) {
      e = provide_ranks(h, kind, src, 0, runs.used.data(), (int)runs.used.size());
      if (e != hipSuccess) return hip_status(e, who);
    }
    BatchWeights wc;
    if (wts) {
      wc = *wts;
      if (wc.item_wset) wc.item_wset += i0;
      if (wc.item_wseed) wc.item_wseed += i0;
    }
    BatchFields fc;
    if (fld) {
      fc = *fld;
      fc.cur += i0;
      if (fc.vint) fc.vint += (size_t)i0 * N;
    }
    e = dev_batch_run(h, kind, sv, n, src.held ? item_trial + i0 : runs.local.data(),
                      need_s ? item_nsites + i0 : nullptr, need_b ? item_nbonds + i0 : nullptr, bo.data(),
                      iout.data(), wts || fld ? false : h->batch_large, wts ? &wc : nullptr, fld ? &fc : nullptr);
    if (e != hipSuccess) return hip_status(e, who);
    for (int i = 0; i < n; ++i) {
      perc_batch_item& it = out[i0 + i];
      const BatchOut& b = bo[i];
      std::memset(&it, 0, sizeof(it));
      it.nclusters = b.nclusters;
      it.nspan = b.nspan;
      it.span_root = b.span_root;
      it.span_sites = b.span_sites;
      it.fallback = b.fallback;
      it.status = b.status;
      it.iter = b.iter;
      it.err = b.err;
      if (b.fallback && src.replay) {
        // several clusters span: the reference's lowest-label rule through
        // the single path, on the context
        const int tr = item_trial[i0 + i];
        const int *ssrc = nullptr, *bsrc = nullptr;
        int slen = 0, blen = 0;
        if ((need_s && !src.site_src) || (need_b && !src.bond_src)) return PERC_EINVAL;
        // the caller's trial's order of a list; seeded: regenerated on the host
        auto order_of = [&](const int* from, int len, std::vector<int>* regen) {
          if (!src.seeded) return from + (size_t)tr * (len + 1);
          regen->resize((size_t)len + 1);
          perc_shuffle_seeded(from[tr], len, regen->data());
          return (const int*)regen->data();
        };
        const int* so = need_s ? order_of(src.site_src, t, &sregen) : nullptr;
        const int* bo = need_b ? order_of(src.bond_src, nb, &bregen) : nullptr;
        if (need_s && !occupy_prefix(so, item_nsites[i0 + i], t, &slist, &ssrc, &slen)) return PERC_EINVAL;
        if (need_b && !occupy_prefix(bo, item_nbonds[i0 + i], nb, &blist, &bsrc, &blen)) return PERC_EINVAL;
        perc_label_info li{};
        int rc = perc_occupy(h, kind, slen, ssrc, blen, bsrc);
        if (fld) canon.resize((size_t)t);
        if (!rc) rc = perc_label(h, &li, fld ? canon.data() : nullptr);
        if (rc) return rc;
        it.nclusters = li.nclusters;
        it.nspan = li.nspan;
        it.span_root = li.span_root;
        it.span_sites = li.span_sites;
        if (solve) {
          perc_cond_result res{};
          // the item's weights on the context, after the labeling; cleared
          // again after the item (the context is left unweighted)
          if (wts && wts->item_wset)
            rc = perc_set_bond_weights(h, wts->weights + (size_t)wts->item_wset[i0 + i] * nb, nb);
          else if (wts)
            rc = perc_set_conductcalc_weights(h, rule, wts->item_wseed[i0 + i]);
          double* vrow = nullptr;
          if (fld) {
            fvint.resize(N);
            vrow = fld->vint ? fc.vint + (size_t)i * N : fvint.data();
          }
          if (!rc) rc = perc_conductance(h, rule, cur_rule, Va, sv.g0, sv.leak, sv.itol, sv.tol, sv.itmax, &res, vrow);
          if (!rc && fld && res.status == 0) {
            // the conducting mask from the occupancy lists and the canonical
            // labels (bond_value's three rules: a conducting bond's end sites
            // share one cluster), then the host's record
            if (fb1.empty()) {
              fb1.resize((size_t)nb);
              fb2.resize((size_t)nb);
              perc_bond_list(h->g.lattice, m, h->g.n, h->g.pbc, fb1.data(), fb2.data());
            }
            focc_s.assign((size_t)t + 1, 0);
            focc_b.assign((size_t)nb + 1, 0);
            for (int k = 0; need_s && k < slen; ++k)
              if (ssrc[k] >= 1 && ssrc[k] <= t) focc_s[ssrc[k]] = 1;
            for (int k = 0; need_b && k < blen; ++k)
              if (bsrc[k] >= 1 && bsrc[k] <= nb) focc_b[bsrc[k]] = 1;
            fmask.assign((size_t)nb, 0);
            for (int id = 1; id <= nb; ++id) {
              const int s1 = fb1[id - 1], s2 = fb2[id - 1];
              const bool occ = (!need_b || focc_b[id]) && (!need_s || (focc_s[s1] && focc_s[s2]));
              fmask[id - 1] = occ && li.span_root > 0 && canon[s1 - 1] == li.span_root;
            }
            rc = perc_current_stats_host(h->g.lattice, m, h->g.n, h->g.pbc, fmask.data(), vrow, Va, sv.g0, fld->cut,
                                         &fc.cur[i]);
          } else if (!rc && fld && fld->vint) {
            std::fill(vrow, vrow + N, 0.0);
          }
          if (wts) {
            const int rc2 = perc_set_bond_weights(h, nullptr, 0);
            if (!rc) rc = rc2;
          }
          if (rc) return rc;
          it.gtop = res.gtop;
          it.gbot = res.gbot;
          it.err = res.err;
          it.iter = res.iter;
          it.status = res.status;
        }
      } else if (solve && b.status == 0) {
        // currents_impl's folds: ascending (bondc.f:587-590), or Itop from
        // site t downward (ConductCalc.m:191-194)
        const double* io = iout.data() + (size_t)i * 2 * m;
        double Ibot = 0.0, Itop = 0.0;
        if (cur_rule == PERC_CUR_FORTRAN) {
          for (int c = 0; c < m; ++c) {
            Ibot = Ibot + io[c];
            Itop = Itop + io[m + c];
          }
        } else {
          for (int c = 0; c < m; ++c) {
            Ibot = io[c] + Ibot;
            Itop = io[2 * m - 1 - c] + Itop;
          }
        }
        it.gtop = Itop / Va;
        it.gbot = std::fabs(Ibot) / Va;
      }
    }
  }
  return PERC_OK;
}

int batch_run_items(perc_ctx* h, const int* orders, int nitems, const int* item_trial,
                    const int* item_count, int solve, bool replay, double Va, double g0, double leak,
                    int itol, double tol, int itmax, perc_batch_item* out) {
  BatchSources src;
  src.bond_src = orders;
  src.held = true;
  src.replay = replay;
  return batch_run_items_kind(h, PERC_BOND, 0, src, nitems, item_trial, nullptr, item_count,
                              BatchSolve{solve, PERC_CUR_FORTRAN, Va, g0, leak, itol, tol, itmax}, out);
}

int batch_scan_uploaded(perc_ctx* h, int ntrials, perc_scan_item* out) {
  hipSetDevice(h->device);
  int have = 0;
  const int* d_rank = dev_batch_ranks(h, PERC_BOND, &have);
  if (!d_rank || have < ntrials) {
    set_error("batch_scan_uploaded: no uploaded group of that many trials");
    return PERC_ESTATE;
  }
  return hip_status(dev_scan_run(h, PERC_BOND, PERC_BOND, ntrials, nullptr, d_rank, nullptr, out),
                    "perc_batch_scan");
}

// the lists the kind reads within the device shuffle's reach
static bool shuffle_lists_ok(perc_ctx* h, int kind) {
  return (kind == PERC_BOND || shuffle_supported(h->g.t)) && (kind == PERC_SITE || shuffle_supported((int)h->nb));
}
static const char* const kShuffleReach = "a list too long for the device shuffle (perc_shuffle_device_supported)";

}  // namespace perc

using namespace perc;

extern "C" {

int perc_batch_supported(int lattice, int m, int n, int pbc) {
  if (lattice != PERC_SQUARE && lattice != PERC_TRIANGULAR) return 0;
  if (m < 1 || n < 1 || (long long)m * n >= (1LL << 31) - 16) return 0;
  return batch_supported(make_geom(lattice, m, n, pbc)) ? 1 : 0;
}

int perc_batch_cond_supported(int kind, int lattice, int m, int n, int pbc) {
  if (kind != PERC_BOND && kind != PERC_SITE && kind != PERC_SITEBOND) return 0;
  if (lattice != PERC_SQUARE && lattice != PERC_TRIANGULAR) return 0;
  if (m < 1 || n < 1 || (long long)m * n >= (1LL << 31) - 16) return 0;
  return batch_supported(make_geom(lattice, m, n, pbc), kind) ? 1 : 0;
}

int perc_batch_large_supported(int kind, int lattice, int m, int n, int pbc) {
  if (kind != PERC_BOND && kind != PERC_SITE && kind != PERC_SITEBOND) return 0;
  if (lattice != PERC_SQUARE && lattice != PERC_TRIANGULAR) return 0;
  if (m < 1 || n < 1 || (long long)m * n > kBatchLargeSites) return 0;
  return batch_large_supported(make_geom(lattice, m, n, pbc), kind) ? 1 : 0;
}

int perc_set_batch_large(perc_ctx* h, int enable) {
  if (!h) return PERC_EINVAL;
  h->batch_large = enable != 0;
  return PERC_OK;
}

int perc_batch_large(perc_ctx* h) { return h ? (h->batch_large ? 1 : 0) : PERC_EINVAL; }

// The one front door of the conductance calls: perc_batch_cond and its
// weighted and currents forms (seeded = false: site_src / bond_src are order
// lists), the seeded forms (true: seed lists, the orders shuffled on the
// device) and perc_batch_bondc (bondc: its own predicates' names in the texts)
static int batch_cond_impl(const char* who, bool seeded, perc_ctx* h, int kind, int rule, int ntrials,
                           const int* site_src, const int* bond_src, int nitems, const int* item_trial,
                           const int* item_nsites, const int* item_nbonds, const BatchSolve& sv,
                           perc_batch_item* out, const BatchWeights* wts = nullptr,
                           const BatchFields* fld = nullptr, bool bondc = false) {
  if (!h) return PERC_EINVAL;
  auto bad = [who](const std::string& text) {
    set_error(std::string(who) + ": " + text);
    return PERC_EINVAL;
  };
  auto unsupported = [&](const char* kernel, const char* predicate) {
    return bad(std::string("lattice not supported by the ") + kernel + (bondc ? " (" : " for this kind (") +
               predicate + ")");
  };
  const bool pair = (kind == PERC_BOND && rule == PERC_RULE_BOND) ||
                    (kind == PERC_SITE && rule == PERC_RULE_SITE) ||
                    (kind == PERC_SITEBOND && rule == PERC_RULE_MIXED);
  if (!pair)
    return bad("kind / rule PERC_BOND / PERC_RULE_BOND, PERC_SITE / PERC_RULE_SITE or PERC_SITEBOND / "
               "PERC_RULE_MIXED only");
  if (sv.cur_rule != PERC_CUR_FORTRAN && sv.cur_rule != PERC_CUR_MATLAB)
    return bad("cur_rule PERC_CUR_FORTRAN or PERC_CUR_MATLAB only");
  if (ntrials < 0 || nitems < 0) return bad("ntrials or nitems < 0");
  if (sv.itmax < 0) return bad("itmax < 0");
  if (sv.solve && sv.itol != 1 && sv.itol != 2) return bad("itol 1 or 2 only");
  if (fld) {  // the default kernel only: the perc_set_batch_large flag is not read
    if (nitems && !fld->cur) return bad("cur missing");
    if (!(fld->cut >= 0.0 && fld->cut <= 1.0)) return bad("cut outside [0, 1]");
    if (!batch_supported(h->g, kind)) return unsupported("batch kernel", "perc_batch_currents_supported");
  } else if (wts) {  // its own kernel: the perc_set_batch_large flag is not read
    if (!batch_w_supported(h->g, kind))
      return unsupported("weighted batch kernel", "perc_batch_weighted_supported");
  } else if (h->batch_large) {
    if (!batch_large_supported(h->g, kind)) return unsupported("large batch kernel", "perc_batch_large_supported");
  } else if (!batch_supported(h->g, kind)) {
    return unsupported("batch kernel", bondc ? "perc_batch_supported" : "perc_batch_cond_supported");
  }
  if (const char* text = check_items(kind != PERC_BOND, kind != PERC_SITE, seeded, ntrials, site_src, bond_src,
                                     nitems, item_trial, item_nsites, item_nbonds, out, h->g.t, (int)h->nb))
    return bad(text);
  if (seeded && !shuffle_lists_ok(h, kind)) return bad(kShuffleReach);
  if (nitems == 0) return PERC_OK;
  BatchSources src;
  src.seeded = seeded;
  src.site_src = site_src;
  src.bond_src = bond_src;
  return batch_run_items_kind(h, kind, ntrials, src, nitems, item_trial, item_nsites, item_nbonds, sv, out, wts,
                              fld);
}

int perc_batch_bondc(perc_ctx* h, int ntrials, const int* orders, int nitems, const int* item_trial,
                     const int* item_count, int solve, double Va, double g0, double leak, int itol,
                     double tol, int itmax, perc_batch_item* out) {
  if (!h || ntrials < 0 || nitems < 0 || (ntrials && !orders) ||
      (nitems && (!item_trial || !item_count || !out)) || itmax < 0)
    return PERC_EINVAL;
  return batch_cond_impl("perc_batch_bondc", false, h, PERC_BOND, PERC_RULE_BOND, ntrials, nullptr, orders,
                         nitems, item_trial, nullptr, item_count,
                         BatchSolve{solve, PERC_CUR_FORTRAN, Va, g0, leak, itol, tol, itmax}, out, nullptr,
                         nullptr, true);
}

int perc_batch_cond(perc_ctx* h, int kind, int rule, int cur_rule, int ntrials, const int* site_orders,
                    const int* bond_orders, int nitems, const int* item_trial, const int* item_nsites,
                    const int* item_nbonds, int solve, double Va, double g0, double leak, int itol,
                    double tol, int itmax, perc_batch_item* out) {
  return batch_cond_impl("perc_batch_cond", false, h, kind, rule, ntrials, site_orders, bond_orders, nitems,
                         item_trial, item_nsites, item_nbonds,
                         BatchSolve{solve, cur_rule, Va, g0, leak, itol, tol, itmax}, out);
}

int perc_batch_cond_seeded(perc_ctx* h, int kind, int rule, int cur_rule, int ntrials,
                           const int* site_seeds, const int* bond_seeds, int nitems,
                           const int* item_trial, const int* item_nsites, const int* item_nbonds,
                           int solve, double Va, double g0, double leak, int itol, double tol, int itmax,
                           perc_batch_item* out) {
  return batch_cond_impl("perc_batch_cond_seeded", true, h, kind, rule, ntrials, site_seeds, bond_seeds, nitems,
                         item_trial, item_nsites, item_nbonds,
                         BatchSolve{solve, cur_rule, Va, g0, leak, itol, tol, itmax}, out);
}

int perc_batch_currents_supported(int kind, int lattice, int m, int n, int pbc) {
  return perc_batch_cond_supported(kind, lattice, m, n, pbc);
}

int perc_batch_cond_currents(perc_ctx* h, int kind, int rule, int cur_rule, int ntrials,
                             const int* site_orders, const int* bond_orders, int nitems,
                             const int* item_trial, const int* item_nsites, const int* item_nbonds,
                             double Va, double g0, double leak, int itol, double tol, int itmax,
                             perc_batch_item* out, double cut, perc_batch_currents* cur, double* vint_out) {
  const BatchFields fld{cut, cur, vint_out};
  return batch_cond_impl("perc_batch_cond_currents", false, h, kind, rule, ntrials, site_orders, bond_orders,
                         nitems, item_trial, item_nsites, item_nbonds,
                         BatchSolve{1, cur_rule, Va, g0, leak, itol, tol, itmax}, out, nullptr, &fld);
}

int perc_batch_cond_currents_seeded(perc_ctx* h, int kind, int rule, int cur_rule, int ntrials,
                                    const int* site_seeds, const int* bond_seeds, int nitems,
                                    const int* item_trial, const int* item_nsites, const int* item_nbonds,
                                    double Va, double g0, double leak, int itol, double tol, int itmax,
                                    perc_batch_item* out, double cut, perc_batch_currents* cur,
                                    double* vint_out) {
  const BatchFields fld{cut, cur, vint_out};
  return batch_cond_impl("perc_batch_cond_currents_seeded", true, h, kind, rule, ntrials, site_seeds, bond_seeds,
                         nitems, item_trial, item_nsites, item_nbonds,
                         BatchSolve{1, cur_rule, Va, g0, leak, itol, tol, itmax}, out, nullptr, &fld);
}

int perc_current_stats_host(int lattice, int m, int n, int pbc, const unsigned char* conducting,
                            const double* vint, double Va, double g0, double cut, perc_batch_currents* out) {
  auto bad = [](const char* text) {
    set_error(std::string("perc_current_stats_host: ") + text);
    return PERC_EINVAL;
  };
  if (lattice != PERC_SQUARE && lattice != PERC_TRIANGULAR) return bad("lattice PERC_SQUARE or PERC_TRIANGULAR only");
  if (m < 1 || n < 1 || (long long)m * n >= (1LL << 31) - 16) return bad("m or n < 1, or m * n too large");
  if (!conducting || !vint || !out) return bad("conducting, vint or out missing");
  if (!(cut >= 0.0 && cut <= 1.0)) return bad("cut outside [0, 1]");
  const int t = m * n, nb = perc_nbonds(lattice, m, n, pbc);
  std::vector<int> b1((size_t)std::max(nb, 1)), b2((size_t)std::max(nb, 1));
  if (perc_bond_list(lattice, m, n, pbc, b1.data(), b2.data()) != nb) return bad("the bond list");
  std::memset(out, 0, sizeof(*out));
  auto interior = [&](int s) { return s > m && s <= t - m; };
  auto V = [&](int s) { return s <= m ? 0.0 : (s > t - m ? Va : vint[s - m - 1]); };
  auto each = [&](auto f) {  // |i| of every counted bond, in id order
    for (int k = 0; k < nb; ++k) {
      if (!conducting[k] || !(interior(b1[k]) || interior(b2[k]))) continue;
      const double d = V(b2[k]) - V(b1[k]);
      const double ib = g0 * d;
      f(std::fabs(ib));
    }
  };
  const int e0 = ilogb(g0 * Va);
  each([&](double a) {
    const double i2 = a * a, i4 = i2 * i2, i6 = i4 * i2;
    ++out->nbonds;
    out->imax = std::fmax(out->imax, a);
    out->s1 = out->s1 + a;
    out->s2 = out->s2 + i2;
    out->s4 = out->s4 + i4;
    out->s6 = out->s6 + i6;
    ++out->hist[current_bin(e0, a)];
  });
  const double thr = cut * out->imax;
  each([&](double a) { out->nabove += a >= thr ? 1 : 0; });
  return PERC_OK;
}

int perc_batch_weighted_supported(int kind, int lattice, int m, int n, int pbc) {
  if (kind != PERC_BOND && kind != PERC_SITE && kind != PERC_SITEBOND) return 0;
  if (lattice != PERC_SQUARE && lattice != PERC_TRIANGULAR) return 0;
  if (m < 1 || n < 1 || (long long)m * n > kBatchLargeSites) return 0;
  return batch_w_supported(make_geom(lattice, m, n, pbc), kind) ? 1 : 0;
}

int perc_batch_cond_weighted(perc_ctx* h, int kind, int rule, int cur_rule, int ntrials,
                             const int* site_orders, const int* bond_orders, int nitems,
                             const int* item_trial, const int* item_nsites, const int* item_nbonds,
                             int nwsets, const double* weights, const int* item_wset,
                             const unsigned int* item_wseed, int solve, double Va, double g0, double leak,
                             int itol, double tol, int itmax, perc_batch_item* out) {
  if (!h) return PERC_EINVAL;
  auto bad = [](const char* text) {
    set_error(std::string("perc_batch_cond_weighted: ") + text);
    return PERC_EINVAL;
  };
  if ((weights != nullptr) != (item_wset != nullptr))
    return bad("weights and item_wset go together: one of them is missing");
  const bool expl = weights != nullptr;
  if (expl && item_wseed) return bad("both weight inputs given: (weights, item_wset) or item_wseed, not both");
  if (!expl && !item_wseed) return bad("no weight input: (weights, item_wset) or item_wseed");
  if (expl && nwsets < 1) return bad("nwsets < 1");
  if (nitems < 0) return bad("ntrials or nitems < 0");
  if (expl)
    for (int i = 0; i < nitems; ++i)
      if (item_wset[i] < 0 || item_wset[i] >= nwsets) return bad("item_wset outside 0..nwsets-1");
  BatchWeights wts;
  wts.nwsets = expl ? nwsets : 0;
  wts.weights = weights;
  wts.item_wset = item_wset;
  wts.item_wseed = item_wseed;
  return batch_cond_impl("perc_batch_cond_weighted", false, h, kind, rule, ntrials, site_orders, bond_orders,
                         nitems, item_trial, item_nsites, item_nbonds,
                         BatchSolve{solve, cur_rule, Va, g0, leak, itol, tol, itmax}, out, &wts);
}

int perc_batch_twister(perc_ctx* h, int nseeds, const unsigned int* seeds, long long n, double* out) {
  if (!h) return PERC_EINVAL;
  if (nseeds < 0 || n < 0) {
    set_error("perc_batch_twister: nseeds or n < 0");
    return PERC_EINVAL;
  }
  if (nseeds == 0 || n == 0) return PERC_OK;
  if (!seeds || !out) {
    set_error("perc_batch_twister: seeds or out missing");
    return PERC_EINVAL;
  }
  hipSetDevice(h->device);
  return hip_status(dev_batch_twister(h, nseeds, seeds, n, out), "perc_batch_twister");
}

int perc_shuffle_device_supported(int N) { return shuffle_supported(N) ? 1 : 0; }

int perc_batch_shuffle(perc_ctx* h, int list, int ntrials, const int* seeds, int* orders_out,
                       int* ranks_out) {
  if (!h) return PERC_EINVAL;
  auto bad = [](const char* text) {
    set_error(std::string("perc_batch_shuffle: ") + text);
    return PERC_EINVAL;
  };
  if (list != PERC_BOND && list != PERC_SITE) return bad("list PERC_BOND or PERC_SITE only");
  if (ntrials < 0) return bad("ntrials < 0");
  const long long N = list == PERC_BOND ? h->nb : (long long)h->g.t;
  if (N > INT_MAX || !shuffle_supported((int)N))
    return bad("a list too long for the device shuffle (perc_shuffle_device_supported)");
  if (ntrials == 0) return PERC_OK;
  if (!seeds) return bad("seeds missing");
  hipSetDevice(h->device);
  return hip_status(dev_shuffle_run(h, list, ntrials, seeds, orders_out, ranks_out), "perc_batch_shuffle");
}

int perc_batch_shuffle_n(perc_ctx* h, int N, int ntrials, const int* seeds, int* orders_out,
                         int* ranks_out) {
  if (!h) return PERC_EINVAL;
  auto bad = [](const char* text) {
    set_error(std::string("perc_batch_shuffle_n: ") + text);
    return PERC_EINVAL;
  };
  if (ntrials < 0) return bad("ntrials < 0");
  if (!shuffle_supported(N)) return bad("a list too long for the device shuffle (perc_shuffle_device_supported)");
  if (ntrials == 0) return PERC_OK;
  if (!seeds) return bad("seeds missing");
  hipSetDevice(h->device);
  return hip_status(dev_shuffle_run(h, kShuffleFree, ntrials, seeds, orders_out, ranks_out, N),
                    "perc_batch_shuffle_n");
}

int perc_scan_supported(int lattice, int m, int n, int pbc) {
  if (lattice != PERC_SQUARE && lattice != PERC_TRIANGULAR) return 0;
  if (m < 1 || n < 1 || (long long)m * n > kScanSites) return 0;
  return scan_supported(make_geom(lattice, m, n, pbc)) ? 1 : 0;
}

// perc_batch_scan (seeded = false: site_src / bond_src are order lists) and
// perc_batch_scan_seeded (true: seed lists, the orders shuffled on the device)
static int batch_scan_impl(const char* who, bool seeded, perc_ctx* h, int kind, int scan, int ntrials,
                           const int* site_src, const int* bond_src, const int* fixed,
                           perc_scan_item* out) {
  if (!h) return PERC_EINVAL;
  auto bad = [who](const char* text) {
    set_error(std::string(who) + ": " + text);
    return PERC_EINVAL;
  };
  if (!scan_supported(h->g)) return bad("lattice not supported by the scan kernel (perc_scan_supported)");
  if (kind != PERC_BOND && kind != PERC_SITE && kind != PERC_SITEBOND)
    return bad("kind PERC_BOND, PERC_SITE or PERC_SITEBOND only");
  if (kind == PERC_SITEBOND && scan != PERC_BOND && scan != PERC_SITE)
    return bad("scan PERC_BOND or PERC_SITE only");
  if (ntrials < 0) return bad("ntrials < 0");
  const bool need_s = kind != PERC_BOND, need_b = kind != PERC_SITE;
  if (seeded && !shuffle_lists_ok(h, kind)) return bad(kShuffleReach);
  if (ntrials == 0) return PERC_OK;
  if ((need_s && !site_src) || (need_b && !bond_src) || !out)
    return bad(seeded ? "a seed list the kind reads (or out) is missing"
                      : "an order list the kind reads (or out) is missing");
  if (kind == PERC_SITEBOND) {
    if (!fixed) return bad("PERC_SITEBOND needs fixed[ntrials]");
    const int cap = scan == PERC_BOND ? h->g.t : (int)h->nb;
    for (int i = 0; i < ntrials; ++i)
      if (fixed[i] < 0 || fixed[i] > cap)
        return bad("fixed outside 0..t (scan PERC_BOND) / 0..nb (scan PERC_SITE)");
  }
  hipSetDevice(h->device);
  BatchSources src;
  src.seeded = seeded;
  src.site_src = site_src;
  src.bond_src = bond_src;
  // a trial is an item: runs of consecutive trials whose rank arrays stay under 64 MB
  ItemRuns runs(nullptr, ntrials, ntrials, (int)std::min<long long>(ntrials, rank_run_cap(h, kind)));
  while (runs.next()) {
    const int i0 = runs.i0, k = runs.n;
    const int *d_s = nullptr, *d_b = nullptr;
    hipError_t e = provide_ranks(h, kind, src, i0, nullptr, k, &d_s, &d_b);
    if (e == hipSuccess)
      e = dev_scan_run(h, kind, scan, k, d_s, d_b, kind == PERC_SITEBOND ? fixed + i0 : nullptr, out + i0);
    if (e != hipSuccess) return hip_status(e, who);
  }
  return PERC_OK;
}

int perc_batch_scan(perc_ctx* h, int kind, int scan, int ntrials, const int* site_orders,
                    const int* bond_orders, const int* fixed, perc_scan_item* out) {
  return batch_scan_impl("perc_batch_scan", false, h, kind, scan, ntrials, site_orders, bond_orders, fixed,
                         out);
}

int perc_batch_scan_seeded(perc_ctx* h, int kind, int scan, int ntrials, const int* site_seeds,
                           const int* bond_seeds, const int* fixed, perc_scan_item* out) {
  return batch_scan_impl("perc_batch_scan_seeded", true, h, kind, scan, ntrials, site_seeds, bond_seeds,
                         fixed, out);
}

int perc_batch_clusters_supported(int lattice, int m, int n, int pbc, int nexact) {
  if (lattice != PERC_SQUARE && lattice != PERC_TRIANGULAR) return 0;
  if (m < 1 || n < 1 || (long long)m * n > kScanSites) return 0;
  return clusters_supported(make_geom(lattice, m, n, pbc), nexact) ? 1 : 0;
}

// perc_batch_clusters (seeded = false: site_src / bond_src are order lists)
// and perc_batch_clusters_seeded (true: seed lists, the orders shuffled on the
// device); geometry: the _geom forms, which also fill geom and rows (optional)
static int batch_clusters_impl(const char* who, bool seeded, perc_ctx* h, int kind, int ntrials,
                               const int* site_src, const int* bond_src, int nitems, const int* item_trial,
                               const int* item_nsites, const int* item_nbonds, int nexact,
                               perc_cluster_item* out, int* hist, bool geometry = false,
                               perc_cluster_geom* geom = nullptr, long long* rows = nullptr) {
  if (!h) return PERC_EINVAL;
  auto bad = [who](const char* text) {
    set_error(std::string(who) + ": " + text);
    return PERC_EINVAL;
  };
  if (kind != PERC_BOND && kind != PERC_SITE && kind != PERC_SITEBOND)
    return bad("kind PERC_BOND, PERC_SITE or PERC_SITEBOND only");
  if (ntrials < 0 || nitems < 0) return bad("ntrials or nitems < 0");
  if (nexact < 0 || nexact > kClusterExactMax) return bad("nexact outside 0..1024");
  if (!clusters_supported(h->g, nexact))
    return bad("lattice not supported by the cluster kernel (perc_batch_clusters_supported)");
  if (geometry && !geometry_supported(h->g, nexact))
    return bad("lattice not supported by the cluster geometry: pbc = 0 only (perc_batch_geometry_supported)");
  if (geometry && nitems && !geom) return bad("geom missing");
  const bool need_s = kind != PERC_BOND, need_b = kind != PERC_SITE;
  if (const char* text = check_items(need_s, need_b, seeded, ntrials, site_src, bond_src, nitems, item_trial,
                                     item_nsites, item_nbonds, out, h->g.t, (int)h->nb))
    return bad(text);
  if (seeded && !shuffle_lists_ok(h, kind)) return bad(kShuffleReach);
  if (nitems == 0) return PERC_OK;
  hipSetDevice(h->device);
  BatchSources src;
  src.seeded = seeded;
  src.site_src = site_src;
  src.bond_src = bond_src;
  // runs whose rank arrays and histogram rows (with the geometry's records
  // and octave rows, where asked) each stay under 64 MB
  const long long nh = (long long)nexact + 32;
  const long long per_item =
      4 * nh + (geometry ? (long long)sizeof(perc_cluster_geom) + (rows ? 8LL * kGeomRowWords : 0) : 0);
  ItemRuns runs(item_trial, nitems, ntrials,
                (int)std::min({(long long)nitems, rank_run_cap(h, kind), (64LL << 20) / per_item}));
  while (runs.next()) {
    const int i0 = runs.i0;
    const int *d_s = nullptr, *d_b = nullptr;
    hipError_t e = provide_ranks(h, kind, src, 0, runs.used.data(), (int)runs.used.size(), &d_s, &d_b);
    if (e == hipSuccess)
      e = dev_clusters_run(h, kind, runs.n, d_s, d_b, runs.local.data(), need_s ? item_nsites + i0 : nullptr,
                           need_b ? item_nbonds + i0 : nullptr, nexact, out + i0,
                           hist ? hist + (size_t)i0 * nh : nullptr, geometry ? geom + i0 : nullptr,
                           geometry && rows ? rows + (size_t)i0 * kGeomRowWords : nullptr);
    if (e != hipSuccess) return hip_status(e, who);
  }
  return PERC_OK;
}

int perc_batch_clusters(perc_ctx* h, int kind, int ntrials, const int* site_orders, const int* bond_orders,
                        int nitems, const int* item_trial, const int* item_nsites, const int* item_nbonds,
                        int nexact, perc_cluster_item* out, int* hist) {
  return batch_clusters_impl("perc_batch_clusters", false, h, kind, ntrials, site_orders, bond_orders, nitems,
                             item_trial, item_nsites, item_nbonds, nexact, out, hist);
}

int perc_batch_clusters_seeded(perc_ctx* h, int kind, int ntrials, const int* site_seeds,
                               const int* bond_seeds, int nitems, const int* item_trial,
                               const int* item_nsites, const int* item_nbonds, int nexact,
                               perc_cluster_item* out, int* hist) {
  return batch_clusters_impl("perc_batch_clusters_seeded", true, h, kind, ntrials, site_seeds, bond_seeds,
                             nitems, item_trial, item_nsites, item_nbonds, nexact, out, hist);
}

int perc_batch_geometry_supported(int lattice, int m, int n, int pbc, int nexact) {
  if (lattice != PERC_SQUARE && lattice != PERC_TRIANGULAR) return 0;
  if (m < 1 || n < 1 || (long long)m * n > kScanSites) return 0;
  return geometry_supported(make_geom(lattice, m, n, pbc), nexact) ? 1 : 0;
}

int perc_batch_clusters_geom(perc_ctx* h, int kind, int ntrials, const int* site_orders, const int* bond_orders,
                             int nitems, const int* item_trial, const int* item_nsites, const int* item_nbonds,
                             int nexact, perc_cluster_item* out, int* hist, perc_cluster_geom* geom,
                             long long* rows) {
  return batch_clusters_impl("perc_batch_clusters_geom", false, h, kind, ntrials, site_orders, bond_orders, nitems,
                             item_trial, item_nsites, item_nbonds, nexact, out, hist, true, geom, rows);
}

int perc_batch_clusters_geom_seeded(perc_ctx* h, int kind, int ntrials, const int* site_seeds,
                                    const int* bond_seeds, int nitems, const int* item_trial,
                                    const int* item_nsites, const int* item_nbonds, int nexact,
                                    perc_cluster_item* out, int* hist, perc_cluster_geom* geom, long long* rows) {
  return batch_clusters_impl("perc_batch_clusters_geom_seeded", true, h, kind, ntrials, site_seeds, bond_seeds,
                             nitems, item_trial, item_nsites, item_nbonds, nexact, out, hist, true, geom, rows);
}

}  // extern "C"
