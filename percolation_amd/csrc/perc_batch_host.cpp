// perc_batch_host.cpp -- host side of the batch path (include/perc.h:
// perc_batch_supported, perc_batch_bondc, perc_batch_cond_supported,
// perc_batch_cond, perc_batch_large_supported, perc_set_batch_large,
// perc_scan_supported, perc_batch_scan and the seeded forms
// perc_batch_shuffle, perc_batch_scan_seeded, perc_batch_cond_seeded, and the
// weighted perc_batch_weighted_supported, perc_batch_cond_weighted,
// perc_batch_twister, and the cluster tables' perc_batch_clusters_supported,
// perc_batch_clusters, perc_batch_clusters_seeded, and the current
// distributions' perc_batch_currents_supported, perc_batch_cond_currents,
// perc_batch_cond_currents_seeded, perc_current_stats_host):
// argument checks, the orders' inverse permutations, the
// launch geometry and LDS layouts, the fold of the terminal currents and the
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

// rank[tr * N + id - 1] = position of id in trial tr's order of N + 1 entries
// (the spill slot 0 takes a position and is no element; INT_MAX: absent)
static void order_ranks(int ntrials, int N, const int* orders, int* rank) {
  std::fill(rank, rank + (size_t)ntrials * N, INT_MAX);
  for (int tr = 0; tr < ntrials; ++tr) {
    const int* o = orders + (size_t)tr * (N + 1);
    int* r = rank + (size_t)tr * N;
    for (int pos = 0; pos <= N; ++pos) {
      const int id = o[pos];
      if (id >= 1 && id <= N && r[id - 1] == INT_MAX) r[id - 1] = pos;
    }
  }
}

int batch_upload_orders(perc_ctx* h, int ntrials, const int* orders) {
  const int nb = (int)h->nb;
  hipSetDevice(h->device);
  std::vector<int> rank((size_t)ntrials * nb);
  order_ranks(ntrials, nb, orders, rank.data());
  hipError_t e = dev_batch_upload(h, ntrials, rank.data());
  if (e != hipSuccess) return hip_status(e, "perc_batch_bondc/upload");
  return PERC_OK;
}

int batch_upload_site_orders(perc_ctx* h, int ntrials, const int* site_orders) {
  const int t = h->g.t;
  hipSetDevice(h->device);
  std::vector<int> rank((size_t)ntrials * t);
  order_ranks(ntrials, t, site_orders, rank.data());
  hipError_t e = dev_batch_upload_sites(h, ntrials, rank.data());
  if (e != hipSuccess) return hip_status(e, "perc_batch_cond/upload");
  return PERC_OK;
}

// the first cnt entries of an order of N + 1 as perc_occupy takes them: the
// whole order (cnt > N) with the spill slot dropped
static bool occupy_prefix(const int* o, int cnt, int N, std::vector<int>* list, const int** src,
                          int* len) {
  *src = o;
  *len = cnt;
  if (cnt <= N) return true;
  list->clear();
  for (int k = 0; k < cnt; ++k)
    if (o[k] != 0) list->push_back(o[k]);
  if ((int)list->size() > N) return false;
  *src = list->data();
  *len = (int)list->size();
  return true;
}

int batch_run_items_kind(perc_ctx* h, int kind, int cur_rule, const int* site_orders,
                         const int* bond_orders, int nitems, const int* item_trial,
                         const int* item_nsites, const int* item_nbonds, int solve, bool replay,
                         double Va, double g0, double leak, int itol, double tol, int itmax,
                         perc_batch_item* out, const int* site_seeds, const int* bond_seeds,
                         const BatchWeights* wts, const BatchFields* fld) {
  const int nb = (int)h->nb, m = h->g.m, t = h->g.t;
  const size_t N = (size_t)h->N;
  const int rule = kind;  // (PERC_RULE_* of a kind has the kind's number)
  const bool need_s = kind != PERC_BOND, need_b = kind != PERC_SITE;
  const char* who = kind == PERC_BOND && cur_rule == PERC_CUR_FORTRAN ? "perc_batch_bondc" : "perc_batch_cond";
  hipSetDevice(h->device);
  hipError_t e;
  const bool literal = h->dot_order != PERC_DOT_FAST;
  // launches of bounded size (the iout rows: 16 m bytes per item)
  int chunk = std::max(1, std::min(16384, (int)((64LL << 20) / (16LL * m))));
  // ... and the weighted kernel's rows (its draws, its scratch: 8 nb bytes per item each)
  if (wts) chunk = std::max(1, std::min(chunk, (int)((64LL << 20) / (8LL * (nb + 16)))));
  // ... and the interior voltages (8 N bytes per item)
  if (fld && fld->vint) chunk = std::max(1, std::min(chunk, (int)((64LL << 20) / (16LL * m + 8LL * (long long)N))));
  std::vector<BatchOut> bo((size_t)std::min(nitems, chunk));
  // a fallback item's record on the host: the bond list, the mask, the voltages
  std::vector<int> fb1, fb2, canon;
  std::vector<unsigned char> focc_s, focc_b, fmask;
  std::vector<double> fvint;
  std::vector<double> iout(solve ? bo.size() * 2 * (size_t)m : 0);
  std::vector<int> slist, blist, sregen, bregen;
  for (int i0 = 0; i0 < nitems; i0 += chunk) {
    const int n = std::min(chunk, nitems - i0);
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
    e = dev_batch_run(h, kind, cur_rule, n, item_trial + i0, need_s ? item_nsites + i0 : nullptr,
                      need_b ? item_nbonds + i0 : nullptr, solve ? 1 : 0, Va, g0, leak, itol, tol, itmax,
                      literal, bo.data(), iout.data(), wts || fld ? false : h->batch_large, wts ? &wc : nullptr,
                      fld ? &fc : nullptr);
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
      if (b.fallback && replay) {
        // several clusters span: the reference's lowest-label rule through
        // the single path, on the context
        const int tr = item_trial[i0 + i];
        const int *ssrc = nullptr, *bsrc = nullptr;
        int slen = 0, blen = 0;
        const int* so = need_s && site_orders ? site_orders + (size_t)tr * (t + 1) : nullptr;
        const int* bo = need_b && bond_orders ? bond_orders + (size_t)tr * (nb + 1) : nullptr;
        if (need_s && !so) {  // the seeded call: this trial's order, on the host
          if (!site_seeds) return PERC_EINVAL;
          sregen.resize((size_t)t + 1);
          perc_shuffle_seeded(site_seeds[tr], t, sregen.data());
          so = sregen.data();
        }
        if (need_b && !bo) {
          if (!bond_seeds) return PERC_EINVAL;
          bregen.resize((size_t)nb + 1);
          perc_shuffle_seeded(bond_seeds[tr], nb, bregen.data());
          bo = bregen.data();
        }
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
          if (!rc) rc = perc_conductance(h, rule, cur_rule, Va, g0, leak, itol, tol, itmax, &res, vrow);
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
            rc = perc_current_stats_host(h->g.lattice, m, h->g.n, h->g.pbc, fmask.data(), vrow, Va, g0, fld->cut,
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
  return batch_run_items_kind(h, PERC_BOND, PERC_CUR_FORTRAN, nullptr, orders, nitems, item_trial, nullptr,
                              item_count, solve, replay, Va, g0, leak, itol, tol, itmax, out);
}

int batch_scan_uploaded(perc_ctx* h, int ntrials, perc_scan_item* out) {
  hipSetDevice(h->device);
  int have = 0;
  const int* d_rank = dev_batch_ranks(h, &have);
  if (!d_rank || have < ntrials) {
    set_error("batch_scan_uploaded: no uploaded group of that many trials");
    return PERC_ESTATE;
  }
  return hip_status(dev_scan_run(h, PERC_BOND, PERC_BOND, ntrials, nullptr, d_rank, nullptr, out),
                    "perc_batch_scan");
}

}  // namespace perc

using namespace perc;

extern "C" {

int perc_batch_supported(int lattice, int m, int n, int pbc) {
  if (lattice != PERC_SQUARE && lattice != PERC_TRIANGULAR) return 0;
  if (m < 1 || n < 1 || (long long)m * n >= (1LL << 31) - 16) return 0;
  return batch_supported(make_geom(lattice, m, n, pbc)) ? 1 : 0;
}

int perc_batch_bondc(perc_ctx* h, int ntrials, const int* orders, int nitems, const int* item_trial,
                     const int* item_count, int solve, double Va, double g0, double leak, int itol,
                     double tol, int itmax, perc_batch_item* out) {
  if (!h || ntrials < 0 || nitems < 0 || (ntrials && !orders) ||
      (nitems && (!item_trial || !item_count || !out)) || itmax < 0)
    return PERC_EINVAL;
  if (solve && itol != 1 && itol != 2) {
    set_error("perc_batch_bondc: itol 1 or 2 only");
    return PERC_EINVAL;
  }
  if (h->batch_large) {
    if (!batch_large_supported(h->g, PERC_BOND)) {
      set_error("perc_batch_bondc: lattice not supported by the large batch kernel "
                "(perc_batch_large_supported)");
      return PERC_EINVAL;
    }
  } else if (!batch_supported(h->g)) {
    set_error("perc_batch_bondc: lattice not supported by the batch kernel (perc_batch_supported)");
    return PERC_EINVAL;
  }
  const int nb = (int)h->nb;
  for (int i = 0; i < nitems; ++i)
    if (item_trial[i] < 0 || item_trial[i] >= ntrials || item_count[i] < 0 || item_count[i] > nb + 1) {
      set_error("perc_batch_bondc: item_trial outside 0..ntrials-1 or item_count outside 0..nb+1");
      return PERC_EINVAL;
    }
  if (nitems == 0) return PERC_OK;
  int rc = batch_upload_orders(h, ntrials, orders);
  if (rc) return rc;
  return batch_run_items(h, orders, nitems, item_trial, item_count, solve, true, Va, g0, leak, itol,
                         tol, itmax, out);
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

// perc_batch_cond (seeded = false: site_src / bond_src are order lists) and
// perc_batch_cond_seeded (true: seed lists, the orders shuffled on the device)
static int batch_cond_impl(const char* who, bool seeded, perc_ctx* h, int kind, int rule, int cur_rule,
                           int ntrials, const int* site_src, const int* bond_src, int nitems,
                           const int* item_trial, const int* item_nsites, const int* item_nbonds,
                           int solve, double Va, double g0, double leak, int itol, double tol, int itmax,
                           perc_batch_item* out, const BatchWeights* wts = nullptr,
                           const BatchFields* fld = nullptr) {
  if (!h) return PERC_EINVAL;
  auto bad = [who](const char* text) {
    set_error(std::string(who) + ": " + text);
    return PERC_EINVAL;
  };
  const bool pair = (kind == PERC_BOND && rule == PERC_RULE_BOND) ||
                    (kind == PERC_SITE && rule == PERC_RULE_SITE) ||
                    (kind == PERC_SITEBOND && rule == PERC_RULE_MIXED);
  if (!pair)
    return bad("kind / rule PERC_BOND / PERC_RULE_BOND, PERC_SITE / PERC_RULE_SITE or PERC_SITEBOND / "
               "PERC_RULE_MIXED only");
  if (cur_rule != PERC_CUR_FORTRAN && cur_rule != PERC_CUR_MATLAB)
    return bad("cur_rule PERC_CUR_FORTRAN or PERC_CUR_MATLAB only");
  if (ntrials < 0 || nitems < 0) return bad("ntrials or nitems < 0");
  if (itmax < 0) return bad("itmax < 0");
  if (solve && itol != 1 && itol != 2) return bad("itol 1 or 2 only");
  if (fld) {  // the default kernel only: the perc_set_batch_large flag is not read
    if (nitems && !fld->cur) return bad("cur missing");
    if (!(fld->cut >= 0.0 && fld->cut <= 1.0)) return bad("cut outside [0, 1]");
    if (!batch_supported(h->g, kind))
      return bad("lattice not supported by the batch kernel for this kind (perc_batch_currents_supported)");
  } else if (wts) {  // its own kernel: the perc_set_batch_large flag is not read
    if (!batch_w_supported(h->g, kind))
      return bad("lattice not supported by the weighted batch kernel for this kind "
                 "(perc_batch_weighted_supported)");
  } else if (h->batch_large) {
    if (!batch_large_supported(h->g, kind))
      return bad("lattice not supported by the large batch kernel for this kind "
                 "(perc_batch_large_supported)");
  } else if (!batch_supported(h->g, kind)) {
    return bad("lattice not supported by the batch kernel for this kind (perc_batch_cond_supported)");
  }
  const bool need_s = kind != PERC_BOND, need_b = kind != PERC_SITE;
  if (ntrials && ((need_s && !site_src) || (need_b && !bond_src)))
    return bad(seeded ? "a seed list the kind reads is missing" : "an order list the kind reads is missing");
  if (nitems && (!item_trial || !out || (need_s && !item_nsites) || (need_b && !item_nbonds)))
    return bad("item_trial, out or a count list the kind reads is missing");
  const int t = h->g.t, nb = (int)h->nb;
  for (int i = 0; i < nitems; ++i) {
    if (item_trial[i] < 0 || item_trial[i] >= ntrials) return bad("item_trial outside 0..ntrials-1");
    if (need_s && (item_nsites[i] < 0 || item_nsites[i] > t + 1)) return bad("item_nsites outside 0..t+1");
    if (need_b && (item_nbonds[i] < 0 || item_nbonds[i] > nb + 1)) return bad("item_nbonds outside 0..nb+1");
  }
  if (seeded && ((need_s && !shuffle_supported(t)) || (need_b && !shuffle_supported(nb))))
    return bad("a list too long for the device shuffle (perc_shuffle_device_supported)");
  if (nitems == 0) return PERC_OK;
  if (seeded) {
    hipSetDevice(h->device);
    if (need_b) {
      const hipError_t e = dev_shuffle_run(h, PERC_BOND, ntrials, bond_src, nullptr, nullptr);
      if (e != hipSuccess) return hip_status(e, who);
    }
    if (need_s) {
      const hipError_t e = dev_shuffle_run(h, PERC_SITE, ntrials, site_src, nullptr, nullptr);
      if (e != hipSuccess) return hip_status(e, who);
    }
    return batch_run_items_kind(h, kind, cur_rule, nullptr, nullptr, nitems, item_trial, item_nsites,
                                item_nbonds, solve, true, Va, g0, leak, itol, tol, itmax, out, site_src,
                                bond_src, wts, fld);
  }
  int rc = need_b ? batch_upload_orders(h, ntrials, bond_src) : PERC_OK;
  if (!rc && need_s) rc = batch_upload_site_orders(h, ntrials, site_src);
  if (rc) return rc;
  return batch_run_items_kind(h, kind, cur_rule, site_src, bond_src, nitems, item_trial, item_nsites,
                              item_nbonds, solve, true, Va, g0, leak, itol, tol, itmax, out, nullptr, nullptr,
                              wts, fld);
}

int perc_batch_cond(perc_ctx* h, int kind, int rule, int cur_rule, int ntrials, const int* site_orders,
                    const int* bond_orders, int nitems, const int* item_trial, const int* item_nsites,
                    const int* item_nbonds, int solve, double Va, double g0, double leak, int itol,
                    double tol, int itmax, perc_batch_item* out) {
  return batch_cond_impl("perc_batch_cond", false, h, kind, rule, cur_rule, ntrials, site_orders,
                         bond_orders, nitems, item_trial, item_nsites, item_nbonds, solve, Va, g0, leak,
                         itol, tol, itmax, out);
}

int perc_batch_cond_seeded(perc_ctx* h, int kind, int rule, int cur_rule, int ntrials,
                           const int* site_seeds, const int* bond_seeds, int nitems,
                           const int* item_trial, const int* item_nsites, const int* item_nbonds,
                           int solve, double Va, double g0, double leak, int itol, double tol, int itmax,
                           perc_batch_item* out) {
  return batch_cond_impl("perc_batch_cond_seeded", true, h, kind, rule, cur_rule, ntrials, site_seeds,
                         bond_seeds, nitems, item_trial, item_nsites, item_nbonds, solve, Va, g0, leak,
                         itol, tol, itmax, out);
}

int perc_batch_currents_supported(int kind, int lattice, int m, int n, int pbc) {
  return perc_batch_cond_supported(kind, lattice, m, n, pbc);
}

int perc_batch_cond_currents(perc_ctx* h, int kind, int rule, int cur_rule, int ntrials,
                             const int* site_orders, const int* bond_orders, int nitems,
                             const int* item_trial, const int* item_nsites, const int* item_nbonds,
                             double Va, double g0, double leak, int itol, double tol, int itmax,
                             perc_batch_item* out, double cut, perc_batch_currents* cur, double* vint_out) {
  BatchFields fld;
  fld.cut = cut;
  fld.cur = cur;
  fld.vint = vint_out;
  return batch_cond_impl("perc_batch_cond_currents", false, h, kind, rule, cur_rule, ntrials, site_orders,
                         bond_orders, nitems, item_trial, item_nsites, item_nbonds, 1, Va, g0, leak, itol, tol,
                         itmax, out, nullptr, &fld);
}

int perc_batch_cond_currents_seeded(perc_ctx* h, int kind, int rule, int cur_rule, int ntrials,
                                    const int* site_seeds, const int* bond_seeds, int nitems,
                                    const int* item_trial, const int* item_nsites, const int* item_nbonds,
                                    double Va, double g0, double leak, int itol, double tol, int itmax,
                                    perc_batch_item* out, double cut, perc_batch_currents* cur,
                                    double* vint_out) {
  BatchFields fld;
  fld.cut = cut;
  fld.cur = cur;
  fld.vint = vint_out;
  return batch_cond_impl("perc_batch_cond_currents_seeded", true, h, kind, rule, cur_rule, ntrials, site_seeds,
                         bond_seeds, nitems, item_trial, item_nsites, item_nbonds, 1, Va, g0, leak, itol, tol,
                         itmax, out, nullptr, &fld);
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
  return batch_cond_impl("perc_batch_cond_weighted", false, h, kind, rule, cur_rule, ntrials, site_orders,
                         bond_orders, nitems, item_trial, item_nsites, item_nbonds, solve, Va, g0, leak,
                         itol, tol, itmax, out, &wts);
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
  const int t = h->g.t, nb = (int)h->nb;
  if (seeded && ((need_s && !shuffle_supported(t)) || (need_b && !shuffle_supported(nb))))
    return bad("a list too long for the device shuffle (perc_shuffle_device_supported)");
  if (ntrials == 0) return PERC_OK;
  if ((need_s && !site_src) || (need_b && !bond_src) || !out)
    return bad(seeded ? "a seed list the kind reads (or out) is missing"
                      : "an order list the kind reads (or out) is missing");
  if (kind == PERC_SITEBOND) {
    if (!fixed) return bad("PERC_SITEBOND needs fixed[ntrials]");
    const int cap = scan == PERC_BOND ? t : nb;
    for (int i = 0; i < ntrials; ++i)
      if (fixed[i] < 0 || fixed[i] > cap)
        return bad("fixed outside 0..t (scan PERC_BOND) / 0..nb (scan PERC_SITE)");
  }
  hipSetDevice(h->device);
  // launches whose rank arrays stay under 64 MB of device memory
  const long long per = 4LL * ((need_s ? t : 0) + (need_b ? nb : 0));
  const int chunk = (int)std::max(1LL, std::min<long long>(ntrials, (64LL << 20) / per));
  std::vector<int> rank_s(need_s && !seeded ? (size_t)chunk * t : 0);
  std::vector<int> rank_b(need_b && !seeded ? (size_t)chunk * nb : 0);
  for (int i0 = 0; i0 < ntrials; i0 += chunk) {
    const int k = std::min(chunk, ntrials - i0);
    const int* fx = kind == PERC_SITEBOND ? fixed + i0 : nullptr;
    hipError_t e = hipSuccess;
    if (seeded) {
      // the chunk's ranks straight into the batch path's buffers, the scan over them
      if (need_s) e = dev_shuffle_run(h, PERC_SITE, k, site_src + i0, nullptr, nullptr);
      if (e == hipSuccess && need_b) e = dev_shuffle_run(h, PERC_BOND, k, bond_src + i0, nullptr, nullptr);
      int have_s = 0, have_b = 0;
      const int* d_s = need_s ? dev_batch_site_ranks(h, &have_s) : nullptr;
      const int* d_b = need_b ? dev_batch_ranks(h, &have_b) : nullptr;
      if (e == hipSuccess) e = dev_scan_run(h, kind, scan, k, d_s, d_b, fx, out + i0);
    } else {
      if (need_s) order_ranks(k, t, site_src + (size_t)i0 * (t + 1), rank_s.data());
      if (need_b) order_ranks(k, nb, bond_src + (size_t)i0 * (nb + 1), rank_b.data());
      e = dev_scan_upload_run(h, kind, scan, k, need_s ? rank_s.data() : nullptr,
                              need_b ? rank_b.data() : nullptr, fx, out + i0);
    }
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
// device).  A launch takes a run of items and the trials they name, numbered
// afresh in order of first use: a run of k items names at most k trials, so
// the bound on the run bounds the launch's rank arrays too.
static int batch_clusters_impl(const char* who, bool seeded, perc_ctx* h, int kind, int ntrials,
                               const int* site_src, const int* bond_src, int nitems, const int* item_trial,
                               const int* item_nsites, const int* item_nbonds, int nexact,
                               perc_cluster_item* out, int* hist) {
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
  const bool need_s = kind != PERC_BOND, need_b = kind != PERC_SITE;
  if (ntrials && ((need_s && !site_src) || (need_b && !bond_src)))
    return bad(seeded ? "a seed list the kind reads is missing" : "an order list the kind reads is missing");
  if (nitems && (!item_trial || !out || (need_s && !item_nsites) || (need_b && !item_nbonds)))
    return bad("item_trial, out or a count list the kind reads is missing");
  const int t = h->g.t, nb = (int)h->nb;
  for (int i = 0; i < nitems; ++i) {
    if (item_trial[i] < 0 || item_trial[i] >= ntrials) return bad("item_trial outside 0..ntrials-1");
    if (need_s && (item_nsites[i] < 0 || item_nsites[i] > t + 1)) return bad("item_nsites outside 0..t+1");
    if (need_b && (item_nbonds[i] < 0 || item_nbonds[i] > nb + 1)) return bad("item_nbonds outside 0..nb+1");
  }
  if (seeded && ((need_s && !shuffle_supported(t)) || (need_b && !shuffle_supported(nb))))
    return bad("a list too long for the device shuffle (perc_shuffle_device_supported)");
  if (nitems == 0) return PERC_OK;
  hipSetDevice(h->device);
  // launches whose rank arrays and histogram rows each stay under 64 MB
  const long long per = 4LL * ((need_s ? t : 0) + (need_b ? nb : 0));
  const long long nh = (long long)nexact + 32;
  const int chunk = (int)std::max(1LL, std::min({(long long)nitems, (64LL << 20) / per, (64LL << 20) / (4 * nh)}));
  std::vector<int> local((size_t)ntrials, -1), used, ltrial((size_t)chunk), seeds_s, seeds_b;
  for (int i0 = 0; i0 < nitems; i0 += chunk) {
    const int n = std::min(chunk, nitems - i0);
    for (int tr : used) local[tr] = -1;
    used.clear();
    for (int i = 0; i < n; ++i) {
      const int tr = item_trial[i0 + i];
      if (local[tr] < 0) {
        local[tr] = (int)used.size();
        used.push_back(tr);
      }
      ltrial[i] = local[tr];
    }
    const int k = (int)used.size();
    const int* ns = need_s ? item_nsites + i0 : nullptr;
    const int* nbc = need_b ? item_nbonds + i0 : nullptr;
    int* hrow = hist ? hist + (size_t)i0 * nh : nullptr;
    hipError_t e = hipSuccess;
    if (seeded) {
      // the run's trials shuffled straight into the batch path's rank buffers
      if (need_s) {
        seeds_s.resize(k);
        for (int j = 0; j < k; ++j) seeds_s[j] = site_src[used[j]];
        e = dev_shuffle_run(h, PERC_SITE, k, seeds_s.data(), nullptr, nullptr);
      }
      if (e == hipSuccess && need_b) {
        seeds_b.resize(k);
        for (int j = 0; j < k; ++j) seeds_b[j] = bond_src[used[j]];
        e = dev_shuffle_run(h, PERC_BOND, k, seeds_b.data(), nullptr, nullptr);
      }
      int have_s = 0, have_b = 0;
      const int* d_s = need_s ? dev_batch_site_ranks(h, &have_s) : nullptr;
      const int* d_b = need_b ? dev_batch_ranks(h, &have_b) : nullptr;
      if (e == hipSuccess)
        e = dev_clusters_run(h, kind, n, d_s, d_b, ltrial.data(), ns, nbc, nexact, out + i0, hrow);
    } else {
      int *rank_s = nullptr, *rank_b = nullptr;
      e = dev_clusters_stage(h, need_s ? (size_t)k * t : 0, need_b ? (size_t)k * nb : 0, &rank_s, &rank_b);
      if (e != hipSuccess) return hip_status(e, who);
      if (need_s)
        for (int j = 0; j < k; ++j)
          order_ranks(1, t, site_src + (size_t)used[j] * (t + 1), rank_s + (size_t)j * t);
      if (need_b)
        for (int j = 0; j < k; ++j)
          order_ranks(1, nb, bond_src + (size_t)used[j] * (nb + 1), rank_b + (size_t)j * nb);
      e = dev_clusters_upload_run(h, kind, k, need_s ? rank_s : nullptr, need_b ? rank_b : nullptr, n,
                                  ltrial.data(), ns, nbc, nexact, out + i0, hrow);
    }
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

}  // extern "C"
