// perc_batch_scan.hip -- k_batch_scan: one workgroup takes one small-lattice
// trial of a threshold scan (bond_perc, site_perc, sb_perc, bs_perc's
// intended rule) through the whole bisection of perc_first_spanning /
// perc_first_spanning_mixed with no host round trip -- occupancy at a count
// from the trial's rank arrays, union-find labeling in LDS (lds_label), the
// spanning rule of k_span_top -- then labels once more at the first spanning
// count for the cluster sizes of k_cluster_sizes.  Many trials per launch
// instead of ~log2 N occupy / label / read-back rounds for each.
#include <climits>

#include "perc_batch.h"
#include "perc_batch_uf.h"

namespace perc {
namespace {

struct ScanArgs {
  Geom g;
  int nb, N;  // bonds; entries of the scanned list (nb or t)
  const int* bond_first;
  const int* rank_s;  // ntrials x t (site and mixed kinds)
  const int* rank_b;  // ntrials x nb (bond and mixed kinds)
  const int* fixed;   // ntrials (mixed kinds): occupied entries of the other list
  int scan;           // mixed kinds: PERC_BOND / PERC_SITE, the scanned list
  perc_scan_item* out;
  ScanLds L;
};

// NT threads, sites t + 1, t + 1 + NT, .. (at most kScanSPT) per thread.
// KIND: PERC_BOND / PERC_SITE / PERC_SITEBOND.
template <int NT, int KIND>
__global__ __launch_bounds__(NT) void k_batch_scan(ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Geom g = a.g;
  const int m = g.m, T = g.t, N = a.N;
  const int t = threadIdx.x;
  const int trial = blockIdx.x;
  int* parent = reinterpret_cast<int*>(smem);
  int* size = reinterpret_cast<int*>(smem + a.L.oSize);
  uint8_t* link = reinterpret_cast<uint8_t*>(smem + a.L.oLink);
  uint8_t* flag = reinterpret_cast<uint8_t*>(smem + a.L.oFlag);
  int* s_i = reinterpret_cast<int*>(smem + a.L.oInt);

  const int* __restrict__ rs = KIND != PERC_BOND ? a.rank_s + (size_t)trial * T : nullptr;
  const int* __restrict__ rb = KIND != PERC_SITE ? a.rank_b + (size_t)trial * a.nb : nullptr;
  const int fx = KIND == PERC_SITEBOND ? a.fixed[trial] : 0;
  const bool scan_sites = KIND == PERC_SITE || (KIND == PERC_SITEBOND && a.scan == PERC_SITE);

  int npass = 0, nlabel = 0;  // (probe builds report them)
  // ---- one labeling at scanned count c (uniform): an element is occupied
  // iff its position in the order < its list's count.  The ranks are read
  // once, into one link byte per site (lds_links); the hook passes read LDS
  // only.
  auto label = [&](int c) {
    const int cs = scan_sites ? c : fx;  // (site kinds)
    const int cb = scan_sites ? fx : c;  // (bond and mixed kinds)
    lds_links<NT, KIND>(g, a.bond_first, rs, rb, cs, cb, parent, size, link);
    npass += lds_label<NT>(g, a.bond_first, parent,
                           [&](int, int s, int k, int, int) { return (link[s] >> k & 1) != 0; });
    ++nlabel;
  };
  // ---- spanning (k_span_top's rule): a root <= m with a member in the top
  // row.  A top-row site s > m whose root is <= m was hooked, so it is a
  // member.  The result is the same in every thread.
  auto spans = [&]() {
    int f = 0;
    for (int c = t; c < m; c += NT) f |= parent[T - m + 1 + c] <= m ? 1 : 0;
    return __syncthreads_or(f) != 0;
  };

  // ---- the bisection of perc_first_spanning (spanning is monotone in c)
  label(N);
  int lo = 0, hi = spans() ? N : 0;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    label(mid);
    if (spans()) hi = mid;
    else lo = mid;
  }
  const int first = hi;

  // ---- at the first spanning count (N: nothing spans): the spanning roots
  // and the per-root sizes, one atomic per contributing site (k_cluster_sizes:
  // a site's occupied forward bonds, or the site itself)
  label(first ? first : N);
  if (t < 8) s_i[t] = t == 2 ? INT_MAX : 0;
  for (int c = t; c <= m; c += NT) flag[c] = 0;
  for (int s = t; s <= T; s += NT) size[s] = 0;
  __syncthreads();
  for (int c = t; c < m; c += NT) {
    const int r = parent[T - m + 1 + c];
    if (r <= m) flag[r] = 1;
  }
  if constexpr (KIND != PERC_SITEBOND)
    (void)lds_root_sizes<NT, KIND>(g, a.bond_first, rb, 0, parent, link, size);
  __syncthreads();
  {
    int nsp = 0, mn = INT_MAX, mx = 0;
    for (int c = t + 1; c <= m; c += NT)
      if (flag[c]) {
        ++nsp;
        mn = min(mn, c);
      }
    if (nsp) {
      atomicAdd(&s_i[1], nsp);
      atomicMin(&s_i[2], mn);
    }
    if constexpr (KIND != PERC_SITEBOND) {
      for (int s = t + 1; s <= T; s += NT) mx = max(mx, size[s]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off, 64));
      if ((t & 63) == 0 && mx) atomicMax(&s_i[3], mx);
    }
  }
  __syncthreads();
  if (t == 0) {
    const int nspan = s_i[1];
    const int root = nspan > 0 ? s_i[2] : 0;
    perc_scan_item o;
    o.first = first;
    o.maxcs = s_i[3];
    o.span_size = root && KIND != PERC_SITEBOND ? size[root] : 0;
    o.nspan = nspan;
#ifdef PERC_SCAN_PASSES  // probe build: hook / flatten passes and labelings of the trial instead of the sizes
    o.maxcs = npass;
    o.span_size = nlabel;
#else
    (void)npass;
    (void)nlabel;
#endif
    a.out[trial] = o;
  }
}

struct ScanState {
  ItemLists<perc_scan_item, 1> trials;  // fixed
  int lds_attr[3][3] = {};  // dynamic LDS granted per instantiation
};

ScanState* scan_state(perc_ctx* h) {
  if (!h->scan) h->scan = new ScanState();
  return static_cast<ScanState*>(h->scan);
}

}  // namespace

void dev_scan_free(perc_ctx* h) {
  ScanState* S = static_cast<ScanState*>(h->scan);
  if (!S) return;
  S->trials.release();
  delete S;
  h->scan = nullptr;
}

hipError_t dev_scan_run(perc_ctx* h, int kind, int scan, int ntrials, const int* d_rank_s,
                        const int* d_rank_b, const int* fixed, perc_scan_item* out) {
  if (ntrials == 0) return hipSuccess;
  ScanState* S = scan_state(h);
  hipStream_t st = h->stream;
  HIP_TRY(S->trials.upload((size_t)ntrials, {kind == PERC_SITEBOND ? fixed : nullptr}, st));
  ScanArgs a;
  a.g = h->g;
  a.nb = (int)h->nb;
  const bool sites = kind == PERC_SITE || (kind == PERC_SITEBOND && scan == PERC_SITE);
  a.N = sites ? h->g.t : (int)h->nb;
  a.bond_first = h->d.bond_first;
  a.rank_s = d_rank_s;
  a.rank_b = d_rank_b;
  a.fixed = S->trials.list(0, ntrials);
  a.scan = scan;
  a.out = S->trials.d_out;
  a.L = scan_lds(h->g);
  HIP_TRY(dispatch_threads(scan_threads(h->g.t), [&](auto nt, int slot) {
    return dispatch_kind_order(kind, false, [&](auto, auto kd) {
      return launch_lds(&k_batch_scan<nt(), kd()>, &S->lds_attr[slot][kd()], a, ntrials, nt(), st, "k_batch_scan");
    });
  }));
  HIP_TRY(hipMemcpyAsync(out, S->trials.d_out, sizeof(perc_scan_item) * ntrials, hipMemcpyDeviceToHost, st));
  return hipStreamSynchronize(st);  // (fixed and out are the caller's)
}

}  // namespace perc
