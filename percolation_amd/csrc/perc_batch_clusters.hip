// perc_batch_clusters.hip -- k_batch_clusters: one workgroup takes one
// (trial, nsites, nbonds) item to its cluster table, the c(label) every
// reference program writes: occupancy from the trial's rank arrays
// (lds_links), union-find labeling in LDS (lds_label), per-root sizes
// (lds_root_sizes), then one pass over the roots for the record (counts,
// moments, the spanning clusters' share) and the size histogram.  Many items
// per launch instead of occupy / label / label_numbers and a host replay for
// each.
//
// The clusters are the reference programs' non-empty c(label) entries; the
// phantom label the shuffle's spill slot opens (hazard H2) is no cluster:
//   PERC_BOND      a connected set of occupied bonds; size = its bonds
//   PERC_SITE      a connected set of occupied sites over the lattice's bonds
//                  (an isolated occupied site: size 1); size = its sites
//   PERC_SITEBOND  a component of occupied sites linked by occupied bonds with
//                  both end sites occupied; size = its sites plus every
//                  occupied bond with at least one end site in it
//                  (sitebond.f's count, replay_sitebond)
//   PERC_SITEBOND, lone bond: an occupied bond with both end sites empty;
//                  size 1, never spans; counted, not labeled
// The sizes do not depend on the order of occupation.  Spanning is
// k_span_top's rule, as in k_batch_scan; several clusters may span, the record
// sums over all of them.
#include <climits>

#include "perc_batch.h"
#include "perc_batch_uf.h"

namespace perc {
namespace {

struct ClusterArgs {
  Geom g;
  int nb, nexact;
  const int* bond_first;
  const int* rank_s;  // ntrials x t (site and mixed kinds)
  const int* rank_b;  // ntrials x nb (bond and mixed kinds)
  const int* item_trial;
  const int* item_nsites;  // (site and mixed kinds)
  const int* item_nbonds;  // (bond and mixed kinds)
  perc_cluster_item* out;
  int* hist;  // nitems x (nexact + 32), or NULL
  ClusterLds L;
};

constexpr int kSums = 7;  // nclusters, nlone, nspan, s1, s2, span_s1, span_s2

// NT threads, sites t + 1, t + 1 + NT, .. (at most kScanSPT) per thread.
// Every loop bound is a kernel argument; lds_label's exit is a workgroup vote.
template <int NT, int KIND>
__global__ __launch_bounds__(NT) void k_batch_clusters(ClusterArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Geom g = a.g;
  const int m = g.m, T = g.t, nexact = a.nexact, nh = a.nexact + 32;
  const int t = threadIdx.x;
  const int item = blockIdx.x;
  int* parent = reinterpret_cast<int*>(smem);
  int* size = reinterpret_cast<int*>(smem + a.L.oSize);
  uint8_t* link = reinterpret_cast<uint8_t*>(smem + a.L.oLink);
  uint8_t* flag = reinterpret_cast<uint8_t*>(smem + a.L.oFlag);
  int* hist = reinterpret_cast<int*>(smem + a.L.oHist);
  long long* red = reinterpret_cast<long long*>(smem + a.L.oRed);  // per wave: kSums sums, min root, max size

  const int trial = a.item_trial[item];
  const int* __restrict__ rs = KIND != PERC_BOND ? a.rank_s + (size_t)trial * T : nullptr;
  const int* __restrict__ rb = KIND != PERC_SITE ? a.rank_b + (size_t)trial * a.nb : nullptr;
  const int cs = KIND != PERC_BOND ? a.item_nsites[item] : 0;
  const int cb = KIND != PERC_SITE ? a.item_nbonds[item] : 0;

  lds_links<NT, KIND>(g, a.bond_first, rs, rb, cs, cb, parent, size, link);
  lds_label<NT>(g, a.bond_first, parent, [&](int, int s, int k, int, int) { return (link[s] >> k & 1) != 0; });

  for (int c = t; c <= m; c += NT) flag[c] = 0;
  for (int s = t; s <= T; s += NT) size[s] = 0;
  for (int k = t; k < nh; k += NT) hist[k] = 0;
  __syncthreads();
  // spanning (k_span_top's rule): a root <= m with a member in the top row
  for (int c = t; c < m; c += NT) {
    const int r = parent[T - m + 1 + c];
    if (r <= m) flag[r] = 1;
  }
  const int lone = lds_root_sizes<NT, KIND>(g, a.bond_first, rb, cb, parent, link, size);
  __syncthreads();

  // ---- the roots: histogram adds in LDS, the sums in registers
  long long v[kSums] = {};
  int mn = INT_MAX, mx = 0;
  for (int s = t + 1; s <= T; s += NT) {
    const int sz = size[s];
    if (parent[s] != s || sz <= 0) continue;
    const long long q = (long long)sz * sz;
    v[0] += 1;
    v[3] += sz;
    v[4] += q;
    mx = max(mx, sz);
    if (sz <= nexact) atomicAdd(&hist[sz - 1], 1);
    atomicAdd(&hist[nexact + 31 - __clz(sz)], 1);
    if (s <= m && flag[s]) {
      v[2] += 1;
      v[5] += sz;
      v[6] += q;
      mn = min(mn, s);
    }
  }
  if (lone) {  // (mixed kind) each a cluster of size 1
    v[0] += lone;
    v[1] += lone;
    v[3] += lone;
    v[4] += lone;
    mx = max(mx, 1);
    if (nexact >= 1) atomicAdd(&hist[0], lone);
    atomicAdd(&hist[nexact], lone);
  }
  // a wave butterfly, then the waves in order (integer sums: any association
  // gives the same result)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int j = 0; j < kSums; ++j) v[j] += __shfl_xor(v[j], off, 64);
    mn = min(mn, __shfl_xor(mn, off, 64));
    mx = max(mx, __shfl_xor(mx, off, 64));
  }
  if ((t & 63) == 0) {
    long long* w = red + (t >> 6) * (kSums + 2);
#pragma unroll
    for (int j = 0; j < kSums; ++j) w[j] = v[j];
    w[kSums] = mn;
    w[kSums + 1] = mx;
  }
  __syncthreads();
  if (t == 0) {
    long long sum[kSums] = {};
    long long rmin = INT_MAX, smax = 0;
#pragma unroll 1  // (unrolled, the 16 waves' words all live at once: scratch at 1024 threads)
    for (int wv = 0; wv < NT / 64; ++wv) {
      const long long* w = red + wv * (kSums + 2);
#pragma unroll
      for (int j = 0; j < kSums; ++j) sum[j] += w[j];
      rmin = min(rmin, w[kSums]);
      smax = max(smax, w[kSums + 1]);
    }
    const int root = sum[2] > 0 ? (int)rmin : 0;
    perc_cluster_item o;
    o.nclusters = (int)sum[0];
    o.nlone = (int)sum[1];
    o.nspan = (int)sum[2];
    o.span_root = root;
    o.span_size = root ? size[root] : 0;
    o.maxcs = (int)smax;
    o.s1 = sum[3];
    o.s2 = sum[4];
    o.span_s1 = sum[5];
    o.span_s2 = sum[6];
    a.out[item] = o;
  }
  if (a.hist) {
    int* __restrict__ row = a.hist + (size_t)item * nh;
    for (int k = t; k < nh; k += NT) row[k] = hist[k];
  }
}

struct ClusterState {
  ItemLists<perc_cluster_item, 3> items;  // item_trial, then item_nsites, then item_nbonds
  int* d_hist = nullptr;
  size_t hist_cap = 0;
  int lds_attr[3][3] = {};  // dynamic LDS granted per instantiation
};

ClusterState* cluster_state(perc_ctx* h) {
  if (!h->clusters) h->clusters = new ClusterState();
  return static_cast<ClusterState*>(h->clusters);
}

}  // namespace

void dev_clusters_free(perc_ctx* h) {
  ClusterState* S = static_cast<ClusterState*>(h->clusters);
  if (!S) return;
  S->items.release();
  (void)hipFree(S->d_hist);
  delete S;
  h->clusters = nullptr;
}

hipError_t dev_clusters_run(perc_ctx* h, int kind, int nitems, const int* d_rank_s, const int* d_rank_b,
                            const int* item_trial, const int* item_nsites, const int* item_nbonds,
                            int nexact, perc_cluster_item* out, int* hist) {
  if (nitems == 0) return hipSuccess;
  ClusterState* S = cluster_state(h);
  hipStream_t st = h->stream;
  const size_t n = (size_t)nitems, nh = (size_t)nexact + 32;
  if (hist) HIP_TRY(grow(&S->d_hist, &S->hist_cap, n * nh));
  HIP_TRY(S->items.upload(n, {item_trial, kind != PERC_BOND ? item_nsites : nullptr,
                              kind != PERC_SITE ? item_nbonds : nullptr}, st));
  ClusterArgs a;
  a.g = h->g;
  a.nb = (int)h->nb;
  a.nexact = nexact;
  a.bond_first = h->d.bond_first;
  a.rank_s = d_rank_s;
  a.rank_b = d_rank_b;
  a.item_trial = S->items.list(0, n);
  a.item_nsites = S->items.list(1, n);
  a.item_nbonds = S->items.list(2, n);
  a.out = S->items.d_out;
  a.hist = hist ? S->d_hist : nullptr;
  a.L = cluster_lds(h->g, nexact);
  HIP_TRY(dispatch_threads(scan_threads(h->g.t), [&](auto nt, int slot) {
    return dispatch_kind_order(kind, false, [&](auto, auto kd) {
      return launch_lds(&k_batch_clusters<nt(), kd()>, &S->lds_attr[slot][kd()], a, nitems, nt(), st,
                        "k_batch_clusters");
    });
  }));
  HIP_TRY(hipMemcpyAsync(out, S->items.d_out, sizeof(perc_cluster_item) * n, hipMemcpyDeviceToHost, st));
  if (hist) HIP_TRY(hipMemcpyAsync(hist, S->d_hist, sizeof(int) * n * nh, hipMemcpyDeviceToHost, st));
  return hipStreamSynchronize(st);  // (the item lists and the outputs are the caller's)
}

}  // namespace perc
