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
//
// The GEOM instantiations go on to the clusters' geometry (include/perc.h,
// perc_cluster_geom): member sites per root, then the gyration sums
// G_c = n_c sum |r_i|^2 - |sum r_i|^2 in integers, summed over all clusters,
// the spanning ones and per octave of n_c, and G_c of the largest cluster and
// of the span_root cluster -- a few more passes over LDS (cluster_geometry).
#include <climits>
#include <type_traits>

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

// ... and what the GEOM instantiations take beside it
struct ClusterGeomArgs : ClusterArgs {
  perc_cluster_geom* geom;
  long long* rows;  // nitems x kGeomRowWords, or NULL
  int oGeo;         // kGeomWords words of 8 bytes
};

constexpr int kSums = 7;  // nclusters, nlone, nspan, s1, s2, span_s1, span_s2

// the geometry words: the octave rows at 0, then
constexpr int kGwSums = kGeomRowWords;  // 12 workgroup sums (cluster_geometry's order)
constexpr int kGwKey = kGwSums + 12;    // max over the roots of (n_c << 32 | INT_MAX - root)
constexpr int kGwSpan = kGwKey + 1;     // the record's span_root

// the lanes' v[0..N) summed over the wave, then lane 0's atomicAdd into w[0..N)
template <int N>
__device__ __forceinline__ void wave_sums_to_lds(long long (&v)[N], unsigned long long* w) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] += __shfl_xor(v[j], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) atomicAdd(&w[j], (unsigned long long)v[j]);
  }
}

// The geometry record and octave rows of the labeled item (parent[] final
// roots, link[] bit 7 the site and mixed kinds' member sites, flag[] the
// spanning roots, gw[0 .. kGwKey] zero, gw[kGwSpan] the record's span_root,
// written before the barrier this starts with).  size[] and the low link bits
// are dead by now and reused: size[root] holds n_c, then the clusters' column
// sums, then their row sums; a root's link byte becomes bit 7 | spanning << 6
// | octave.  Coordinates: x = column (weight wx = 3 on the triangular lattice,
// else 1), y = row on the square lattice, 2 row - (column & 1) + 1 >= 0 on the
// triangular one.  Every product that can pass 2^31 is formed in 64 bits; all
// sums are integers, so any association gives the same result.  Every barrier
// is reached by every thread.
template <int NT, int KIND>
__device__ __forceinline__ void cluster_geometry(const Geom& g, int item, const int* parent, int* size,
                                                 uint8_t* link, const uint8_t* flag, unsigned long long* gw,
                                                 perc_cluster_geom* geom, long long* rows) {
  const int m = g.m, T = g.t, t = threadIdx.x;
  const bool tri = g.lattice == kTriangular;
  const int wx = tri ? 3 : 1;
  auto coords = [&](int s, int* x, int* y) {
    const int r = div_m(g, s - 1);
    *x = s - 1 - r * m;
    *y = tri ? 2 * r - (*x & 1) + 1 : r;
  };
  __syncthreads();  // the record's read of size[], the row's reads of hist[]
  // bond kind: a member site is an end of an occupied bond -- not a root, or a root with bonds
  for (int s = t + 1; s <= T; s += NT) {
    if constexpr (KIND == PERC_BOND) link[s] = (parent[s] != s || size[s] > 0) ? 0x80 : 0;
    size[s] = 0;
  }
  __syncthreads();
  for (int s = t + 1; s <= T; s += NT)
    if (link[s] & 0x80) atomicAdd(&size[parent[s]], 1);
  __syncthreads();

  // ---- the roots: n_c sums, the octave rows' counts, the largest cluster
  {
    long long v[4] = {};  // n1, n2, span_n1, span_n2
    unsigned long long key = 0;
    for (int s = t + 1; s <= T; s += NT) {
      if (parent[s] != s || !(link[s] & 0x80)) continue;
      const int nc = size[s], b = 31 - __builtin_clz((unsigned)nc);  // (nc >= 1)
      const long long q = (long long)nc * nc;
      const bool sp = s <= m && flag[s];
      v[0] += nc;
      v[1] += q;
      if (sp) {
        v[2] += nc;
        v[3] += q;
      }
      atomicAdd(&gw[b], 1ull);
      atomicAdd(&gw[32 + b], (unsigned long long)q);
      key = max(key, (unsigned long long)nc << 32 | (unsigned)(INT_MAX - s));
      link[s] = (uint8_t)(0x80 | (sp ? 0x40 : 0) | b);
    }
    wave_sums_to_lds(v, gw + kGwSums);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) key = max(key, __shfl_xor(key, off, 64));
    if ((t & 63) == 0) atomicMax(&gw[kGwKey], key);
  }
  __syncthreads();
  const unsigned long long top = gw[kGwKey];
  const int big = top ? INT_MAX - (int)(unsigned)top : 0;
  const int sroot = (int)gw[kGwSpan];
  const int big_n = size[big], root_n = size[sroot];  // (size[0] == 0)

  // ---- the sites: sum of n_c |r_i|^2 (all, spanning, per octave: runs of one
  // octave in a register, one LDS atomic per run), the two named clusters' own sums
  long long v[8] = {};  // g2, span_g2, then sum |r|^2, sum x, sum y of big and of span_root
  {
    int cur = -1;
    unsigned long long acc = 0;
    for (int s = t + 1; s <= T; s += NT) {
      if (!(link[s] & 0x80)) continue;
      const int root = parent[s];
      const unsigned lr = link[root];
      int x, y;
      coords(s, &x, &y);
      const int q = wx * x * x + y * y;
      const long long nq = (long long)size[root] * q;
      v[0] += nq;
      if (lr & 0x40) v[1] += nq;
      const int b = lr & 31;
      if (b != cur) {
        if (cur >= 0) atomicAdd(&gw[64 + cur], acc);
        cur = b;
        acc = 0;
      }
      acc += (unsigned long long)nq;
      if (root == big) {
        v[2] += q;
        v[3] += x;
        v[4] += y;
      }
      if (root == sroot) {
        v[5] += q;
        v[6] += x;
        v[7] += y;
      }
    }
    if (cur >= 0) atomicAdd(&gw[64 + cur], acc);
  }
  // ---- minus |sum r_i|^2 per cluster: the column sums, then the row sums
#pragma unroll 1
  for (int ax = 0; ax < 2; ++ax) {
    __syncthreads();  // size[] is read no more
    for (int s = t + 1; s <= T; s += NT) size[s] = 0;
    __syncthreads();
    for (int s = t + 1; s <= T; s += NT) {
      if (!(link[s] & 0x80)) continue;
      int x, y;
      coords(s, &x, &y);
      atomicAdd(&size[parent[s]], ax ? y : x);
    }
    __syncthreads();
    for (int s = t + 1; s <= T; s += NT) {
      const unsigned lk = link[s];
      if (parent[s] != s || !(lk & 0x80)) continue;
      const long long c = size[s];
      const long long sq = c * c * (ax ? 1 : wx);
      v[0] -= sq;
      if (lk & 0x40) v[1] -= sq;
      atomicAdd(&gw[64 + (lk & 31)], (unsigned long long)-sq);
    }
  }
  wave_sums_to_lds(v, gw + kGwSums + 4);
  __syncthreads();
  if (t == 0) {
    const long long* w = reinterpret_cast<const long long*>(gw) + kGwSums;
    perc_cluster_geom o;
    o.n1 = (int)w[0];
    o.span_n1 = (int)w[2];
    o.big_root = big;
    o.big_n = big_n;
    o.root_n = root_n;
    o.pad = 0;
    o.n2 = w[1];
    o.g2 = w[4];
    o.span_n2 = w[3];
    o.span_g2 = w[5];
    o.big_g2 = big_n * w[6] - wx * w[7] * w[7] - w[8] * w[8];
    o.root_g2 = root_n * w[9] - wx * w[10] * w[10] - w[11] * w[11];
    geom[item] = o;
  }
  if (rows) {
    long long* __restrict__ row = rows + (size_t)item * kGeomRowWords;
    for (int k = t; k < kGeomRowWords; k += NT) row[k] = (long long)gw[k];
  }
}

// NT threads, sites t + 1, t + 1 + NT, .. (at most kScanSPT) per thread.
// Every loop bound is a kernel argument; lds_label's exit is a workgroup vote.
template <int NT, int KIND, bool GEOM>
__global__ __launch_bounds__(NT) void k_batch_clusters(std::conditional_t<GEOM, ClusterGeomArgs, ClusterArgs> a) {
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
  if constexpr (GEOM) {
    unsigned long long* gw = reinterpret_cast<unsigned long long*>(smem + a.oGeo);
    for (int k = t; k < kGwSpan; k += NT) gw[k] = 0;
  }
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
    if constexpr (GEOM) reinterpret_cast<unsigned long long*>(smem + a.oGeo)[kGwSpan] = (unsigned long long)root;
  }
  if (a.hist) {
    int* __restrict__ row = a.hist + (size_t)item * nh;
    for (int k = t; k < nh; k += NT) row[k] = hist[k];
  }
  if constexpr (GEOM)
    cluster_geometry<NT, KIND>(g, item, parent, size, link, flag,
                               reinterpret_cast<unsigned long long*>(smem + a.oGeo), a.geom, a.rows);
}

struct ClusterState {
  ItemLists<perc_cluster_item, 3> items;  // item_trial, then item_nsites, then item_nbonds
  int* d_hist = nullptr;
  size_t hist_cap = 0;
  perc_cluster_geom* d_geom = nullptr;  // (the GEOM launches' outputs)
  size_t geom_cap = 0;
  long long* d_rows = nullptr;
  size_t rows_cap = 0;
  int lds_attr[3][3] = {};  // dynamic LDS granted per instantiation
  int lds_attr_g[3][3] = {};
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
  (void)hipFree(S->d_geom);
  (void)hipFree(S->d_rows);
  delete S;
  h->clusters = nullptr;
}

hipError_t dev_clusters_run(perc_ctx* h, int kind, int nitems, const int* d_rank_s, const int* d_rank_b,
                            const int* item_trial, const int* item_nsites, const int* item_nbonds,
                            int nexact, perc_cluster_item* out, int* hist, perc_cluster_geom* geom,
                            long long* rows) {
  if (nitems == 0) return hipSuccess;
  ClusterState* S = cluster_state(h);
  hipStream_t st = h->stream;
  const size_t n = (size_t)nitems, nh = (size_t)nexact + 32;
  if (hist) HIP_TRY(grow(&S->d_hist, &S->hist_cap, n * nh));
  HIP_TRY(S->items.upload(n, {item_trial, kind != PERC_BOND ? item_nsites : nullptr,
                              kind != PERC_SITE ? item_nbonds : nullptr}, st));
  ClusterGeomArgs a;
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
  a.geom = nullptr;
  a.rows = nullptr;
  a.oGeo = 0;
  if (geom) {
    // (the kernel writes every item's record and rows; zeroed all the same, so
    // that nothing of an earlier launch can be read back)
    HIP_TRY(grow(&S->d_geom, &S->geom_cap, n));
    HIP_TRY(hipMemsetAsync(S->d_geom, 0, sizeof(perc_cluster_geom) * n, st));
    if (rows) {
      HIP_TRY(grow(&S->d_rows, &S->rows_cap, n * kGeomRowWords));
      HIP_TRY(hipMemsetAsync(S->d_rows, 0, sizeof(long long) * n * kGeomRowWords, st));
    }
    a.geom = S->d_geom;
    a.rows = rows ? S->d_rows : nullptr;
    a.L = cluster_geom_lds(h->g, nexact, &a.oGeo);
  }
  HIP_TRY(dispatch_threads(scan_threads(h->g.t), [&](auto nt, int slot) {
    return dispatch_kind_order(kind, false, [&](auto, auto kd) {
      if (geom)
        return launch_lds(&k_batch_clusters<nt(), kd(), true>, &S->lds_attr_g[slot][kd()], a, nitems, nt(), st,
                          "k_batch_clusters");
      return launch_lds(&k_batch_clusters<nt(), kd(), false>, &S->lds_attr[slot][kd()],
                        static_cast<const ClusterArgs&>(a), nitems, nt(), st, "k_batch_clusters");
    });
  }));
  HIP_TRY(hipMemcpyAsync(out, S->items.d_out, sizeof(perc_cluster_item) * n, hipMemcpyDeviceToHost, st));
  if (hist) HIP_TRY(hipMemcpyAsync(hist, S->d_hist, sizeof(int) * n * nh, hipMemcpyDeviceToHost, st));
  if (geom) HIP_TRY(hipMemcpyAsync(geom, S->d_geom, sizeof(perc_cluster_geom) * n, hipMemcpyDeviceToHost, st));
  if (geom && rows)
    HIP_TRY(hipMemcpyAsync(rows, S->d_rows, sizeof(long long) * n * kGeomRowWords, hipMemcpyDeviceToHost, st));
  return hipStreamSynchronize(st);  // (the item lists and the outputs are the caller's)
}

}  // namespace perc
