// perc_batch_uf.h -- the in-LDS union-find the one-workgroup kernels share
// (perc_batch_item.h: the conductance kernels' batch_front;
// perc_batch_scan.hip: k_batch_scan; perc_batch_clusters.hip:
// k_batch_clusters): the
// root walk and the hook / flatten passes over a bond predicate, and, for the
// scan and the cluster statistics, the link byte per site and the per-root
// sizes.
#pragma once
#include "perc_common.h"

namespace perc {
namespace {

// root of x (parents only decrease along a chain; hooks of other threads may
// land while it is walked: every value read is an ancestor at some moment)
__device__ __forceinline__ int lds_find(int* parent, int x) {
  while (true) {
    const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}

// Labeling of parent[0..T] (parent[s] == s on entry, written before a
// workgroup barrier): hook the larger root under the smaller over every
// forward bond (s, q = nn[k] > s, bond-list index id) that link(pass, s, k,
// q, id) accepts, flatten, until a pass hooks nothing (the flag is
// workgroup-uniform).  NT threads, sites t + 1, t + 1 + NT, ..; every parent
// is its root on return, after a barrier.  Returns the number of passes.
template <int NT, class Link>
__device__ __forceinline__ int lds_label(const Geom& g, const int* __restrict__ bond_first, int* parent,
                                         Link link) {
  const int m = g.m, T = g.t, t = threadIdx.x;
  for (int pass = 0;; ++pass) {
    int changed = 0;
    for (int s = t + 1; s < T; s += NT) {
      const int sr = div_m(g, s - 1);
      int nn[6];
      nearestn_rc(g, s, sr, s - 1 - sr * m, nn);
      int id = bond_first[s];
      for (int k = 0; k < g.scn; ++k) {
        const int q = nn[k];
        if (q <= s) continue;
        if (link(pass, s, k, q, id)) {
          const int ra = lds_find(parent, s), rb = lds_find(parent, q);
          if (ra != rb) {
            atomicMin(&parent[max(ra, rb)], min(ra, rb));
            changed = 1;
          }
        }
        ++id;
      }
    }
    changed = __syncthreads_or(changed);
    // each thread walks, then writes only its own entries
    for (int s = t + 1; s <= T; s += NT) {
      const int r = lds_find(parent, s);
      __hip_atomic_store(&parent[s], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (!changed) return pass + 1;
  }
}

// The occupancy of one labeling as one link byte per site (bit k: the forward
// bond to nearestn slot k connects; bit 7: member site -- the site and mixed
// kinds' occupied sites), from the trial's rank arrays: an element is occupied
// iff its position in the order < its list's count (cs sites, cb bonds).  Sets
// parent[s] = s too; size[] holds the site occupancy meanwhile (its words are
// free until lds_root_sizes).  Ends with a barrier: lds_label may follow, its
// predicate (link[s] >> k & 1).  KIND: PERC_BOND / PERC_SITE / PERC_SITEBOND.
template <int NT, int KIND>
__device__ __forceinline__ void lds_links(const Geom& g, const int* __restrict__ bond_first,
                                          const int* __restrict__ rs, const int* __restrict__ rb, int cs,
                                          int cb, int* parent, int* size, uint8_t* link) {
  const int m = g.m, T = g.t, t = threadIdx.x;
  for (int s = t; s <= T; s += NT) parent[s] = s;
  if constexpr (KIND != PERC_BOND) {
    // the site occupancy, for the neighbours' threads
    for (int s = t + 1; s <= T; s += NT) size[s] = rs[s - 1] < cs ? 1 : 0;
    __syncthreads();
  }
  for (int s = t + 1; s <= T; s += NT) {
    const int sr = div_m(g, s - 1);
    int nn[6];
    nearestn_rc(g, s, sr, s - 1 - sr * m, nn);
    unsigned lk = 0;
    bool on = true;
    if constexpr (KIND != PERC_BOND) {
      on = size[s] != 0;
      lk = on ? 0x80u : 0u;
    }
    if (on) {
      int id = bond_first[s];
      for (int k = 0; k < g.scn; ++k) {
        const int q = nn[k];
        if (q <= s) continue;
        bool con = true;
        if constexpr (KIND != PERC_BOND) con = size[q] != 0;
        if constexpr (KIND != PERC_SITE) con = con && rb[id] < cb;
        lk |= (con ? 1u : 0u) << k;
        ++id;
      }
    }
    link[s] = (uint8_t)lk;
  }
  __syncthreads();
}

// The per-root cluster sizes of a labeling (parent[] final roots, link[] as
// lds_links left it, size[0..T] zero on entry, after a barrier): one LDS
// atomicAdd per contributing site.  Bond kind: a site's occupied forward
// bonds; site kind: the site itself; mixed kind (sitebond.f's count): the
// site, plus each occupied forward bond with at least one occupied end, added
// to the root of its occupied end (the lower site's when both are: they share
// a root) -- the bond ranks are read once more for it.  Returns the thread's
// lone bonds (mixed kind: occupied, both ends empty; they are in no size[]).
// No barrier at the end.
template <int NT, int KIND>
__device__ __forceinline__ int lds_root_sizes(const Geom& g, const int* __restrict__ bond_first,
                                              const int* __restrict__ rb, int cb, const int* parent,
                                              const uint8_t* link, int* size) {
  const int T = g.t, t = threadIdx.x;
  int lone = 0;
  for (int s = t + 1; s <= T; s += NT) {
    const unsigned lk = link[s];
    if constexpr (KIND != PERC_SITEBOND) {
      const int c = KIND == PERC_BOND ? __popc(lk & 0x3fu) : (int)(lk >> 7);
      if (c) atomicAdd(&size[parent[s]], c);
    } else {
      const bool on = (lk >> 7) != 0;
      int own = on ? 1 : 0;
      const int sr = div_m(g, s - 1);
      int nn[6];
      nearestn_rc(g, s, sr, s - 1 - sr * g.m, nn);
      int id = bond_first[s];
      for (int k = 0; k < g.scn; ++k) {
        const int q = nn[k];
        if (q <= s) continue;
        if (rb[id] < cb) {
          if (on) ++own;
          else if (link[q] >> 7) atomicAdd(&size[parent[q]], 1);
          else ++lone;
        }
        ++id;
      }
      if (own) atomicAdd(&size[parent[s]], own);
    }
  }
  return lone;
}

}  // namespace
}  // namespace perc
