// perc_batch_uf.h -- the in-LDS union-find the one-workgroup kernels share
// (perc_batch_item.h: the conductance kernels' batch_front;
// perc_batch_scan.hip: k_batch_scan): the
// root walk and the hook / flatten passes over a bond predicate.
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

}  // namespace
}  // namespace perc
