// perc_batch_item.h -- what the one-workgroup conductance kernels share
// (perc_batch.hip: k_batch_cond; perc_batch_large.hip: k_batch_cond_large;
// perc_batch_weighted.hip: k_batch_cond_w): the item's front end (occupancy
// from the trial's rank arrays, union-find labeling in LDS, the spanning rule
// of k_span_top, the BatchOut header and the stop), the workgroup sums of both
// dot orders, x on the electrode-adjacent rows and the electrode rows'
// currents.  A kernel owns its LDS plan's solver view, its assembly and its CG
// loop; everything here takes the arrays it works on as arguments.
#pragma once
#include <climits>

#include "perc_asm_row.h"
#include "perc_batch.h"
#include "perc_batch_uf.h"

namespace perc {
namespace {

// The labeling view of a kernel's arena (BatchLabelView's offsets in its LDS
// plan): parent at 0, the bond occupancy, the member and spanning flags, and
// the site occupancy of the site and mixed kinds (the bond kind has none).
struct LabelArrays {
  int* parent;
  uint8_t *bocc, *member, *flag, *socc;
};
template <int KIND>
__device__ __forceinline__ LabelArrays label_arrays(char* smem, int oBocc, int oMem, int oFlag, int oSocc) {
  return {reinterpret_cast<int*>(smem), reinterpret_cast<uint8_t*>(smem + oBocc),
          reinterpret_cast<uint8_t*>(smem + oMem), reinterpret_cast<uint8_t*>(smem + oFlag),
          KIND != PERC_BOND ? reinterpret_cast<uint8_t*>(smem + oSocc) : nullptr};
}

// The spanning cluster's root (0: none, or several and no solve) and whether
// the item ends here; both workgroup-uniform.
struct BatchFront {
  int root;
  bool stop;
};

// Item blockIdx.x from its counts to its BatchOut header.  NT threads.  KIND:
// PERC_BOND / PERC_SITE / PERC_SITEBOND.  sF and s_off receive the form table
// (load_forms), s_i the counters (the first 8 ints; written here, read by no
// caller).  On return every parent is its root and bocc / socc hold the
// occupancy, after a barrier; a stopped item's header is complete.  g: the
// kernel's own copy of a.g.  The common block comes by value and a plan's
// offsets as ints (label_arrays): the address of a kernel's argument block,
// once taken, reorders all its kernel-argument loads and costs registers
// (profiles/batch_front_isa_compare.txt).
template <int NT, int KIND>
__device__ __forceinline__ BatchFront batch_front(const BatchItemArgs a, const Geom& g, const LabelArrays& v,
                                                  StencilForms* sF, int* s_off, int* s_i) {
  const int m = g.m, T = g.t;
  const int t = threadIdx.x;
  const int item = blockIdx.x;
  int* parent = v.parent;
  uint8_t *bocc = v.bocc, *member = v.member, *flag = v.flag, *socc = v.socc;

  const int trial = a.item_trial[item];
  const int count = KIND != PERC_SITE ? a.item_count[item] : 0;
  const int nsite = KIND != PERC_BOND ? a.item_nsites[item] : 0;
  const int* __restrict__ rank = KIND != PERC_SITE ? a.rank + (size_t)trial * a.nb : nullptr;
  const int* __restrict__ rank_s = KIND != PERC_BOND ? a.rank_s + (size_t)trial * T : nullptr;
  BatchOut* out = a.out + item;

  // ---- occupancy: an element is occupied iff its position in its order <
  // its count.  Site kinds: the member flag is the occupied site (perc_cc.h);
  // the site kind reads no bond ranks, bocc is all zero as perc_label leaves it
  {
    const int nw = (int)(sizeof(StencilForms) / 4);
    const int* src = reinterpret_cast<const int*>(a.forms);
    int* dst = reinterpret_cast<int*>(sF);
    for (int k = t; k < nw; k += NT) dst[k] = src[k];
  }
  if (t < 8) s_i[t] = t == 2 ? INT_MAX : 0;
  for (int s = t; s <= T; s += NT) {
    parent[s] = s;
    if constexpr (KIND == PERC_BOND) {
      member[s] = 0;
    } else {
      const uint8_t o = s >= 1 && rank_s[s - 1] < nsite ? 1 : 0;
      socc[s] = o;
      member[s] = o;
    }
  }
  for (int c = t; c <= m; c += NT) flag[c] = 0;
  if constexpr (KIND == PERC_SITE) {
    for (int id = t; id < a.nb; id += NT) bocc[id] = 0;
  } else {
    for (int id = t; id < a.nb; id += NT) bocc[id] = rank[id] < count ? 1 : 0;
  }
  load_forms(*a.forms, s_off);  // (ends with a workgroup barrier)

  // ---- labeling: hook the larger root under the smaller over every bond
  // that connects (cc_link's rule of the kind), flatten, until a pass hooks
  // nothing (lds_label)
  lds_label<NT>(g, a.bond_first, parent, [&](int pass, int s, int, int q, int id) {
    if constexpr (KIND == PERC_BOND) {
      if (!bocc[id]) return false;
      if (pass == 0) {
        member[s] = 1;
        member[q] = 1;
      }
      return true;
    } else if constexpr (KIND == PERC_SITE) {
      return socc[s] && socc[q];
    } else {
      return bocc[id] && socc[s] && socc[q];
    }
  });

  // ---- spanning (k_span_top's rule): root <= m and a top-row member
  for (int c = t; c < m; c += NT) {
    const int s = T - m + 1 + c;
    if (member[s] && parent[s] <= m) flag[parent[s]] = 1;
  }
  __syncthreads();
  {
    int ncl = 0, nsp = 0, mn = INT_MAX;
    for (int s = t + 1; s <= T; s += NT) ncl += parent[s] == s && member[s];
    for (int c = t + 1; c <= m; c += NT)
      if (flag[c]) {
        ++nsp;
        mn = min(mn, c);
      }
    if (ncl) atomicAdd(&s_i[0], ncl);
    if (nsp) {
      atomicAdd(&s_i[1], nsp);
      atomicMin(&s_i[2], mn);
    }
  }
  __syncthreads();
  const int nclusters = s_i[0], nspan = s_i[1];
  const int root = nspan > 0 ? s_i[2] : 0;
  if (root) {
    int cnt = 0;
    for (int s = t + 1; s <= T; s += NT) cnt += member[s] && parent[s] == root;
    if (cnt) atomicAdd(&s_i[3], cnt);
  }
  __syncthreads();
  const int span_sites = s_i[3];
  const bool stop = nspan != 1 || !a.solve;  // (uniform: LDS values after a barrier)
  if (t == 0) {
    out->nclusters = nclusters;
    out->nspan = nspan;
    out->span_root = root;
    out->span_sites = span_sites;
    out->fallback = nspan > 1 ? 1 : 0;  // the lowest-label rule: host replay
    out->pad = 0;
    if (stop) {
      out->status = nspan == 0 ? 1 : 0;
      out->iter = 0;
      out->err = 0.0;
    }
  }
  return {root, stop};
}

// electrode site idx of 2m: the bottom row's sites, then the top row's
__device__ __forceinline__ int electrode_site(const Geom& g, int idx) {
  return idx < g.m ? idx + 1 : g.t - g.m + 1 + (idx - g.m);
}

// The electrode rows' slot values as 2-bit codes in s_cur[2m] (0: no bond,
// 1: -leak, 2: -g0; slot j of sorted_neighbours in bits 2j, 2j + 1), for the
// kernels whose bonds take two values.  Reads the labeling arrays.
template <int NT, int RULE>
__device__ __forceinline__ void encode_electrode_rows(const Geom& g, const int* bond_first,
                                                      const LabelArrays& v, int root, double g0,
                                                      double leak, uint16_t* s_cur) {
#pragma unroll 1
  for (int idx = threadIdx.x; idx < 2 * g.m; idx += NT) {
    const int s = electrode_site(g, idx);
    const int ps = v.parent[s];
    int nbr[6];
    const int cnt = sorted_neighbours(g, s, nbr);
    unsigned cc = 0;
    for (int j = 0; j < cnt; ++j) {
      const int c = nbr[j];
      const int id = s < c ? bond_id(g, bond_first, s, c) : bond_id(g, bond_first, c, s);
      unsigned kind = 0;  // no bond: 0.0 (k_currents)
      if (id >= 0)
        kind = bond_value(RULE, id, s, c, ps, v.bocc, v.socc, root, g0, leak, nullptr) == -g0 ? 2u : 1u;
      cc |= kind << (2 * j);
    }
    s_cur[idx] = (uint16_t)cc;
  }
}
// slot j's value from such a code
__device__ __forceinline__ double electrode_code_value(unsigned cc, int j, double g0, double leak) {
  const unsigned kind = (cc >> (2 * j)) & 3u;
  return kind == 0 ? 0.0 : (kind == 2 ? -g0 : -leak);
}

// k_currents' expression of the current rule at electrode site s: gj(j) the
// value of neighbour slot j (sorted_neighbours' order, 0.0 where there is no
// bond), V(c) the voltage of site c.
template <class GJ, class VF>
__device__ __forceinline__ double electrode_current(const Geom& g, int s, int cur_rule, GJ gj, VF V) {
  int nbr[6];
  const int cnt = sorted_neighbours(g, s, nbr);
  double gv[6];
  double rowsum = 0.0;
  for (int j = 0; j < cnt; ++j) {
    gv[j] = gj(j);
    rowsum = rowsum + gv[j];
  }
  const double d = -rowsum;
  double acc;
  if (cur_rule == PERC_CUR_FORTRAN) {
    acc = d * V(s);
    for (int j = 0; j < cnt; ++j)
      if (fabs(gv[j]) >= 1.0e-10) acc = acc + gv[j] * V(nbr[j]);
  } else {  // no threshold, the diagonal term before the first neighbour > s
    acc = 0.0;
    bool done = false;
    for (int j = 0; j < cnt; ++j) {
      if (!done && nbr[j] > s) {
        acc = acc + d * V(s);
        done = true;
      }
      acc = acc + gv[j] * V(nbr[j]);
    }
    if (!done) acc = acc + d * V(s);
  }
  return acc;
}

// Workgroup sum of two values: per-wave butterfly, then the waves in order.
// s_red: 32 doubles (16 wave totals per value).
template <int NT>
__device__ __forceinline__ void wg_sum2(double* s_red, double v0, double v1, double* o0, double* o1) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v0 = wave_sum(v0);
  v1 = wave_sum(v1);
  if (lane == 0) {
    s_red[wid] = v0;
    s_red[16 + wid] = v1;
  }
  __syncthreads();
  double t0 = s_red[0], t1 = s_red[16];
  for (int w = 1; w < NT / 64; ++w) {
    t0 = t0 + s_red[w];
    t1 = t1 + s_red[16 + w];
  }
  __syncthreads();  // s_red reuse
  *o0 = t0;
  *o1 = t1;
}

// Literal order, one round of K sums: every thread's row-j terms into the
// staging row s_st[K][NT] (rows j NT .. j NT + NT - 1, ascending in t); wave 0
// folds them into its accumulators, which it carries from round to round.
template <int K, int NT>
__device__ __forceinline__ void lit_round(double* s_st, int N, int j, bool have, const double (&tm)[K],
                                          double (&acc)[K]) {
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  if (have) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_st[k * NT + t] = tm[k];
  }
  __syncthreads();
  if (wid == 0) {
    const int cnt = min(NT, N - j * NT);
    for (int c0 = 0; c0 < cnt; c0 += 64) {
      const int l = min(c0 + lane, cnt - 1);
      double tz[K];
#pragma unroll
      for (int k = 0; k < K; ++k) tz[k] = s_st[k * NT + l];
      fold_chunk<K, 8>(tz, min(64, cnt - c0), acc);
    }
  }
  __syncthreads();  // the staging row is free again
}

// x on the rows the currents read, s_x[2m]: rows below m, then rows from N - m
// (a row can be both).  x = 0 by the owners of rows t, t + NT, .. (EPT each)
template <int NT, int EPT>
__device__ __forceinline__ void x_clear(double* s_x, int m, int N) {
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const int i = threadIdx.x + j * NT;
    if (i < N) {
      if (i < m) s_x[i] = 0.0;
      if (i >= N - m) s_x[m + (i - (N - m))] = 0.0;
    }
  }
}
// x(i) += ak p(i), by row i's owner
__device__ __forceinline__ void x_add(double* s_x, int m, int N, int i, double akp) {
  if (i < m) s_x[i] = s_x[i] + akp;
  if (i >= N - m) s_x[m + (i - (N - m))] = s_x[m + (i - (N - m))] + akp;
}
// x(i) of such a row
__device__ __forceinline__ double x_at(const double* s_x, int m, int N, int i) {
  return i < m ? s_x[i] : s_x[m + (i - (N - m))];
}

}  // namespace
}  // namespace perc
