// perc_batch_large.hip -- k_batch_cond_large: k_batch_cond's one-workgroup
// realisation (occupancy from ranks, union-find labeling in LDS, the spanning
// rule, assemble_row, the CG loop in both dot orders, the currents) for
// lattices up to 128 x 128.  1024 threads, at most 16 rows per thread.  Of
// the N-sized solver arrays only p(k) lies in LDS: a thread keeps the u16
// codes of its own rows in registers (two per VGPR) beside r, x is carried
// on the 2m rows the currents read, and q never goes to LDS: the fast order
// holds a thread's 16 q in registers between the two passes, the literal
// order rebuilds q in the r update from p with the call that formed it for
// q.p, bitwise the same (the march's way).  Nothing takes this
// path unless asked (perc_set_batch_large).
#include <climits>

#include "perc_asm_row.h"
#include "perc_batch.h"
#include "perc_batch_uf.h"

namespace perc {
namespace {

constexpr int kLargeNT = kBatchLargeThreads;
constexpr int kLargeEPT = kBatchLargeEPT;
// The fast order's q: held in registers between the passes (15 more VGPRs,
// no scratch; 12 % faster over a 128 x 128 batch call than rebuilding it).
// Probe builds with -DPERC_BATCH_LARGE_REBUILDQ rebuild it as the literal
// order does; DESIGN 4.5 has both listings and the A/B.
#ifdef PERC_BATCH_LARGE_REBUILDQ
constexpr bool kHoldQ = false;
#else
constexpr bool kHoldQ = true;
#endif

// Rows t, t + 1024, .. per thread.  LIT: the literal dot order -- every sum
// folded by wave 0 in ascending row order, in rounds of 1024 rows through
// one staging row in LDS; bitwise k_fold_init + k_cg_small<true, true>.
// Else per thread in row order, wave butterfly, waves in order
// (k_batch_cond's tree).  KIND as k_batch_cond's.
template <bool LIT, int KIND>
__global__ __launch_bounds__(kLargeNT) void k_batch_cond_large(BatchLargeArgs a) {
  static_assert(PERC_RULE_BOND == PERC_BOND && PERC_RULE_SITE == PERC_SITE &&
                    PERC_RULE_MIXED == PERC_SITEBOND, "a kind's rule has its number");
  constexpr int RULE = KIND;
  constexpr int NT = kLargeNT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Geom g = a.g;
  const int m = g.m, T = g.t, N = a.N;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int item = blockIdx.x;
  // labeling view of the arena
  int* parent = reinterpret_cast<int*>(smem);
  uint8_t* bocc = reinterpret_cast<uint8_t*>(smem + a.L.oBocc);
  uint8_t* member = reinterpret_cast<uint8_t*>(smem + a.L.oMem);
  uint8_t* flag = reinterpret_cast<uint8_t*>(smem + a.L.oFlag);
  uint8_t* socc = KIND != PERC_BOND ? reinterpret_cast<uint8_t*>(smem + a.L.oSocc) : nullptr;
  // solver view
  double* s_p = reinterpret_cast<double*>(smem);
  double* s_x = reinterpret_cast<double*>(smem + a.L.oX);    // rows 0..m-1, then N-m..N-1
  double* s_st = reinterpret_cast<double*>(smem + a.L.oStage);  // [2][NT]
  // outside both views
  double* s_red = reinterpret_cast<double*>(smem + a.L.oRed);
  int* s_off = reinterpret_cast<int*>(smem + a.L.oOff);
  StencilForms* sF = reinterpret_cast<StencilForms*>(smem + a.L.oF);
  uint16_t* s_cur = reinterpret_cast<uint16_t*>(smem + a.L.oCur);
  int* s_i = reinterpret_cast<int*>(smem + a.L.oInt);

  const int trial = a.item_trial[item];
  const int count = KIND != PERC_SITE ? a.item_count[item] : 0;
  const int nsite = KIND != PERC_BOND ? a.item_nsites[item] : 0;
  const int* __restrict__ rank = KIND != PERC_SITE ? a.rank + (size_t)trial * a.nb : nullptr;
  const int* __restrict__ rank_s = KIND != PERC_BOND ? a.rank_s + (size_t)trial * T : nullptr;
  BatchOut* out = a.out + item;

  // ---- occupancy (k_batch_cond's statements)
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

  // ---- labeling
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
  if (stop) return;

  // ---- assembly: the thread that owns row i assembles it; its code goes
  // into the thread's packed code registers and its rhs (zero below the top
  // system row) into r.  j is uniform: the register is picked by selects.
  const double g0 = a.g0, leak = a.leak, Va = a.Va;
  unsigned cw[kLargeEPT / 2];
  double rv[kLargeEPT];
#pragma unroll
  for (int k = 0; k < kLargeEPT / 2; ++k) cw[k] = 0u;
#pragma unroll
  for (int j = 0; j < kLargeEPT; ++j) rv[j] = 0.0;
#pragma unroll 1
  for (int i = t; i < N; i += NT) {
    uint16_t c;
    double b;
    assemble_row_vals<false>(g, i, a.bond_first, bocc, socc, parent, nullptr, nullptr, nullptr, &b,
                             &c, a.sflag, *sF, a.fast, a.fl, a.fr, a.bf_closed, RULE, g0, leak, Va,
                             root, nullptr);
    const int j = i / NT;  // (uniform)
    const unsigned cs = (unsigned)c << (16 * (j & 1));
#pragma unroll
    for (int k = 0; k < kLargeEPT / 2; ++k) cw[k] |= k == (j >> 1) ? cs : 0u;
#pragma unroll
    for (int jj = 0; jj < kLargeEPT; ++jj) rv[jj] = jj == j ? b : rv[jj];
  }
#pragma unroll 1
  for (int idx = t; idx < 2 * m; idx += NT) {
    const int s = idx < m ? idx + 1 : T - m + 1 + (idx - m);
    const int ps = parent[s];
    int nbr[6];
    const int cnt = sorted_neighbours(g, s, nbr);
    unsigned cc = 0;
    for (int j = 0; j < cnt; ++j) {
      const int c = nbr[j];
      const int id = s < c ? bond_id(g, a.bond_first, s, c) : bond_id(g, a.bond_first, c, s);
      unsigned kind = 0;  // no bond: 0.0 (k_currents)
      if (id >= 0)
        kind = bond_value(RULE, id, s, c, ps, bocc, socc, root, g0, leak, nullptr) == -g0 ? 2u : 1u;
      cc |= kind << (2 * j);
    }
    s_cur[idx] = (uint16_t)cc;
  }
  __syncthreads();  // the labeling arrays are dead from here: p, x and the staging row take their place

  // ---- solve: k_cg_small<true, LIT>, the prologue included (x = 0, r = b)
  const double ng0 = -g0, nleak = -leak;
  // row j's code (j a compile-time constant under a full unroll)
  auto code_at = [&](int j) -> unsigned { return (cw[j >> 1] >> (16 * (j & 1))) & 0xffffu; };
  // ... and for a uniform run-time j (the literal order's rounds)
  auto code_sel = [&](int j) -> unsigned {
    unsigned w = 0u;
#pragma unroll
    for (int k = 0; k < kLargeEPT / 2; ++k) w = k == (j >> 1) ? cw[k] : w;
    return (w >> (16 * (j & 1))) & 0xffffu;
  };
  auto r_sel = [&](int j) -> double {
    double v = 0.0;
#pragma unroll
    for (int jj = 0; jj < kLargeEPT; ++jj) v = jj == j ? rv[jj] : v;
    return v;
  };
  // q(i) = (A p)(i), dsprsax order, from p in LDS
  auto row_q = [&](int i, unsigned c, double pi) -> double {
    const int f = c >> 11, cnt = (c >> 8) & 7;
    double xn[kMaxSlots];
    bool use[kMaxSlots];
#pragma unroll
    for (int e = 0; e < kMaxSlots; ++e) {
      const int col = i + s_off[f * kMaxSlots + e];
      use[e] = e < cnt && (unsigned)col < (unsigned)N;
      xn[e] = s_p[use[e] ? col : i];
    }
    return st_combine<kMaxSlots>(c, xn, use, pi, ng0, nleak);
  };
  // x += ak p on the rows the currents read (rows below m, rows from N - m)
  auto x_add = [&](int i, double akp) {
    if (i < m) s_x[i] = s_x[i] + akp;
    if (i >= N - m) s_x[m + (i - (N - m))] = s_x[m + (i - (N - m))] + akp;
  };
#pragma unroll
  for (int j = 0; j < kLargeEPT; ++j) {  // x = 0, by the row's owner
    const int i = t + j * NT;
    if (i < N) {
      if (i < m) s_x[i] = 0.0;
      if (i >= N - m) s_x[m + (i - (N - m))] = 0.0;
    }
  }
  // workgroup sum: per-wave butterfly, then the waves in order
  auto wg_sum = [&](double v0, double v1, double* o0, double* o1) {
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
  };
  // literal order, one round: every thread's row-j term(s) into the staging
  // row (rows j NT .. j NT + NT - 1, ascending in t); wave 0 folds them into
  // its accumulator, which it carries from round to round
  auto lit_round2 = [&](int j, bool have, double t0, double t1, double (&acc)[2]) {
    if (have) {
      s_st[t] = t0;
      s_st[NT + t] = t1;
    }
    __syncthreads();
    if (wid == 0) {
      const int cnt = min(NT, N - j * NT);
      for (int c0 = 0; c0 < cnt; c0 += 64) {
        const int l = min(c0 + lane, cnt - 1);
        const double tz[2] = {s_st[l], s_st[NT + l]};
        fold_chunk<2, 8>(tz, min(64, cnt - c0), acc);
      }
    }
    __syncthreads();  // the staging row is free again
  };
  auto lit_round1 = [&](int j, bool have, double t0, double (&acc)[1]) {
    if (have) s_st[t] = t0;
    __syncthreads();
    if (wid == 0) {
      const int cnt = min(NT, N - j * NT);
      for (int c0 = 0; c0 < cnt; c0 += 64) {
        const int l = min(c0 + lane, cnt - 1);
        const double tz[1] = {s_st[l]};
        fold_chunk<1, 8>(tz, min(64, cnt - c0), acc);
      }
    }
    __syncthreads();
  };
  const int itol = a.itol, itmax = a.itmax;
  const double tol = a.tol;
  double bnrm, bknum;
  if constexpr (LIT) {  // k_fold_init: bnrm^2 and the first bknum in ascending j
    double acc[2] = {0.0, 0.0};
#pragma unroll 1
    for (int j = 0; j * NT < N; ++j) {
      const int i = t + j * NT;
      const double rj = r_sel(j);
      const double dj = i < N ? code_diag(code_sel(j), ng0, nleak) : 1.0;
      const double zb = itol == 1 ? rj : rj / dj, z = rj / dj;
      lit_round2(j, i < N, zb * zb, z * rj, acc);
    }
    if (t == 0) {
      s_red[32] = sqrt(acc[0]);
      s_red[33] = acc[1];
    }
    __syncthreads();
    bnrm = s_red[32];
    bknum = s_red[33];
    __syncthreads();
  } else {
    double b2 = 0.0, zr0 = 0.0;
#pragma unroll
    for (int j = 0; j < kLargeEPT; ++j) {
      const int i = t + j * NT;
      if (i < N) {
        const double dj = code_diag(code_at(j), ng0, nleak);
        const double zb = itol == 1 ? rv[j] : rv[j] / dj, z = rv[j] / dj;
        b2 = b2 + zb * zb;
        zr0 = zr0 + z * rv[j];
      }
    }
    double tb, tz;
    wg_sum(b2, zr0, &tb, &tz);
    bnrm = sqrt(tb);
    bknum = tz;
  }
  double bk = 0.0, ak = 0.0, err = 0.0;
  int k = 0;
  // What a pass derives from the codes and the thread's row numbers (16
  // diagonals, 96 slot values, the row addresses) is loop-invariant, and held
  // across the loop it spills: the codes and the thread id pass through an
  // empty asm before every pass, so each row's are formed where they are used
  int tt = t;
  auto fresh = [&]() {
#pragma unroll
    for (int kk = 0; kk < kLargeEPT / 2; ++kk) asm volatile("" : "+v"(cw[kk]));
    asm volatile("" : "+v"(tt));
  };
  while (true) {
    ++k;
    fresh();
    // p(k) = bk p(k-1) + z (k = 1: p = z), linbcg :789-797.  Every thread is
    // past the previous iteration's second pass (its reduction's barriers),
    // so no neighbour of an overwritten p(k-1) is still to be read
#pragma unroll
    for (int j = 0; j < kLargeEPT; ++j) {
      const int i = tt + j * NT;
      if (i < N) {
        const double z = rv[j] / code_diag(code_at(j), ng0, nleak);
        s_p[i] = k == 1 ? z : bk * s_p[i] + z;
      }
    }
    __syncthreads();
    // pass 1: q = A p (dsprsax order) and q.p
    double akden, unused;
    [[maybe_unused]] double qv[kHoldQ ? kLargeEPT : 1];
    if constexpr (LIT) {
      double acc[1] = {0.0};
#pragma unroll 1
      for (int j = 0; j * NT < N; ++j) {
        const int i = t + j * NT;
        double tq = 0.0;
        if (i < N) {
          const double pi = s_p[i];
          tq = row_q(i, code_sel(j), pi) * pi;  // akden, bondc.f:803-805
        }
        lit_round1(j, i < N, tq, acc);
      }
      if (t == 0) s_red[32] = acc[0];
      __syncthreads();
      akden = s_red[32];
      __syncthreads();
    } else {
      double dot = 0.0;
      fresh();
#pragma unroll
      for (int j = 0; j < kLargeEPT; ++j) {
        const int i = tt + j * NT;
        if (i < N) {
          const double pi = s_p[i];
          const double q = row_q(i, code_at(j), pi);
          if constexpr (kHoldQ) qv[j] = q;
          dot = dot + q * pi;
        }
      }
      wg_sum(dot, 0.0, &akden, &unused);
    }
    ak = bknum / akden;
    // pass 2: q held (fast order) or formed again by the same call on the
    // same operands (literal order), then
    // x += ak p, r -= ak q, z = r/d, z.r and r.r (linbcg :801-806, 808-813)
    double tzr, trr;
    if constexpr (LIT) {
      double acc[2] = {0.0, 0.0};
#pragma unroll 1
      for (int j = 0; j * NT < N; ++j) {
        const int i = t + j * NT;
        double t0 = 0.0, t1 = 0.0;
        if (i < N) {
          const unsigned c = code_sel(j);
          const double pi = s_p[i];
          const double q = row_q(i, c, pi);
          x_add(i, ak * pi);
          const double rn = r_sel(j) - ak * q;
#pragma unroll
          for (int jj = 0; jj < kLargeEPT; ++jj) rv[jj] = jj == j ? rn : rv[jj];
          const double zj = rn / code_diag(c, ng0, nleak);
          t0 = zj * rn;  // bknum :785-787
          t1 = rn * rn;  // snrm :872-875
        }
        lit_round2(j, i < N, t0, t1, acc);
      }
      if (t == 0) {
        s_red[32] = acc[0];
        s_red[33] = acc[1];
      }
      __syncthreads();
      tzr = s_red[32];
      trr = s_red[33];
      __syncthreads();
    } else {
      double zr = 0.0, rr = 0.0;
      fresh();
#pragma unroll
      for (int j = 0; j < kLargeEPT; ++j) {
        const int i = tt + j * NT;
        if (i < N) {
          const unsigned c = code_at(j);
          const double pi = s_p[i];
          double q;
          if constexpr (kHoldQ) q = qv[j];
          else q = row_q(i, c, pi);
          x_add(i, ak * pi);
          const double rn = rv[j] - ak * q;
          rv[j] = rn;
          const double z = rn / code_diag(c, ng0, nleak);
          zr = zr + z * rn;
          rr = rr + rn * rn;
        }
      }
      wg_sum(zr, rr, &tzr, &trr);
    }
    err = sqrt(trr) / bnrm;
    bk = tzr / bknum;
    bknum = tzr;
    // err comes from one LDS value in every thread: a uniform break
    if (!(err > tol) || k >= itmax + 1) break;
  }

  // ---- currents: k_currents' expression of the current rule on the 2m
  // electrode sites; their interior neighbours are rows below m or from N - m
  __syncthreads();
  auto xe = [&](int i) -> double { return i < m ? s_x[i] : s_x[m + (i - (N - m))]; };
  double* iout = a.iout + (size_t)item * 2 * m;
#pragma unroll 1
  for (int idx = t; idx < 2 * m; idx += NT) {
    const int s = idx < m ? idx + 1 : T - m + 1 + (idx - m);
    int nbr[6];
    const int cnt = sorted_neighbours(g, s, nbr);
    const unsigned cc = s_cur[idx];
    double gv[6];
    double rowsum = 0.0;
    for (int j = 0; j < cnt; ++j) {
      const unsigned kind = (cc >> (2 * j)) & 3u;
      gv[j] = kind == 0 ? 0.0 : (kind == 2 ? -g0 : -leak);
      rowsum = rowsum + gv[j];
    }
    const double d = -rowsum;
    auto V = [&](int c) -> double { return c <= m ? 0.0 : (c > T - m ? Va : xe(c - m - 1)); };
    double acc;
    if (a.cur_rule == PERC_CUR_FORTRAN) {
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
    iout[idx] = acc;
  }
  if (t == 0) {
    out->status = 0;
    out->iter = k;
    out->err = err;
  }
}

template <bool LIT, int KIND>
hipError_t launch(perc_ctx* h, const BatchLargeArgs& a, int nitems) {
  if (h->large_lds[LIT][KIND] < a.L.total) {  // dynamic LDS beyond the default limit
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_batch_cond_large<LIT, KIND>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, a.L.total));
    h->large_lds[LIT][KIND] = a.L.total;
  }
  k_batch_cond_large<LIT, KIND><<<nitems, kLargeNT, a.L.total, h->stream>>>(a);
  return dbg_sync(h->stream, "k_batch_cond_large");
}

}  // namespace

hipError_t dev_batch_large_launch(perc_ctx* h, int kind, bool literal, BatchLargeArgs a, int nitems) {
  a.L = batch_large_lds(h->g, kind);
  if (kind == PERC_BOND)
    return literal ? launch<true, PERC_BOND>(h, a, nitems) : launch<false, PERC_BOND>(h, a, nitems);
  if (kind == PERC_SITE)
    return literal ? launch<true, PERC_SITE>(h, a, nitems) : launch<false, PERC_SITE>(h, a, nitems);
  return literal ? launch<true, PERC_SITEBOND>(h, a, nitems) : launch<false, PERC_SITEBOND>(h, a, nitems);
}

}  // namespace perc
