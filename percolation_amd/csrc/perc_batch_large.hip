// perc_batch_large.hip -- k_batch_cond_large: k_batch_cond's one-workgroup
// realisation (perc_batch_item.h's front end, sums and currents around this
// file's assembly and CG loop in both dot orders) for lattices up to
// 128 x 128.  1024 threads, at most 16 rows per thread.  Of
// the N-sized solver arrays only p(k) lies in LDS: a thread keeps the u16
// codes of its own rows in registers (two per VGPR) beside r, x is carried
// on the 2m rows the currents read, and q never goes to LDS: the fast order
// holds a thread's 16 q in registers between the two passes, the literal
// order rebuilds q in the r update from p with the call that formed it for
// q.p, bitwise the same (the march's way).  Nothing takes this
// path unless asked (perc_set_batch_large).
#include "perc_batch_item.h"

namespace perc {
namespace {

struct BatchLargeArgs : BatchItemArgs {
  BatchLargeLds L;
};

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
// one staging row in LDS (lit_round); bitwise k_fold_init + k_cg_small<true, true>.
// Else per thread in row order, wave butterfly, waves in order
// (wg_sum2).  KIND as k_batch_cond's.
template <bool LIT, int KIND>
__global__ __launch_bounds__(kLargeNT) void k_batch_cond_large(BatchLargeArgs a) {
  static_assert(PERC_RULE_BOND == PERC_BOND && PERC_RULE_SITE == PERC_SITE &&
                    PERC_RULE_MIXED == PERC_SITEBOND, "a kind's rule has its number");
  constexpr int RULE = KIND;
  constexpr int NT = kLargeNT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Geom g = a.g;
  const int m = g.m, T = g.t, N = a.N;
  const int t = threadIdx.x;
  const int item = blockIdx.x;
  // labeling view of the arena
  const LabelArrays lv = label_arrays<KIND>(smem, a.L.oBocc, a.L.oMem, a.L.oFlag, a.L.oSocc);
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

  // ---- occupancy, labeling, spanning, the item's header (perc_batch_item.h)
  const BatchFront front = batch_front<NT, KIND>(a, g, lv, sF, s_off, s_i);
  if (front.stop) return;
  const int root = front.root;

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
    assemble_row_vals<false>(g, i, a.bond_first, lv.bocc, lv.socc, lv.parent, nullptr, nullptr, nullptr, &b,
                             &c, a.sflag, *sF, a.fast, a.fl, a.fr, a.bf_closed, RULE, g0, leak, Va,
                             root, nullptr);
    const int j = i / NT;  // (uniform)
    const unsigned cs = (unsigned)c << (16 * (j & 1));
#pragma unroll
    for (int k = 0; k < kLargeEPT / 2; ++k) cw[k] |= k == (j >> 1) ? cs : 0u;
#pragma unroll
    for (int jj = 0; jj < kLargeEPT; ++jj) rv[jj] = jj == j ? b : rv[jj];
  }
  encode_electrode_rows<NT, RULE>(g, a.bond_first, lv, root, g0, leak, s_cur);
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
  x_clear<NT, kLargeEPT>(s_x, m, N);  // x = 0, by the row's owner
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
      lit_round<2, NT>(s_st, N, j, i < N, {zb * zb, z * rj}, acc);
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
    wg_sum2<NT>(s_red, b2, zr0, &tb, &tz);
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
        lit_round<1, NT>(s_st, N, j, i < N, {tq}, acc);
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
      wg_sum2<NT>(s_red, dot, 0.0, &akden, &unused);
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
          x_add(s_x, m, N, i, ak * pi);
          const double rn = r_sel(j) - ak * q;
#pragma unroll
          for (int jj = 0; jj < kLargeEPT; ++jj) rv[jj] = jj == j ? rn : rv[jj];
          const double zj = rn / code_diag(c, ng0, nleak);
          t0 = zj * rn;  // bknum :785-787
          t1 = rn * rn;  // snrm :872-875
        }
        lit_round<2, NT>(s_st, N, j, i < N, {t0, t1}, acc);
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
          x_add(s_x, m, N, i, ak * pi);
          const double rn = rv[j] - ak * q;
          rv[j] = rn;
          const double z = rn / code_diag(c, ng0, nleak);
          zr = zr + z * rn;
          rr = rr + rn * rn;
        }
      }
      wg_sum2<NT>(s_red, zr, rr, &tzr, &trr);
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
  double* iout = a.iout + (size_t)item * 2 * m;
  auto V = [&](int c) -> double { return c <= m ? 0.0 : (c > T - m ? Va : x_at(s_x, m, N, c - m - 1)); };
#pragma unroll 1
  for (int idx = t; idx < 2 * m; idx += NT) {
    const unsigned cc = s_cur[idx];
    iout[idx] = electrode_current(
        g, electrode_site(g, idx), a.cur_rule,
        [&](int j) -> double { return electrode_code_value(cc, j, g0, leak); }, V);
  }
  if (t == 0) {
    BatchOut* out = a.out + item;
    out->status = 0;
    out->iter = k;
    out->err = err;
  }
}

}  // namespace

hipError_t dev_batch_large_launch(perc_ctx* h, int kind, bool literal, const BatchItemArgs& c, int nitems) {
  const BatchLargeArgs a{c, batch_large_lds(h->g, kind)};
  return dispatch_kind_order(kind, literal, [&](auto lit, auto kd) {
    return launch_lds(&k_batch_cond_large<lit(), kd()>, &h->large_lds[lit()][kd()], a, nitems, kLargeNT,
                      h->stream, "k_batch_cond_large");
  });
}

}  // namespace perc
