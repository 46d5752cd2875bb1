// perc_batch_weighted.hip -- the batch path with per-bond conductance
// multipliers (ConductCalc.m condtype 2, perc_batch_cond_weighted).
// k_twister_stream: MT19937 streams on the device, one wave per seed, bit for
// bit perc_twister_uniform.  k_batch_cond_w: k_batch_cond_large's
// one-workgroup realisation (perc_batch_item.h's front end, sums and currents
// around this file's weights, assembly and CG loop in both dot orders) with
// the rows' slot values themselves in LDS where the other
// two kernels rebuild them from a two-value code: G = -g0 w[id] takes as
// many values as there are bonds.  The operator is the CSR one of the single
// path's weighted solve (dsprsax order: the diagonal, then the used slots in
// slot order), so the literal order is bitwise perc_set_bond_weights +
// perc_conductance under PERC_DOT_LITERAL.
#include "perc_batch_item.h"

namespace perc {
namespace {

struct BatchWArgs : BatchItemArgs {
  BatchWLds L;
  BatchWItems w;  // (after the plan: see profiles/batch_front_isa_compare.txt)
};

// ---------------------------------------------------------------------------
// MT19937 (Matsumoto & Nishimura), perc_host.cpp's Twister on one wave: the
// state in LDS, init_genrand serial, the twist in the three index ranges in
// which no word read is one the range writes -- k < 227 reads the old k,
// k + 1 and k + 397; 227 <= k < 454 the new k - 227 and the old k, k + 1;
// 454 <= k < 623 the same; k = 623 the new 396, the old 623 and the new 0.
// Within a range every lane reads its words before any lane writes.  One
// twist gives 312 genrand_res53 doubles (output pairs 2j, 2j + 1).
constexpr int kMtN = 624, kMtM = 397;

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// words lo .. hi - 1 (at most 256 of them): mt[k] = mt[k + src] ^ twist(mt[k], mt[k + 1])
__device__ __forceinline__ void mt_range(uint32_t* mt, int lo, int hi, int src, int lane) {
  uint32_t y[4], mm[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = lo + lane + 64 * q;
    if (k < hi) {
      y[q] = (mt[k] & 0x80000000u) | (mt[k + 1] & 0x7fffffffu);
      mm[q] = mt[k + src];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = lo + lane + 64 * q;
    if (k < hi) mt[k] = mm[q] ^ (y[q] >> 1) ^ ((y[q] & 1u) ? 0x9908b0dfu : 0u);
  }
  __syncthreads();
}

__global__ __launch_bounds__(64) void k_twister_stream(int nseeds, const unsigned* __restrict__ seeds,
                                                       long long n, double* __restrict__ out) {
  __shared__ uint32_t mt[kMtN];
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= nseeds) return;
  if (lane == 0) {  // init_genrand
    uint32_t x = seeds[blockIdx.x];
    mt[0] = x;
    for (int i = 1; i < kMtN; ++i) {
      x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
      mt[i] = x;
    }
  }
  __syncthreads();
  double* o = out + (size_t)blockIdx.x * (size_t)n;
  for (long long base = 0; base < n; base += kMtN / 2) {
    mt_range(mt, 0, kMtN - kMtM, kMtM, lane);
    mt_range(mt, kMtN - kMtM, 2 * (kMtN - kMtM), -(kMtN - kMtM), lane);
    mt_range(mt, 2 * (kMtN - kMtM), kMtN - 1, -(kMtN - kMtM), lane);
    if (lane == 0) {
      const uint32_t y = (mt[kMtN - 1] & 0x80000000u) | (mt[0] & 0x7fffffffu);
      mt[kMtN - 1] = mt[kMtM - 1] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    __syncthreads();
    for (int j = lane; j < kMtN / 2 && base + j < n; j += 64) {  // genrand_res53
      const uint32_t a = mt_temper(mt[2 * j]) >> 5, b = mt_temper(mt[2 * j + 1]) >> 6;
      o[base + j] = (a * 67108864.0 + b) * (1.0 / 9007199254740992.0);
    }
    __syncthreads();  // the outputs are read before the next twist writes
  }
}

// ---------------------------------------------------------------------------
// Rows t, t + NT, .. (at most kBatchWEPT) per thread.  LIT: the literal dot
// order -- every sum folded by wave 0 in ascending row order, in rounds of NT
// rows through one staging row in LDS (k_batch_cond_large's rounds); bitwise
// k_fold_init + k_cg_small<false, true> on the weighted CSR system.  Else per
// thread in row order, wave butterfly, waves in order.  KIND as k_batch_cond's.
template <int NT, bool LIT, int KIND>
__global__ __launch_bounds__(NT) void k_batch_cond_w(BatchWArgs a) {
  static_assert(PERC_RULE_BOND == PERC_BOND && PERC_RULE_SITE == PERC_SITE &&
                    PERC_RULE_MIXED == PERC_SITEBOND, "a kind's rule has its number");
  constexpr int RULE = KIND;
  constexpr int EPT = kBatchWEPT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Geom g = a.g;
  const int m = g.m, T = g.t, N = a.N;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int item = blockIdx.x;
  // labeling view of the arena
  const LabelArrays lv = label_arrays<KIND>(smem, a.L.oBocc, a.L.oMem, a.L.oFlag, a.L.oSocc);
  int* parent = lv.parent;
  uint8_t *bocc = lv.bocc, *socc = lv.socc;
  // solver view
  double* s_p = reinterpret_cast<double*>(smem);
  double* s_x = reinterpret_cast<double*>(smem + a.L.oX);       // rows 0..m-1, then N-m..N-1
  double* s_st = reinterpret_cast<double*>(smem + a.L.oStage);  // [2][NT]
  // outside both views
  double* s_v = reinterpret_cast<double*>(smem + a.L.oVal);  // [scn][N]: slot e of row i at e N + i
  double* s_el = reinterpret_cast<double*>(smem + a.L.oEl);  // [2m][6]: the electrode rows' slot values
  double* s_red = reinterpret_cast<double*>(smem + a.L.oRed);
  int* s_off = reinterpret_cast<int*>(smem + a.L.oOff);
  StencilForms* sF = reinterpret_cast<StencilForms*>(smem + a.L.oF);
  int* s_i = reinterpret_cast<int*>(smem + a.L.oInt);  // 8 counters, 16 wave totals

  // ---- occupancy, labeling, spanning, the item's header (perc_batch_item.h)
  const BatchFront front = batch_front<NT, KIND>(a, g, lv, sF, s_off, s_i);
  if (front.stop) return;
  const int root = front.root;

  // ---- weights by bond id.  Explicit: the item's row.  ConductCalc: one
  // draw per bond the rule gives -g0 (k_bond_mask's predicate), in bond-list
  // order -- bonds are numbered bond_first[s] + r, so an exclusive count over
  // the sites in site order (a run of consecutive sites per thread, the
  // threads' totals scanned over the workgroup) is each bond's place in the
  // draws; the others get 1.0.  The row goes to the launch's scratch and is
  // read back like an explicit one after the barrier.
  const double* w;
  if (a.w.item_wset) {
    w = a.w.wrows + (size_t)a.w.item_wset[item] * a.nb;
  } else {
    double* wr = a.w.wscratch + (size_t)item * a.w.wstride;
    const double* __restrict__ u = a.w.u + (size_t)item * a.nb;
    const int per = (T - 1 + NT - 1) / NT;
    const int s0 = 1 + t * per, s1 = min(T, s0 + per);  // sites s0 .. s1 - 1 of 1 .. T - 1
    auto walk = [&](auto&& f) {
      for (int s = s0; s < s1; ++s) {
        const int row = div_m(g, s - 1);
        int nn[6];
        nearestn_rc(g, s, row, s - 1 - row * m, nn);
        const int fb = a.bond_first[s];
        const bool sroot = parent[s] == root;
        int r = 0;
        for (int k = 0; k < g.scn; ++k) {
          const int q = nn[k];
          if (q <= s) continue;
          const int id = fb + r++;
          bool in;
          if constexpr (RULE == PERC_RULE_BOND) in = bocc[id] && sroot;
          else if constexpr (RULE == PERC_RULE_SITE) in = socc[s] && socc[q] && sroot;
          else in = bocc[id] && socc[s] && socc[q] && sroot;
          f(id, in);
        }
      }
    };
    int c = 0;
    walk([&](int, bool in) { c += in ? 1 : 0; });
    int inc = c;  // inclusive scan over the wave's lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(inc, off, 64);
      if (lane >= off) inc += v;
    }
    if (lane == 63) s_i[8 + wid] = inc;
    __syncthreads();
    int k = inc - c;
    for (int w2 = 0; w2 < wid; ++w2) k += s_i[8 + w2];
    walk([&](int id, bool in) { wr[id] = in ? u[k++] : 1.0; });
    __threadfence_block();
    __syncthreads();
    w = wr;
  }

  // ---- assembly: the thread that owns row i assembles it; the slot values
  // go to LDS, the form and count, the diagonal (-rowsum in slot order, the
  // assembly's own sum) and the rhs (zero below the top system row) into the
  // thread's registers.  j is uniform: the register is picked by selects.
  const double g0 = a.g0, leak = a.leak, Va = a.Va;
  int fc[EPT];
  double rv[EPT], dv[EPT];
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    fc[j] = 0;
    rv[j] = 0.0;
    dv[j] = 1.0;
  }
#pragma unroll 1
  for (int i = t; i < N; i += NT) {
    uint16_t c;
    double b;
    assemble_row_vals<false>(g, i, a.bond_first, bocc, socc, parent, nullptr, nullptr, nullptr, &b,
                             &c, a.sflag, *sF, a.fast, a.fl, a.fr, a.bf_closed, RULE, g0, leak, Va,
                             root, w, s_v + i, N);
    const int cnt = (c >> 8) & 7;
    double rowsum = 0.0;
    for (int e = 0; e < cnt; ++e) rowsum = rowsum + s_v[e * N + i];
    const double d = -rowsum;
    const int j = i / NT;  // (uniform)
#pragma unroll
    for (int jj = 0; jj < EPT; ++jj) {
      fc[jj] = jj == j ? (int)(c >> 8) : fc[jj];
      rv[jj] = jj == j ? b : rv[jj];
      dv[jj] = jj == j ? d : dv[jj];
    }
  }
#pragma unroll 1
  for (int idx = t; idx < 2 * m; idx += NT) {
    const int s = electrode_site(g, idx);
    const int ps = parent[s];
    int nbr[6];
    const int cnt = sorted_neighbours(g, s, nbr);
    for (int j = 0; j < cnt; ++j) {
      const int c = nbr[j];
      const int id = s < c ? bond_id(g, a.bond_first, s, c) : bond_id(g, a.bond_first, c, s);
      // no bond: 0.0 (k_currents)
      s_el[idx * 6 + j] = id < 0 ? 0.0 : bond_value(RULE, id, s, c, ps, bocc, socc, root, g0, leak, w);
    }
  }
  __syncthreads();  // the labeling arrays are dead from here: p, x and the staging row take their place

  // ---- solve: k_cg_small<false, LIT>, the prologue included (x = 0, r = b)
  // q(i) = (A p)(i), dsprsax order, from p and the stored values in LDS
  auto row_q = [&](int i, int fcv, double d, double pi) -> double {
    const int f = fcv >> 3, cnt = fcv & 7;
    double xn[kMaxSlots], vv[kMaxSlots];
    bool use[kMaxSlots];
#pragma unroll
    for (int e = 0; e < kMaxSlots; ++e) {
      const int col = i + s_off[f * kMaxSlots + e];
      use[e] = e < cnt && (unsigned)col < (unsigned)N;
      xn[e] = s_p[use[e] ? col : i];
      vv[e] = s_v[(use[e] ? e : 0) * N + i];
    }
    double acc = d * pi;
#pragma unroll
    for (int e = 0; e < kMaxSlots; ++e) {
      const double pr = vv[e] * xn[e];
      acc = use[e] ? acc + pr : acc;
    }
    return acc;
  };
  x_clear<NT, EPT>(s_x, m, N);  // x = 0, by the row's owner
  const int itol = a.itol, itmax = a.itmax;
  const double tol = a.tol;
  double bnrm, bknum;
  if constexpr (LIT) {  // k_fold_init: bnrm^2 and the first bknum in ascending j
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      if (j * NT < N) {  // (uniform)
        const int i = t + j * NT;
        const double zb = itol == 1 ? rv[j] : rv[j] / dv[j], z = rv[j] / dv[j];
        lit_round<2, NT>(s_st, N, j, i < N, {zb * zb, z * rv[j]}, acc);
      }
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
    for (int j = 0; j < EPT; ++j) {
      const int i = t + j * NT;
      if (i < N) {
        const double zb = itol == 1 ? rv[j] : rv[j] / dv[j], z = rv[j] / dv[j];
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
  while (true) {
    ++k;
    // p(k) = bk p(k-1) + z (k = 1: p = z), linbcg :789-797.  Every thread is
    // past the previous iteration's second pass (its reduction's barriers),
    // so no neighbour of an overwritten p(k-1) is still to be read
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      const int i = t + j * NT;
      if (i < N) {
        const double z = rv[j] / dv[j];
        s_p[i] = k == 1 ? z : bk * s_p[i] + z;
      }
    }
    __syncthreads();
    // pass 1: q = A p (dsprsax order) and q.p
    double akden, unused;
    [[maybe_unused]] double qv[EPT];
    if constexpr (LIT) {
      double acc[1] = {0.0};
#pragma unroll
      for (int j = 0; j < EPT; ++j) {
        if (j * NT < N) {
          const int i = t + j * NT;
          double tq = 0.0;
          if (i < N) {
            const double pi = s_p[i];
            tq = row_q(i, fc[j], dv[j], pi) * pi;  // akden, bondc.f:803-805
          }
          lit_round<1, NT>(s_st, N, j, i < N, {tq}, acc);
        }
      }
      if (t == 0) s_red[32] = acc[0];
      __syncthreads();
      akden = s_red[32];
      __syncthreads();
    } else {
      double dot = 0.0;
#pragma unroll
      for (int j = 0; j < EPT; ++j) {
        const int i = t + j * NT;
        if (i < N) {
          const double pi = s_p[i];
          const double q = row_q(i, fc[j], dv[j], pi);
          qv[j] = q;
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
#pragma unroll
      for (int j = 0; j < EPT; ++j) {
        if (j * NT < N) {
          const int i = t + j * NT;
          double t0 = 0.0, t1 = 0.0;
          if (i < N) {
            const double pi = s_p[i];
            const double q = row_q(i, fc[j], dv[j], pi);
            x_add(s_x, m, N, i, ak * pi);
            const double rn = rv[j] - ak * q;
            rv[j] = rn;
            const double zj = rn / dv[j];
            t0 = zj * rn;  // bknum :785-787
            t1 = rn * rn;  // snrm :872-875
          }
          lit_round<2, NT>(s_st, N, j, i < N, {t0, t1}, acc);
        }
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
#pragma unroll
      for (int j = 0; j < EPT; ++j) {
        const int i = t + j * NT;
        if (i < N) {
          const double pi = s_p[i];
          x_add(s_x, m, N, i, ak * pi);
          const double rn = rv[j] - ak * qv[j];
          rv[j] = rn;
          const double z = rn / dv[j];
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
  // electrode sites, on the stored slot values; their interior neighbours are
  // rows below m or from N - m
  __syncthreads();
  double* iout = a.iout + (size_t)item * 2 * m;
  auto V = [&](int c) -> double { return c <= m ? 0.0 : (c > T - m ? Va : x_at(s_x, m, N, c - m - 1)); };
#pragma unroll 1
  for (int idx = t; idx < 2 * m; idx += NT)
    iout[idx] = electrode_current(
        g, electrode_site(g, idx), a.cur_rule, [&](int j) -> double { return s_el[idx * 6 + j]; }, V);
  if (t == 0) {
    BatchOut* out = a.out + item;
    out->status = 0;
    out->iter = k;
    out->err = err;
  }
}

}  // namespace

hipError_t dev_batch_w_launch(perc_ctx* h, int kind, bool literal, const BatchItemArgs& c,
                              const BatchWItems& w, int nitems) {
  const BatchWArgs a{c, batch_w_lds(h->g, kind), w};
  return dispatch_threads(batch_w_threads(h->N), [&](auto nt, int slot) {
    return dispatch_kind_order(kind, literal, [&](auto lit, auto kd) {
      return launch_lds(&k_batch_cond_w<nt(), lit(), kd()>, &h->w_lds[slot][lit()][kd()], a, nitems, nt(),
                        h->stream, "k_batch_cond_w");
    });
  });
}

hipError_t dev_twister_launch(perc_ctx* h, int nseeds, const unsigned* d_seeds, long long n, double* d_out) {
  if (nseeds <= 0 || n <= 0) return hipSuccess;
  k_twister_stream<<<nseeds, 64, 0, h->stream>>>(nseeds, d_seeds, n, d_out);
  return dbg_sync(h->stream, "k_twister_stream");
}

}  // namespace perc
