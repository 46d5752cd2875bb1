// perc_batch.hip -- k_batch_cond: one workgroup takes one small realisation
// (PERC_BOND with PERC_RULE_BOND, PERC_SITE with PERC_RULE_SITE or
// PERC_SITEBOND with PERC_RULE_MIXED; either current rule) from occupancy to
// terminal currents with no host round trip -- occupancy from the trial's
// rank arrays, union-find labeling in LDS, the spanning rule of k_span_top,
// assemble_row, k_cg_small's loop (both dot orders) and k_currents' per-site
// expression.  Many items per launch: the ensemble's (trial, grid point)
// pairs side by side instead of a dozen launches and one busy CU each.
// The front end, the workgroup sum and the currents are perc_batch_item.h's,
// shared with k_batch_cond_large and k_batch_cond_w; this file keeps the
// kernel's assembly and CG loop, the batch path's device buffers and
// dev_batch_run, which fills the common argument block for all three.
#include "perc_batch_currents.h"

namespace perc {
namespace {

struct BatchArgs : BatchItemArgs {
  BatchLds L;
};
// ... of the FIELDS instantiations: the items' records, their interior
// voltages (items x N, or NULL) and the backbone cut (device pointers)
struct BatchFieldArgs : BatchArgs {
  perc_batch_currents* cur;
  double* vint;
  double cut;
};

// NT threads, rows t, t + NT, .. (at most kBatchEPT) per thread.  LIT: the
// literal dot order (wave 0 folds every sum in ascending j, fold_chunk) --
// bitwise k_fold_init + k_cg_small<true, true>; else per thread in row
// order, wave butterfly, waves in order.  KIND: PERC_BOND / PERC_SITE /
// PERC_SITEBOND, with the kind's own conductance rule (the rules' numbers are
// the kinds').  FIELDS: after the electrode currents, the item's bond-current
// record (perc_batch_currents.h) and, where asked for, x itself -- an epilogue
// over what the solve leaves in LDS: x in s_q (p is dead), the row codes, the
// form table; the record's scratch is s_red.  The other instantiations take
// BatchArgs and hold none of it.
template <int NT, bool LIT, int KIND, bool FIELDS>
__global__ __launch_bounds__(NT) void k_batch_cond(std::conditional_t<FIELDS, BatchFieldArgs, BatchArgs> a) {
  static_assert(PERC_RULE_BOND == PERC_BOND && PERC_RULE_SITE == PERC_SITE &&
                    PERC_RULE_MIXED == PERC_SITEBOND, "a kind's rule has its number");
  constexpr int RULE = KIND;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Geom g = a.g;
  const int m = g.m, T = g.t, N = a.N;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int item = blockIdx.x;
  // labeling view of the arena
  const LabelArrays lv = label_arrays<KIND>(smem, a.L.oBocc, a.L.oMem, a.L.oFlag, a.L.oSocc);
  // solver view
  double* s_p = reinterpret_cast<double*>(smem);
  double* s_q = reinterpret_cast<double*>(smem + a.L.oQ);
  uint16_t* s_c = reinterpret_cast<uint16_t*>(smem + a.L.oC);
  double* s_red = reinterpret_cast<double*>(smem + a.L.oRed);
  int* s_off = reinterpret_cast<int*>(smem + a.L.oOff);
  StencilForms* sF = reinterpret_cast<StencilForms*>(smem + a.L.oF);
  double* s_rhs = reinterpret_cast<double*>(smem + a.L.oRhs);
  uint16_t* s_cur = reinterpret_cast<uint16_t*>(smem + a.L.oCur);
  int* s_i = reinterpret_cast<int*>(smem + a.L.oInt);

  // ---- occupancy, labeling, spanning, the item's header (perc_batch_item.h)
  const BatchFront front = batch_front<NT, KIND>(a, g, lv, sF, s_off, s_i);
  if (front.stop) return;
  const int root = front.root;

  // ---- assembly: row codes into LDS, the top system row's rhs (the only
  // rows with a non-zero one), the electrode rows' slot values as 2-bit codes
  const double g0 = a.g0, leak = a.leak, Va = a.Va;
#pragma unroll 1
  for (int i = t; i < N; i += NT) {
    uint16_t c;
    double b;
    assemble_row_vals<false>(g, i, a.bond_first, lv.bocc, lv.socc, lv.parent, nullptr, nullptr, nullptr, &b,
                             &c, a.sflag, *sF, a.fast, a.fl, a.fr, a.bf_closed, RULE, g0, leak, Va,
                             root, nullptr);
    s_c[i] = c;
    if (i >= N - m) s_rhs[i - (N - m)] = b;
  }
  encode_electrode_rows<NT, RULE>(g, a.bond_first, lv, root, g0, leak, s_cur);
  __syncthreads();  // the labeling arrays are dead from here: p and q take their place

  // ---- solve: k_cg_small<true, LIT>, the prologue included (x = 0, r = b)
  const double ng0 = -g0, nleak = -leak;
  // the literal order at 1024 threads (128 VGPRs per thread) rebuilds a row's
  // diagonal from its code in LDS where the p update needs it, rather than
  // hold eight of them across the loop: the same value, and no scratch
  constexpr bool kKeepDiag = !(LIT && NT == 1024);
  double rv[kBatchEPT], dv[kBatchEPT], xv[kBatchEPT];
#pragma unroll
  for (int j = 0; j < kBatchEPT; ++j) {
    const int i = t + j * NT;
    const unsigned c = i < N ? (unsigned)s_c[i] : 0u;
    rv[j] = i < N && i >= N - m ? s_rhs[i - (N - m)] : 0.0;
    xv[j] = 0.0;
    dv[j] = i < N ? code_diag(c, ng0, nleak) : 1.0;
  }
  const int itol = a.itol, itmax = a.itmax;
  const double tol = a.tol;
  double bnrm, bknum;
  if constexpr (LIT) {  // k_fold_init: bnrm^2 and the first bknum in ascending j
#pragma unroll
    for (int j = 0; j < kBatchEPT; ++j) {
      const int i = t + j * NT;
      if (i < N) s_q[i] = rv[j];
    }
    __syncthreads();
    if (wid == 0) {
      double acc[2] = {0.0, 0.0};
      for (int j0 = 0; j0 < N; j0 += 64) {
        const int j = min(j0 + lane, N - 1);
        const double rj = s_q[j];
        const double dj = code_diag(s_c[j], ng0, nleak);
        const double zb = itol == 1 ? rj : rj / dj, z = rj / dj;
        const double tz[2] = {zb * zb, z * rj};
        fold_chunk<2>(tz, min(64, N - j0), acc);
      }
      if (lane == 0) {
        s_red[32] = sqrt(acc[0]);
        s_red[33] = acc[1];
      }
    }
    __syncthreads();
    bnrm = s_red[32];
    bknum = s_red[33];
    __syncthreads();
  } else {
    double b2 = 0.0, zr0 = 0.0;
#pragma unroll
    for (int j = 0; j < kBatchEPT; ++j) {
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
    // p(k) = bk p(k-1) + z (k = 1: p = z), linbcg :789-797
#pragma unroll
    for (int j = 0; j < kBatchEPT; ++j) {
      const int i = t + j * NT;
      if (i < N) {
        const double z = rv[j] / (kKeepDiag ? dv[j] : code_diag(s_c[i], ng0, nleak));
        s_p[i] = k == 1 ? z : bk * s_p[i] + z;
      }
    }
    __syncthreads();
    // q = A p (dsprsax order) into LDS, and q.p
    double dot = 0.0;
#pragma unroll 1
    for (int i = t; i < N; i += NT) {
      const double pi = s_p[i];
      const unsigned c = s_c[i];
      const int f = c >> 11, cnt = (c >> 8) & 7;
      double xn[kMaxSlots];
      bool use[kMaxSlots];
#pragma unroll
      for (int e = 0; e < kMaxSlots; ++e) {
        const int col = i + s_off[f * kMaxSlots + e];
        use[e] = e < cnt && (unsigned)col < (unsigned)N;
        xn[e] = s_p[use[e] ? col : i];
      }
      const double q = st_combine<kMaxSlots>(c, xn, use, pi, ng0, nleak);
      dot = dot + q * pi;
      s_q[i] = q;
    }
    double akden, unused;
    if constexpr (LIT) {
      __syncthreads();  // s_q complete
      if (wid == 0) {
        double acc[1] = {0.0};
        for (int j0 = 0; j0 < N; j0 += 64) {
          const int j = min(j0 + lane, N - 1);
          const double tq[1] = {s_q[j] * s_p[j]};  // akden, bondc.f:803-805
          fold_chunk<1>(tq, min(64, N - j0), acc);
        }
        if (lane == 0) s_red[32] = acc[0];
      }
      __syncthreads();
      akden = s_red[32];
      __syncthreads();
    } else {
      wg_sum2<NT>(s_red, dot, 0.0, &akden, &unused);
    }
    ak = bknum / akden;
    // x += ak p, r -= ak q, z = r/d, z.r and r.r (linbcg :801-806, 808-813)
    double zr = 0.0, rr = 0.0;
#pragma unroll
    for (int j = 0; j < kBatchEPT; ++j) {
      const int i = t + j * NT;
      if (i < N) {
        xv[j] = xv[j] + ak * s_p[i];
        const double rn = rv[j] - ak * s_q[i];
        rv[j] = rn;
        const double z = rn / dv[j];
        zr = zr + z * rn;
        rr = rr + rn * rn;
      }
    }
    double tzr, trr;
    if constexpr (LIT) {
      // r(k+1) through LDS (q is dead until the next iteration's)
#pragma unroll
      for (int j = 0; j < kBatchEPT; ++j) {
        const int i = t + j * NT;
        if (i < N) s_q[i] = rv[j];
      }
      __syncthreads();
      if (wid == 0) {
        double acc[2] = {0.0, 0.0};
        for (int j0 = 0; j0 < N; j0 += 64) {
          const int j = min(j0 + lane, N - 1);
          const double rj = s_q[j];
          const double zj = rj / code_diag(s_c[j], ng0, nleak);
          const double tz[2] = {zj * rj, rj * rj};  // bknum :785-787, snrm :872-875
          fold_chunk<2>(tz, min(64, N - j0), acc);
        }
        if (lane == 0) {
          s_red[32] = acc[0];
          s_red[33] = acc[1];
        }
      }
      __syncthreads();
      tzr = s_red[32];
      trr = s_red[33];
      __syncthreads();
    } else {
      wg_sum2<NT>(s_red, zr, rr, &tzr, &trr);
    }
    err = sqrt(trr) / bnrm;
    bk = tzr / bknum;
    bknum = tzr;
    // err comes from one LDS value in every thread: a uniform break
    if (!(err > tol) || k >= itmax + 1) break;
  }

  // ---- currents: k_currents' expression of the current rule on the 2m
  // electrode sites, x through LDS (q is dead)
#pragma unroll
  for (int j = 0; j < kBatchEPT; ++j) {
    const int i = t + j * NT;
    if (i < N) s_q[i] = xv[j];
  }
  __syncthreads();
  const double* x = s_q;
  double* iout = a.iout + (size_t)item * 2 * m;
  auto V = [&](int c) -> double { return c <= m ? 0.0 : (c > T - m ? Va : x[c - m - 1]); };
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
  if constexpr (FIELDS) {
    if (a.vint) {  // (a kernel argument: uniform) x(i) as its owner left it in LDS, coalesced over t
      double* v = a.vint + (size_t)item * N;
#pragma unroll 1
      for (int i = t; i < N; i += NT) v[i] = x[i];
    }
    batch_currents_record<NT>(N, x, s_c, s_off, s_red, g0, Va, a.cut, a.cur + item);
  }
}

// The context's one rank store: per list (0: bonds, ntrials x nb; 1: sites,
// ntrials x t) the ranks in device memory with the trials they hold, and the
// pinned host row a call forms them in (a fresh pageable array of a launch's
// 64 MB costs more in page faults and the runtime's staged copy than the
// kernels run).  perc_batch.h states its contract.
struct RankStore {
  int* d_rank[2] = {};
  size_t cap[2] = {};
  int held[2] = {};
  int* h_row[2] = {};
  size_t hcap[2] = {};
  bool in_flight[2] = {};  // a commit's copy may still read h_row
};

struct BatchState {
  RankStore ranks;
  ItemLists<BatchOut, 3> items;  // item_trial, then item_count, then item_nsites
  double* d_iout = nullptr;
  size_t iout_cap = 0;
  int* d_sflag = nullptr;
  int lds_attr[3][2][3] = {};  // dynamic LDS granted per instantiation
  int lds_attr_f[3][2][3] = {};  // ... of the FIELDS ones
  // perc_batch_cond_currents: the launch's records and interior voltages
  perc_batch_currents* d_cur = nullptr;
  double* d_vint = nullptr;
  size_t cur_cap = 0, vint_cap = 0;
  // perc_batch_cond_weighted: the chunk's explicit weight rows or its draws
  // (d_wsrc), the ConductCalc rows the kernel writes (d_wscr, items x nb), the
  // items' row numbers or seeds (d_wsel); perc_batch_twister's seeds and
  // output go through d_wsel and d_wsrc too
  double* d_wsrc = nullptr;
  double* d_wscr = nullptr;
  unsigned* d_wsel = nullptr;
  size_t wsrc_cap = 0, wscr_cap = 0, wsel_cap = 0;
};

}  // namespace

static BatchState* batch_state(perc_ctx* h) {
  if (!h->batch) h->batch = new BatchState();
  return static_cast<BatchState*>(h->batch);
}

void dev_batch_free(perc_ctx* h) {
  BatchState* B = static_cast<BatchState*>(h->batch);
  if (!B) return;
  for (int l = 0; l < 2; ++l) {
    (void)hipFree(B->ranks.d_rank[l]);
    if (B->ranks.h_row[l]) (void)hipHostFree(B->ranks.h_row[l]);
  }
  B->items.release();
  (void)hipFree(B->d_iout);
  (void)hipFree(B->d_sflag);
  (void)hipFree(B->d_wsrc);
  (void)hipFree(B->d_wscr);
  (void)hipFree(B->d_wsel);
  (void)hipFree(B->d_cur);
  (void)hipFree(B->d_vint);
  delete B;
  h->batch = nullptr;
}

// a list's slot in the store, and the ints of one trial of it
static int rank_slot(int list) { return list == PERC_BOND ? 0 : 1; }
static size_t rank_len(perc_ctx* h, int list) { return (size_t)(list == PERC_BOND ? h->nb : h->g.t); }

const int* dev_batch_ranks(perc_ctx* h, int list, int* ntrials) {
  BatchState* B = static_cast<BatchState*>(h->batch);
  const int l = rank_slot(list);
  *ntrials = B && B->ranks.d_rank[l] ? B->ranks.held[l] : 0;
  return B ? B->ranks.d_rank[l] : nullptr;
}

hipError_t dev_batch_reserve(perc_ctx* h, int list, int ntrials, int** d_rank) {
  RankStore& R = batch_state(h)->ranks;
  const int l = rank_slot(list);
  R.held[l] = 0;
  HIP_TRY(grow(&R.d_rank[l], &R.cap[l], (size_t)ntrials * rank_len(h, list)));
  R.held[l] = ntrials;
  *d_rank = R.d_rank[l];
  return hipSuccess;
}

hipError_t dev_batch_stage(perc_ctx* h, int list, int ntrials, int** row) {
  RankStore& R = batch_state(h)->ranks;
  const int l = rank_slot(list);
  if (R.in_flight[l]) HIP_TRY(hipStreamSynchronize(h->stream));
  R.in_flight[l] = false;
  HIP_TRY(grow_pinned(&R.h_row[l], &R.hcap[l], (size_t)ntrials * rank_len(h, list)));
  *row = R.h_row[l];
  return hipSuccess;
}

hipError_t dev_batch_commit(perc_ctx* h, int list, int ntrials) {
  RankStore& R = batch_state(h)->ranks;
  const int l = rank_slot(list);
  const size_t n = (size_t)ntrials * rank_len(h, list);
  if (R.hcap[l] < n) return hipErrorInvalidValue;  // (no stage of that many trials)
  int* d_rank = nullptr;
  HIP_TRY(dev_batch_reserve(h, list, ntrials, &d_rank));
  R.in_flight[l] = n > 0;
  if (n) HIP_TRY(hipMemcpyAsync(d_rank, R.h_row[l], sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  return hipSuccess;
}

hipError_t dev_batch_twister(perc_ctx* h, int nseeds, const unsigned* seeds, long long n, double* out) {
  if (nseeds <= 0 || n <= 0) return hipSuccess;
  BatchState* B = batch_state(h);
  hipStream_t st = h->stream;
  // launches whose output stays under 64 MB of device memory
  const long long per = std::max(1LL, std::min<long long>(nseeds, (64LL << 20) / (8 * n)));
  HIP_TRY(grow(&B->d_wsel, &B->wsel_cap, (size_t)per));
  HIP_TRY(grow(&B->d_wsrc, &B->wsrc_cap, (size_t)per * (size_t)n));
  for (long long s0 = 0; s0 < nseeds; s0 += per) {
    const int k = (int)std::min<long long>(per, nseeds - s0);
    HIP_TRY(hipMemcpyAsync(B->d_wsel, seeds + s0, sizeof(unsigned) * k, hipMemcpyHostToDevice, st));
    HIP_TRY(dev_twister_launch(h, k, B->d_wsel, n, B->d_wsrc));
    HIP_TRY(hipMemcpyAsync(out + (size_t)s0 * (size_t)n, B->d_wsrc, sizeof(double) * (size_t)k * (size_t)n,
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return hipSuccess;
}

hipError_t dev_batch_run(perc_ctx* h, int kind, const BatchSolve& sv, int nitems, const int* item_trial,
                         const int* item_nsites, const int* item_count, BatchOut* out, double* iout, bool large,
                         const BatchWeights* wts, const BatchFields* fld) {
  if (nitems == 0) return hipSuccess;
  BatchState* B = batch_state(h);
  hipStream_t st = h->stream;
  const int m = h->g.m;
  const bool need_s = kind != PERC_BOND, need_b = kind != PERC_SITE;
  // every item's trial must lie in the rank arrays the store holds for the kind
  int have = INT_MAX, held = 0;
  const int* d_rank_b = dev_batch_ranks(h, PERC_BOND, &held);
  if (need_b) have = std::min(have, held);
  const int* d_rank_s = dev_batch_ranks(h, PERC_SITE, &held);
  if (need_s) have = std::min(have, held);
  for (int i = 0; i < nitems; ++i)
    if (item_trial[i] < 0 || item_trial[i] >= have) {
      set_error("k_batch_cond: an item's trial lies outside the uploaded rank arrays");
      return hipErrorInvalidValue;
    }
  if (!B->d_sflag) {
    HIP_TRY(dmalloc(&B->d_sflag, 4));
    HIP_TRY(hipMemsetAsync(B->d_sflag, 0, 4 * sizeof(int), st));
  }
  const int solve = sv.solve ? 1 : 0;
  const bool literal = sv.literal;
  const size_t niout = solve ? (size_t)nitems * 2 * m : 0;
  HIP_TRY(grow(&B->d_iout, &B->iout_cap, niout));
  HIP_TRY(B->items.upload((size_t)nitems,
                          {item_trial, need_b ? item_count : nullptr, need_s ? item_nsites : nullptr}, st));
  // an item that stops before the currents leaves its iout row unwritten
  if (niout) HIP_TRY(hipMemsetAsync(B->d_iout, 0, sizeof(double) * niout, st));
  // ... and its record and voltages: all zero
  const size_t nvint = fld && fld->vint ? (size_t)nitems * (size_t)h->N : 0;
  if (fld) {
    HIP_TRY(grow(&B->d_cur, &B->cur_cap, (size_t)nitems));
    HIP_TRY(grow(&B->d_vint, &B->vint_cap, nvint));
    HIP_TRY(hipMemsetAsync(B->d_cur, 0, sizeof(perc_batch_currents) * nitems, st));
    if (nvint) HIP_TRY(hipMemsetAsync(B->d_vint, 0, sizeof(double) * nvint, st));
  }
  BatchItemArgs c;
  c.g = h->g;
  c.N = h->N;
  c.nb = (int)h->nb;
  c.bond_first = h->d.bond_first;
  c.forms = h->d.forms_dev;
  c.rank = d_rank_b;
  c.rank_s = d_rank_s;
  c.item_trial = B->items.list(0, nitems);
  c.item_count = B->items.list(1, nitems);
  c.item_nsites = B->items.list(2, nitems);
  c.out = B->items.d_out;
  c.iout = B->d_iout;
  c.sflag = B->d_sflag;
  asm_closed_forms(h, &c.fast, &c.fl, &c.fr);
  c.bf_closed = h->bf_closed ? 1 : 0;
  c.solve = solve;
  c.itol = sv.itol;
  c.itmax = sv.itmax;
  c.cur_rule = sv.cur_rule;
  c.Va = sv.Va;
  c.g0 = sv.g0;
  c.leak = sv.leak;
  c.tol = sv.tol;
  hipError_t e;
  if (fld) {  // k_batch_cond's FIELDS instantiations: the common block, the plan and the fields
    BatchFieldArgs a;
    static_cast<BatchItemArgs&>(a) = c;
    a.L = batch_lds(h->g, kind);
    a.cur = B->d_cur;
    a.vint = nvint ? B->d_vint : nullptr;
    a.cut = fld->cut;
    e = dispatch_threads(batch_threads(h->N), [&](auto nt, int slot) {
      return dispatch_kind_order(kind, literal, [&](auto lit, auto kd) {
        return launch_lds(&k_batch_cond<nt(), lit(), kd(), true>, &B->lds_attr_f[slot][lit()][kd()], a, nitems,
                          nt(), st, "k_batch_cond");
      });
    });
  } else if (wts) {  // k_batch_cond_w (perc_batch_weighted.hip): the common block and the weights
    const size_t nb = (size_t)c.nb;
    BatchWItems b;
    HIP_TRY(grow(&B->d_wsel, &B->wsel_cap, (size_t)nitems));
    if (wts->item_wset) {
      // the rows this launch's items name, each uploaded once, numbered as met
      std::vector<int> local((size_t)wts->nwsets, -1), sel((size_t)nitems), rows;
      for (int i = 0; i < nitems; ++i) {
        int& l = local[(size_t)wts->item_wset[i]];
        if (l < 0) {
          l = (int)rows.size();
          rows.push_back(wts->item_wset[i]);
        }
        sel[i] = l;
      }
      HIP_TRY(grow(&B->d_wsrc, &B->wsrc_cap, rows.size() * nb));
      for (size_t r = 0; r < rows.size(); ++r)
        HIP_TRY(hipMemcpyAsync(B->d_wsrc + r * nb, wts->weights + (size_t)rows[r] * nb, sizeof(double) * nb,
                               hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(B->d_wsel, sel.data(), sizeof(int) * nitems, hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));  // (sel goes away)
      b.item_wset = reinterpret_cast<const int*>(B->d_wsel);
      b.wrows = B->d_wsrc;
    } else {
      HIP_TRY(grow(&B->d_wsrc, &B->wsrc_cap, (size_t)nitems * nb));
      b.wstride = (c.nb + 15) & ~15;
      HIP_TRY(grow(&B->d_wscr, &B->wscr_cap, (size_t)nitems * (size_t)b.wstride));
      HIP_TRY(hipMemcpyAsync(B->d_wsel, wts->item_wseed, sizeof(unsigned) * nitems, hipMemcpyHostToDevice, st));
      HIP_TRY(dev_twister_launch(h, nitems, B->d_wsel, (long long)nb, B->d_wsrc));
      b.u = B->d_wsrc;
      b.wscratch = B->d_wscr;
    }
    e = dev_batch_w_launch(h, kind, literal, c, b, nitems);
  } else if (large) {  // k_batch_cond_large (perc_batch_large.hip)
    e = dev_batch_large_launch(h, kind, literal, c, nitems);
  } else {
    const BatchArgs a{c, batch_lds(h->g, kind)};
    e = dispatch_threads(batch_threads(h->N), [&](auto nt, int slot) {
      return dispatch_kind_order(kind, literal, [&](auto lit, auto kd) {
        return launch_lds(&k_batch_cond<nt(), lit(), kd(), false>, &B->lds_attr[slot][lit()][kd()], a, nitems,
                          nt(), st, "k_batch_cond");
      });
    });
  }
  HIP_TRY(e);
  int flag = 0;
  HIP_TRY(hipMemcpyAsync(out, B->items.d_out, sizeof(BatchOut) * nitems, hipMemcpyDeviceToHost, st));
  if (niout) HIP_TRY(hipMemcpyAsync(iout, B->d_iout, sizeof(double) * niout, hipMemcpyDeviceToHost, st));
  if (fld) {
    HIP_TRY(hipMemcpyAsync(fld->cur, B->d_cur, sizeof(perc_batch_currents) * nitems, hipMemcpyDeviceToHost, st));
    if (nvint) HIP_TRY(hipMemcpyAsync(fld->vint, B->d_vint, sizeof(double) * nvint, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipMemcpyAsync(&flag, B->d_sflag, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (flag & 3) {  // a row without its stencil bond or form: perc_batch_supported excludes it
    set_error("k_batch_cond: a row does not fit the stencil operator");
    return hipErrorInvalidValue;
  }
  return hipSuccess;
}

}  // namespace perc

