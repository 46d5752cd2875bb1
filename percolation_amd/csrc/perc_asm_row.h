// perc_asm_row.h -- one row of the Kirchhoff assembly (bondc.f:482-538,
// ConductCalc.m:88-165): device code shared by perc_assemble.hip (k_assemble)
// and perc_batch.hip (k_batch_cond).  Anonymous namespace: each translation
// unit keeps its own copy.
#pragma once
#include "perc_stencil.h"

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
namespace perc {
namespace {

// ---------------------------------------------------------------------------
// Kirchhoff assembly (bondc.f:482-538, ConductCalc.m:88-165)
// w (optional): ConductCalc.m condtype 2, G = -g0*rand for the bonds of the
// spanning cluster (ConductCalc.m:94-97): per-bond multipliers w[id]
__device__ __forceinline__ double bond_value(int rule, int id, int s, int c, int ps,
                                             const uint8_t* bocc, const uint8_t* socc,
                                             int span_root, double g0, double leak,
                                             const double* w) {
  bool in;
  if (rule == PERC_RULE_BOND) in = bocc[id] && ps == span_root;
  else if (rule == PERC_RULE_SITE) in = socc[s] && socc[c] && ps == span_root;
  else in = bocc[id] && socc[s] && socc[c] && ps == span_root;
  return in ? (w ? -g0 * w[id] : -g0) : -leak;
}

// CSR: also the NR-ordered CSR values and the diagonal array (the CSR and
// split formats, perc_get_system, the probes).  The stencil solvers read
// only code and rhs, so dev_assemble writes the CSR copy only when a
// consumer asks for it (ensure_csr): 2 + 8 B per row instead of 50.
// assemble_row_vals: the row's code and rhs returned through *code_out /
// *rhs_out (the batch kernel keeps them in LDS and registers);
// assemble_row stores them at code[i] / rhs[i].  gvs_out (optional): the
// row's slot values gvs_out[j * gvs_stride], j < cnt, in slot order, 0.0 for
// a slot without its bond (the weighted batch kernel's per-slot arrays in
// LDS; a null pointer, the default, leaves every other instantiation as it
// was).
template <bool CSR>
__device__ __forceinline__ void assemble_row_vals(
    const Geom& g, int i, const int* bond_first, const uint8_t* bocc, const uint8_t* socc,
    const int* parent, const int* rowptr, double* val, double* diag, double* rhs_out,
    uint16_t* code_out, int* sflag, const StencilForms& F, int fast_form, int fast_l, int fast_r, int bf_closed,
    int rule, double g0,
    double leak, double Va, int span_root, const double* w, double* gvs_out = nullptr,
    int gvs_stride = 1) {
  const int m = g.m, t = g.t, s = i + m + 1;
  const int ps = parent[s];
  const int sr = div_m(g, s - 1), sc = s - 1 - sr * m;
  // Square lattice, closed forms (the host found each form in the table and
  // checked its deltas): the sorted neighbours and their bond ids follow
  // from nearestn_square case by case --
  //   interior column: s-m, s-1, s+1, s+m; ids bf(s-m)+1, bf(s-1), fb, fb+1
  //     (s is the 2nd forward neighbour of s-m, the 1st of s-1 -- every
  //     nearestn_square case lists +1 before +m);
  //   column 0: s-m, s+1, [s+m-1 (pbc)], s+m; ids bf(s-m)+1, fb, [fb+2], fb+1
  //     (s's forward order is s+1, s+m, s+m-1);
  //   column m-1: s-m, [s-m+1 (pbc)], s-1, s+m; ids bf(s-m), [bf(s-m+1)+2],
  //     bf(s-1), fb (s-m's only forward neighbour is s; s is the 3rd of s-m+1).
  // RHS (top system row): the one forward neighbour above, s+m (the pbc
  // wrap neighbour s+m-1 of column 0 is in s's own row).  Every load is issued before any
  // is used (bond_value's short-circuit loads would serialise the latencies).
  const int kind_c = sc >= 1 && sc <= m - 2 ? 0 : (sc == 0 ? 1 : 2);
  const int cform = kind_c == 0 ? fast_form : kind_c == 1 ? fast_l : fast_r;
  if (cform >= 0) {
    const bool pb = g.pbc != 0;
    int fb, bl, bd, bw = 0;  // bond_first of s, s-1, s-m, s-m+1
    if (bf_closed) {
      fb = bf_square(g, sr, sc);
      bl = sc > 0 ? bf_square(g, sr, sc - 1) : 0;
      bd = bf_square(g, sr - 1, sc);
      bw = bf_square(g, sr, 0);
    } else {
      fb = bond_first[s];
      bl = sc > 0 ? bond_first[s - 1] : 0;
      bd = bond_first[s - m];
      bw = kind_c == 2 && pb ? bond_first[s - m + 1] : 0;
    }
    int cs[4], ids[4], cnt;
    if (kind_c == 0) {
      cnt = 4;
      cs[0] = s - m; cs[1] = s - 1; cs[2] = s + 1; cs[3] = s + m;
      ids[0] = bd + 1; ids[1] = bl; ids[2] = fb; ids[3] = fb + 1;
    } else if (kind_c == 1) {
      cnt = pb ? 4 : 3;
      cs[0] = s - m; cs[1] = s + 1; cs[2] = pb ? s + m - 1 : s + m; cs[3] = s + m;
      ids[0] = bd + 1; ids[1] = fb; ids[2] = pb ? fb + 2 : fb + 1; ids[3] = fb + 1;
    } else {
      cnt = pb ? 4 : 3;
      cs[0] = s - m; cs[1] = pb ? s - m + 1 : s - 1; cs[2] = pb ? s - 1 : s + m; cs[3] = s + m;
      ids[0] = bd; ids[1] = pb ? bw + 2 : bl; ids[2] = pb ? bl : fb; ids[3] = fb;
    }
    unsigned bo[4], so[4] = {1u, 1u, 1u, 1u}, ss = 1u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bo[j] = rule == PERC_RULE_SITE ? 1u : bocc[ids[j]];
    if (rule != PERC_RULE_BOND) {
      ss = socc[s];
#pragma unroll
      for (int j = 0; j < 4; ++j) so[j] = socc[cs[j]];
    }
    const bool root = ps == span_root;
    double gvs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // bond_value
      const bool in = root && bo[j] != 0u && ss != 0u && so[j] != 0u;
      gvs[j] = in ? (w ? -g0 * w[ids[j]] : -g0) : -leak;
    }
    double rowsum = 0.0;
    unsigned bits = 0;
    int k = CSR ? rowptr[i] : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= cnt) break;
      const double gv = gvs[j];
      if (gv == -g0) bits |= 1u << j;
      rowsum = rowsum + gv;
      if (CSR && cs[j] > m && cs[j] <= t - m) val[k++] = gv;
      if (gvs_out) gvs_out[j * gvs_stride] = gv;
    }
    *code_out = (uint16_t)(bits | (unsigned)cnt << 8 | (unsigned)cform << 11);
    if (CSR) diag[i] = -rowsum;
    double acc = 0.0;
    if (s > t - 2 * m) acc = acc - (gvs[cnt - 1] * Va);  // (s, s+m): the last slot
    *rhs_out = acc;
    return;
  }
  // one division per neighbour (div_m); nearestn of the row once and of
  // each smaller neighbour once -- the bond ids of bond_id
  int nn[6];
  nearestn_rc(g, s, sr, sc, nn);
  const int fb = bond_first[s];
  int nbr[6], cnt = 0;  // sorted_neighbours
  for (int k = 0; k < g.scn; ++k)
    if (nn[k] != 0) {
      const int v = nn[k];
      int j = cnt;
      while (j > 0 && nbr[j - 1] > v) { nbr[j] = nbr[j - 1]; --j; }
      nbr[j] = v;
      ++cnt;
    }
  double rowsum = 0.0;  // bondc.f:500-504: ascending-column dense row sum
  int k = CSR ? rowptr[i] : 0;
  unsigned bits = 0;
  int drs[6], dcs[6];
  for (int j = 0; j < cnt; ++j) {
    const int c = nbr[j];
    const int cr = div_m(g, c - 1), cc = c - 1 - cr * m;
    int d = cc - sc;  // lattice_delta
    if (d > 1) d -= m;
    else if (d < -1) d += m;
    drs[j] = cr - sr;
    dcs[j] = d;
    int id;
    if (s < c) {
      id = fwd_bond_id(g, nn, fb, s, c);
    } else {
      int nc[6];
      nearestn_rc(g, c, cr, cc, nc);
      id = fwd_bond_id(g, nc, bond_first[c], c, s);
    }
    if (id < 0) {  // no bond in this slot: the stencil operator cannot be used
      atomicOr(sflag, 1);
      if (gvs_out) gvs_out[j * gvs_stride] = 0.0;
      continue;
    }
    const double gv = bond_value(rule, id, s, c, ps, bocc, socc, span_root, g0, leak, w);
    if (gvs_out) gvs_out[j * gvs_stride] = gv;
    if (gv == -g0) bits |= 1u << j;
    rowsum = rowsum + gv;
    if (CSR && c > m && c <= t - m) val[k++] = gv;
  }
  int form = -1;  // the row's form: same count and offsets
  for (int f = 0; f < F.nforms && form < 0; ++f) {
    bool same = F.cnt[f] == cnt;
    for (int j = 0; j < cnt && same; ++j) same = F.off[f][j] == nbr[j] - s;
    if (same) form = f;
  }
  if (form < 0) {
    atomicOr(sflag, 2);
    form = 0;
  }
  for (int j = 0; j < cnt; ++j) {  // the tiled kernel reads slot j at (row, col) + (dr, dc)
    const int dr = drs[j], dc = dcs[j];
    if (dr != F.dr[form][j] || dc != F.dc[form][j] || dr < -1 || dr > 1 || dc < -1 || dc > 1)
      atomicOr(sflag, 4);
  }
  *code_out = (uint16_t)(bits | (unsigned)cnt << 8 | (unsigned)form << 11);
  if (CSR) diag[i] = -rowsum;
  // RHS in bond-list order (bondc.f:490-497)
  double acc = 0.0;
  if (s > t - 2 * m && s <= t - m) {
    int r = 0;
    for (int kk = 0; kk < g.scn; ++kk) {
      const int q = nn[kk];
      if (q <= s) continue;
      if (q > t - m) {
        const double gv =
            bond_value(rule, fb + r, s, q, ps, bocc, socc, span_root, g0, leak, w);
        acc = acc - (gv * Va);
      }
      ++r;
    }
  }
  *rhs_out = acc;
}

template <bool CSR>
__device__ __forceinline__ void assemble_row(
    const Geom& g, int i, const int* bond_first, const uint8_t* bocc, const uint8_t* socc,
    const int* parent, const int* rowptr, double* val, double* diag, double* rhs, uint16_t* code,
    int* sflag, const StencilForms& F, int fast_form, int fast_l, int fast_r, int bf_closed,
    int rule, double g0,
    double leak, double Va, int span_root, const double* w) {
  uint16_t c;
  double b;
  assemble_row_vals<CSR>(g, i, bond_first, bocc, socc, parent, rowptr, val, diag, &b, &c, sflag, F,
                         fast_form, fast_l, fast_r, bf_closed, rule, g0, leak, Va, span_root, w);
  code[i] = c;
  rhs[i] = b;
}

}  // namespace
}  // namespace perc
#pragma clang diagnostic pop
