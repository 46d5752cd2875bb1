// perc_batch_currents.h -- the bond-current epilogue of k_batch_cond's FIELDS
// instantiations (perc_batch.hip; the definition: include/perc.h,
// perc_batch_currents): over the conducting bonds
// with an interior end site, |i| = |g0 (V[b2] - V[b1])| into the count, the
// maximum, four power sums, an octave histogram and the count at or above
// cut * max.  The bin is perc_batch.h's current_bin, shared with the host.
#pragma once
#include "perc_batch_item.h"

namespace perc {
namespace {

// Every conducting bond with an interior end site, once: thread t walks rows
// t, t + NT, .., a row's slots ascending; a slot is taken when its in-bit is
// set (bit e of the row code: bond_value gave it g0) and its column lies
// above the row inside the system, or outside it -- below 0 the bottom
// electrode (V = 0), from N on the top one (V = Va): k_batch_cond's own test
// for a slot's column.  f(|i|) per bond.  x: the interior voltages in LDS.
template <int NT, class F>
__device__ __forceinline__ void walk_bond_currents(int N, const double* x, const uint16_t* s_c,
                                                   const int* s_off, double g0, double Va, F&& f) {
#pragma unroll 1
  for (int i = threadIdx.x; i < N; i += NT) {
    const unsigned c = s_c[i];
    const int fo = (int)(c >> 11) * kMaxSlots, cnt = (c >> 8) & 7;
    const double xi = x[i];
#pragma unroll 1  // (one pass per item beside hundreds of iterations: registers before speed)
    for (int e = 0; e < cnt; ++e) {
      if (!((c >> e) & 1u)) continue;
      const int col = i + s_off[fo + e];
      const bool inside = (unsigned)col < (unsigned)N;
      if (inside && col <= i) continue;  // the row below counts this bond
      const double xo = x[inside ? col : i];
      const double ib = inside ? g0 * (xo - xi) : (col < 0 ? g0 * (xi - 0.0) : g0 * (Va - xi));
      f(fabs(ib));
    }
  }
}

// Workgroup maximum of non-negative values: per-wave butterfly, then the
// waves in order (wg_sum2's tree; a maximum is the same in any order).
// s_red: 16 doubles.
template <int NT>
__device__ __forceinline__ double wg_max(double* s_red, double v) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  if (lane == 0) s_red[wid] = v;
  __syncthreads();
  double m = s_red[0];
  for (int w = 1; w < NT / 64; ++w) m = fmax(m, s_red[w]);
  __syncthreads();  // s_red reuse
  return m;
}

// The item's record.  Called by every thread of the workgroup after the
// solve, x complete in LDS behind a barrier; s_red (48 doubles) is free: as
// 96 ints it holds the histogram (0..63) in pass 1, then -- the bins copied
// into the first 64 threads' registers -- wg_sum2's and wg_max's wave totals
// in its first 32 doubles, with the two counters (ints 80, 81) beyond them.
// Every barrier is reached by every thread: no branch here depends on more
// than the thread's own rows.
template <int NT>
__device__ __forceinline__ void batch_currents_record(int N, const double* x, const uint16_t* s_c,
                                                      const int* s_off, double* s_red, double g0, double Va,
                                                      double cut, perc_batch_currents* rec) {
  static_assert(NT >= 96, "the first 96 threads clear s_red");
  const int t = threadIdx.x;
  int* si = reinterpret_cast<int*>(s_red);
  if (t < 96) si[t] = 0;
  __syncthreads();
  const int e0 = ilogb(g0 * Va);
  // pass 1: per thread in row order, slots ascending
  int nb = 0;
  double mx = 0.0, s1 = 0.0, s2 = 0.0, s4 = 0.0, s6 = 0.0;
  walk_bond_currents<NT>(N, x, s_c, s_off, g0, Va, [&](double a) {
    const double i2 = a * a, i4 = i2 * i2, i6 = i4 * i2;
    ++nb;
    mx = fmax(mx, a);
    s1 = s1 + a;
    s2 = s2 + i2;
    s4 = s4 + i4;
    s6 = s6 + i6;
    atomicAdd(&si[current_bin(e0, a)], 1);
  });
  if (nb) atomicAdd(&si[80], nb);
  __syncthreads();
  const int hv = t < 64 ? si[t] : 0;
  const int nbonds = si[80];
  __syncthreads();  // the bins are in registers: the sums take their place
  // (thread 0 stores a pair of sums as soon as it has them: held to the end,
  // every thread would keep the waves' totals in registers for it)
  double ta, tb;
  wg_sum2<NT>(s_red, s1, s2, &ta, &tb);
  if (t == 0) {
    rec->s1 = ta;
    rec->s2 = tb;
  }
  wg_sum2<NT>(s_red, s4, s6, &ta, &tb);
  if (t == 0) {
    rec->s4 = ta;
    rec->s6 = tb;
  }
  const double imax = wg_max<NT>(s_red, mx);  // (one LDS word per wave, read after a barrier)
  // pass 2: the same walk against cut * imax
  const double thr = cut * imax;
  int na = 0;
  walk_bond_currents<NT>(N, x, s_c, s_off, g0, Va, [&](double a) { na += a >= thr ? 1 : 0; });
  if (na) atomicAdd(&si[81], na);
  __syncthreads();
  if (t < 64) rec->hist[t] = hv;
  if (t == 0) {
    rec->nbonds = nbonds;
    rec->nabove = si[81];
    rec->imax = imax;
  }
}

}  // namespace
}  // namespace perc
