// CPU check of the register march's band split (percolation_amd/csrc/perc_bands.h):
// the bands of every strip are contiguous, do not overlap and cover [0, nrows)
// exactly, and the host's tallest band is the tallest of them.  Built and run
// by test_march_bands.py; prints one line per violation, exits 1 on any.
#include <cstdio>

#include "perc_bands.h"

int main() {
  using namespace perc;
  const int rows[] = {2, 3, 158, 510, 1022, 1398, 4094}, cycles[] = {1, 2, 64, 256}, heights[] = {1, 2, 8, 64};
  // the default P and B weights (kSlotW) and one lopsided set
  const int weights[3][4] = {{100, 76, 48, 40}, {100, 78, 55, 50}, {1, 1, 400, 1}};
  int bad = 0, checked = 0;
  auto fail = [&](const char* what, int nrows, int Q, int ns, int w, int at, int got) {
    std::printf("%s: nrows=%d Q=%d ns=%d weights=%d at=%d got=%d\n", what, nrows, Q, ns, w, at, got);
    ++bad;
  };
  for (int nrows : rows)
    for (int Q : cycles)
      for (int ns = 2; ns <= 4; ++ns)
        for (int w = 0; w < 3; ++w) {
          int wcum[5] = {0}, next = 0, hmax = 0;
          for (int i = 0; i < ns; ++i) wcum[i + 1] = wcum[i] + weights[w][i];
          for (int q = 0; q < Q; ++q)
            for (int sl = 0; sl < ns; ++sl, ++checked) {
              const BandRows b = slot_band(nrows, Q, q, ns, sl, wcum);
              if (b.r0 != next) fail("gap or overlap", nrows, Q, ns, w, next, b.r0);
              if (b.rend < b.r0) fail("negative band", nrows, Q, ns, w, b.r0, b.rend);
              if (b.rend - b.r0 > hmax) hmax = b.rend - b.r0;
              next = b.rend;
            }
          if (next != nrows) fail("rows not covered", nrows, Q, ns, w, nrows, next);
          const int t = tallest_slot_band(nrows, Q, ns, wcum);
          if (t != hmax) fail("tallest band", nrows, Q, ns, w, hmax, t);
        }
  // the static split: bands of H rows over the grid's waves of one strip
  for (int nrows : rows)
    for (int H : heights) {
      int next = 0;
      const int bands = march_grid_for(1, nrows, H) * kMarchWaves;
      for (int band = 0; band < bands; ++band, ++checked) {
        const BandRows b = static_band(nrows, H, band);
        if (b.r0 < nrows && (b.r0 != next || b.rend <= b.r0 || b.rend - b.r0 > H))
          fail("static band", nrows, H, 0, 0, next, b.r0);
        if (b.r0 < nrows) next = b.rend;
      }
      if (next != nrows) fail("static rows not covered", nrows, H, 0, 0, nrows, next);
    }
  std::printf("%d bands checked, %d violations\n", checked, bad);
  return bad ? 1 : 0;
}
