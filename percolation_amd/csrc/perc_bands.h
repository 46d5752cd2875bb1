// perc_bands.h -- which rows a wave of the register march walks, and the grid
// that covers them.  The one copy of the band arithmetic: k_cg_march forms its
// band with it, the host sizes grids and B's LDS edge staging with it
// (tests/march_bands_check.cpp checks the split on the CPU).  No HIP headers:
// host and device code under hipcc, plain C++ otherwise.
#pragma once

#ifdef __HIPCC__
#define PERC_BANDS_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PERC_BANDS_FN inline
#endif

namespace perc {

constexpr int kMarchW = 128;    // columns per wave strip
constexpr int kMarchWaves = 4;  // waves (strips) per workgroup
// band rows whose edge pairs the march B can stage in LDS (k_cg_march ESR):
// the strip-major march, and the row-major march on its 8-row bands
constexpr int kEdgeRows = 64;
constexpr int kEdgeRowsRm = 16;

struct BandRows {
  int r0, rend;  // rows [r0, rend)
};

// static split: bands of H rows
PERC_BANDS_FN BandRows static_band(int nrows, int H, int band) {
  const int r0 = band * H;
  return {r0, r0 + H < nrows ? r0 + H : nrows};
}

// slot-weighted split (PERC_MARCH_SLOTS): every strip's rows in Q cycles of
// ns neighbouring bands, cycle q's rows divided by the rounds' cumulative
// weights wc[0 .. ns]; the band of round sl
PERC_BANDS_FN BandRows slot_band(int nrows, int Q, int q, int ns, int sl, const int* wc) {
  const int c0 = (int)((long long)q * nrows / Q), hc = (int)((long long)(q + 1) * nrows / Q) - c0;
  return {c0 + hc * wc[sl] / wc[ns], c0 + hc * wc[sl + 1] / wc[ns]};
}

// rows of the tallest slot-weighted band
inline int tallest_slot_band(int nrows, int Q, int ns, const int* wcum) {
  int hmax = 0;
  for (int q = 0; q < Q; ++q)
    for (int sl = 0; sl < ns; ++sl) {
      const BandRows b = slot_band(nrows, Q, q, ns, sl, wcum);
      if (b.rend - b.r0 > hmax) hmax = b.rend - b.r0;
    }
  return hmax;
}

// workgroups of the static split: one wave per strip and band of h rows
inline int march_grid_for(int spr, int rows, int h) {
  const long long waves = (long long)spr * ((rows + h - 1) / h);
  return (int)((waves + kMarchWaves - 1) / kMarchWaves);
}

}  // namespace perc
