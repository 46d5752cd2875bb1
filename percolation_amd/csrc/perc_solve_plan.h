// perc_solve_plan.h -- what a CG solve runs, decided on the host from plain
// values: the solver family and its flags (solve_plan), the k_cg_march variant
// of a launch (select_march over the one variant list), the march's band
// height and slot-weighted geometry, and the launch loop's chunk schedule.
// The one copy of these rules: perc_solve.hip fills in the facts and stores
// the answers, tests/solve_plan_check.cpp checks them on the CPU.  No HIP
// headers: plain C++ under g++, as perc_bands.h.
#pragma once

#include <cstddef>

#include "../../include/perc.h"
#include "perc_bands.h"

namespace perc {

// one-workgroup solve (k_cg_small): 1024 threads x 8 rows each
constexpr int kSmallRows = 8192;
// a vector larger than this does not stay in the 256 MB Infinity Cache
// between kernels (L = 8192: 537 MB; L = 4096: 134 MB)
constexpr size_t kLargeVector = (size_t)256 << 20;
constexpr int kMaxSlotRounds = 4;  // workgroup rounds per CU of the slot-weighted bands
constexpr int kNT = 2;             // buffer access aux bits: nontemporal
constexpr int kMarchDepth = 2;     // rows the row-major march prefetches (perc_march.h)
constexpr int kMarchPQ = 0, kMarchP = 1, kMarchB = 2;  // k_cg_march's MODE (perc_march.h)

// ---------------------------------------------------------------------------
// The solver family and its flags
struct SolvePlan {
  bool stencil = false;      // solver kernels use the stencil operator
  bool fused = false;        // stencil P+S fused into the LDS-tiled kernel
  bool march = false;        // fused format runs the register-march kernel
  bool qfree = false;        // march B rebuilds q (52N / iteration)
  bool march_alt = false;    // alternating walk directions
  bool strips = false;       // march solve in the strip-major layout
  bool march_slots = false;  // q-free strip-major march: slot-weighted bands
  bool march_tag = false;    // q-free strip-major march: tagged-granule reductions
  bool resident = false;     // persistent resident solve (k_cg_res)
  bool small = false;        // one-workgroup solve of a small system (k_cg_small)
  // the kernel family a solve runs (perc_last_solve's out4[0]; 0: the other
  // launched kernels -- LDS tiles, split stencil, CSR)
  int family() const {
    return small ? PERC_RAN_SMALL : (resident ? PERC_RAN_RESIDENT : (march ? PERC_RAN_MARCH : 0));
  }
};

struct SolveRequest {  // what the caller set
  int fmt_req;         // perc_set_matrix_format
  int march_mode;      // perc_set_march_mode
  int dot_order;       // perc_set_dot_order
  int march_rows_req;  // perc_set_march_rows (0: auto)
};

struct SolveFacts {  // what the lattice and the assembly allow
  long long N;       // interior rows
  bool stencil_ok;   // every stencil slot of the assembled system has a bond
  bool tiled_ok;     // every row's slots are (row, col) +-1 steps of its form
  bool march_ok;     // register-march kernel usable (m % 128 == 0, tileable)
  int res_G;         // the resident solve's grid (0: none)
  int wm_slots;      // slot-weighted bands: workgroup rounds (0: not available)
  bool has_rowptr;   // a CSR row pointer exists (k_cg_small reads it)
};

inline SolvePlan solve_plan(const SolveRequest& q, const SolveFacts& f) {
  SolvePlan p;
  p.stencil = q.fmt_req != PERC_FMT_CSR && f.stencil_ok;
  p.fused = p.stencil && f.tiled_ok && q.fmt_req != PERC_FMT_STENCIL_SPLIT;
  p.march = p.fused && f.march_ok && q.fmt_req != PERC_FMT_STENCIL_TILED;
  // the literal dot order runs the production kernels: the q-free march and
  // the resident solve store their rows' dot terms (a.lit / ResArgs::lit,
  // 3 N doubles addressed by 32-bit buffer offsets: < 2 GB), which the
  // serial folds sum; past that size the q-storing march (the folds then
  // form the terms from q, p, r)
  const bool literal = q.dot_order != PERC_DOT_FAST;
  const bool lit_ok = !literal || f.N * 24 < (1ll << 31);
  // (dev_solve only: the march kernels stay selected for the probes; the
  // host-folded literal order runs the launched march, whose kernels the
  // host can fold between)
  p.resident = p.fused && f.res_G > 0 && q.fmt_req != PERC_FMT_STENCIL_TILED &&
               (q.march_mode & PERC_SOLVE_RESIDENT) && q.march_rows_req == 0 && lit_ok &&
               q.dot_order != PERC_DOT_LITERAL_HOST;
  p.qfree = p.march && (q.march_mode & PERC_MARCH_QFREE) && lit_ok;
  p.march_alt = p.march && (q.march_mode & PERC_MARCH_ALT);
  // one-workgroup solve for small systems, under the default format only
  // (an explicit format keeps its launched kernels, e.g. for the tests)
  p.small = q.fmt_req == PERC_FMT_AUTO && f.N > 0 && f.N <= kSmallRows &&
            (q.march_mode & PERC_SOLVE_RESIDENT) && f.has_rowptr;
  // strip-major q-free march only while a vector fits the Infinity Cache
  // (L <= 4096): past it the row-major march is faster (L = 8192, round 4
  // with nibble codes and slot bands: 0.652 vs 0.734 ms per iteration,
  // profiles/r4_4_l8192_strips_ab.json; round 2: 0.439 vs 0.480 ms); its
  // whole-array buffer views also need < 2 GB
  p.strips = p.qfree && (q.march_mode & PERC_MARCH_STRIPS) && (size_t)f.N * sizeof(double) <= kLargeVector;
  // slot-weighted bands of the strip-major march (to_strips applies them)
  p.march_slots = (q.march_mode & PERC_MARCH_SLOTS) && p.strips && f.wm_slots > 0;
  // tagged-granule reductions of the strip-major march (PERC_MARCH_TAG);
  // their tags are (epoch << 24) | iteration, so solves of >= 2^24 - 2
  // iterations take the ticket reduction
  p.march_tag = (q.march_mode & PERC_MARCH_TAG) && p.strips;
  return p;
}

// ---------------------------------------------------------------------------
// The march variants: k_cg_march's template arguments as a value, and the
// list of every instantiation libperc compiles -- the only place one is
// named.  perc_march.h pairs each row with its kernel (PERC_MARCH_ROW),
// perc_solve.hip builds its lookup table from the pairs and picks a key per
// launch (select_march); the row-slab solves launch the q-storing entry alone
// (march_pq_kernel), so perc_slabs.hip compiles just that one.
struct MarchKey {
  int mode;  // kMarchPQ / kMarchP / kMarchB
  bool sm;   // strip-major layout
  int d, paux;
  bool tr, tag, pk, lit;
  int esr;
  bool open;  // strip-major nibble codes on an open lattice: the open-square path alone
};

constexpr bool operator==(const MarchKey& a, const MarchKey& b) {
  return a.mode == b.mode && a.sm == b.sm && a.d == b.d && a.paux == b.paux && a.tr == b.tr && a.tag == b.tag &&
         a.pk == b.pk && a.lit == b.lit && a.esr == b.esr && a.open == b.open;
}

// q-storing P+S: row slabs, modes without QFREE, literal order past 2 GB of terms
#define PERC_MARCH_PQ kMarchPQ, false, 3, 0, false, false, false, false, 0
// tagged strip-major P on the u16 codes: the kernel whose occupancy sizes the
// bands (march_rows_for, slot_geometry)
#define PERC_MARCH_OCC kMarchP, true, 3, kNT, false, true, false, false, 0

// Strip-major rows (the default solve at L <= 4096): 3 rows prefetched,
// nontemporal last-use loads.  Row-major rows (vectors past the Infinity
// Cache): kMarchDepth rows, P and B on B's 8-row bands (L = 8192: P 0.314 vs
// 0.355 ms, r4_8; B's nontemporal r(k) loads 0.300 vs 0.331 ms, r4_3).
// Columns: MODE, SM, D, PAUX, TR, TAG, PK, LIT, ESR, OPEN (k_cg_march's
// order; a row without the last column has OPEN false).  Every strip-major
// nibble row has an OPEN twin: the twin runs on the open lattice, the row
// itself under pbc (select_march).
#define PERC_MARCH_VARIANTS(X) \
  X(PERC_MARCH_PQ)                                                   /* q-storing P+S */ \
  X(kMarchP, true, 3, kNT, false, false, false, false, 0)            /* strip-major P, u16, ticket reduction */ \
  X(kMarchP, true, 3, kNT, true, false, false, false, 0)             /* strip-major P, u16, ticket reduction, phase probe */ \
  X(PERC_MARCH_OCC)                                                  /* strip-major P, u16, tagged granules */ \
  X(kMarchP, true, 3, kNT, true, true, false, false, 0)              /* strip-major P, u16, tagged granules, phase probe */ \
  X(kMarchP, true, 3, kNT, false, false, false, true, 0)             /* strip-major P, u16, literal order */ \
  X(kMarchP, true, 3, kNT, false, true, false, true, 0)              /* strip-major P, u16, literal order, solve tagged */ \
  X(kMarchP, true, 3, kNT, false, false, true, false, 0)             /* strip-major P, nibble, ticket reduction */ \
  X(kMarchP, true, 3, kNT, false, false, true, false, 0, true)       /* strip-major P, nibble, ticket reduction, open lattice */ \
  X(kMarchP, true, 3, kNT, true, false, true, false, 0)              /* strip-major P, nibble, ticket reduction, phase probe */ \
  X(kMarchP, true, 3, kNT, true, false, true, false, 0, true)        /* strip-major P, nibble, ticket reduction, phase probe, open lattice */ \
  X(kMarchP, true, 3, kNT, false, true, true, false, 0)              /* strip-major P, nibble, tagged granules (pbc) */ \
  X(kMarchP, true, 3, kNT, false, true, true, false, 0, true)        /* strip-major P, nibble, tagged granules, open lattice: the default P */ \
  X(kMarchP, true, 3, kNT, true, true, true, false, 0)               /* strip-major P, nibble, tagged granules, phase probe */ \
  X(kMarchP, true, 3, kNT, true, true, true, false, 0, true)         /* strip-major P, nibble, tagged granules, phase probe, open lattice */ \
  X(kMarchP, true, 3, kNT, false, false, true, true, 0)              /* strip-major P, nibble, literal order */ \
  X(kMarchP, true, 3, kNT, false, false, true, true, 0, true)        /* strip-major P, nibble, literal order, open lattice */ \
  X(kMarchP, true, 3, kNT, false, true, true, true, 0)               /* strip-major P, nibble, literal order, solve tagged */ \
  X(kMarchP, true, 3, kNT, false, true, true, true, 0, true)         /* strip-major P, nibble, literal order, solve tagged, open lattice */ \
  X(kMarchB, true, 3, kNT, false, false, false, false, 0)            /* strip-major B, u16, ticket reduction */ \
  X(kMarchB, true, 3, kNT, true, false, false, false, 0)             /* strip-major B, u16, ticket reduction, phase probe */ \
  X(kMarchB, true, 3, kNT, false, true, false, false, 0)             /* strip-major B, u16, tagged granules */ \
  X(kMarchB, true, 3, kNT, true, true, false, false, 0)              /* strip-major B, u16, tagged granules, phase probe */ \
  X(kMarchB, true, 3, kNT, false, false, false, true, 0)             /* strip-major B, u16, literal order */ \
  X(kMarchB, true, 3, kNT, false, true, false, true, 0)              /* strip-major B, u16, literal order, solve tagged */ \
  X(kMarchB, true, 3, kNT, false, true, false, false, kEdgeRows)     /* strip-major B, u16, edge pairs staged in LDS */ \
  X(kMarchB, true, 3, kNT, true, true, false, false, kEdgeRows)      /* strip-major B, u16, staged edge pairs, phase probe */ \
  X(kMarchB, true, 3, kNT, false, false, true, false, 0)             /* strip-major B, nibble, ticket reduction */ \
  X(kMarchB, true, 3, kNT, false, false, true, false, 0, true)       /* strip-major B, nibble, ticket reduction, open lattice */ \
  X(kMarchB, true, 3, kNT, true, false, true, false, 0)              /* strip-major B, nibble, ticket reduction, phase probe */ \
  X(kMarchB, true, 3, kNT, true, false, true, false, 0, true)        /* strip-major B, nibble, ticket reduction, phase probe, open lattice */ \
  X(kMarchB, true, 3, kNT, false, true, true, false, 0)              /* strip-major B, nibble, tagged granules */ \
  X(kMarchB, true, 3, kNT, false, true, true, false, 0, true)        /* strip-major B, nibble, tagged granules, open lattice */ \
  X(kMarchB, true, 3, kNT, true, true, true, false, 0)               /* strip-major B, nibble, tagged granules, phase probe */ \
  X(kMarchB, true, 3, kNT, true, true, true, false, 0, true)         /* strip-major B, nibble, tagged granules, phase probe, open lattice */ \
  X(kMarchB, true, 3, kNT, false, false, true, true, 0)              /* strip-major B, nibble, literal order */ \
  X(kMarchB, true, 3, kNT, false, false, true, true, 0, true)        /* strip-major B, nibble, literal order, open lattice */ \
  X(kMarchB, true, 3, kNT, false, true, true, true, 0)               /* strip-major B, nibble, literal order, solve tagged */ \
  X(kMarchB, true, 3, kNT, false, true, true, true, 0, true)         /* strip-major B, nibble, literal order, solve tagged, open lattice */ \
  X(kMarchB, true, 3, kNT, false, true, true, false, kEdgeRows)      /* strip-major B, nibble, edge pairs staged in LDS (pbc) */ \
  X(kMarchB, true, 3, kNT, false, true, true, false, kEdgeRows, true) /* strip-major B, nibble, edge pairs staged in LDS, open lattice: the default B */ \
  X(kMarchB, true, 3, kNT, true, true, true, false, kEdgeRows)       /* strip-major B, nibble, staged edge pairs, phase probe */ \
  X(kMarchB, true, 3, kNT, true, true, true, false, kEdgeRows, true) /* strip-major B, nibble, staged edge pairs, phase probe, open lattice */ \
  X(kMarchP, false, kMarchDepth, 0, false, false, false, false, 0)   /* row-major P, u16 */ \
  X(kMarchP, false, kMarchDepth, 0, false, false, false, true, 0)    /* row-major P, u16, literal order */ \
  X(kMarchP, false, kMarchDepth, 0, false, false, true, false, 0)    /* row-major P, nibble (128 VGPRs unspilled at the 4-wave bound): past the cache */ \
  X(kMarchP, false, kMarchDepth, 0, false, false, true, true, 0)     /* row-major P, nibble, literal order */ \
  X(kMarchB, false, kMarchDepth, kNT, false, false, false, false, 0) /* row-major B, u16 */ \
  X(kMarchB, false, kMarchDepth, kNT, false, false, false, true, 0)  /* row-major B, u16, literal order */ \
  X(kMarchB, false, kMarchDepth, kNT, false, false, true, false, 0)  /* row-major B, nibble, edge pairs stored per step */ \
  X(kMarchB, false, kMarchDepth, kNT, false, false, true, true, 0)   /* row-major B, nibble, literal order */ \
  X(kMarchB, false, kMarchDepth, kNT, false, false, true, false, kEdgeRowsRm) /* row-major B, nibble, edge pairs staged in LDS: past the cache */

#define PERC_MARCH_KEY(...) MarchKey{__VA_ARGS__},
constexpr MarchKey kMarchKeys[] = {PERC_MARCH_VARIANTS(PERC_MARCH_KEY)};

// What decides the march kernel of a launch: the plan's qfree and the launch
// arguments' layout (sm), literal terms, nibble codes, tagged granules, phase
// trace, B's staged edge pairs (mes), the row-major P's nibble codes
// (rm_pnib) and the open-square path.
struct MarchSel {
  bool qfree, sm, lit, nib, tag, tr, mes, rm_pnib, open;
};

// The march kernel of a launch: mode kMarchP for the P side (P of the q-free
// march, else the q-storing P+S), kMarchB for the q-free B.
//  strip-major pair (the default solve at L <= 4096; phase probe: tr):
//    staged edges (B, mes) > literal > tagged > trace > plain; with nibble
//    codes on an open lattice, outside a slab solve, the OPEN twin of each
//    (open: the open-square path alone; the row itself runs under pbc)
//  row-major pair (vectors past the Infinity Cache): literal and nibble codes
//    independently (P's nibble codes: rm_pnib), B's staged edges without lit
inline MarchKey select_march(int mode, const MarchSel& s) {
  if (!s.qfree) return MarchKey{PERC_MARCH_PQ};
  if (!s.sm) {
    if (mode == kMarchP) return {kMarchP, false, kMarchDepth, 0, false, false, s.nib && s.rm_pnib, s.lit, 0, false};
    return {kMarchB, false, kMarchDepth, kNT, false, false, s.nib, s.lit, !s.lit && s.nib && s.mes ? kEdgeRowsRm : 0,
            false};
  }
  MarchKey k = {mode, true, 3, kNT, false, s.tag, s.nib, false, 0, s.open};
  if (mode == kMarchB && s.mes && !s.lit && s.tag) k.tr = s.tr, k.esr = kEdgeRows;
  else if (s.lit) k.lit = true;
  else k.tr = s.tr;
  return k;
}

// ---------------------------------------------------------------------------
// The band policy of the register march.
//
// Per-round weights of the slot-weighted bands (PERC_MARCH_SLOTS): one
// workgroup per CU and round, bands cycling over the rounds, weights = the
// rounds' relative streaming rates with equal bands ([0]: P, [1]: B of the
// strip-major march; same-box A/Bs, profiles/r3_4_ab_slotw_L4096.log; round 6
// re-tuned P's for the nibble-code tagged march, whose third slot walked ~2 us
// longer than the others (profiles/r5_4_mtrace_summary_L4096.txt): 100:76:48
// against 100:75:50, P 73.2 vs 75.0 us, 0.1489 vs 0.1511 ms per iteration,
// r6_4_def_ab_w*.json, r6_5_weights.json; and B's 100:78:55 against 100:80:60
// once B stores the edge {p, z}: B 71.6 vs 72.4 us, r6_17_weights.json,
// r6_18_weights.json)
constexpr int kSlotW[2][kMaxSlotRounds] = {{100, 76, 48, 40}, {100, 78, 55, 50}};

// band height of the register-march kernel over `nrows` rows of m columns:
// the requested height (perc_set_march_rows); vectors past the Infinity
// Cache: 8-row bands for the row-major march P and B (B 0.310 vs 0.318 ms at
// 16 rows at L = 8192; 16 rows without PERC_MARCH_SLOTS); else one round of
// resident waves, the height that gives every wave slot of the chip one
// strip-band.  cus, per_cu: the device's CUs and the workgroups a CU holds of
// the kernel that sizes the bands (PERC_MARCH_OCC)
inline int march_rows_for(int m, int nrows, int cus, int per_cu, int march_mode, int rows_req) {
  if (rows_req > 0) return rows_req;
  if ((size_t)m * nrows * sizeof(double) > kLargeVector) return (march_mode & PERC_MARCH_SLOTS) ? 8 : 16;
  const long long slots = (long long)(cus > 1 ? cus : 1) * (per_cu > 1 ? per_cu : 1) * kMarchWaves;
  const long long bands = slots / (m / kMarchW) > 1 ? slots / (m / kMarchW) : 1;
  const long long h = (nrows + bands - 1) / bands;
  return h > 2 ? (int)h : 2;
}

// the slot-weighted bands over nrows rows of m columns: per_cu rounds of one
// workgroup per CU where the chip's waves divide evenly over the strips of a
// row and every band gets a row; slots == 0: not available (static split)
struct SlotGeometry {
  int slots = 0;                          // workgroup rounds
  int grid = 0;                           // CUs x rounds
  int cum[2][kMaxSlotRounds + 1] = {};    // cumulative round weights (P, B)
};
inline SlotGeometry slot_geometry(int m, int nrows, int cus, int per_cu, const int (*w)[kMaxSlotRounds]) {
  SlotGeometry s;
  if (m <= 0 || m % kMarchW != 0 || nrows <= 0) return s;
  const int spr = m / kMarchW;
  const long long waves = (long long)cus * kMarchWaves;
  bool ok = cus > 0 && per_cu >= 2 && per_cu <= kMaxSlotRounds && waves % spr == 0 &&
            (waves / spr) * per_cu <= nrows;
  for (int i = 0; ok && i < per_cu; ++i) ok = w[0][i] > 0 && w[1][i] > 0;
  if (!ok) return s;
  s.slots = per_cu;
  s.grid = cus * per_cu;
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < per_cu; ++i) s.cum[k][i + 1] = s.cum[k][i] + w[k][i];
  return s;
}

// ---------------------------------------------------------------------------
// The launch loop's chunks: iterations are launched `chunk` at a time and the
// device scalars read back after each chunk (the device stop flag makes the
// surplus launches no-ops): 8, then doubling up to 256.  The march's Krylov
// front starts after the first chunk's read-back.
struct ChunkSchedule {
  static constexpr int kFirst = 8, kMax = 256;
  int chunk = kFirst;
  long long launched = 0;
  int kiter(int j) const { return (int)(launched + j + 1); }  // launch j of the current chunk
  void chunk_done() { launched += chunk; }
  bool first_done() const { return launched == kFirst; }
  // cannot happen in a working solve: the device stops at itmax + 1
  bool overrun(int itmax) const { return launched > (long long)itmax + 2; }
  void grow() { chunk = chunk * 2 < kMax ? chunk * 2 : kMax; }
};

}  // namespace perc
