// CPU check of percolation_amd/csrc/perc_solve_plan.h, the one copy of the
// host rules that decide what a CG solve runs.  Built and run by
// test_solve_plan.py; prints one line per violation, exits 1 on any.
//  1. solve_plan over the whole request x facts grid folds to the digest the
//     previous select_format gave (kParentDigest);
//  2. a hand table, one case per rule;
//  3. select_march returns a compiled variant for every input the host can
//     form, and every compiled variant is returned for some input;
//  4. the band policy (march_rows_for, slot_geometry) and the chunk schedule.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "perc_solve_plan.h"

using namespace perc;

static int bad = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      std::printf("FAIL %s: ", #cond); \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
      ++bad;                        \
    }                               \
  } while (0)

// the ten flags in SolvePlan's order, one FNV-1a step each
static void plan_flags(const SolvePlan& p, bool f[10]) {
  const bool v[10] = {p.stencil, p.fused,       p.march,     p.qfree,    p.march_alt,
                      p.strips,  p.march_slots, p.march_tag, p.resident, p.small};
  std::memcpy(f, v, sizeof(v));
}
static void fold(uint64_t& h, const SolvePlan& p) {
  bool f[10];
  plan_flags(p, f);
  for (bool b : f) h = (h ^ (uint64_t)(b ? 1 : 0)) * 0x100000001b3ull;
}

constexpr int kModeBits[7] = {PERC_MARCH_QFREE, PERC_MARCH_ALT,    PERC_SOLVE_RESIDENT, PERC_MARCH_STRIPS,
                              PERC_MARCH_SLOTS, PERC_MARCH_TAG,    PERC_MARCH_NIBBLE};
// the edges of kSmallRows, kLargeVector / 8 and 2^31 / 24
constexpr long long kGridN[7] = {4096, 8192, 8193, 1ll << 25, (1ll << 25) + 1, 89478485, 89478486};

// The digest of the same sweep over the select_format this header replaced:
// a scratch program (not kept) filled a perc_ctx per grid point -- fmt_req,
// march_mode, dot_order, stencil_ok, tiled_ok, march_ok, res_G, wm_slots,
// march_rows_req, d.rowptr (null or not) and N, in this loop order -- called
// perc::select_format from the parent commit's libperc.so on a CPU-only
// machine (it makes no HIP call) and folded the ten booleans it wrote into
// the context, in SolvePlan's order, exactly as fold() does.
constexpr uint64_t kParentDigest = 0xe53b15fb41743825ull;

static uint64_t sweep(long long* points) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (int fmt = PERC_FMT_AUTO; fmt <= PERC_FMT_STENCIL_TILED; ++fmt)
    for (int mi = 0; mi < 128; ++mi) {
      int mode = 0;
      for (int b = 0; b < 7; ++b)
        if (mi >> b & 1) mode |= kModeBits[b];
      for (int dot = PERC_DOT_FAST; dot <= PERC_DOT_LITERAL_HOST; ++dot)
        for (int ok = 0; ok < 8; ++ok)
          for (int res_G = 0; res_G <= 32; res_G += 32)
            for (int wm = 0; wm <= 3; wm += 3)
              for (int rows = 0; rows <= 8; rows += 8)
                for (int rp = 0; rp < 2; ++rp)
                  for (long long N : kGridN) {
                    const SolveRequest q = {fmt, mode, dot, rows};
                    const SolveFacts f = {N, (ok & 1) != 0, (ok & 2) != 0, (ok & 4) != 0, res_G, wm, rp != 0};
                    fold(h, solve_plan(q, f));
                    ++*points;
                  }
    }
  return h;
}

// ---------------------------------------------------------------------------
struct Case {
  const char* rule;
  SolveRequest q;
  SolveFacts f;
  const char* flags;  // stencil fused march qfree alt strips slots tag resident small
  int family;
};
constexpr int D = PERC_MARCH_DEFAULT;
constexpr long long kMid = 1ll << 20;  // 1024 x 1024 rows: fits the cache, not small
constexpr long long kLitMax = 89478485, kCache = 1ll << 25;
#define FACTS(N) {N, true, true, true, 32, 3, true}
static const Case kCases[] = {
    {"default: the resident solve where its grid exists", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, FACTS(kMid), "1111111110", PERC_RAN_RESIDENT},
    {"PERC_FMT_STENCIL asks for the same kernels", {PERC_FMT_STENCIL, D, PERC_DOT_FAST, 0}, FACTS(kMid), "1111111110", PERC_RAN_RESIDENT},
    {"PERC_FMT_CSR: no stencil, so nothing built on it", {PERC_FMT_CSR, D, PERC_DOT_FAST, 0}, FACTS(kMid), "0000000000", 0},
    {"a stencil slot without a bond: CSR", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, {kMid, false, true, true, 32, 3, true}, "0000000000", 0},
    {"PERC_FMT_STENCIL_SPLIT: stencil, not fused", {PERC_FMT_STENCIL_SPLIT, D, PERC_DOT_FAST, 0}, FACTS(kMid), "1000000000", 0},
    {"rows that are not +-1 steps of their form: not fused", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, {kMid, true, false, true, 32, 3, true}, "1000000000", 0},
    {"PERC_FMT_STENCIL_TILED: fused, neither march nor resident", {PERC_FMT_STENCIL_TILED, D, PERC_DOT_FAST, 0}, FACTS(kMid), "1100000000", 0},
    {"no march (m % 128 != 0): the tiled kernel; resident still applies", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, {kMid, true, true, false, 32, 3, true}, "1100000010", PERC_RAN_RESIDENT},
    {"no resident grid: the march", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, {kMid, true, true, true, 0, 3, true}, "1111111100", PERC_RAN_MARCH},
    {"without PERC_SOLVE_RESIDENT: the march", {PERC_FMT_AUTO, D & ~PERC_SOLVE_RESIDENT, PERC_DOT_FAST, 0}, FACTS(kMid), "1111111100", PERC_RAN_MARCH},
    {"a requested band height: the march", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 8}, FACTS(kMid), "1111111100", PERC_RAN_MARCH},
    {"literal order runs the production kernels", {PERC_FMT_AUTO, D, PERC_DOT_LITERAL, 0}, FACTS(kMid), "1111111110", PERC_RAN_RESIDENT},
    {"PERC_DOT_LITERAL_HOST is never resident", {PERC_FMT_AUTO, D, PERC_DOT_LITERAL_HOST, 0}, FACTS(kMid), "1111111100", PERC_RAN_MARCH},
    {"literal terms just under 2 GB (N * 24 < 2^31): q-free, resident", {PERC_FMT_AUTO, D, PERC_DOT_LITERAL, 0}, FACTS(kLitMax), "1111100010", PERC_RAN_RESIDENT},
    {"literal terms of 2 GB: the q-storing march, not resident", {PERC_FMT_AUTO, D, PERC_DOT_LITERAL, 0}, FACTS(kLitMax + 1), "1110100000", PERC_RAN_MARCH},
    {"... the host-folded literal order too", {PERC_FMT_AUTO, D, PERC_DOT_LITERAL_HOST, 0}, FACTS(kLitMax + 1), "1110100000", PERC_RAN_MARCH},
    {"... the fast order has no such bound", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, FACTS(kLitMax + 1), "1111100010", PERC_RAN_RESIDENT},
    {"without PERC_MARCH_QFREE: no strips, slots or tag either", {PERC_FMT_AUTO, D & ~PERC_MARCH_QFREE, PERC_DOT_FAST, 0}, FACTS(kMid), "1110100010", PERC_RAN_RESIDENT},
    {"without PERC_MARCH_ALT", {PERC_FMT_AUTO, D & ~PERC_MARCH_ALT, PERC_DOT_FAST, 0}, FACTS(kMid), "1111011110", PERC_RAN_RESIDENT},
    {"without PERC_MARCH_STRIPS: slots and tag only with strips", {PERC_FMT_AUTO, D & ~PERC_MARCH_STRIPS, PERC_DOT_FAST, 0}, FACTS(kMid), "1111100010", PERC_RAN_RESIDENT},
    {"without PERC_MARCH_SLOTS", {PERC_FMT_AUTO, D & ~PERC_MARCH_SLOTS, PERC_DOT_FAST, 0}, FACTS(kMid), "1111110110", PERC_RAN_RESIDENT},
    {"no slot geometry on this device", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, {kMid, true, true, true, 32, 0, true}, "1111110110", PERC_RAN_RESIDENT},
    {"without PERC_MARCH_TAG", {PERC_FMT_AUTO, D & ~PERC_MARCH_TAG, PERC_DOT_FAST, 0}, FACTS(kMid), "1111111010", PERC_RAN_RESIDENT},
    {"PERC_MARCH_NIBBLE is not the plan's (to_strips / to_nib_rows)", {PERC_FMT_AUTO, D & ~PERC_MARCH_NIBBLE, PERC_DOT_FAST, 0}, FACTS(kMid), "1111111110", PERC_RAN_RESIDENT},
    {"a vector of exactly kLargeVector (N * 8): strips", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, FACTS(kCache), "1111111110", PERC_RAN_RESIDENT},
    {"one row more: the row-major march", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, FACTS(kCache + 1), "1111100010", PERC_RAN_RESIDENT},
    {"N = kSmallRows under PERC_FMT_AUTO: the one-workgroup solve", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, FACTS(8192), "1111111111", PERC_RAN_SMALL},
    {"N = kSmallRows + 1: not small", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, FACTS(8193), "1111111110", PERC_RAN_RESIDENT},
    {"an explicit format keeps its launched kernels", {PERC_FMT_STENCIL, D, PERC_DOT_FAST, 0}, FACTS(4096), "1111111110", PERC_RAN_RESIDENT},
    {"small needs PERC_SOLVE_RESIDENT", {PERC_FMT_AUTO, D & ~PERC_SOLVE_RESIDENT, PERC_DOT_FAST, 0}, FACTS(4096), "1111111100", PERC_RAN_MARCH},
    {"small needs the CSR row pointer", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, {4096, true, true, true, 32, 3, false}, "1111111110", PERC_RAN_RESIDENT},
    {"small on a CSR-only system", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, {4096, false, false, false, 0, 0, true}, "0000000001", PERC_RAN_SMALL},
    {"an empty system is not small", {PERC_FMT_AUTO, D, PERC_DOT_FAST, 0}, {0, false, false, false, 0, 0, true}, "0000000000", 0},
};

static void check_table() {
  for (const Case& c : kCases) {
    const SolvePlan p = solve_plan(c.q, c.f);
    bool f[10];
    plan_flags(p, f);
    char got[11] = {0};
    for (int i = 0; i < 10; ++i) got[i] = f[i] ? '1' : '0';
    CHECK(std::strcmp(got, c.flags) == 0, "%s: got %s want %s", c.rule, got, c.flags);
    CHECK(p.family() == c.family, "%s: family %d want %d", c.rule, p.family(), c.family);
  }
}

// ---------------------------------------------------------------------------
static void check_select_march() {
  constexpr int nkeys = sizeof(kMarchKeys) / sizeof(kMarchKeys[0]);
  bool reached[nkeys] = {};
  int inputs = 0;
  for (int mode : {kMarchP, kMarchB})
    for (int v = 0; v < 512; ++v) {
      const MarchSel s = {(v & 1) != 0,  (v & 2) != 0,  (v & 4) != 0,   (v & 8) != 0,  (v & 16) != 0,
                          (v & 32) != 0, (v & 64) != 0, (v & 128) != 0, (v & 256) != 0};
      // what the host can set: tagged granules and the open path only
      // strip-major, the row-major P's nibble codes only row-major, the open
      // path only on nibble codes
      if ((s.tag || s.open) && !s.sm) continue;
      if (s.rm_pnib && s.sm) continue;
      if (s.open && !s.nib) continue;
      ++inputs;
      const MarchKey k = select_march(mode, s);
      int at = -1;
      for (int i = 0; i < nkeys; ++i)
        if (kMarchKeys[i] == k) at = i;
      CHECK(at >= 0, "mode %d sel %d: {%d, %d, %d, %d, %d, %d, %d, %d, %d, %d} is not compiled", mode, v, k.mode, k.sm,
            k.d, k.paux, k.tr, k.tag, k.pk, k.lit, k.esr, k.open);
      if (at >= 0) reached[at] = true;
      CHECK(k.esr != kEdgeRows || k.sm, "mode %d sel %d: the strip-major staging depth on a row-major key", mode, v);
      CHECK(k.esr == 0 || k.mode == kMarchB, "mode %d sel %d: staged edges outside B", mode, v);
      CHECK(s.qfree || k == MarchKey{PERC_MARCH_PQ}, "mode %d sel %d: not q-free must be the q-storing P+S", mode, v);
    }
  for (int i = 0; i < nkeys; ++i)
    CHECK(reached[i], "variant %d {%d, %d, %d, %d, %d, %d, %d, %d, %d, %d} is never selected", i, kMarchKeys[i].mode,
          kMarchKeys[i].sm, kMarchKeys[i].d, kMarchKeys[i].paux, kMarchKeys[i].tr, kMarchKeys[i].tag, kMarchKeys[i].pk,
          kMarchKeys[i].lit, kMarchKeys[i].esr, kMarchKeys[i].open);
  for (int i = 0; i < nkeys; ++i)
    for (int j = i + 1; j < nkeys; ++j) CHECK(!(kMarchKeys[i] == kMarchKeys[j]), "variants %d and %d are the same", i, j);
  std::printf("select_march: %d inputs, %d variants\n", inputs, nkeys);
}

// ---------------------------------------------------------------------------
static void check_bands() {
  const int occ[2][2] = {{256, 3}, {0, 0}};
  for (const auto& o : occ) {
    const int cus = o[0], per_cu = o[1];
    // a request is the answer
    for (int req : {1, 8, 1024}) CHECK(march_rows_for(4096, 4094, cus, per_cu, D, req) == req, "request %d", req);
    // past the Infinity Cache (8192 x 8190 doubles = 537 MB)
    CHECK(march_rows_for(8192, 8190, cus, per_cu, D, 0) == 8, "cus %d", cus);
    CHECK(march_rows_for(8192, 8190, cus, per_cu, D & ~PERC_MARCH_SLOTS, 0) == 16, "cus %d", cus);
    // else one round of resident waves
    const int ms[] = {128, 384, 1024, 4096}, rows[] = {1, 2, 38, 510, 4094, 8190};
    for (int m : ms)
      for (int nrows : rows) {
        const long long slots = (long long)(cus > 1 ? cus : 1) * (per_cu > 1 ? per_cu : 1) * kMarchWaves;
        const long long bands = slots / (m / kMarchW) > 1 ? slots / (m / kMarchW) : 1;
        const int want = (int)((nrows + bands - 1) / bands) > 2 ? (int)((nrows + bands - 1) / bands) : 2;
        for (int mode : {D, D & ~PERC_MARCH_SLOTS})
          CHECK(march_rows_for(m, nrows, cus, per_cu, mode, 0) == want, "m %d nrows %d cus %d: %d want %d", m, nrows,
                cus, march_rows_for(m, nrows, cus, per_cu, mode, 0), want);
      }
    CHECK(slot_geometry(4096, 4094, cus, per_cu, kSlotW).slots == (cus ? 3 : 0), "cus %d", cus);
  }
  CHECK(march_rows_for(4096, 4094, 256, 3, D, 0) == 43, "the default solve's bands at L = 4096");
  // the slot geometry of 256 CUs x 3 workgroups at L = 4096
  const SlotGeometry g = slot_geometry(4096, 4094, 256, 3, kSlotW);
  const int cum[2][5] = {{0, 100, 176, 224, 0}, {0, 100, 178, 233, 0}};
  CHECK(g.slots == 3 && g.grid == 768 && std::memcmp(g.cum, cum, sizeof(cum)) == 0, "slots %d grid %d", g.slots,
        g.grid);
  CHECK(slot_geometry(4096, 4094, 256, 2, kSlotW).slots == 2, "two rounds");
  CHECK(slot_geometry(4096, 4094, 256, 4, kSlotW).grid == 1024, "four rounds");
  // refused: the chip's waves do not divide over the strips of a row
  CHECK(slot_geometry(384, 4094, 256, 3, kSlotW).slots == 0, "waves %% spr");
  CHECK(slot_geometry(4096, 4094, 250, 3, kSlotW).slots == 0, "waves %% spr");
  // refused: fewer than 2 or more than kMaxSlotRounds workgroups per CU
  CHECK(slot_geometry(4096, 4094, 256, 1, kSlotW).slots == 0, "per_cu 1");
  CHECK(slot_geometry(4096, 4094, 256, kMaxSlotRounds + 1, kSlotW).slots == 0, "per_cu 5");
  // refused: more bands than rows (32 cycles x 3 > 95), a width off the strips, a weight <= 0
  CHECK(slot_geometry(4096, 96, 256, 3, kSlotW).slots == 3, "96 rows");
  CHECK(slot_geometry(4096, 95, 256, 3, kSlotW).slots == 0, "95 rows");
  CHECK(slot_geometry(4000, 4094, 256, 3, kSlotW).slots == 0, "m %% 128");
  const int zero[2][kMaxSlotRounds] = {{100, 76, 0, 40}, {100, 78, 55, 50}};
  CHECK(slot_geometry(4096, 4094, 256, 3, zero).slots == 0, "zero weight");
  CHECK(slot_geometry(4096, 4094, 256, 2, zero).slots == 2, "zero weight past the rounds in use");
  // the chunk schedule: 8, doubling, 256; launch numbers from 1
  ChunkSchedule cs;
  const int want[] = {8, 16, 32, 64, 128, 256, 256};
  long long launched = 0;
  for (int c : want) {
    CHECK(cs.chunk == c && cs.kiter(0) == launched + 1 && cs.kiter(c - 1) == launched + c, "chunk %d", cs.chunk);
    cs.chunk_done();
    launched += c;
    CHECK(cs.first_done() == (launched == 8), "first chunk at %lld", launched);
    CHECK(cs.overrun((int)launched - 2) == false && cs.overrun((int)launched - 3) == true, "overrun at %lld", launched);
    cs.grow();
  }
}

int main() {
  long long points = 0;
  const uint64_t h = sweep(&points);
  std::printf("sweep: %lld points, digest %016llx\n", points, (unsigned long long)h);
  CHECK(h == kParentDigest, "digest %016llx, the parent's select_format gave %016llx", (unsigned long long)h,
        (unsigned long long)kParentDigest);
  check_table();
  check_select_march();
  check_bands();
  std::printf("%d cases, %d violations\n", (int)(sizeof(kCases) / sizeof(kCases[0])), bad);
  return bad ? 1 : 0;
}
