// Stand-alone host check of the two memory owners of perc_common.h (DevBuf,
// PinnedBuf): every block is freed exactly once -- on scope exit, reset,
// re-allocation and move -- and never after a release.  The four HIP
// allocation calls are defined here over malloc / free with a live-block
// table, so the program needs no GPU and a host sanitizer sees every block:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Wno-unused-value -Xarch_host -fsanitize=address,undefined \
//     -I percolation_amd/csrc tests/owner_check.cpp -o owner_check && ./owner_check
// Prints one line per violation, exits 1 on any.
#include <set>

#include "perc_common.h"

static std::set<void*> live[2];  // [0] device, [1] pinned
static int bad = 0, frees = 0;

static hipError_t fake_alloc(int kind, void** p, size_t bytes) {
  *p = malloc(bytes);
  live[kind].insert(*p);
  return hipSuccess;
}
static hipError_t fake_free(int kind, void* p) {
  ++frees;
  if (!live[kind].erase(p)) {
    printf("FAIL: %s free of a block that is not live\n", kind ? "pinned" : "device");
    ++bad;
    return hipErrorInvalidValue;
  }
  free(p);
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(0, p, bytes); }
hipError_t hipFree(void* p) { return fake_free(0, p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return fake_alloc(1, p, bytes); }
hipError_t hipHostFree(void* p) { return fake_free(1, p); }
}

#define CHECK(cond)                                   \
  do {                                                \
    if (!(cond)) {                                    \
      printf("FAIL line %d: %s\n", __LINE__, #cond);  \
      ++bad;                                          \
    }                                                 \
  } while (0)

template <typename Buf>
static hipError_t early_return(bool fail) {
  Buf a, b;
  HIP_TRY(a.alloc(8));
  HIP_TRY(b.alloc(8));
  HIP_TRY(fail ? hipErrorInvalidValue : hipSuccess);  // (the owners free on this path too)
  return hipSuccess;
}

template <typename Buf>
static void exercise(int kind) {
  using namespace perc;
  const std::set<void*>& L = live[kind];
  {
    Buf a;
    CHECK(!a && a.get() == nullptr);
    a.reset();  // empty: nothing to free
    CHECK(frees == 0 || L.empty());
    CHECK(a.alloc(16) == hipSuccess && a && L.size() == 1);
    a[0] = 1.0;
    a[15] = 2.0;
    void* first = a.get();
    CHECK(a.alloc(0) == hipSuccess && L.size() == 1 && !L.count(first));  // re-allocation frees the old block
    Buf b(std::move(a));  // move construction: the source is empty
    CHECK(!a && b && L.size() == 1);
    Buf c;
    CHECK(c.alloc(4) == hipSuccess && L.size() == 2);
    c = std::move(b);  // move assignment frees the target's block
    CHECK(!b && c && L.size() == 1);
    Buf& self = c;
    c = std::move(self);  // self-assignment keeps it
    CHECK(c && L.size() == 1);
    c.reset();
    c.reset();  // a second reset frees nothing
    CHECK(!c && L.empty());
    CHECK(c.alloc(4) == hipSuccess);
    double* raw = c.release();  // release hands the block over
    CHECK(!c && L.size() == 1);
    c.reset(raw);  // ... and reset(p) takes one
    CHECK(c.get() == raw);
    Buf d;
    CHECK(d.alloc(2) == hipSuccess && L.size() == 2);
  }  // scope exit frees c and d, not the moved-from a and b
  CHECK(L.empty());
  CHECK(early_return<Buf>(true) == hipErrorInvalidValue && L.empty());
  CHECK(early_return<Buf>(false) == hipSuccess && L.empty());
}

int main() {
  exercise<perc::DevBuf<double>>(0);
  exercise<perc::PinnedBuf<double>>(1);
  CHECK(live[0].empty() && live[1].empty());
  printf("owner_check: %d frees, %d violations\n", frees, bad);
  return bad ? 1 : 0;
}
