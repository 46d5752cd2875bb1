// The batch calls' host-only plan (perc_batch_plan.h) on the CPU: the run
// planner exhaustively over small inputs, check_items on both edges of every
// bound and for every kind's pointers, order_ranks with the spill slot at the
// front, in the middle and at the end and with a repeated id.
#include <cstdio>
#include <cstring>
#include <vector>

#include "perc_batch_plan.h"

using namespace perc;

static long long cases = 0, bad = 0;

static void fail(const char* what, int a, int b, int c) {
  if (++bad <= 20) std::printf("VIOLATION %s (%d, %d, %d)\n", what, a, b, c);
}

// every run of one (item_trial, ntrials, cap)
static void check_runs(const std::vector<int>& trial, int ntrials, int cap) {
  const int nitems = (int)trial.size();
  ++cases;
  ItemRuns runs(trial.data(), nitems, ntrials, cap);
  int at = 0;
  while (runs.next()) {
    if (runs.i0 != at || runs.n < 1) fail("the runs do not tile the items in order", runs.i0, at, runs.n);
    if (runs.n > cap) fail("a run exceeds its cap in items", runs.n, cap, nitems);
    const int k = (int)runs.used.size();
    if (k > cap || k > runs.n) fail("a run exceeds its cap in distinct trials", k, cap, runs.n);
    if ((int)runs.local.size() != runs.n) fail("local has not one entry per item", (int)runs.local.size(), runs.n, 0);
    int seen = 0;  // trials met so far: used is in order of first use, without duplicates
    for (int i = 0; i < runs.n && i < (int)runs.local.size(); ++i) {
      const int l = runs.local[i];
      if (l < 0 || l >= k) {
        fail("a local trial outside used", l, k, i);
        continue;
      }
      if (runs.used[l] != trial[runs.i0 + i]) fail("used[local[i]] != item_trial[i]", l, runs.used[l], trial[at + i]);
      if (l > seen) fail("used is not in order of first use", l, seen, i);
      if (l == seen) ++seen;
    }
    if (seen != k) fail("used names a trial no item of the run has", seen, k, 0);
    for (int a = 0; a < k; ++a)
      for (int b = a + 1; b < k; ++b)
        if (runs.used[a] == runs.used[b]) fail("used has a duplicate", a, b, runs.used[a]);
    at += runs.n;
  }
  if (at != nitems) fail("the runs end before the last item", at, nitems, cap);
  if (runs.next() || runs.n != 0) fail("next() after the last run", runs.n, 0, 0);
  // the bounds alone: the same tiling, nothing renumbered
  ItemRuns plain(nullptr, nitems, ntrials, cap);
  int pat = 0;
  while (plain.next()) {
    if (plain.i0 != pat || plain.n < 1 || plain.n > cap || !plain.used.empty() || !plain.local.empty())
      fail("the plain runs", plain.i0, pat, plain.n);
    pat += plain.n;
  }
  if (pat != nitems) fail("the plain runs end before the last item", pat, nitems, cap);
}

static void planner() {
  for (int nitems = 0; nitems <= 12; ++nitems)
    for (int ntrials = 1; ntrials <= 5; ++ntrials) {
      std::vector<std::vector<int>> maps;
      std::vector<int> v((size_t)nitems);
      for (int one = 0; one < ntrials; ++one) {  // all one trial
        for (int i = 0; i < nitems; ++i) v[i] = one;
        maps.push_back(v);
      }
      for (int i = 0; i < nitems; ++i) v[i] = i % ntrials;  // all distinct (as far as ntrials goes), cyclic
      maps.push_back(v);
      for (int i = 0; i < nitems; ++i) v[i] = ntrials - 1 - i % ntrials;  // descending
      maps.push_back(v);
      for (int gap = 1; gap <= 4; ++gap) {  // trial 0 repeated after a gap of other trials
        for (int i = 0; i < nitems; ++i) v[i] = i % (gap + 1) == 0 ? 0 : std::min(ntrials - 1, 1 + i % (gap + 1) % ntrials);
        maps.push_back(v);
      }
      for (int rep = 1; rep <= 3; ++rep) {  // blocks of rep items per trial
        for (int i = 0; i < nitems; ++i) v[i] = (i / rep) % ntrials;
        maps.push_back(v);
      }
      unsigned s = 12345u + 97u * nitems + ntrials;  // and some without a pattern
      for (int r = 0; r < 8; ++r) {
        for (int i = 0; i < nitems; ++i) {
          s = s * 1664525u + 1013904223u;
          v[i] = (int)((s >> 16) % (unsigned)ntrials);
        }
        maps.push_back(v);
      }
      for (const auto& mp : maps)
        for (int cap = 1; cap <= 13; ++cap) check_runs(mp, ntrials, cap);
    }
}

static void items() {
  const int t = 12, nb = 17, ntrials = 3;
  const int orders[1] = {0};
  int out[1];
  for (int kind = 0; kind < 3; ++kind) {  // bond, site, mixed
    const bool need_s = kind != 0, need_b = kind != 1;
    for (int seeded = 0; seeded < 2; ++seeded) {
      // (what, item_trial, item_nsites, item_nbonds, expected text or NULL)
      struct Case {
        int tr, ns, nbc;
        const char* want;
      };
      const Case edge[] = {
          {0, 0, 0, nullptr},
          {ntrials - 1, t + 1, nb + 1, nullptr},
          {-1, 0, 0, "item_trial outside 0..ntrials-1"},
          {ntrials, 0, 0, "item_trial outside 0..ntrials-1"},
          {0, -1, 0, need_s ? "item_nsites outside 0..t+1" : nullptr},
          {0, t + 2, 0, need_s ? "item_nsites outside 0..t+1" : nullptr},
          {0, 0, -1, need_b ? "item_nbonds outside 0..nb+1" : nullptr},
          {0, 0, nb + 2, need_b ? "item_nbonds outside 0..nb+1" : nullptr},
      };
      for (const Case& c : edge) {
        ++cases;
        // the offending item last of three: every item is checked
        const int tr[3] = {0, 1, c.tr}, ns[3] = {1, t, c.ns}, nbc[3] = {1, nb, c.nbc};
        const char* got = check_items(need_s, need_b, seeded, ntrials, orders, orders, 3, tr, ns, nbc, out, t, nb);
        if ((got == nullptr) != (c.want == nullptr) || (got && std::strcmp(got, c.want)))
          fail(got ? got : "an item passes that must not", kind, c.ns, c.nbc);
      }
      // the pointers the kind reads, each missing in turn; the ones it does not read may be NULL
      const int tr[1] = {0}, cnt[1] = {1};
      const char* lists = seeded ? "a seed list the kind reads is missing" : "an order list the kind reads is missing";
      const char* ptrs = "item_trial, out or a count list the kind reads is missing";
      struct Ptrs {
        const int *so, *bo, *it, *ns, *nbc;
        const void* out;
        const char* want;
      };
      const Ptrs ps[] = {
          {need_s ? orders : nullptr, need_b ? orders : nullptr, tr, need_s ? cnt : nullptr, need_b ? cnt : nullptr, out,
           nullptr},
          {nullptr, orders, tr, cnt, cnt, out, need_s ? lists : nullptr},
          {orders, nullptr, tr, cnt, cnt, out, need_b ? lists : nullptr},
          {orders, orders, nullptr, cnt, cnt, out, ptrs},
          {orders, orders, tr, nullptr, cnt, out, need_s ? ptrs : nullptr},
          {orders, orders, tr, cnt, nullptr, out, need_b ? ptrs : nullptr},
          {orders, orders, tr, cnt, cnt, nullptr, ptrs},
      };
      for (const Ptrs& q : ps) {
        ++cases;
        const char* got = check_items(need_s, need_b, seeded, ntrials, q.so, q.bo, 1, q.it, q.ns, q.nbc, q.out, t, nb);
        if ((got == nullptr) != (q.want == nullptr) || (got && std::strcmp(got, q.want)))
          fail(got ? got : "a missing pointer passes", kind, seeded, (int)(&q - ps));
      }
      // nothing to read: no trials and no items need no pointer at all
      ++cases;
      if (check_items(need_s, need_b, seeded, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, t, nb))
        fail("an empty call fails", kind, seeded, 0);
    }
  }
}

static void ranks() {
  const int N = 5, X = INT_MAX;
  struct Case {
    int order[N + 1], want[N];
  };
  const Case cs[] = {
      {{0, 3, 1, 5, 2, 4}, {2, 4, 1, 5, 3}},  // the spill slot at the front
      {{3, 1, 0, 5, 2, 4}, {1, 4, 0, 5, 3}},  // in the middle
      {{3, 1, 5, 2, 4, 0}, {1, 3, 0, 4, 2}},  // at the end
      {{3, 1, 3, 0, 2, 4}, {1, 4, 0, 5, X}},  // a repeated id: its first position; 5 absent
      {{7, -2, 0, 0, 6, 1}, {5, X, X, X, X}},  // ids outside 1..N are no elements
  };
  std::vector<int> all, rank((size_t)5 * N, -7);
  for (const Case& c : cs) all.insert(all.end(), c.order, c.order + N + 1);
  order_ranks(5, N, all.data(), rank.data());  // the five as one call's trials
  for (int k = 0; k < 5; ++k) {
    ++cases;
    int one[N];
    order_ranks(1, N, cs[k].order, one);  // ... and each alone
    for (int id = 0; id < N; ++id)
      if (rank[(size_t)k * N + id] != cs[k].want[id] || one[id] != cs[k].want[id])
        fail("order_ranks", k, id, rank[(size_t)k * N + id]);
  }
  // occupy_prefix: a prefix as it stands; the whole order without its spill slot
  std::vector<int> list;
  const int* src = nullptr;
  int len = -1;
  ++cases;
  if (!occupy_prefix(cs[1].order, 3, N, &list, &src, &len) || src != cs[1].order || len != 3)
    fail("occupy_prefix of a prefix", len, 0, 0);
  ++cases;
  const int whole[N] = {3, 1, 5, 2, 4};
  if (!occupy_prefix(cs[1].order, N + 1, N, &list, &src, &len) || len != N || std::memcmp(src, whole, sizeof(whole)))
    fail("occupy_prefix of the whole order", len, 0, 0);
  ++cases;
  const int nospill[N + 1] = {3, 1, 5, 2, 4, 1};
  if (occupy_prefix(nospill, N + 1, N, &list, &src, &len)) fail("occupy_prefix of N + 1 ids", len, 0, 0);
}

int main() {
  planner();
  items();
  ranks();
  std::printf("%lld cases, %lld violations\n", cases, bad);
  return bad ? 1 : 0;
}
