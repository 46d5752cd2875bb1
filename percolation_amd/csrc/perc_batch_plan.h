// perc_batch_plan.h -- the host-only plan of a batch call (no HIP, no device):
// an order's inverse permutation (order_ranks), the occupied prefix of an
// order as perc_occupy takes it (occupy_prefix), the checks every entry point
// makes of its lists and items (check_items) and the cut of a call's items
// into runs with the trials of a run numbered afresh (ItemRuns).
// tests/batch_plan_check.cpp runs all four on the CPU.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>

namespace perc {

// rank[tr * N + id - 1] = position of id in trial tr's order of N + 1 entries
// (the spill slot 0 takes a position and is no element; INT_MAX: absent)
inline void order_ranks(int ntrials, int N, const int* orders, int* rank) {
  std::fill(rank, rank + (size_t)ntrials * N, INT_MAX);
  for (int tr = 0; tr < ntrials; ++tr) {
    const int* o = orders + (size_t)tr * (N + 1);
    int* r = rank + (size_t)tr * N;
    for (int pos = 0; pos <= N; ++pos) {
      const int id = o[pos];
      if (id >= 1 && id <= N && r[id - 1] == INT_MAX) r[id - 1] = pos;
    }
  }
}

// the first cnt entries of an order of N + 1 as perc_occupy takes them: the
// whole order (cnt > N) with the spill slot dropped
inline bool occupy_prefix(const int* o, int cnt, int N, std::vector<int>* list, const int** src, int* len) {
  *src = o;
  *len = cnt;
  if (cnt <= N) return true;
  list->clear();
  for (int k = 0; k < cnt; ++k)
    if (o[k] != 0) list->push_back(o[k]);
  if ((int)list->size() > N) return false;
  *src = list->data();
  *len = (int)list->size();
  return true;
}

// The lists and items of a call of a kind that reads the site lists (need_s)
// and / or the bond lists (need_b): the order or seed lists it reads present,
// item_trial, out and its count lists present, every item_trial inside
// 0..ntrials-1, item_nsites inside 0..t+1, item_nbonds inside 0..nb+1.
// NULL, or what is wrong (the caller reports it under its own name).
inline const char* check_items(bool need_s, bool need_b, bool seeded, int ntrials, const int* site_src,
                               const int* bond_src, int nitems, const int* item_trial, const int* item_nsites,
                               const int* item_nbonds, const void* out, int t, int nb) {
  if (ntrials && ((need_s && !site_src) || (need_b && !bond_src)))
    return seeded ? "a seed list the kind reads is missing" : "an order list the kind reads is missing";
  if (nitems && (!item_trial || !out || (need_s && !item_nsites) || (need_b && !item_nbonds)))
    return "item_trial, out or a count list the kind reads is missing";
  for (int i = 0; i < nitems; ++i) {
    if (item_trial[i] < 0 || item_trial[i] >= ntrials) return "item_trial outside 0..ntrials-1";
    if (need_s && (item_nsites[i] < 0 || item_nsites[i] > t + 1)) return "item_nsites outside 0..t+1";
    if (need_b && (item_nbonds[i] < 0 || item_nbonds[i] > nb + 1)) return "item_nbonds outside 0..nb+1";
  }
  return nullptr;
}

// A call's items cut into runs of at most cap items, in order: next() moves
// to the following run, items [i0, i0 + n), and is false after the last.  A
// run names its trials afresh in order of first use -- used[j] is the call's
// trial behind the run's trial j, local[i - i0] the run's trial of item i --
// so a run of k items names at most k trials and the bound on the run bounds
// its rank arrays too.  item_trial NULL: the bounds alone (the caller's trial
// numbers stand); else every entry lies inside 0..ntrials-1 (check_items).
struct ItemRuns {
  int i0 = 0, n = 0;
  std::vector<int> used, local;
  ItemRuns(const int* item_trial, int nitems, int ntrials, int cap)
      : trial_(item_trial), nitems_(nitems), cap_(std::max(1, cap)), slot_(item_trial ? (size_t)ntrials : 0, -1) {}
  bool next() {
    i0 += n;
    n = std::max(0, std::min(cap_, nitems_ - i0));
    if (n == 0 || !trial_) return n > 0;
    for (int tr : used) slot_[tr] = -1;
    used.clear();
    local.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
      int& s = slot_[trial_[i0 + i]];
      if (s < 0) {
        s = (int)used.size();
        used.push_back(trial_[i0 + i]);
      }
      local[i] = s;
    }
    return true;
  }

 private:
  const int* trial_;
  int nitems_, cap_;
  std::vector<int> slot_;  // a trial's number in the current run, or -1
};

}  // namespace perc
