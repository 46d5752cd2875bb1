// perc_batch_shuffle.hip -- k_shuffle_ranks: one wave runs one trial's
// reference shuffle (srand(seed) + the REAL*4 Fisher-Yates of bondc.f:162-174,
// perc_shuffle_seeded) on ids 1..N with the spill slot 0, the order in LDS as
// N + 1 entries of 16 bits, and leaves the order's inverse permutation in
// device memory: rank[trial * N + id - 1] = position of id, the layout
// order_ranks uploads for k_batch_cond and k_batch_scan.  A trial's swaps are
// serial; the trials of a launch are independent, one workgroup of one wave
// each.  Every loop is bounded by N; no polling, no word shared between
// workgroups.
#include <cstdlib>
#include <cstring>

#include "perc_batch.h"
#include "perc_common.h"

namespace perc {
namespace {

struct ShuffleArgs {
  int N;
  const int* seeds;  // ntrials
  int* rank;         // ntrials x N
  int* orders;       // ntrials x (N + 1), or NULL
  ShuffleLds L;
};

constexpr unsigned long long kLcgA = 16807ULL, kLcgM = 2147483647ULL;

// LocalRand's state after srand(seed) (perc_ensemble.cpp)
__device__ inline unsigned long long lcg_seed(int seed) {
  return seed ? (unsigned long long)seed : 123459876ULL;
}

// the swap target of step i from the generator's state s after its update:
// LocalRand::next's REAL*4 mapping and perc_shuffle_seeded's index, operation
// for operation.  (float)2147483646 is 2^31: the quotient is exact.
__device__ inline int swap_target(unsigned long long s, int i, int N) {
  const unsigned v = (unsigned)((int)s - 1) & (~0u << 9);
  const float r = (float)v / (float)2147483646;
  const float prod = (float)(N - i + 1) * r;
  int j = (int)((float)i + prod);
  return min(max(j, 1), N + 1);
}

// JUMP = false: lane 0 runs the generator and the swaps.  JUMP = true: the 64
// lanes compute the targets of 64 consecutive steps by jump-ahead -- lane k's
// state is 16807^k * s mod 2^31 - 1, one product under 2^62 -- and lane 0
// applies them.  The orders are the same bit for bit.
template <bool JUMP>
__global__ __launch_bounds__(64) void k_shuffle_ranks(ShuffleArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* o = reinterpret_cast<unsigned short*>(smem);
  int* sj = reinterpret_cast<int*>(smem + a.L.oJ);
  const int N = a.N, lane = threadIdx.x;
  const int trial = blockIdx.x;

  for (int k = lane; k < N; k += 64) o[k] = (unsigned short)(k + 1);
  if (lane == 0) o[N] = 0;
  __syncthreads();

  // the first update takes the raw seed (a negative one wraps as unsigned 64
  // bit, as on the host); every later state lies under 2^31 - 1
  unsigned long long s = (kLcgA * lcg_seed(a.seeds[trial])) % kLcgM;
  if (!JUMP) {
    if (lane == 0) {
      for (int i = 1; i <= N; ++i) {
        const int j = swap_target(s, i, N);
        const unsigned short x = o[i - 1], y = o[j - 1];
        o[i - 1] = y;
        o[j - 1] = x;
        s = (kLcgA * s) % kLcgM;
      }
    }
  } else {
    unsigned long long mult = 1;  // 16807^lane mod 2^31 - 1
    for (int q = 0; q < lane; ++q) mult = (mult * kLcgA) % kLcgM;
    for (int i0 = 1; i0 <= N; i0 += 64) {
      const unsigned long long sl = (mult * s) % kLcgM;  // the state of step i0 + lane
      sj[lane] = i0 + lane <= N ? swap_target(sl, i0 + lane, N) : 0;
      // lane 63's state, once more: the state of step i0 + 64
      s = (kLcgA * (unsigned long long)__builtin_amdgcn_readlane((int)sl, 63)) % kLcgM;
      __syncthreads();
      if (lane == 0) {
        int jj[64];
#pragma unroll
        for (int k = 0; k < 64; ++k) jj[k] = sj[k];
#pragma unroll
        for (int k = 0; k < 64; ++k) {
          const int i = i0 + k;
          if (i > N) break;
          const unsigned short x = o[i - 1], y = o[jj[k] - 1];
          o[i - 1] = y;
          o[jj[k] - 1] = x;
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();

  int* __restrict__ rank = a.rank + (size_t)trial * N;
  for (int pos = lane; pos <= N; pos += 64) {
    const int id = o[pos];
    if (id != 0) rank[id - 1] = pos;
  }
  if (a.orders) {
    int* __restrict__ ord = a.orders + (size_t)trial * (N + 1);
    for (int pos = lane; pos <= N; pos += 64) ord[pos] = o[pos];
  }
}

struct ShuffleState {
  int* d_seeds = nullptr;
  size_t seed_cap = 0;
  int* d_orders = nullptr;
  size_t order_cap = 0;
  int* d_rank = nullptr;  // the ranks of a free-standing list (kShuffleFree)
  size_t rank_cap = 0;
  int lds_attr[2] = {};  // dynamic LDS granted per instantiation
};

}  // namespace

void dev_shuffle_free(perc_ctx* h) {
  ShuffleState* S = static_cast<ShuffleState*>(h->shuffle);
  if (!S) return;
  (void)hipFree(S->d_seeds);
  (void)hipFree(S->d_orders);
  (void)hipFree(S->d_rank);
  delete S;
  h->shuffle = nullptr;
}

hipError_t dev_shuffle_run(perc_ctx* h, int list, int ntrials, const int* seeds, int* orders_out,
                           int* ranks_out, int nfree) {
  if (ntrials == 0) return hipSuccess;
  if (!h->shuffle) h->shuffle = new ShuffleState();
  ShuffleState* S = static_cast<ShuffleState*>(h->shuffle);
  hipStream_t st = h->stream;
  const int N = list == kShuffleFree ? nfree : (list == PERC_BOND ? (int)h->nb : h->g.t);
  int* d_rank = nullptr;
  if (list == kShuffleFree) {
    HIP_TRY(grow(&S->d_rank, &S->rank_cap, (size_t)ntrials * (size_t)N));
    d_rank = S->d_rank;
  } else {
    HIP_TRY(dev_batch_reserve(h, list, ntrials, &d_rank));
  }
  HIP_TRY(grow(&S->d_seeds, &S->seed_cap, (size_t)ntrials));
  const size_t nord = orders_out ? (size_t)ntrials * ((size_t)N + 1) : 0;
  HIP_TRY(grow(&S->d_orders, &S->order_cap, nord));
  HIP_TRY(hipMemcpyAsync(S->d_seeds, seeds, sizeof(int) * ntrials, hipMemcpyHostToDevice, st));
  ShuffleArgs a;
  a.N = N;
  a.seeds = S->d_seeds;
  a.rank = d_rank;
  a.orders = nord ? S->d_orders : nullptr;
  a.L = shuffle_lds(N);
  // PERC_SHUFFLE_FORM=plain: lane 0 alone (the A/B of tools/scan_bench.py)
  const char* form = std::getenv("PERC_SHUFFLE_FORM");
  if (form && !std::strcmp(form, "plain"))
    HIP_TRY(launch_lds(&k_shuffle_ranks<false>, &S->lds_attr[0], a, ntrials, 64, st, "k_shuffle_ranks"));
  else HIP_TRY(launch_lds(&k_shuffle_ranks<true>, &S->lds_attr[1], a, ntrials, 64, st, "k_shuffle_ranks"));
  if (nord) HIP_TRY(hipMemcpyAsync(orders_out, S->d_orders, sizeof(int) * nord, hipMemcpyDeviceToHost, st));
  if (ranks_out)
    HIP_TRY(hipMemcpyAsync(ranks_out, d_rank, sizeof(int) * (size_t)ntrials * (size_t)N,
                           hipMemcpyDeviceToHost, st));
  return hipStreamSynchronize(st);  // (seeds and the outputs are the caller's)
}

}  // namespace perc
