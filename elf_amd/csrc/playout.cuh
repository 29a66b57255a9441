// The playout the device kernels share: one step (rng draw, legal moves, the policy's cut, the x-major pick, forward), the loop
// around it, the workgroup prologue that copies the Zobrist constants and the pick's reciprocal table into LDS, and playout_pairs,
// the persistent-wave harness of the kernels that play K playouts per source row.  Used by k_playout_own<N, Policy> (ownership.cuh),
// k_playout_ld (region.cuh) and, without the harness, k_playout_cand (candidates.cuh).  k_playout (elf_amd.hip) plays EyePolicy's game
// from a text of its own: its file is under the hash of the profiled kernel sources (elf_amd._lib.KERNEL_SOURCES), so folding
// it onto playout_step, like a translation unit of their own for these kernels, waits for the next re-profiling visit.
//   Policy: `template <int N> u64 keep(const Board<N>&, u64 cand) const` returns the subset of `cand` (legal minus own true
//           eyes, lane-distributed, bd.at_cache fresh) to pick from; the object travels as a kernel argument.
//   Tally:  what a playout_pairs kernel counts: its LDS accumulators and output pointers behind flush / play (see playout_pairs).
#pragma once
#include "go_board.cuh"
#include "engine_host.h"

#define PLAYOUT_WAVE 64
#define PLAYOUT_WAVES 4   // boards per workgroup of every playout kernel
#define OWN_WAVE PLAYOUT_WAVE
#define OWN_WAVES PLAYOUT_WAVES   // boards per workgroup of a playout_pairs kernel; the ElfGoOwnership record areas are sized by it

// seed(i, k) = seeds[i] + k * 0x9E3779B97F4A7C15 (mod 2^64): playout 0 of a row is what k_playout plays with seeds[i]
__device__ __forceinline__ u64 own_seed(u64 row_seed, int k) { return row_seed + (u64)k * 0x9E3779B97F4A7C15ull; }

// k_playout's policy: every legal point that is no true eye of the mover.
struct EyePolicy {
  template <int N>
  __device__ __forceinline__ u64 keep(const Board<N>&, u64 cand) const { return cand; }
};

// zlds[G::P] = the Zobrist constants, mlds[G::NP + 2] = floor(2^32 / d) for the pick's rng % candidates; all THREADS threads of
// the workgroup call it, and a __syncthreads() of the caller's comes before the first use.
template <int N, int THREADS>
__device__ __forceinline__ void playout_tables(const u64* zob, u64* zlds, u32* mlds) {
  using G = Geo<N>;
  for (int j = threadIdx.x; j < G::P; j += THREADS) zlds[j] = zob[j];
  for (int j = threadIdx.x; j < G::NP + 2; j += THREADS) mlds[j] = (u32)zob[G::ZOBW + 4 * G::R + j];
}

// k_playout's pick: the (x % total)-th set bit of the lane-distributed candidate bitboard in x-major order, -1 when there is none.
// Inclusive prefix sum of the word counts over the lanes of row 0 on the DPP network, the word, the rank inside it; mlds[d] =
// floor(2^32 / d) (the estimate of x / total is at most one too small).
template <int N>
__device__ __forceinline__ int playout_pick(u64 cand, u32 x, const u32* mlds) {
  using G = Geo<N>;
  const int cnt = __popcll(cand);
  int inc = cnt;
  inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xf, 0xf, true);
  inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xf, 0xf, true);
  if (G::R > 4) inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xf, 0xf, true);
  const int total = rl(inc, G::R - 1);
  if (total <= 0) return -1;
  const u32 qd = __umulhi(x, (u32)rfl((int)mlds[total]));
  u32 rr = x - qd * (u32)total;
  if (rr >= (u32)total) rr -= (u32)total;
  const int kw = __popc((u32)bal_le((u32)inc, rr) & ((1u << G::R) - 1u));
  const int base = rl(inc - cnt, kw);
  const u64 wk = rl64(cand, kw);
  const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(wk >> 32), __builtin_amdgcn_mbcnt_lo((u32)wk, 0));
  const u64 sel = bal_eq(rank, rr - (u32)base) & wk;
  return kw * 64 + (int)__builtin_ctzll(sel);
}

// One move: uniform over pol.keep(legal, non-true-eye points) in x-major order, rng % count with playout_rng_k(key, ply), pass
// when there is none.  Returns 0 when forward refused (the game is over).
template <int N, class Policy>
__device__ __forceinline__ int playout_step(Board<N>& bd, const GameSK<N>& sk, u32 key, Policy pol, const u32* mlds) {
  const u32 x = playout_rng_k(key, (u32)bd.ply);   // depends on the ply only: issued ahead of the legal-move work
  u64 legal, cand;
  bd.template legal_moves<true, true>(legal, cand);
  cand = pol.template keep<N>(bd, cand);
  const int pick_a = playout_pick<N>(cand, x, mlds);
  // a candidate comes from the legal mask of this very position: forward_legal_action skips TryPlay's re-check
  return pick_a >= 0 ? bd.forward_legal_action(pick_a, sk) : bd.forward(M_PASS, sk);
}

// Plays bd on until the game ends or max_steps moves are made; returns the moves made.  bd.playout_begin has run.
template <int N, class Policy>
__device__ __forceinline__ int playout_run(Board<N>& bd, const GameSK<N>& sk, u32 key, int max_steps, Policy pol, const u32* mlds) {
  int steps = 0;
  while (steps < max_steps && !bd.terminated()) {
    if (!playout_step<N>(bd, sk, key, pol, mlds)) break;
    ++steps;
  }
  return steps;
}

// The persistent-wave harness of k_playout_own and k_playout_ld: for source row i < n and playout k < K one wave plays a private
// copy of slot ids[i] (ids null = slot i) and the kernel's tally counts the result.  Called by every thread of the workgroup, after
// the kernel's LDS prologue (playout_tables, zeroed accumulators, __syncthreads()).
//  * The source slot is only read.  The copy lives in the wave's LDS slot of lds_all[OWN_WAVES]; its super-ko records go to the
//    wave's own record area in `scratch` ([waves in flight][MAXMOVE+2][SKW] u64, the ElfGoOwnership handle's), which receives the
//    source's first sk_len records whenever the wave turns to another slot (a playout only appends behind them, so they survive
//    from one playout of a slot to the next).
//  * Waves are persistent: the (i, k) pairs, row-major, are cut into groups of OWN_WAVES consecutive pairs and workgroup g plays a
//    contiguous run of groups, one pair per wave.  Scratch is therefore bounded by the waves in flight.  A row whose slot id lies
//    outside the pool ([0, capacity)) is not played: the tally never sees it.
//  * Counters are accumulated in LDS for the row the workgroup is on (the row of a group's first pair) and flushed when that row
//    changes and at the end; a wave whose pair already belongs to the next row (a group may straddle two rows) adds to the global
//    counters directly.  Integer atomics only, so the sums do not depend on who adds first.
//   t.flush(row): all threads of the workgroup; adds the LDS accumulators into global row `row` and clears them.
//   t.play(bd, sk, row, k, local, wv, zlds, mlds): one wave, bd freshly loaded; plays pair (row, k) and adds to the LDS accumulators
//           when `local`, else to global row `row`.  wv = the wave's index in the workgroup, for per-wave LDS of the tally's own.
template <int N, class Tally>
__device__ __forceinline__ void playout_pairs(const Pool<N>& pool, int capacity, u64* scratch, const int32_t* ids, int n, int K,
                                              Slot<N>* lds_all, const u64* zlds, const u32* mlds, Tally& t) {
  using G = Geo<N>;
  const int wv = rfl((int)(threadIdx.x >> 6));   // wave-uniform by construction
  u64* const rec = scratch + (size_t)(blockIdx.x * OWN_WAVES + wv) * (G::MAXMOVE + 2) * G::SKW;
  Board<N> bd;
  bd.init(&lds_all[wv], pool.zob, rec);
  const GameSK<N> sk{rec};
  const int pairs = n * K, groups = (pairs + OWN_WAVES - 1) / OWN_WAVES;   // n * K < 2^31 - OWN_WAVES: checked by the host
  const int q0 = (int)((long long)groups * blockIdx.x / gridDim.x), q1 = (int)((long long)groups * (blockIdx.x + 1) / gridDim.x);
  int have = -1;     // the slot whose record prefix `rec` holds
  int wg_row = -1;   // the row the tally's LDS accumulators count for
  for (int q = q0; q < q1; ++q) {
    const int row0 = q * OWN_WAVES / K;
    if (row0 != wg_row) {   // the same decision in every wave of the workgroup
      if (wg_row >= 0) { t.flush(wg_row); __syncthreads(); }
      wg_row = row0;
    }
    const int p = q * OWN_WAVES + wv;
    const int row = p < pairs ? p / K : 0, k = p - row * K;
    const int b = p < pairs ? rfl(ids ? ids[row] : row) : -1;
    if (b >= 0 && b < capacity) {
      bd.load(&pool.slots[b]);
      if (b != have) {
        const u64* src = pool.skr(b);
        for (int j = bd.lane; j < bd.sk_len * G::SKW; j += OWN_WAVE) rec[j] = src[j];
        have = b;
      }
      t.play(bd, sk, row, k, row == wg_row, wv, zlds, mlds);
    }
    __syncthreads();   // this group's LDS adds are in before a flush reads them
  }
  if (wg_row >= 0) t.flush(wg_row);
}
