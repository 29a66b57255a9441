// The playout the device kernels share: one step (rng draw, legal moves, the policy's cut, the x-major pick, forward), the loop
// around it, and the workgroup prologue that copies the Zobrist constants and the pick's reciprocal table into LDS.  Used by
// k_playout_own<N, Policy> (ownership.cuh) and k_playout_cand (candidates.cuh).  k_playout (elf_amd.hip) plays EyePolicy's game
// from a text of its own: its file is under the hash of the profiled kernel sources (elf_amd._lib.KERNEL_SOURCES), so folding
// it onto playout_step, like a translation unit of their own for these kernels, waits for the next re-profiling visit.
//   Policy: `template <int N> u64 keep(const Board<N>&, u64 cand) const` returns the subset of `cand` (legal minus own true
//           eyes, lane-distributed, bd.at_cache fresh) to pick from; the object travels as a kernel argument.
#pragma once
#include "go_board.cuh"
#include "engine_host.h"

#define PLAYOUT_WAVE 64
#define PLAYOUT_WAVES 4   // boards per workgroup of every playout kernel

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
