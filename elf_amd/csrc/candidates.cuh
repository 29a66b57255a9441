// Self-atari reading and the reference's candidate-move policy: isSelfAtari (base/board.cc:254-297) for every point of a position
// at once, FindAllCandidateMoves (board.cc:850-890) on top of it (k_candidates), and the playout kernels that pick from that list
// instead of "legal minus own true eyes" (k_playout_cand, k_playout_own_cand).  One wave64 = one board, as everywhere else;
// Board<N> is used through its public members only, and the slot's labels and liberties are only read.
//   self-atari: the group that stands on the point after the move has exactly one liberty; num_stones is its size.
//   prefilter:  isSelfAtari's two early exits, for all points at once on bitboards: two or more empty neighbours, or an own
//               neighbour whose group has more than two liberties, and the move cannot end with one liberty (both are implied
//               by the exact count, so the filter only saves work).  An enemy neighbour in atari counts like an empty one: the
//               move captures it.
//   lone:       a point the filter leaves that has no own neighbour is a self-atari of one stone (its liberties are those
//               neighbours, and a legal move has one): settled on the bitboards, no labels read.
//   count:      per remaining point ("suspect"), wave-uniform.  One own neighbour group and no capture: that group's liberties
//               minus the point plus the empty neighbours no other stone of the group touches (MergeToGroup's count, as
//               Board::forward has it).  Otherwise the own neighbour groups plus the stone as a bitboard (a label compare over
//               the R rounds, the labels read once per position and only when there is a suspect), the stones of enemy
//               neighbour groups in atari as a second one, and liberties = |dilate(group) & (empty - point + captured)| -- a
//               union, so a liberty two merged groups share counts once.  The group's size is counted only for a point that
//               is a self-atari, and only where it is read.
#pragma once
#include "go_board.cuh"
#include "engine_host.h"
#include "ownership.cuh"

#define CAND_WAVE 64
#define CAND_WAVES 4   // boards per workgroup of the playout kernels: k_playout's PLAYOUT_WAVES

// The self-atari points among `test` (lane-distributed, a subset of the legal points of the side to move) whose group would
// have at least `thres` stones: what FindAllCandidateMoves drops (board.cc:880-885).  bd.at_cache must be the atari set of the
// position (legal_moves<.., true> has just run).  STONES: also stones_row[a] = num_stones for EVERY self-atari point of `test`,
// whatever its size (the caller has zeroed the row; LDS).  No global memory is touched; control flow is wave-uniform throughout
// (ctz over the suspect words).
template <int N, bool STONES>
__device__ __forceinline__ u64 self_atari_drop(const Board<N>& bd, u64 test, int thres, int16_t* stones_row) {
  using G = Geo<N>;
  constexpr int R = G::R;
  const Slot<N>* const L = bd.L;
  const int lane = bd.lane;
  const int player = bd.next_player;
  const u64 mblack = player == S_BLACK ? ~0ull : 0ull;
  const u32 ownbit = player == S_WHITE ? 0x8000u : 0u;
  const u64 Own = (bd.Bw & mblack) | (bd.Ww & ~mblack), Opp = (bd.Ww & mblack) | (bd.Bw & ~mblack);
  const u64 E = ~(bd.Bw | bd.Ww) & bd.mValid;
  // a neighbour that is empty, or an enemy stone in atari (the move captures it), is a liberty of the group on the point after
  // the move: two of them, and it is no self-atari
  const u64 F = E | (Opp & bd.at_cache);
  const u64 n1 = bd.sh_m1(F), n2 = bd.sh_p1(F), n3 = bd.sh_mN(F), n4 = bd.sh_pN(F);
  const u64 le1 = test & ~((n1 & n2) | (n3 & n4) | ((n1 | n2) & (n3 | n4)));
  const u64 nearOwn = bd.dilate(Own);
  // no own neighbour: a lone stone whose liberties are exactly those neighbours -- one of them (none would be suicide), so
  // every such point is a self-atari of one stone
  const u64 lone = le1 & ~nearOwn;
  u64 drop = thres <= 1 ? lone : 0ull;
  if (STONES) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if ((rl64(lone, k) >> lane) & 1) stones_row[k * 64 + lane] = 1;
    }
  }
  u64 suspect = le1 & nearOwn;
  if (bal_ne64(suspect, 0ull)) {
    // labels of every point, kept for the group compares below; an own neighbour whose group has more than two liberties
    // keeps two of them
    u32 v[R], lb[R];
#pragma unroll
    for (int k = 0; k < R; ++k) v[k] = L->pt[bd.idx[k]];
#pragma unroll
    for (int k = 0; k < R; ++k) lb[k] = L->libs[v[k] & 0x7FFFu];
    u64 big = 0;
#pragma unroll
    for (int k = 0; k < R; ++k) set_lane64(big, k, bal_gt(lb[k], 2u));
    suspect &= ~bd.dilate(Own & big);
#pragma unroll 1
    for (int k = 0; k < R; ++k) {
      u64 sm = rl64(suspect, k);
      u64 dk = rl64(drop, k);
      while (sm) {   // at most 64 rounds: one bit leaves per round
        const int la = (int)__builtin_ctzll(sm);
        sm &= sm - 1;
        const int a = k * 64 + la;
        const int i = Board<N>::a2i_u(a);
        // lanes 0..3: label of the neighbour and liberties of its group (libs[0] = 0 serves empty and border labels)
        const u32 nv = lane < 4 ? (u32)L->pt[i + bd.dl4] : (u32)PT_BORDER;
        const u32 nl = L->libs[nv & 0x7FFFu];
        const u64 stone = bal_ne(nv & 0x7FFFu, 0u);
        const u64 ownm = stone & bal_eq(nv & 0x8000u, ownbit);
        const u32 capm = (u32)(stone & ~ownm & bal_eq(nl, 1u));   // neighbours whose (enemy) group the move captures
        // the point has an own neighbour (it is in dilate(Own)): the first one's label
        const int f = (int)__builtin_ctzll(ownm);
        const u32 lab = (u32)rl((int)nv, f);
        const bool one_group = capm == 0 && (ownm & bal_ne(nv, lab)) == 0;
        int libs;
        u64 gw = 0;
        if (one_group) {
          // one own group joins and nothing is captured, the common case: MergeToGroup's count (board.cc:677-708) as
          // Board::forward restates it -- the point stops being a liberty, an empty neighbour is a new one unless another
          // stone of the group already touches it (lanes 0..11: the three other sides of neighbour lane / 3).  No bitboard.
          const u32 side = *reinterpret_cast<const u16*>(reinterpret_cast<const char*>(&L->pt[i]) + bd.t12_off);
          const u32 t = (u32)bal_eq(side, lab) & 0xFFFu;
          const u32 emp4 = (u32)bal_eq(nv, 0u) & 0xFu;
          const int add = ((emp4 & 1u) && ((t & 7u) == 0)) + ((emp4 & 2u) && (((t >> 3) & 7u) == 0)) +
                          ((emp4 & 4u) && (((t >> 6) & 7u) == 0)) + ((emp4 & 8u) && (((t >> 9) & 7u) == 0));
          libs = rl((int)nl, f) - 1 + add;
        } else {
          // the own neighbour groups as a bitboard (~0: no label), the captured stones as another, and the union's liberties
          const u32 ov = lane_bit(ownm) ? nv : ~0u;
          const u32 o0 = (u32)rl((int)ov, 0), o1 = (u32)rl((int)ov, 1), o2 = (u32)rl((int)ov, 2), o3 = (u32)rl((int)ov, 3);
          u64 capw = 0;
#pragma unroll
          for (int q = 0; q < R; ++q) set_lane64(gw, q, bal_eq(v[q], o0) | bal_eq(v[q], o1) | bal_eq(v[q], o2) | bal_eq(v[q], o3));
          gw &= bd.mValid;   // drops the clamped lanes of the last round (they re-read point 0)
          if (capm) {
            const u32 cv = lane_bit((u64)capm) ? nv : ~0u;
            const u32 c0 = (u32)rl((int)cv, 0), c1 = (u32)rl((int)cv, 1), c2 = (u32)rl((int)cv, 2), c3 = (u32)rl((int)cv, 3);
#pragma unroll
            for (int q = 0; q < R; ++q) set_lane64(capw, q, bal_eq(v[q], c0) | bal_eq(v[q], c1) | bal_eq(v[q], c2) | bal_eq(v[q], c3));
            capw &= bd.mValid;
          }
          const u64 abit = lane == k ? (1ull << la) : 0ull;
          libs = bd.popc_lanes(bd.dilate(gw | abit) & ((E & ~abit) | capw));
        }
        if (libs == 1) {
          int num = thres;   // where nobody reads the size (no stones row, every self-atari dropped), only "num >= thres" matters
          if (STONES || thres > 1) {
            if (one_group) {
#pragma unroll
              for (int q = 0; q < R; ++q) set_lane64(gw, q, bal_eq(v[q], lab));
              gw &= bd.mValid;
            }
            num = bd.popc_lanes(gw) + 1;
          }
          if (num >= thres) dk |= 1ull << la;
          if (STONES) { if (lane == 0) stones_row[a] = (int16_t)num; }
        }
      }
      set_lane64(drop, k, dk);
    }
  }
  return drop;
}

// mask[i][a] = 1 iff a = x*N + y is in FindAllCandidateMoves(board, next_player, thres); stones[i][a] = the num_stones isSelfAtari
// writes where it returns true (every legal point of the mover, own true eyes included), else 0.  The pool slot is only read.
// A row whose slot id lies outside the pool reads nothing: mask 0, stones -1.
template <int N>
__global__ __launch_bounds__(CAND_WAVE) void k_candidates(Pool<N> pool, int capacity, const int32_t* ids, int n, int thres, uint8_t* mask,
                                                           int16_t* stones) {
  using G = Geo<N>;
  constexpr int R = G::R;
  __shared__ Slot<N> lds;
  __shared__ int16_t st[G::NP];
  const int row = blockIdx.x;
  const int b = rfl(ids ? ids[row] : row);
  const int lane = threadIdx.x;
  uint8_t* const mrow = mask ? mask + (size_t)row * G::NP : nullptr;
  int16_t* const srow = stones ? stones + (size_t)row * G::NP : nullptr;
  if (b < 0 || b >= capacity) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int a = k * 64 + lane;
      if (a < G::NP) {
        if (mrow) mrow[a] = 0;
        if (srow) srow[a] = (int16_t)-1;
      }
    }
    return;
  }
  for (int a = lane; a < G::NP; a += CAND_WAVE) st[a] = 0;
  Board<N> bd;
  bd.init(&lds, pool.zob, pool.skr(b));
  bd.load(&pool.slots[b]);   // its fence orders the zero fill of st before the counts below
  u64 legal, cand;
  bd.template legal_moves<true, true>(legal, cand);   // INCR: leaves the atari set in bd.at_cache
  const u64 drop = self_atari_drop<N, true>(bd, legal, thres, st);
  Board<N>::wsync();
  const u64 keep = cand & ~drop;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int a = k * 64 + lane;
    const u64 wk = rl64(keep, k);
    if (a < G::NP) {
      if (mrow) mrow[a] = (uint8_t)((wk >> lane) & 1);
      if (srow) srow[a] = st[a];
    }
  }
}

// k_playout's pick: the (x % total)-th set bit of the lane-distributed candidate bitboard in x-major order, -1 when there is none.
// Inclusive prefix sum of the word counts over the lanes of row 0 on the DPP network, the word, the rank inside it; mlds[d] =
// floor(2^32 / d) (the estimate of x / total is at most one too small).
template <int N>
__device__ __forceinline__ int cand_pick(u64 cand, u32 x, const u32* mlds) {
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

// One playout step with the candidate policy; returns 0 when forward refused (the game is over).  A threshold above N*N drops
// nothing (no group is that large): the self-atari reading is skipped and the step is k_playout's.
template <int N>
__device__ __forceinline__ int cand_step(Board<N>& bd, const GameSK<N>& sk, u32 key, int thres, const u32* mlds) {
  const u32 x = playout_rng_k(key, (u32)bd.ply);
  u64 legal, cand;
  bd.template legal_moves<true, true>(legal, cand);
  if (thres <= Geo<N>::NP && bal_ne64(cand, 0ull)) cand &= ~self_atari_drop<N, false>(bd, cand, thres, nullptr);
  const int pick_a = cand_pick<N>(cand, x, mlds);
  return pick_a >= 0 ? bd.forward_legal_action(pick_a, sk) : bd.forward(M_PASS, sk);
}

// k_playout (elf_amd.hip) with the candidate policy: the same RNG, x-major pick, termination and `out` words.
template <int N>
__global__ __launch_bounds__(CAND_WAVE * CAND_WAVES) void k_playout_cand(Pool<N> pool, const int32_t* ids, const u64* seeds, int n,
                                                                          int max_steps, int thres, uint32_t* out) {
  using G = Geo<N>;
  __shared__ Slot<N> lds_all[CAND_WAVES];
  __shared__ u64 zlds[G::P];
  __shared__ u32 mlds[G::NP + 2];   // floor(2^32 / d) for the pick's rng % candidates
  for (int j = threadIdx.x; j < G::P; j += CAND_WAVE * CAND_WAVES) zlds[j] = pool.zob[j];
  for (int j = threadIdx.x; j < G::NP + 2; j += CAND_WAVE * CAND_WAVES) mlds[j] = (u32)pool.zob[G::ZOBW + 4 * G::R + j];
  __syncthreads();
  const int wv = rfl((int)(threadIdx.x >> 6));   // wave-uniform by construction
  const int game = blockIdx.x * CAND_WAVES + wv;
  if (game >= n) return;
  Slot<N>& lds = lds_all[wv];
  const int b = rfl(ids ? ids[game] : game);
  Board<N> bd;
  bd.init(&lds, pool.zob, pool.skr(b));
  bd.load(&pool.slots[b]);
  const GameSK<N> sk{pool.skr(b)};
  const u32 key = playout_key(seeds[game]);
  bd.playout_begin(zlds);
  int steps = 0;
  while (steps < max_steps && !bd.terminated()) {
    if (!cand_step<N>(bd, sk, key, thres, mlds)) break;
    ++steps;
  }
  bd.store(&pool.slots[b]);
  if (bd.lane == 0) {
    const u64 h = bd.hash;
    uint32_t* o = out + (size_t)game * 4;
    o[0] = (u32)h; o[1] = (u32)(h >> 32); o[2] = (u32)bd.ply; o[3] = (u32)steps;
  }
}

// k_playout_own (ownership.cuh) with the candidate policy: the same seed rule, work split, record areas and integer sums.
template <int N>
__global__ __launch_bounds__(CAND_WAVE * CAND_WAVES) void k_playout_own_cand(Pool<N> pool, u64* scratch, const int32_t* ids, const u64* seeds,
                                                                              int n, int K, int max_steps, float komi, int thres,
                                                                              int32_t* counts, unsigned long long* stats) {
  using G = Geo<N>;
  static_assert(CAND_WAVES == OWN_WAVES && CAND_WAVE == OWN_WAVE, "the ownership handle's record areas are sized for OWN_WAVES waves per workgroup");
  __shared__ Slot<N> lds_all[CAND_WAVES];
  __shared__ u64 zlds[G::P];
  __shared__ u32 mlds[G::NP + 2];
  __shared__ int acc[2 * G::NP];
  for (int j = threadIdx.x; j < G::P; j += CAND_WAVE * CAND_WAVES) zlds[j] = pool.zob[j];
  for (int j = threadIdx.x; j < G::NP + 2; j += CAND_WAVE * CAND_WAVES) mlds[j] = (u32)pool.zob[G::ZOBW + 4 * G::R + j];
  for (int j = threadIdx.x; j < 2 * G::NP; j += CAND_WAVE * CAND_WAVES) acc[j] = 0;
  __syncthreads();
  const int wv = rfl((int)(threadIdx.x >> 6));
  u64* const rec = scratch + (size_t)(blockIdx.x * CAND_WAVES + wv) * (G::MAXMOVE + 2) * G::SKW;
  Slot<N>& lds = lds_all[wv];
  Board<N> bd;
  bd.init(&lds, pool.zob, rec);
  const GameSK<N> sk{rec};
  const int pairs = n * K, groups = (pairs + CAND_WAVES - 1) / CAND_WAVES;   // n * K < 2^31 - CAND_WAVES: checked by the host
  const int q0 = (int)((long long)groups * blockIdx.x / gridDim.x), q1 = (int)((long long)groups * (blockIdx.x + 1) / gridDim.x);
  int have = -1;     // the slot whose record prefix `rec` holds
  int wg_row = -1;   // the row `acc` counts for
  auto flush = [&]() {
    int* g = counts + (size_t)wg_row * 2 * G::NP;
    for (int j = threadIdx.x; j < 2 * G::NP; j += CAND_WAVE * CAND_WAVES) {
      const int v = acc[j];
      if (v) { atomicAdd(&g[j], v); acc[j] = 0; }
    }
  };
  for (int q = q0; q < q1; ++q) {
    const int row0 = q * CAND_WAVES / K;
    if (row0 != wg_row) {   // the same decision in every wave of the workgroup
      if (wg_row >= 0) { flush(); __syncthreads(); }
      wg_row = row0;
    }
    const int p = q * CAND_WAVES + wv;
    if (p < pairs) {
      const int row = p / K, k = p - row * K;
      const int b = rfl(ids ? ids[row] : row);
      bd.load(&pool.slots[b]);
      if (b != have) {
        const u64* src = pool.skr(b);
        for (int j = bd.lane; j < bd.sk_len * G::SKW; j += CAND_WAVE) rec[j] = src[j];
        have = b;
      }
      const u32 key = playout_key(own_seed(seeds[row], k));
      bd.playout_begin(zlds);
      int steps = 0;
      while (steps < max_steps && !bd.terminated()) {
        if (!cand_step<N>(bd, sk, key, thres, mlds)) break;
        ++steps;
      }
      u32 ab, aw;
      area_rows<N>(bd, ab, aw);
      const int diff = area_diff(ab, aw);
      if (row == wg_row) own_add_rows<N>(acc, ab, aw, bd.lane);
      else own_add_rows<N>(counts + (size_t)row * 2 * G::NP, ab, aw, bd.lane);
      if (bd.lane == 0) {
        unsigned long long* st = stats + (size_t)row * 4;
        atomicAdd(&st[0], (unsigned long long)(long long)diff);
        if ((float)diff - komi > 0.0f) atomicAdd(&st[1], 1ull);
        if (bd.superko) atomicAdd(&st[2], 1ull);
        atomicAdd(&st[3], (unsigned long long)steps);
      }
    }
    __syncthreads();   // this group's LDS adds are in before a flush reads them
  }
  if (wg_row >= 0) flush();
}
