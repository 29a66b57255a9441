// Self-atari reading and the reference's candidate-move policy: isSelfAtari (base/board.cc:254-297) for every point of a position
// at once, FindAllCandidateMoves (board.cc:850-890) on top of it (k_candidates), and the playout kernels that pick from that list
// instead of "legal minus own true eyes": CandPolicy, the policy of k_playout_cand here and of k_playout_own<N, CandPolicy>
// (ownership.cuh).  One wave64 = one board, as everywhere else; Board<N> is used through its public members only, and the slot's
// labels and liberties are only read.
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
#include "playout.cuh"

#define CAND_WAVE 64   // k_candidates: one board per workgroup

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

// The candidate policy of the playouts: FindAllCandidateMoves' cut of the self-atari points of at least `thres` stones.  A
// threshold above N*N drops nothing (no group is that large): the self-atari reading is skipped and the step is k_playout's.
struct CandPolicy {
  int thres;
  template <int N>
  __device__ __forceinline__ u64 keep(const Board<N>& bd, u64 cand) const {
    if (thres <= Geo<N>::NP && bal_ne64(cand, 0ull)) cand &= ~self_atari_drop<N, false>(bd, cand, thres, nullptr);
    return cand;
  }
};

// k_playout (elf_amd.hip) with the candidate policy: the same RNG, x-major pick, termination and `out` words.
template <int N>
__global__ __launch_bounds__(PLAYOUT_WAVE * PLAYOUT_WAVES) void k_playout_cand(Pool<N> pool, const int32_t* ids, const u64* seeds, int n,
                                                                                int max_steps, int thres, uint32_t* out) {
  using G = Geo<N>;
  __shared__ Slot<N> lds_all[PLAYOUT_WAVES];
  __shared__ u64 zlds[G::P];
  __shared__ u32 mlds[G::NP + 2];
  playout_tables<N, PLAYOUT_WAVE * PLAYOUT_WAVES>(pool.zob, zlds, mlds);
  __syncthreads();
  const int wv = rfl((int)(threadIdx.x >> 6));   // wave-uniform by construction
  const int game = blockIdx.x * PLAYOUT_WAVES + wv;
  if (game >= n) return;
  Slot<N>& lds = lds_all[wv];
  const int b = rfl(ids ? ids[game] : game);
  Board<N> bd;
  bd.init(&lds, pool.zob, pool.skr(b));
  bd.load(&pool.slots[b]);
  const GameSK<N> sk{pool.skr(b)};
  const u32 key = playout_key(seeds[game]);
  bd.playout_begin(zlds);
  const int steps = playout_run<N>(bd, sk, key, max_steps, CandPolicy{thres}, mlds);
  bd.store(&pool.slots[b]);
  if (bd.lane == 0) {
    const u64 h = bd.hash;
    uint32_t* o = out + (size_t)game * 4;
    o[0] = (u32)h; o[1] = (u32)(h >> 32); o[2] = (u32)bd.ply; o[3] = (u32)steps;
  }
}
