// Position setup: stones in, complete board state out (k_setup).  One wave64 = one board, as everywhere else; Board<N> is used
// through its public members only.
//   result:  what clearBoard leaves (base/board.cc:79-107) plus the group tables of the stones, the Zobrist hash of the
//            stones (set_color, board.cc:38-51) and the side to move -- for black stones only, PlaceHandicap's board
//            (board.cc:109-126: ply stays 1, last moves stay invalid) -- with the position pushed as the one entry of the
//            history ring.  (The reference's applyHandicap leaves GoState::_history empty, so its net would see an empty
//            board under handicap stones: a defect nobody exercises there, not reproduced here.)
//   groups:  row bitboards in registers (lane x = row x, bit y), area_rows' layout: one flood fill to a fixed point per group,
//            seeded at the first stone no earlier fill has reached; liberties = popcount(dilate(group) & empty).  The label of
//            a group is its seed point (any representative is a valid root, go_board.cuh).
#pragma once
#include "go_board.cuh"
#include "engine_host.h"

#define SETUP_WAVE 64

// rows [x] = bits [x*N, x*N+N) of a bitboard given as its R wave-uniform words; lanes >= N get 0
template <int N>
__device__ __forceinline__ u32 setup_row(const u64 (&wd)[Geo<N>::R], int lane) {
  constexpr int R = Geo<N>::R;
  const int bit0 = (lane < N ? lane : 0) * N, w = bit0 >> 6, s = bit0 & 63;
  u64 lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    if (w == k) lo = wd[k];
    if (w + 1 == k) hi = wd[k];
  }
  const u32 r = (u32)(s ? ((lo >> s) | (hi << (64 - s))) : lo) & ((1u << N) - 1);
  return lane < N ? r : 0u;
}

// the 4-neighbourhood of a row bitboard (not masked: the caller ANDs with the rows it is interested in)
template <int N>
__device__ __forceinline__ u32 setup_dilate_rows(u32 g, int lane) {
  u32 up = __shfl_up(g, 1, 64), dn = __shfl_down(g, 1, 64);
  if (lane == 0) up = 0;
  if (lane >= N - 1) dn = 0;
  return (g << 1) | (g >> 1) | up | dn;
}

// stones[i][a]: 0 empty, 1 black, 2 white, a = x*N + y; next_player[i] 1 / 2 (NULL = Black).  ok[i] = 1 done, 0 refused (a byte
// above 2, a player other than 1 / 2, a group without a liberty, a slot id outside the pool): a refused slot is not written.
template <int N>
__global__ __launch_bounds__(SETUP_WAVE) void k_setup(Pool<N> pool, int capacity, const int32_t* ids, const uint8_t* stones,
                                                       const uint8_t* next_player, int n, uint8_t* ok) {
  using G = Geo<N>;
  constexpr int R = G::R, S = G::S;
  __shared__ Slot<N> lds;
  const int row = blockIdx.x;
  const int b = ids ? ids[row] : row;
  const int player = next_player ? (int)next_player[row] : S_BLACK;
  const int lane = threadIdx.x;
  // the stones, 64 points per round, as wave masks
  u32 st[R];
  u64 bw[R], ww[R];
  u64 too_big = 0;
  const uint8_t* src = stones + (size_t)row * G::NP;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int a = k * 64 + lane;
    st[k] = a < G::NP ? (u32)src[a] : 0u;
    bw[k] = bal_eq(st[k], (u32)S_BLACK);
    ww[k] = bal_eq(st[k], (u32)S_WHITE);
    too_big |= bal_gt(st[k], (u32)S_WHITE);
  }
  if (b < 0 || b >= capacity || too_big != 0 || (player != S_BLACK && player != S_WHITE)) {
    if (lane == 0 && ok) ok[row] = 0;
    return;
  }
  Board<N> bd;
  bd.init(&lds, pool.zob, pool.skr(b));
  bd.reset();
  // hash = XOR of the stones' Zobrist words (white: halves swapped)
  u64 xh = 0;
#pragma unroll
  for (int k = 0; k < R; ++k)
    if (st[k]) xh ^= zob_col(bd.zob[bd.idx[k]], (int)st[k]);
  const u64 hash = wave_xor64(xh);
  // groups: one fill per group on row bitboards
  const u32 Brow = setup_row<N>(bw, lane), Wrow = setup_row<N>(ww, lane);
  const u32 Erow = lane < N ? (~(Brow | Wrow) & ((1u << N) - 1)) : 0u;
  u32 rem_b = Brow, rem_w = Wrow;   // stones no fill has reached yet
  bool dead = false;
  for (;;) {
    const u64 mb = bal_ne(rem_b, 0u), mw = bal_ne(rem_w, 0u);
    if ((mb | mw) == 0) break;
    const bool white = mb == 0;   // black groups first, then white
    const int x0 = (int)__builtin_ctzll(white ? mw : mb);
    const int y0 = (int)__builtin_ctz((u32)rl((int)(white ? rem_w : rem_b), x0));
    const u32 own = white ? Wrow : Brow;
    u32 g = lane == x0 ? (1u << y0) : 0u;
    for (;;) {
      u32 ng = g | (own & setup_dilate_rows<N>(g, lane));
      // finish the in-row run before the next vertical exchange
      for (int q = 0; q < 5; ++q) ng |= own & ((ng << 1) | (ng >> 1));
      const bool ch = ng != g;
      g = ng;
      if (!__any(ch)) break;
    }
    int nl = __popc(Erow & setup_dilate_rows<N>(g, lane));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nl += __shfl_xor(nl, o, 64);
    nl = rfl(nl);
    if (nl == 0) { dead = true; break; }
    const int root = (x0 + 1) * S + (y0 + 1);
    const u16 label = (u16)((white ? 0x8000u : 0u) | (u32)root);
    u32 m = g;   // lanes >= N hold none
    while (m) {
      const int y = __builtin_ctz(m);
      m &= m - 1;
      lds.pt[(lane + 1) * S + (y + 1)] = label;
    }
    if (lane == 0) lds.libs[root] = (u16)nl;
    if (white) rem_w &= ~g; else rem_b &= ~g;
  }
  if (dead) {
    if (lane == 0 && ok) ok[row] = 0;
    return;
  }
  // the position as the current bitboards and as the one entry of the history ring
  u64 Bw = 0, Ww = 0;
#pragma unroll
  for (int k = 0; k < R; ++k) { set_lane64(Bw, k, bw[k]); set_lane64(Ww, k, ww[k]); }
  if (lane < R) { lds.hist[0][0][lane] = Bw; lds.hist[0][1][lane] = Ww; }
  bd.Bw = Bw; bd.Ww = Ww;
  bd.hash = hash;
  bd.next_player = player;
  bd.hist_cnt = 1;
  Board<N>::wsync();
  bd.store(&pool.slots[b]);
  if (lane == 0 && ok) ok[row] = 1;
}
