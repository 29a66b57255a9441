// Eye classes, two-eye life reading and the fast score: the reference's static life reading for every point of a position at once
// (k_life_map).  isEye / isSemiEye / isFakeEye / isTrueEye / getEyeColor (base/board.cc:1850-1922), getFastScore (:1924-1952),
// GivenGroupLives / OneGroupLives (:1108-1221), getBoardBBox / GuessLDAttacker (:1024-1106).  One wave64 = one board, as
// everywhere else; Board<N> is used through its public members only, and the slot is only read.
//   eyes:   bitboard algebra on the action-order words, for BOTH colours.  eye = empty and no neighbour that is empty or an enemy
//           stone -- no legality term (legal_moves<true> builds the mover's eyes from the legal points; isEye has no such term: a
//           point whose four neighbours are own stones is an eye even where playing it is suicide, or it is the ko point).
//           fake = an enemy stone on a diagonal of a first-line point, two on the diagonals elsewhere; it is answered at every
//           on-board point, stones included, as the reference function answers there.  semi = eye whose diagonals hold no enemy
//           stone (first line) / exactly one (elsewhere) and exactly one empty point that is not itself an eye of the colour; that
//           point is the move.  The four diagonal neighbours of a bitboard are formed as legal_moves forms them: (a-1 | a+1) packed
//           into one register, then -N / +N on both at once.
//   life:   GivenGroupLives is per GROUP: the candidates are the true eyes of the group's colour adjacent to THIS group, an
//           empty diagonal of a candidate counts as territory only if it is itself a candidate of this group (a true eye next to
//           another group of the colour does not), own stones on the diagonals count whatever their group.  Per lane over
//           (true eye, neighbour label) pairs: the lane of a true eye reads its four neighbour labels, its diagonals and -- for a
//           diagonal that is a true eye of the colour -- that point's four neighbour labels, and adds one to an LDS counter per
//           distinct neighbour group for which the eye qualifies (off_board >= 1 && off_board + territory == 4, or off_board == 0
//           && territory >= 3).  A group lives with two qualifying eyes and more than one liberty.  No loop over groups.
//   box:    the region of OneGroupLives / GuessLDAttacker; getBoardBBox of the position when the caller gives none.  The
//           attacker scan is one pass over the N steps of a line: lanes 0..31 take the rows of the box, lanes 32..63 its columns,
//           each remembers the first and the last stone of its line inside the box.
//   shared: the eye count of GivenGroupLives, the caller's box, the bounding box and the attacker scan are functions
//           (life_count_eyes, life_region_read, life_bbox, life_attacker_counts) that the kernels of region.cuh call too, beside
//           life_true_eyes for callers that want no more.
#pragma once
#include "go_board.cuh"
#include "engine_host.h"

#define LIFE_WAVE 64   // k_life_map: one board per workgroup
#define LIFE_SUMMARY_WORDS 12

// bit a of d1..d4 = bit of X at the diagonal neighbours (x-1,y-1), (x-1,y+1), (x+1,y-1), (x+1,y+1) of a = x*N + y (0 off the
// board); X lane-distributed (lanes 0..R-1), so are the results
template <int N>
__device__ __forceinline__ void life_diag4(const Board<N>& bd, u64 X, u64& d1, u64& d2, u64& d3, u64& d4) {
  const u64 pk = bd.sh_m1(X) | dpp_u64<0x118>(bd.sh_p1(X));   // lanes 0..R-1: from a-1; lanes 8..: from a+1
  const u64 m = bd.sh_mN(pk), p = bd.sh_pN(pk);
  d1 = m & bd.mValid; d3 = p & bd.mValid;
  d2 = dpp_u64<0x108>(m) & bd.mValid; d4 = dpp_u64<0x108>(p) & bd.mValid;
}
__device__ __forceinline__ u64 life_ge1(u64 a, u64 b, u64 c, u64 d) { return a | b | c | d; }
__device__ __forceinline__ u64 life_ge2(u64 a, u64 b, u64 c, u64 d) { return (a & b) | (c & d) | ((a | b) & (c | d)); }

// The true eyes of both colours (isTrueEye, board.cc:1850-1914) of the board's current stones: k_life_map's eye algebra without
// the fake / semi classes it also reports, for callers that only want GivenGroupLives (region.cuh).
template <int N>
__device__ __forceinline__ void life_true_eyes(const Board<N>& bd, u64& trueB, u64& trueW) {
  const u64 B = bd.Bw, W = bd.Ww;
  const u64 E = ~(B | W) & bd.mValid;
  u64 nearEW, nearEB;
  bd.dilate2(E | W, E | B, nearEW, nearEB);
  const u64 eyeB = E & ~nearEW, eyeW = E & ~nearEB;
  u64 w1, w2, w3, w4, b1, b2, b3, b4;
  life_diag4<N>(bd, W, w1, w2, w3, w4);
  life_diag4<N>(bd, B, b1, b2, b3, b4);
  const u64 edge = bd.mEdge, inner = bd.mValid & ~bd.mEdge;
  trueB = eyeB & ~((edge & life_ge1(w1, w2, w3, w4)) | (inner & life_ge2(w1, w2, w3, w4)));
  trueW = eyeW & ~((edge & life_ge1(b1, b2, b3, b4)) | (inner & life_ge2(b1, b2, b3, b4)));
}

// The caller's box: regions[row] = {left, top, right, bottom}, half-open, clamped into [0, N]; wave-uniform.  One statement of the
// rule for k_life_map and the region kernels (region.cuh).
template <int N>
__device__ __forceinline__ void life_region_read(const int32_t* regions, int row, int lane, int& left, int& top, int& right, int& bottom) {
  const int v = lane < 4 ? regions[(size_t)row * 4 + lane] : 0;
  const int c = v < 0 ? 0 : v > N ? N : v;
  left = rl(c, 0); top = rl(c, 1); right = rl(c, 2); bottom = rl(c, 3);
}

// The three functions below take the lane index as an argument, like Board::init: a kernel that calls them inside a loop
// (k_playout_ld) passes an opaque copy, which keeps their per-lane constants from being hoisted and held across the loop.
// getBoardBBox (:1024-1038) of the board's current stones; span[2] (LDS, this wave's) holds 0 on entry.
template <int N>
__device__ __forceinline__ void life_bbox(const Board<N>& bd, int lane, u32* span, int& left, int& top, int& right, int& bottom) {
  using G = Geo<N>;
  constexpr int R = G::R;
  const u64 occ = bd.Bw | bd.Ww;
  u32 xs = 0, ys = 0;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const u32 a = (u32)(k * 64 + lane);
    const u32 x = __umul24(a, (u32)G::DN_M) >> G::DN_S, y = a - __umul24(x, (u32)N);
    if (lane_bit(rl64(occ, k))) { xs |= 1u << x; ys |= 1u << y; }
  }
  if (xs) { atomicOr(&span[0], xs); atomicOr(&span[1], ys); }
  Board<N>::wsync();
  const u32 sx = (u32)rfl((int)span[0]), sy = (u32)rfl((int)span[1]);
  left = sx ? (int)__builtin_ctz(sx) : N; right = sx ? 32 - (int)__builtin_clz(sx) : 0;
  top = sy ? (int)__builtin_ctz(sy) : N; bottom = sy ? 32 - (int)__builtin_clz(sy) : 0;
}

// GivenGroupLives' eye count (:1108-1181), per (true eye, neighbour group): cnt[root] += 1 per qualifying eye of the group.
// cnt[G::PP] and te[G::PP] (LDS, this wave's) hold 0 on entry; te ends as 1 / 2 on the true eyes of Black / White.
template <int N>
__device__ __forceinline__ void life_count_eyes(const Board<N>& bd, int lane, u64 trueB, u64 trueW, u32* cnt, unsigned char* te) {
  using G = Geo<N>;
  constexpr int R = G::R, S = G::S;
  const Slot<N>* const L = bd.L;
  const u64 T = trueB | trueW;
  if (bal_ne64(T, 0ull)) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (lane_bit(rl64(trueB, k))) te[bd.idx[k]] = 1;
      if (lane_bit(rl64(trueW, k))) te[bd.idx[k]] = 2;
    }
    Board<N>::wsync();
#pragma unroll 1
    for (int k = 0; k < R; ++k) {
      const u64 tk = rl64(T, k);
      if (tk == 0) continue;
      if (lane_bit(tk)) {
        const u32 a = (u32)(k * 64 + lane);
        const int p = (int)(a + S + 1 + 2 * (__umul24(a, (u32)G::DN_M) >> G::DN_S));
        const u32 mine = te[p];                          // 1 / 2
        const u32 cb = mine == 2 ? 0x8000u : 0u;
        // the four neighbours are own stones or border (label 0x8000: root 0)
        const u32 g0 = L->pt[p - S], g1 = L->pt[p - 1], g2 = L->pt[p + S], g3 = L->pt[p + 1];
        int off = 0, own = 0;
        // the neighbour labels of a diagonal that is a true eye of the colour, else 0 (no stone carries label 0): two of its
        // neighbours are neighbours of this eye too (read above), the two on its far sides are read here
        u32 dn[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int sx = (q & 2) ? S : -S, sy = (q & 1) ? 1 : -1;
          const int dp = p + sx + sy;
          const u32 dv = L->pt[dp];
          dn[q][0] = dn[q][1] = dn[q][2] = dn[q][3] = 0;
          if (dv == PT_BORDER) off++;
          else if (dv == 0) {
            if (te[dp] == mine) { dn[q][0] = (q & 2) ? g2 : g0; dn[q][1] = (q & 1) ? g3 : g1; dn[q][2] = L->pt[dp + sx]; dn[q][3] = L->pt[dp + sy]; }
          } else if ((dv & 0x8000u) == cb) own++;
        }
        const u32 gs[4] = {g0, g1, g2, g3};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u32 g = gs[j];
          bool first = (g & 0x7FFFu) != 0;               // not the border
#pragma unroll
          for (int i = 0; i < j; ++i) first = first && gs[i] != g;   // an eye touched by several stones of the group counts once
          if (first) {
            int terr = own;
#pragma unroll
            for (int q = 0; q < 4; ++q) terr += (dn[q][0] == g || dn[q][1] == g || dn[q][2] == g || dn[q][3] == g) ? 1 : 0;
            const bool ok = off >= 1 ? (off + terr == 4) : (terr >= 3);
            if (ok) atomicAdd(&cnt[g & 0x7FFFu], 1u);
          }
        }
      }
    }
    Board<N>::wsync();
  }
}

// GuessLDAttacker's two counts (:1040-1106) over the box: lanes 0..31 the rows of the box (fixed y, x runs), lanes 32..63 its columns
template <int N>
__device__ __forceinline__ void life_attacker_counts(const Board<N>& bd, int lane, int left, int top, int right, int bottom, int& black, int& white) {
  constexpr int S = Geo<N>::S;
  const Slot<N>* const L = bd.L;
  black = 0; white = 0;
  const int t = lane & 31;
  const bool col = lane >= 32;
  const bool active = col ? (t >= left && t < right) : (t >= top && t < bottom);
  const int lo = col ? top : left, hi = col ? bottom : right;
  u32 first = 0, last = 0;
#pragma unroll   // the N reads are independent: all in flight before the first is consumed
  for (int s = 0; s < N; ++s) {
    const bool in = active && s >= lo && s < hi;
    const int x = col ? t : s, y = col ? s : t;
    const u32 v = L->pt[in ? (x + 1) * S + (y + 1) : 0];   // pt[0] is a border point
    const u32 c = (in && (v & 0x7FFFu) != 0) ? ((v & 0x8000u) ? (u32)S_WHITE : (u32)S_BLACK) : 0u;
    if (c) { if (!first) first = c; last = c; }
  }
  const u64 rows = 0xFFFFFFFFull, cols = ~rows;
  const u64 fB = bal_eq(first, (u32)S_BLACK), fW = bal_eq(first, (u32)S_WHITE), lB = bal_eq(last, (u32)S_BLACK), lW = bal_eq(last, (u32)S_WHITE);
  if (left > 0) { black += __popcll(fB & rows); white += __popcll(fW & rows); }
  if (top > 0) { black += __popcll(fB & cols); white += __popcll(fW & cols); }
  if (right < N) { black += __popcll(lB & rows); white += __popcll(lW & rows); }
  if (bottom < N) { black += __popcll(lB & cols); white += __popcll(lW & cols); }
}

// eye [n][NP] uint8: Black's answers in bits 0-3, White's in bits 4-7: 1 isEye, 2 isFakeEye, 4 isTrueEye, 8 isSemiEye.
// semi_move [n][2][NP] int16: the action of isSemiEye's *move where it returns true for that colour, else -1.
// alive [n][NP] uint8: 1 on every stone of a group for which GivenGroupLives holds.  summary [n][12] int32: see include/elf_amd.h.
// regions [n][4] int32 (may be null): left, top, right, bottom, half-open, clamped into [0, N] here.
// A row whose slot id lies outside the pool reads nothing: maps 0, semi_move -1, summary -1.
template <int N>
__global__ __launch_bounds__(LIFE_WAVE) void k_life_map(Pool<N> pool, int capacity, const int32_t* ids, int n, const int32_t* regions,
                                                         uint8_t* eye, int16_t* semi_move, uint8_t* alive, int32_t* summary) {
  using G = Geo<N>;
  constexpr int R = G::R, NP = G::NP;
  __shared__ Slot<N> lds;
  __shared__ u32 cnt[G::PP];             // per root: qualifying eyes (low half), bit 16 / 17: a living black / white stone of the group is in the box
  __shared__ unsigned char te[G::PP];    // per point (LDS index): 1 / 2 = true eye of Black / White
  __shared__ u32 span[2];                // bit x / bit y of every stone (getBoardBBox)
  const int row = blockIdx.x;
  const int b = rfl(ids ? ids[row] : row);
  const int lane = threadIdx.x;
  uint8_t* const erow = eye ? eye + (size_t)row * NP : nullptr;
  int16_t* const mrow = semi_move ? semi_move + (size_t)row * 2 * NP : nullptr;
  uint8_t* const arow = alive ? alive + (size_t)row * NP : nullptr;
  int32_t* const srow = summary ? summary + (size_t)row * LIFE_SUMMARY_WORDS : nullptr;
  if (b < 0 || b >= capacity) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int a = k * 64 + lane;
      if (a < NP) {
        if (erow) erow[a] = 0;
        if (mrow) { mrow[a] = (int16_t)-1; mrow[NP + a] = (int16_t)-1; }
        if (arow) arow[a] = 0;
      }
    }
    if (srow && lane < LIFE_SUMMARY_WORDS) srow[lane] = -1;
    return;
  }
  const bool need_life = arow || srow;
  for (int j = lane; j < G::PP; j += LIFE_WAVE) { cnt[j] = 0; te[j] = 0; }
  if (lane < 2) span[lane] = 0;
  Board<N> bd;
  bd.init(&lds, pool.zob, pool.skr(b));
  bd.load(&pool.slots[b]);   // its fence orders the zero fills before the counts below
  const Slot<N>* const L = bd.L;
  const u64 B = bd.Bw, W = bd.Ww;
  const u64 E = ~(B | W) & bd.mValid;

  // ---- eye classes of both colours (board.cc:1850-1914)
  u64 nearEW, nearEB;   // points with a neighbour that is empty or White / empty or Black
  bd.dilate2(E | W, E | B, nearEW, nearEB);
  const u64 eyeB = E & ~nearEW, eyeW = E & ~nearEB;
  u64 w1, w2, w3, w4, b1, b2, b3, b4;   // White / Black stones on the diagonals
  life_diag4<N>(bd, W, w1, w2, w3, w4);
  life_diag4<N>(bd, B, b1, b2, b3, b4);
  const u64 edge = bd.mEdge, inner = bd.mValid & ~bd.mEdge;
  const u64 fakeB = (edge & life_ge1(w1, w2, w3, w4)) | (inner & life_ge2(w1, w2, w3, w4));
  const u64 fakeW = (edge & life_ge1(b1, b2, b3, b4)) | (inner & life_ge2(b1, b2, b3, b4));
  const u64 trueB = eyeB & ~fakeB, trueW = eyeW & ~fakeW;
  // isSemiEye (:1863-1885): the empty diagonals that are not eyes of the colour
  u64 p1, p2, p3, p4, q1, q2, q3, q4;
  u64 semiB = 0, semiW = 0;
  if (erow || mrow) {
    life_diag4<N>(bd, E & ~eyeB, p1, p2, p3, p4);
    life_diag4<N>(bd, E & ~eyeW, q1, q2, q3, q4);
    const u64 oneP = life_ge1(p1, p2, p3, p4) & ~life_ge2(p1, p2, p3, p4), oneQ = life_ge1(q1, q2, q3, q4) & ~life_ge2(q1, q2, q3, q4);
    const u64 w_ge1 = life_ge1(w1, w2, w3, w4), b_ge1 = life_ge1(b1, b2, b3, b4);
    semiB = eyeB & oneP & ((edge & ~w_ge1) | (inner & w_ge1 & ~life_ge2(w1, w2, w3, w4)));
    semiW = eyeW & oneQ & ((edge & ~b_ge1) | (inner & b_ge1 & ~life_ge2(b1, b2, b3, b4)));
  } else {
    p1 = p2 = p3 = p4 = q1 = q2 = q3 = q4 = 0;
  }

  // ---- eye and semi_move rows
  if (erow) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int a = k * 64 + lane;
      u32 v = 0;
      v |= lane_bit(rl64(eyeB, k)) ? 1u : 0u;
      v |= lane_bit(rl64(fakeB, k)) ? 2u : 0u;
      v |= lane_bit(rl64(trueB, k)) ? 4u : 0u;
      v |= lane_bit(rl64(semiB, k)) ? 8u : 0u;
      v |= lane_bit(rl64(eyeW, k)) ? 16u : 0u;
      v |= lane_bit(rl64(fakeW, k)) ? 32u : 0u;
      v |= lane_bit(rl64(trueW, k)) ? 64u : 0u;
      v |= lane_bit(rl64(semiW, k)) ? 128u : 0u;
      if (a < NP) erow[a] = (uint8_t)v;
    }
  }
  if (mrow) {
    // where a point is a semi-eye exactly one of its four diagonal boards holds it
    const bool anyB = bal_ne64(semiB, 0ull) != 0, anyW = bal_ne64(semiW, 0ull) != 0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int a = k * 64 + lane;
      int mb = -1, mw = -1;
      if (anyB) {
        const int d = lane_bit(rl64(p1, k)) ? -N - 1 : lane_bit(rl64(p2, k)) ? -N + 1 : lane_bit(rl64(p3, k)) ? N - 1 : N + 1;
        if (lane_bit(rl64(semiB, k))) mb = a + d;
      }
      if (anyW) {
        const int d = lane_bit(rl64(q1, k)) ? -N - 1 : lane_bit(rl64(q2, k)) ? -N + 1 : lane_bit(rl64(q3, k)) ? N - 1 : N + 1;
        if (lane_bit(rl64(semiW, k))) mw = a + d;
      }
      if (a < NP) { mrow[a] = (int16_t)mb; mrow[NP + a] = (int16_t)mw; }
    }
  }
  if (!need_life) return;

  // ---- the box: the caller's, clamped, or getBoardBBox (:1024-1038)
  int left, top, right, bottom;
  if (regions) {
    life_region_read<N>(regions, row, lane, left, top, right, bottom);
  } else {
    life_bbox<N>(bd, lane, span, left, top, right, bottom);
  }

  // ---- GivenGroupLives (:1108-1181), per (true eye, neighbour group)
  life_count_eyes<N>(bd, lane, trueB, trueW, cnt, te);

  // ---- alive row, OneGroupLives over the box (:1198-1221), living groups in the box
  u64 aliveBox = 0;   // living stones inside the box
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const u32 a = (u32)(k * 64 + lane);
    const u32 v = L->pt[bd.idx[k]];
    const u32 root = v & 0x7FFFu;
    const bool stone = lane_bit(rl64(B | W, k));   // drops the clamped lanes of the last round
    const bool lives = stone && (cnt[root] & 0xFFFFu) >= 2u && L->libs[root] > 1;
    const int x = (int)(__umul24(a, (u32)G::DN_M) >> G::DN_S), y = (int)a - x * N;
    const bool inbox = x >= left && x < right && y >= top && y < bottom;
    if (arow && a < (u32)NP) arow[a] = lives ? 1 : 0;
    const u64 m = __ballot(lives && inbox);
    set_lane64(aliveBox, k, m);
    if (srow && lives && inbox) atomicOr(&cnt[root], (v & 0x8000u) ? 0x20000u : 0x10000u);
  }
  if (!srow) return;
  Board<N>::wsync();
  int livingB = 0, livingW = 0;
  for (int j0 = 0; j0 < G::PP; j0 += LIFE_WAVE) {
    const int j = j0 + lane;
    const u32 c = j < G::PP ? cnt[j] : 0u;
    livingB += __popcll(bal_ne(c & 0x10000u, 0u));
    livingW += __popcll(bal_ne(c & 0x20000u, 0u));
  }

  // ---- GuessLDAttacker (:1040-1106)
  int black, white;
  life_attacker_counts<N>(bd, lane, left, top, right, bottom, black, white);

  // ---- getFastScore (:1924-1952): getEyeColor asks White first; the two true-eye sets are disjoint anyway
  const int eb = bd.popc_lanes(trueB & ~trueW), ew = bd.popc_lanes(trueW);
  const int sb = bd.popc_lanes(B), sw = bd.popc_lanes(W);
  const int ab = bd.popc_lanes(aliveBox & B), aw = bd.popc_lanes(aliveBox & W);
  int out = 0;
  switch (lane) {
    case 0: out = eb + sb - ew - sw; break;                         // RULE_CHINESE
    case 1: out = eb - ew + bd.b_cap - bd.w_cap; break;             // RULE_JAPANESE: _rollout_passes is never written, 0
    case 2: out = ab > 0; break;
    case 3: out = aw > 0; break;
    case 4: out = left; break;
    case 5: out = top; break;
    case 6: out = right; break;
    case 7: out = bottom; break;
    case 8: out = black > white ? S_BLACK : S_WHITE; break;
    case 9: out = livingB; break;
    case 10: out = livingW; break;
    default: out = 0; break;
  }
  if (lane < LIFE_SUMMARY_WORDS) srow[lane] = out;
}
