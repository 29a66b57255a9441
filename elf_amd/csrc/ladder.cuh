// Ladder reading (k_ladder_map): for every point of a position, does the side to move extend a group out of atari there and
// still get captured in a ladder, and after how many plies.  The reference's checkLadder / checkLadderUseSearch
// (base/board.cc:299-439, :476-524), move for move.  One wave64 = one board, as everywhere else; Board<N> is used through its
// public members only.
//   prefilter: checkLadder's own test, for all points at once from the labels and liberties of the slot: the point is empty
//              and not the simple-ko point, exactly two of its neighbours are empty, and the other two are one enemy stone
//              whose group has >= 3 liberties and one own stone whose group has exactly 1.  (With two empty neighbours there
//              are only two stones to look at, so GroupId4's distinct-group bookkeeping and the "a second enemy / own group
//              clears the flag" quirk come to the same thing; two empty neighbours also rule out suicide, so this is TryPlay2's
//              verdict as well.)
//   search:    the recursion is a line of play that forks only where the capturer has two ways to atari and neither escape
//              point has three empty neighbours.  It is run as a loop over ONE working copy in LDS: the line's moves are kept
//              on a stack, a fork pushes its second alternative, and a failed line reloads the slot from the pool, replays the
//              stack up to the deepest open fork and plays the alternative there -- O(depth) per backtrack, no board
//              snapshots.  num_call counts the nodes entered (replays are not nodes); from MAX_LADDER_SEARCH on a fork plays
//              its first escape only.
//   play:      Board::forward is GoState::forward, the reference searches on a bare Board with TryPlay2 + Play: no super-ko
//              record or test, no termination test, no move limit.  The working copy therefore gets a super-ko policy that
//              records and finds nothing, and its private header is normalised: superko = 0, the last two moves M_INVALID
//              at the root (the search reads last moves only after it has played two of its own) and ply = 1 before every
//              play.  What is left of forward is exactly TryPlay2 (occupied, simple ko, suicide) + Play.
//   bounds:    every loop is counted.  A line longer than LADDER_STACK moves or a point that needs more than LADDER_MAX_PLAYS
//              plays (replays included) ends with calls = -1 and depth = 0 for that point, never in a spin.
#pragma once
#include "go_board.cuh"
#include "engine_host.h"

#define LADDER_WAVE 64

constexpr int LADDER_MAX_SEARCH = 1024;    // MAX_LADDER_SEARCH (board.cc:299)
constexpr int LADDER_STACK = 1024;         // moves of one line of play, the candidate move included
constexpr int LADDER_MAX_PLAYS = 32000;    // plays per searched point, replays included; num_call <= plays, so it fits int16

// forward's super-ko policy for a bare Board: nothing is recorded, nothing is ever found
struct LadderNoSK {
  __device__ __forceinline__ void record(int, u64, u64, u64, int) const {}
  __device__ __forceinline__ bool exact_hit(int, u64, u64, u64, int) const { return false; }
};

template <int N>
struct LadderStack {
  u16 mv[LADDER_STACK];      // the line of play as reference Coords; mv[0] is the candidate move
  u16 fork_at[LADDER_STACK]; // open forks, deepest last: index into mv of the move that has a second alternative ...
  u16 fork_mv[LADDER_STACK]; // ... and that alternative
  u32 cand[2 * Geo<N>::R];   // prefilter result: wave masks of the R rounds, low / high halves
};

// lanes 0..3: label of the neighbour of internal point i in FOR4 order (L, T, R, B = Board::dir4); other lanes: the border mark
template <int N>
__device__ __forceinline__ u32 ladder_nb(const Board<N>& bd, int i) {
  return bd.lane < 4 ? (u32)bd.L->pt[i + bd.dl4] : (u32)PT_BORDER;
}
template <int N>
__device__ __forceinline__ u32 ladder_empty4(const Board<N>& bd, int i) { return (u32)bal_eq(ladder_nb<N>(bd, i), 0u) & 0xFu; }
// reference Coord <-> internal index of an on-board point (Board::tr with the small-range division)
template <int N>
__device__ __forceinline__ int ladder_tr(int c) {
  const int q = Board<N>::div_s(c);
  return (c - q * Geo<N>::S) * Geo<N>::S + q;
}

// depth[i][a] = checkLadder(board, ids of a, next_player) where a = x*N + y is legal by TryPlay2, else 0;
// calls[i][a] (optional) = num_call after the search of a, 0 where none ran, -1 where a bound of this kernel cut it.
// The pool slot is only read.  A row whose slot id lies outside the pool reads nothing: depth 0, calls -1.
template <int N>
__global__ __launch_bounds__(LADDER_WAVE) void k_ladder_map(Pool<N> pool, int capacity, const int32_t* ids, int n, int16_t* depth,
                                                             int16_t* calls) {
  using G = Geo<N>;
  constexpr int R = G::R;
  __shared__ Slot<N> lds;
  __shared__ LadderStack<N> st;
  const int row = blockIdx.x;
  const int b = rfl(ids ? ids[row] : row);
  const int lane = threadIdx.x;
  int16_t* const drow = depth + (size_t)row * G::NP;
  int16_t* const crow = calls ? calls + (size_t)row * G::NP : nullptr;
  const bool bad = b < 0 || b >= capacity;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int a = k * 64 + lane;
    if (a < G::NP) {
      drow[a] = 0;
      if (crow) crow[a] = bad ? (int16_t)-1 : (int16_t)0;
    }
  }
  if (bad) return;
  const CBoard<N>* const src = reinterpret_cast<const CBoard<N>*>(&pool.slots[b]);
  Board<N> bd;
  bd.init(&lds, pool.zob, pool.skr(b));
  bd.load(&pool.slots[b]);
  const int vic = bd.next_player;   // the victim: the side to move of the position
  const u32 ownbit = vic == S_WHITE ? 0x8000u : 0u;
  const bool ko_live = bd.ko_pt != 0 && bd.ko_age == 0 && bd.ko_color == vic;
  // ---- prefilter, 64 points per round
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int a = k * 64 + lane, i = bd.idx[k];
    int nemp = 0, own1 = 0, en3 = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u32 v = lds.pt[i + Board<N>::dir4(q)];
      const u32 l = lds.libs[v & 0x7FFFu];
      nemp += v == 0;
      own1 += is_stone(v) && (v & 0x8000u) == ownbit && l == 1;
      en3 += is_stone(v) && (v & 0x8000u) != ownbit && l >= 3;
    }
    const bool pass = a < G::NP && lds.pt[i] == 0 && nemp == 2 && own1 == 1 && en3 == 1 && !(ko_live && a == bd.ko_a);
    const u64 m = __ballot(pass);
    if (lane == 0) { st.cand[2 * k] = (u32)m; st.cand[2 * k + 1] = (u32)(m >> 32); }
  }
  Board<N>::wsync();
  const LadderNoSK sk{};
  // ---- the searches, one candidate after the other
#pragma unroll 1
  for (int k = 0; k < R; ++k) {
    u64 cm = ((u64)(u32)rfl((int)st.cand[2 * k + 1]) << 32) | (u32)rfl((int)st.cand[2 * k]);
    while (cm) {   // at most 64 rounds: one bit leaves per round
      const int la = (int)__builtin_ctzll(cm);
      cm &= cm - 1;
      const int a = k * 64 + la;
      if (lane == 0) st.mv[0] = (u16)Board<N>::a2c_u(a);
      Board<N>::wsync();
      int len = 1;      // moves of the current line; mv[len - 1] has not been played yet
      int cnt = 0;      // moves of the line played on the working copy since the slot was loaded
      int nfork = 0;    // open forks
      int ncall = 0, plays = 0, result = 0;
      bool over = false, reload = true;
      for (;;) {
        if (plays >= LADDER_MAX_PLAYS) { over = true; break; }
        if (reload) {
          bd.load(src);
          bd.superko = 0; bd.lm0 = M_INVALID; bd.lm1 = M_INVALID; bd.sk_len = 0;
          cnt = 0; reload = false;
        }
        const int c = rfl((int)st.mv[cnt]);
        bd.ply = 1;
        const int ok = bd.forward(c, sk);
        ++plays;
        bool fail = false;
        if (cnt + 1 < len) {
          // a replay towards a fork: these moves were accepted on this very position before
          if (!ok) { over = true; break; }
          ++cnt;
          continue;
        }
        ++cnt;
        if (!ok) {
          fail = true;   // TryPlay2 refused: this alternative is skipped
        } else {
          const int ci = ladder_tr<N>(bd.lm0);
          const int lib = rfl((int)lds.libs[lds.pt[ci] & 0x7FFFu]);
          int next = 0, alt = 0;
          if (bd.next_player != vic) {
            // the victim has just moved.  After a flee (not after the candidate move itself) :416-431: free again with >= 3
            // liberties, or with 2 and an adjacent capturer's group in atari
            if (len > 1) {
              if (lib >= 3) fail = true;
              else if (lib == 2) {
                const u32 v = ladder_nb<N>(bd, ci);
                const u32 l = lds.libs[v & 0x7FFFu];
                if (__ballot(is_stone(v) && (v & 0x8000u) != ownbit && l == 1) != 0) fail = true;
              }
            }
            if (!fail) {
              // capturer's node :309-391
              ++ncall;
              if (lib == 1) { result = len; break; }
              const u32 em = ladder_empty4<N>(bd, ci);
              if (lib >= 3 || __popc(em) <= 1) fail = true;
              else {
                const int e0 = ci + Board<N>::dir4((int)__builtin_ctz(em));
                const int e1 = ci + Board<N>::dir4((int)__builtin_ctz(em & (em - 1)));
                int must = 0;
                if (__popc(ladder_empty4<N>(bd, e0)) == 3) must = e0;
                else if (__popc(ladder_empty4<N>(bd, e1)) == 3) must = e1;
                if (!must && ncall >= LADDER_MAX_SEARCH) must = e0;
                if (must) next = must;
                else { next = e0; alt = e1; }
              }
            }
          } else {
            // victim's node :393-436: the capturer has just moved
            ++ncall;
            if (lib == 1) fail = true;   // the capturer put himself in atari
            else {
              const int c2 = ladder_tr<N>(bd.lm1);
              const u32 em = ladder_empty4<N>(bd, c2);
              if (em == 0) fail = true;   // (the reference aborts here; a ladder position cannot reach it)
              else next = c2 + Board<N>::dir4((int)__builtin_ctz(em));
            }
          }
          if (!fail) {
            if (len >= LADDER_STACK) { over = true; break; }
            if (lane == 0) {
              st.mv[len] = (u16)ladder_tr<N>(next);
              if (alt) { st.fork_at[nfork] = (u16)len; st.fork_mv[nfork] = (u16)ladder_tr<N>(alt); }
            }
            if (alt) ++nfork;   // nfork <= len < LADDER_STACK
            ++len;
            Board<N>::wsync();
            continue;
          }
        }
        // this line failed: back to the deepest open fork, or the answer is 0
        if (nfork == 0) break;
        --nfork;
        const int m = rfl((int)st.fork_at[nfork]);
        const u32 fm = st.fork_mv[nfork];
        Board<N>::wsync();
        if (lane == 0) st.mv[m] = (u16)fm;
        Board<N>::wsync();
        len = m + 1;
        reload = true;
      }
      if (lane == la) {
        drow[a] = over ? (int16_t)0 : (int16_t)result;
        if (crow) crow[a] = over ? (int16_t)-1 : (int16_t)ncall;
      }
    }
  }
}

