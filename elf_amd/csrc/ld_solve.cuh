// Exact life-and-death search over a box (k_ld_solve): the minimax value of every first move of a position, by tree search on
// the device.  The problem is k_playout_ld's (region.cuh: ld_frame -- box, attacker, defender), the moves of a node are
// FindAllCandidateMovesInRegion's list (RegionCandPolicy), the static verdict is OneGroupLives(defender, box)
// (ld_one_group_lives) and the stones left inside the box; what is new here is the search.  include/elf_amd.h states the
// semantics (elfgo_ld_solve); this file is how they are computed.
//   split:    one wave64 = one (row, root move), one wave per workgroup.  The grid is root-list capacity (N*N) x rows; every
//             wave loads the slot and works out the problem and the root's list for itself (the k_region_moves body: a fraction
//             of one node), takes the m-th move of that list and leaves if there is none.  No second launch, no device-side
//             count, no atomics: a wave owns value[row][its move] and nodes[row][its move]; wave 0 of a row also writes info and
//             the cells of the points that are no root move.  A handful of rows fills the chip, and a first move's answer does
//             not depend on what another wave does.
//   search:   depth-first alpha-beta on the values 0 / 1 / 2, started with the full window [0, 2] below the first move, so the
//             value of the first move is exact; inner nodes return bounds.  A defender node stops at a child worth 2 (>= beta
//             in the full window), an attacker node at a child worth 0.  The whole wave walks one line: every decision is
//             wave-uniform (SGPRs), the loop is a two-state machine -- "enter the node the working copy stands on" / "a child
//             returned a value to the node at depth d" -- and each turn plays at most one move, so Board::forward, the
//             candidate list and the life reading are one call site each (the root is depth 0 of the same loop).
//   undo:     LDS snapshots, not replay.  A node that gets children stores its compact board (CBoard: the slot without its Bloom
//             words, 2624 B at 19x19 -- no super-ko is kept, so the filter is dead weight) on a stack beside the working Slot,
//             16 B per lane; coming back for the next child copies it down again (Board::store / Board::load on LDS pointers).
//             That is 3 (19x19) or 1 (9x9) vector stores per lane against one forward per ply of the line: the ladder reader's
//             replay from the root is right for its long unforked lines (a backtrack is rare, a snapshot per ply would be paid
//             on every move), and wrong here, where every node forks and a replay would cost depth forwards per child.
//             The stack is dynamic LDS sized by the call's max_depth: max_depth - 1 entries, since a node at max_depth is a
//             leaf and the root is re-read from the pool by nobody (its waves never come back to it).
//   state:    per open node one word (running best, alpha, beta, who moves, passes in a row, "the only move is a pass")
//             and its remaining-move bitboard (R words) in an LDS table; the next move is the lowest set bit, i.e. ascending
//             action order.
//   play:     ladder.cuh's bare Board: forward under LadderNoSK with superko = 0, ply = 1 before every move, and the last two
//             moves M_INVALID at the root -- TryPlay2 + Play, simple ko included, nothing else.
//   bounds:   every loop is counted.  Nodes entered per first move <= max_nodes; a turn of the loop enters a node or returns
//             from one, so 2 * max_nodes + 4 turns is the loop's own limit; depth <= max_depth <= LD_SOLVE_MAX_DEPTH; moves per
//             node <= N*N + 1 (a bit leaves the bitboard per child).  A bound that trips, or a move of a list that forward
//             refuses (never expected), writes -2 for that first move and ends the wave.
#pragma once
#include "go_board.cuh"
#include "engine_host.h"
#include "ladder.cuh"
#include "region.cuh"

#define LD_SOLVE_WAVE 64
// max_depth of a call.  The stack of a 19x19 call at this depth is 21 compact boards = 55 104 B; with the working Slot, the life
// reading's scratch and the table below that is 62.4 KB of LDS, inside the 64 KB a workgroup gets without asking for more.
constexpr int LD_SOLVE_MAX_DEPTH = 22;

enum { LD_V_DEAD = 0, LD_V_UNSETTLED = 1, LD_V_ALIVE = 2, LD_V_NOT_A_MOVE = -1, LD_V_CUT = -2 };

template <int N>
struct LdSolveTable {
  u64 rem[LD_SOLVE_MAX_DEPTH][Geo<N>::R];   // moves of the open node at depth d that have not been played yet
  u32 word[LD_SOLVE_MAX_DEPTH];             // ld_solve_pack
};
// best is -1 .. 3 (the two ends: no child yet of a defender / an attacker node)
__device__ __forceinline__ u32 ld_solve_pack(int best, int alpha, int beta, int dm, int pc, int only_pass) {
  return (u32)(best + 1) | ((u32)alpha << 4) | ((u32)beta << 8) | ((u32)dm << 12) | ((u32)pc << 13) | ((u32)only_pass << 15);
}

// the snapshot stack of a call: a node at max_depth is a leaf, so depths 1 .. max_depth - 1 can be open
template <int N>
constexpr size_t ld_solve_stack_bytes(int max_depth) { return max_depth > 1 ? (size_t)(max_depth - 1) * sizeof(CBoard<N>) : 0; }
static_assert(ld_solve_stack_bytes<19>(LD_SOLVE_MAX_DEPTH) + sizeof(Slot<19>) + sizeof(LdSolveTable<19>) + 5 * Geo<19>::PP + 8 <= 65536,
              "a 19x19 workgroup at LD_SOLVE_MAX_DEPTH stays inside 64 KB of LDS");

// value / nodes / info: see include/elf_amd.h.  blockIdx.x = index into the root's list, blockIdx.y = row - row0.  The pool slot
// is only read.
template <int N>
__global__ __launch_bounds__(LD_SOLVE_WAVE) void k_ld_solve(Pool<N> pool, int capacity, const int32_t* ids, int row0, const int32_t* regions,
                                                             const uint8_t* attackers, int max_depth, int max_nodes, int thres,
                                                             int32_t* info, int8_t* value, int32_t* nodes) {
  using G = Geo<N>;
  constexpr int R = G::R, NP = G::NP, NA = G::NA;
  extern __shared__ uint4 ld_solve_stack[];   // ld_solve_stack_bytes<N>(max_depth)
  CBoard<N>* const stack = reinterpret_cast<CBoard<N>*>(ld_solve_stack);
  __shared__ Slot<N> lds;
  __shared__ LdSolveTable<N> tb;
  __shared__ u32 cnt[G::PP];
  __shared__ unsigned char te[G::PP];
  __shared__ u32 span[2];
  const int row = row0 + (int)blockIdx.y;
  const int m = (int)blockIdx.x;
  const int b = rfl(ids ? ids[row] : row);
  const int lane = threadIdx.x;
  int8_t* const vrow = value + (size_t)row * NA;
  int32_t* const nrow = nodes ? nodes + (size_t)row * NA : nullptr;
  int32_t* const irow = info ? info + (size_t)row * LD_INFO_WORDS : nullptr;
  if (b < 0 || b >= capacity) {
    if (m == 0) {
      for (int j = lane; j < NA; j += LD_SOLVE_WAVE) { vrow[j] = (int8_t)LD_V_NOT_A_MOVE; if (nrow) nrow[j] = 0; }
      if (irow && lane < LD_INFO_WORDS) irow[lane] = 0;
    }
    return;
  }
  Board<N> bd;
  bd.init(&lds, pool.zob, pool.skr(b));
  bd.load(&pool.slots[b]);
  bd.superko = 0; bd.lm0 = M_INVALID; bd.lm1 = M_INVALID; bd.sk_len = 0;
  int left, top, right, bottom, att;
  const u64 box = ld_frame<N>(bd, lane, row, regions, attackers, span, left, top, right, bottom, att);
  const int def = S_BLACK + S_WHITE - att;
  const LadderNoSK sk{};
  const RegionCandPolicy pol{thres, box};

  int d = 0;                             // depth of the node the turn is about
  int ret = -1;                          // >= 0: the value a child returns to the node at depth d; -1: the node at depth d is entered
  int a_in = LD_V_DEAD, b_in = LD_V_ALIVE, pc_in = 0;   // window and passes in a row of the node that is entered
  int count = 0, result = LD_V_CUT, first_a = 0;
  const u64 turns = 2ull * (u64)max_nodes + 4ull;
#pragma unroll 1
  for (u64 turn = 0; turn < turns; ++turn) {
    int best = 0, alpha, beta, dm = 0, pc, only_pass, a = NP;
    u64 rem;
    if (ret < 0) {
      // ---- enter the node the working copy stands on
      if (d > 0) {
        if (count >= max_nodes) break;
        ++count;
      }
      const int v = ld_one_group_lives<N>(bd, box, def, cnt, te) ? LD_V_ALIVE
                    : bal_ne64((def == S_BLACK ? bd.Bw : bd.Ww) & box, 0ull) ? LD_V_UNSETTLED : LD_V_DEAD;
      const bool leaf = v != LD_V_UNSETTLED || d >= max_depth || pc_in >= 2;
      if (d == 0 && m == 0) {
        int w = 0;
        switch (lane) {
          case 0: w = left; break;
          case 1: w = top; break;
          case 2: w = right; break;
          case 3: w = bottom; break;
          case 4: w = att; break;
          case 5: w = def; break;
          case 6: w = bd.next_player; break;
          default: w = v; break;
        }
        if (irow && lane < LD_INFO_WORDS) irow[lane] = w;
        if (leaf) {
          for (int j = lane; j < NA; j += LD_SOLVE_WAVE) { vrow[j] = (int8_t)LD_V_NOT_A_MOVE; if (nrow) nrow[j] = 0; }
        }
      }
      if (leaf) {
        if (d == 0) return;   // a terminal root: nothing is searched
        ret = v; --d;
        continue;
      }
      u64 legal, cand;
      bd.at_dirty = 1;   // the general forward does not keep the atari set
      bd.template legal_moves<true, true>(legal, cand);   // INCR: leaves the atari set in bd.at_cache
      rem = pol.template keep<N>(bd, cand);
      only_pass = bal_ne64(rem, 0ull) ? 0 : 1;
      if (d == 0) {
        // the root: this wave's first move is the m-th of the list; wave 0 fills the cells of the points that are no root move
        if (m == 0) {
#pragma unroll
          for (int k = 0; k < R; ++k) {
            const int j = k * 64 + lane;
            if (j < NP && !lane_bit(rl64(rem, k))) { vrow[j] = (int8_t)LD_V_NOT_A_MOVE; if (nrow) nrow[j] = 0; }
          }
          if (!only_pass && lane == 0) { vrow[NP] = (int8_t)LD_V_NOT_A_MOVE; if (nrow) nrow[NP] = 0; }
        }
        a = NP;
        int skip = m;
        if (only_pass) {
          if (m > 0) return;
        } else {
#pragma unroll 1
          for (int k = 0; k < R && a == NP; ++k) {
            u64 wk = rl64(rem, k);
            const int c = __popcll(wk);
            if (skip < c) {
              for (int j = 0; j < skip; ++j) wk &= wk - 1;   // skip < 64
              a = k * 64 + (int)__builtin_ctzll(wk);
            }
            skip -= c;
          }
          if (a == NP) return;   // the list is shorter than m + 1
        }
        first_a = a;
        alpha = LD_V_DEAD; beta = LD_V_ALIVE; pc = 0;
      } else {
        dm = bd.next_player == def ? 1 : 0;
        best = dm ? -1 : 3;
        alpha = a_in; beta = b_in; pc = pc_in;
        bd.store(&stack[d - 1]);   // d < max_depth: the stack has max_depth - 1 entries
      }
    } else {
      // ---- a child returned `ret` to the node at depth d
      if (d == 0) { result = ret; break; }
      const u32 w = (u32)rfl((int)tb.word[d]);
      best = (int)(w & 15u) - 1; alpha = (int)((w >> 4) & 15u); beta = (int)((w >> 8) & 15u);
      dm = (int)((w >> 12) & 1u); pc = (int)((w >> 13) & 3u); only_pass = (int)((w >> 15) & 1u);
      rem = lane < R ? tb.rem[d][lane] : 0ull;
      bool done;
      if (dm) {
        best = ret > best ? ret : best;
        done = best >= LD_V_ALIVE || best >= beta;
        alpha = best > alpha ? best : alpha;
      } else {
        best = ret < best ? ret : best;
        done = best <= LD_V_DEAD || best <= alpha;
        beta = best < beta ? best : beta;
      }
      if (done || !(bal_ne64(rem, 0ull) || only_pass)) {
        ret = best; --d;
        continue;
      }
      bd.load(&stack[d - 1]);
      ret = -1;
    }
    // ---- the next move of the node at depth d: the lowest remaining action, or the pass of an empty list
    if (d > 0) {
      a = NP;
      if (only_pass) {
        only_pass = 0;
      } else {
#pragma unroll 1
        for (int k = 0; k < R && a == NP; ++k) {
          const u64 wk = rl64(rem, k);
          if (wk) {
            a = k * 64 + (int)__builtin_ctzll(wk);
            if (lane == k) rem &= rem - 1;
          }
        }
      }
      Board<N>::wsync();
      if (lane < R) tb.rem[d][lane] = rem;
      if (lane == 0) tb.word[d] = ld_solve_pack(best, alpha, beta, dm, pc, only_pass);
      Board<N>::wsync();
    }
    bd.ply = 1;
    if (!bd.forward(a == NP ? (int)M_PASS : Board<N>::a2c_u(a), sk)) break;   // a move of the list is legal: never expected
    a_in = alpha; b_in = beta; pc_in = a == NP ? pc + 1 : 0;
    ++d;
  }
  if (lane == 0) {
    vrow[first_a] = (int8_t)result;
    if (nrow) nrow[first_a] = count;
  }
}
