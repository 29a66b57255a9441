// The reference's Region functions and a Monte-Carlo life-and-death reader on top of them.
//   k_region_moves: FindAllCandidateMovesInRegion (base/board.cc:892-947), FindAllValidMovesInRegion (:970-1005) and
//                   GroupInRegion (:1183-1196) for every point of a position at once.  One wave64 = one board, as in k_candidates.
//   RegionCandPolicy: the playout policy "candidates inside the box" (playout.cuh's Policy): CandPolicy on cand & box.
//   k_playout_ld:   playout.cuh's harness (playout_pairs) with that policy; its tally (LdTally) judges every playout where it stops
//                   by OneGroupLives(defender, box) (:1198-1221) and by the stones left inside the box.
// The box is a lane-distributed bitboard built once per row (region_box); the lists are the whole-board lists ANDed with it, which
// keeps the reference's x-major order.  The life reading is life.cuh's (life_true_eyes, life_count_eyes, life_bbox,
// life_attacker_counts): one text for k_life_map and for the verdicts here.  Board<N> is used through its public members only.
#pragma once
#include "go_board.cuh"
#include "engine_host.h"
#include "playout.cuh"
#include "candidates.cuh"
#include "life.cuh"

#define REGION_WAVE 64   // k_region_moves: one board per workgroup
#define LD_INFO_WORDS 8
#define LD_STAT_WORDS 8

// bit a = x*N + y of the result (lane-distributed, lanes 0..R-1) is set iff left <= x < right and top <= y < bottom
template <int N>
__device__ __forceinline__ u64 region_box(const Board<N>& bd, int lane, int left, int top, int right, int bottom) {
  using G = Geo<N>;
  u64 box = 0;
#pragma unroll
  for (int k = 0; k < G::R; ++k) {
    const u32 a = (u32)(k * 64 + lane);
    const int x = (int)(__umul24(a, (u32)G::DN_M) >> G::DN_S), y = (int)a - x * N;
    set_lane64(box, k, __ballot(x >= left && x < right && y >= top && y < bottom));
  }
  return box & bd.mValid;
}

// cand[i][a] / valid[i][a] / groups[i][a], a = x*N + y: see include/elf_amd.h.  regions null = the whole board (the reference's
// nullptr).  The pool slot is only read.  A row whose slot id lies outside the pool reads nothing and gets zeros.
template <int N>
__global__ __launch_bounds__(REGION_WAVE) void k_region_moves(Pool<N> pool, int capacity, const int32_t* ids, int n, const int32_t* regions,
                                                               int thres, uint8_t* cand_out, uint8_t* valid_out, uint8_t* groups_out) {
  using G = Geo<N>;
  constexpr int R = G::R, NP = G::NP;
  __shared__ Slot<N> lds;
  __shared__ unsigned char inreg[G::PP];   // per root: a stone of the group lies in the box
  const int row = blockIdx.x;
  const int b = rfl(ids ? ids[row] : row);
  const int lane = threadIdx.x;
  uint8_t* const crow = cand_out ? cand_out + (size_t)row * NP : nullptr;
  uint8_t* const vrow = valid_out ? valid_out + (size_t)row * NP : nullptr;
  uint8_t* const grow = groups_out ? groups_out + (size_t)row * NP : nullptr;
  if (b < 0 || b >= capacity) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int a = k * 64 + lane;
      if (a < NP) {
        if (crow) crow[a] = 0;
        if (vrow) vrow[a] = 0;
        if (grow) grow[a] = 0;
      }
    }
    return;
  }
  for (int j = lane; j < G::PP; j += REGION_WAVE) inreg[j] = 0;
  Board<N> bd;
  bd.init(&lds, pool.zob, pool.skr(b));
  bd.load(&pool.slots[b]);   // its fence orders the zero fill of inreg before the flags below
  int left = 0, top = 0, right = N, bottom = N;
  if (regions) life_region_read<N>(regions, row, lane, left, top, right, bottom);
  const u64 box = region_box<N>(bd, lane, left, top, right, bottom);
  u64 keep = 0, legal = 0;
  if (crow || vrow) {
    u64 cand;
    bd.template legal_moves<true, true>(legal, cand);   // INCR: leaves the atari set in bd.at_cache
    legal &= box;
    keep = cand & box;
    // a threshold above N*N drops nothing (CandPolicy's shortcut)
    if (crow && thres <= NP && bal_ne64(keep, 0ull)) keep &= ~self_atari_drop<N, false>(bd, keep, thres, nullptr);
  }
  const u64 occ = bd.Bw | bd.Ww;
  u32 v[R] = {};
  if (grow) {
    // GroupInRegion: every stone inside the box raises its root's flag; a stone is reported when its root's flag is up
#pragma unroll
    for (int k = 0; k < R; ++k) {
      v[k] = bd.L->pt[bd.idx[k]];
      if (lane_bit(rl64(occ & box, k))) inreg[v[k] & 0x7FFFu] = 1;
    }
    Board<N>::wsync();
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int a = k * 64 + lane;
    const bool ck = lane_bit(rl64(keep, k)), lk = lane_bit(rl64(legal, k)), sk = lane_bit(rl64(occ, k));
    if (a < NP) {
      if (crow) crow[a] = ck ? 1 : 0;
      if (vrow) vrow[a] = lk ? 1 : 0;
      if (grow) grow[a] = (sk && inreg[v[k] & 0x7FFFu]) ? 1 : 0;
    }
  }
}

// The region policy of the playouts: FindAllCandidateMovesInRegion's list.  The box belongs to a row, so the tally builds the
// object per (row, playout); with the whole-board box it is CandPolicy's game.
struct RegionCandPolicy {
  int thres;
  u64 box;   // lane-distributed (region_box)
  template <int N>
  __device__ __forceinline__ u64 keep(const Board<N>& bd, u64 cand) const { return CandPolicy{thres}.template keep<N>(bd, cand & box); }
};

// A copy of the lane index the compiler cannot see through: what is computed from it stays where it is written.  The life reading
// and the box are per-lane arithmetic on constants; hoisted out of k_playout_ld's loops they would sit in ~70 VGPRs across the
// playout.
__device__ __forceinline__ int ld_opaque(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

// OneGroupLives(colour, box) (:1198-1221) of the board's current stones: a stone of the colour inside the box whose group has two
// qualifying eyes and more than one liberty.  cnt[G::PP] / te[G::PP]: this wave's LDS scratch, any contents on entry.
template <int N>
__device__ __forceinline__ bool ld_one_group_lives(const Board<N>& bd, u64 box, int colour, u32* cnt, unsigned char* te) {
  using G = Geo<N>;
  constexpr int R = G::R;
  const u64 C = (colour == S_BLACK ? bd.Bw : bd.Ww) & box;
  if (!bal_ne64(C, 0ull)) return false;
  const int lane = ld_opaque(bd.lane);
  for (int j = lane; j < G::PP; j += 64) { cnt[j] = 0; te[j] = 0; }
  Board<N>::wsync();
  u64 trueB, trueW;
  life_true_eyes<N>(bd, trueB, trueW);
  life_count_eyes<N>(bd, lane, trueB, trueW, cnt, te);
  bool any = false;
#pragma unroll   // bd.idx[k] must be a register: a run-time k would put the whole Board object on the stack
  for (int k = 0; k < R; ++k) {
    const u64 ck = rl64(C, k);
    if (ck == 0) continue;
    const u32 root = bd.L->pt[bd.idx[k]] & 0x7FFFu;
    const bool lives = lane_bit(ck) && cnt[root] >= 2u && bd.L->libs[root] > 1;
    any = any || __ballot(lives) != 0;
  }
  return any;
}

// The life-and-death tally of playout_pairs (playout.cuh): pair (row, k) is played with seed(row, k) from the list of
// FindAllCandidateMovesInRegion(board, box, next_player, thres) until the game terminates or max_steps moves are made, and judged
// where it stands.  info / stats / first: see include/elf_amd.h.
//  * The box, the attacker and the source position's verdict are worked out by every wave from its fresh copy of the slot (they
//    cost a fraction of one playout move each); playout 0 of a row writes them to info.
template <int N>
struct LdTally {
  using G = Geo<N>;
  static constexpr int NA = G::NA, FW = 3 * NA;
  int* facc; unsigned long long* sacc;                                          // the workgroup's LDS counters for first / stats
  u32 (*cnt_all)[G::PP]; unsigned char (*te_all)[G::PP]; u32 (*span_all)[2];   // per-wave LDS scratch of the life reading
  const u64* seeds; int max_steps, thres; const int32_t* regions; const uint8_t* attackers;   // the kernel's arguments
  int32_t* info; unsigned long long* stats; int32_t* first;
  __device__ __forceinline__ void flush(int row) {
    int* g = first + (size_t)row * FW;
    for (int j = threadIdx.x; j < FW; j += OWN_WAVE * OWN_WAVES) {
      const int v = facc[j];
      if (v) { atomicAdd(&g[j], v); facc[j] = 0; }
    }
    if (threadIdx.x < LD_STAT_WORDS) {
      const unsigned long long v = sacc[threadIdx.x];
      if (v) { atomicAdd(&stats[(size_t)row * LD_STAT_WORDS + threadIdx.x], v); sacc[threadIdx.x] = 0ull; }
    }
  }
  __device__ __forceinline__ void play(Board<N>& bd, const GameSK<N>& sk, int row, int k, bool local, int wv, const u64* zlds, const u32* mlds) {
    u32* const span = span_all[wv];
    // ---- the problem: box, attacker, defender, the source position's verdict
    const int ol = ld_opaque(bd.lane);
    int left, top, right, bottom;
    if (regions) {
      life_region_read<N>(regions, row, ol, left, top, right, bottom);
    } else {
      if (ol < 2) span[ol] = 0;
      Board<N>::wsync();
      life_bbox<N>(bd, ol, span, left, top, right, bottom);
    }
    const u64 box = region_box<N>(bd, ol, left, top, right, bottom);
    int att = attackers ? rfl((int)attackers[row]) : 0;
    if (att != S_BLACK && att != S_WHITE) {
      int black, white;
      life_attacker_counts<N>(bd, ol, left, top, right, bottom, black, white);
      att = rfl(black > white ? S_BLACK : S_WHITE);
    }
    const int def = S_BLACK + S_WHITE - att;
    // ---- phase 0 (playout 0 of a row only): the source position's verdict goes to info; phase 1: the playout and its verdict.
    // One loop, so that the life reading is one call site.
    int steps = 0, first_c = 0, lived = 0;
#pragma unroll 1
    for (int phase = k == 0 ? 0 : 1; phase < 2; ++phase) {
      if (phase == 1) {
        // playout_run in two parts, so that the first move can be read off the board: one move, then the rest.  A loop and
        // not two calls: the step is inlined once.
        const u32 key = playout_key(own_seed(seeds[row], k));
        const RegionCandPolicy pol{thres, box};
        bd.playout_begin(zlds);
#pragma unroll 1
        for (int part = 0; part < 2; ++part) {
          const int limit = part == 0 ? (max_steps < 1 ? max_steps : 1) : max_steps - steps;
          const int made = playout_run<N>(bd, sk, key, limit, pol, mlds);
          if (part == 0) {
            if (made == 0) break;
            first_c = bd.lm0;
          }
          steps += made;
        }
      }
      lived = ld_one_group_lives<N>(bd, box, def, cnt_all[wv], te_all[wv]) ? 1 : 0;
      if (phase == 0) {
        int w = 0;
        switch (bd.lane) {
          case 0: w = left; break;
          case 1: w = top; break;
          case 2: w = right; break;
          case 3: w = bottom; break;
          case 4: w = att; break;
          case 5: w = def; break;
          case 6: w = bd.next_player; break;
          default: w = lived; break;
        }
        if (bd.lane < LD_INFO_WORDS) info[(size_t)row * LD_INFO_WORDS + bd.lane] = w;
      }
    }
    // ---- the counters
    const u64 D = (def == S_BLACK ? bd.Bw : bd.Ww) & box, A = (def == S_BLACK ? bd.Ww : bd.Bw) & box;
    const int nd = bd.popc_lanes(D), na = bd.popc_lanes(A);
    const int survived = nd > 0 ? 1 : 0;
    if (bd.lane == 0) {
      unsigned long long* st = local ? sacc : stats + (size_t)row * LD_STAT_WORDS;
      if (lived) atomicAdd(&st[0], 1ull);
      if (survived) atomicAdd(&st[1], 1ull);
      if (nd) atomicAdd(&st[2], (unsigned long long)nd);
      if (na) atomicAdd(&st[3], (unsigned long long)na);
      if (bd.superko) atomicAdd(&st[4], 1ull);
      if (steps) atomicAdd(&st[5], (unsigned long long)steps);
      atomicAdd(&st[6], (unsigned long long)bd.hash);
      if (steps > 0) {
        const int fa = first_c == M_PASS ? G::NP : Board<N>::c2a_u(first_c);
        int* f = local ? facc : first + (size_t)row * FW;
        atomicAdd(&f[fa], 1);
        if (lived) atomicAdd(&f[NA + fa], 1);
        if (survived) atomicAdd(&f[2 * NA + fa], 1);
      }
    }
  }
};

// Life-and-death reading by region playouts (elfgo_ld_run): LdTally over playout_pairs, on the record areas of the ElfGoOwnership
// handle.  A row whose slot id lies outside the pool is not played: its outputs stay zero.
template <int N>
__global__ __launch_bounds__(OWN_WAVE * OWN_WAVES) void k_playout_ld(Pool<N> pool, int capacity, u64* scratch, const int32_t* ids,
                                                                      const u64* seeds, int n, int K, int max_steps, int thres,
                                                                      const int32_t* regions, const uint8_t* attackers, int32_t* info,
                                                                      unsigned long long* stats, int32_t* first) {
  using G = Geo<N>;
  constexpr int FW = LdTally<N>::FW;
  __shared__ Slot<N> lds_all[OWN_WAVES];
  __shared__ u64 zlds[G::P];
  __shared__ u32 mlds[G::NP + 2];
  __shared__ int facc[FW];
  __shared__ unsigned long long sacc[LD_STAT_WORDS];
  __shared__ u32 cnt_all[OWN_WAVES][G::PP];
  __shared__ unsigned char te_all[OWN_WAVES][G::PP];
  __shared__ u32 span_all[OWN_WAVES][2];
  playout_tables<N, OWN_WAVE * OWN_WAVES>(pool.zob, zlds, mlds);
  for (int j = threadIdx.x; j < FW; j += OWN_WAVE * OWN_WAVES) facc[j] = 0;
  if (threadIdx.x < LD_STAT_WORDS) sacc[threadIdx.x] = 0ull;
  __syncthreads();
  LdTally<N> t{facc, sacc, cnt_all, te_all, span_all, seeds, max_steps, thres, regions, attackers, info, stats, first};
  playout_pairs<N>(pool, capacity, scratch, ids, n, K, lds_all, zlds, mlds, t);
}
