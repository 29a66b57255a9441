// Per-point answers from the board engine: the Tromp-Taylor area map of a position (k_area_map) and Monte-Carlo ownership
// from device playouts (k_playout_own).  One wave64 = one board, as everywhere else; Board<N> is used through its public
// members only.
//   area:    simple_flood_fill per colour + the black && !white / white && !black rule of simple_tt_scoring
//            (base/go_state.h:32-93) -- Board::tt_area()'s fill, restated here because it must keep the rows it popcounts
//   playout: playout.cuh's harness (playout_pairs) under OwnTally and the kernel's Policy argument; with EyePolicy k_playout's game
#pragma once
#include "go_board.cuh"
#include "engine_host.h"
#include "playout.cuh"

// Area rows of the board's current stones: lane x < N ends with bit y of `ab` / `aw` set iff point a = x*N + y is black / white
// area; lanes >= N hold 0.  Row-bitboard flood fill in registers, both colours at once, to a fixed point.
template <int N>
__device__ __forceinline__ void area_rows(const Board<N>& bd, u32& ab, u32& aw) {
  constexpr int R = Geo<N>::R;
  const int lane = bd.lane;
  // re-slice the action-order bitboards into rows: row x = bits [x*N, x*N+N)
  const int bit0 = (lane < N ? lane : 0) * N, w = bit0 >> 6, s = bit0 & 63;
  u64 bl = 0, bh = 0, wl = 0, wh = 0;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const u64 bk = rl64(bd.Bw, k), wk = rl64(bd.Ww, k);
    if (w == k) { bl = bk; wl = wk; }
    if (w + 1 == k) { bh = bk; wh = wk; }
  }
  const u32 rowmask = (1u << N) - 1;
  u32 B = 0, Wt = 0;
  if (lane < N) {
    B = (u32)(s ? ((bl >> s) | (bh << (64 - s))) : bl) & rowmask;
    Wt = (u32)(s ? ((wl >> s) | (wh << (64 - s))) : wl) & rowmask;
  }
  const u32 E = (lane < N) ? (~(B | Wt) & rowmask) : 0u;
  u32 rb = B, rw = Wt;
  for (;;) {
    u32 ub = __shfl_up(rb, 1, 64), db = __shfl_down(rb, 1, 64);
    u32 uw = __shfl_up(rw, 1, 64), dw = __shfl_down(rw, 1, 64);
    if (lane == 0) { ub = 0; uw = 0; }
    if (lane >= N - 1) { db = 0; dw = 0; }
    u32 nb = rb | (E & ((rb << 1) | (rb >> 1) | ub | db));
    u32 nw = rw | (E & ((rw << 1) | (rw >> 1) | uw | dw));
    // finish the in-row run before the next vertical exchange
    for (int q = 0; q < 5; ++q) {
      nb |= E & ((nb << 1) | (nb >> 1));
      nw |= E & ((nw << 1) | (nw >> 1));
    }
    const bool ch = (nb != rb) || (nw != rw);
    rb = nb; rw = nw;
    if (!__any(ch)) break;
  }
  ab = rb & ~rw;
  aw = rw & ~rb;
}

// area(black) - area(white) of the rows above, wave-uniform
__device__ __forceinline__ int area_diff(u32 ab, u32 aw) {
  int d = __popc(ab) - __popc(aw);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
  return rfl(d);
}

// out[i][a] = 0 neutral, 1 black area, 2 white area; a = x*N + y.  The super-ko rule of GoState::evaluate plays no part.
template <int N>
__global__ __launch_bounds__(OWN_WAVE) void k_area_map(Pool<N> pool, const int32_t* ids, int n, uint8_t* out) {
  using G = Geo<N>;
  __shared__ Slot<N> lds;
  const int b = ids ? ids[blockIdx.x] : (int)blockIdx.x;
  Board<N> bd;
  bd.init(&lds, pool.zob, pool.skr(b));
  bd.load(&pool.slots[b]);
  u32 ab, aw;
  area_rows<N>(bd, ab, aw);
  if (bd.lane < N) {
    uint8_t* o = out + (size_t)blockIdx.x * G::NP + bd.lane * N;
    for (int y = 0; y < N; ++y) o[y] = (uint8_t)(((ab >> y) & 1u) | (((aw >> y) & 1u) << 1));
  }
}

// +1 into dst[0][a] for every black-area point of this lane's row and into dst[1][a] for every white-area one.  dst is the
// workgroup's LDS counters or a row of the global ones; integer adds, so the sums do not depend on who adds first.
template <int N>
__device__ __forceinline__ void own_add_rows(int* dst, u32 ab, u32 aw, int lane) {
  constexpr int NP = Geo<N>::NP;
  // one pass over the set bits (lanes >= N hold none); a loop, not N unrolled tests: the unrolled form's 2N addresses are
  // invariant in the caller's playout loop and would be kept in registers across it
  u32 m = ab | aw;
  while (m) {
    const int y = __builtin_ctz(m);
    m &= m - 1;
    atomicAdd(&dst[((ab >> y) & 1u ? 0 : NP) + lane * N + y], 1);
  }
}

// The ownership tally of playout_pairs (playout.cuh): pair (row, k) is played to the end with seed(row, k) under `pol` and its area
// rows are added into counts[row][2][N*N]; stats[row] = {sum of (black area - white area), playouts with (float)diff - komi > 0,
// playouts that ended on a super-ko repeat, steps played}.  acc[2][N*N]: the workgroup's LDS counters.
template <int N, class Policy>
struct OwnTally {
  using G = Geo<N>;
  int* acc;
  const u64* seeds; int max_steps; float komi; int32_t* counts; unsigned long long* stats; Policy pol;   // the kernel's arguments
  __device__ __forceinline__ void flush(int row) {
    int* g = counts + (size_t)row * 2 * G::NP;
    for (int j = threadIdx.x; j < 2 * G::NP; j += OWN_WAVE * OWN_WAVES) {
      const int v = acc[j];
      if (v) { atomicAdd(&g[j], v); acc[j] = 0; }
    }
  }
  __device__ __forceinline__ void play(Board<N>& bd, const GameSK<N>& sk, int row, int k, bool local, int wv, const u64* zlds, const u32* mlds) {
    const u32 key = playout_key(own_seed(seeds[row], k));
    bd.playout_begin(zlds);
    const int steps = playout_run<N>(bd, sk, key, max_steps, pol, mlds);
    u32 ab, aw;
    area_rows<N>(bd, ab, aw);
    const int diff = area_diff(ab, aw);
    if (local) own_add_rows<N>(acc, ab, aw, bd.lane);
    else own_add_rows<N>(counts + (size_t)row * 2 * G::NP, ab, aw, bd.lane);
    if (bd.lane == 0) {
      unsigned long long* st = stats + (size_t)row * 4;
      atomicAdd(&st[0], (unsigned long long)(long long)diff);
      if ((float)diff - komi > 0.0f) atomicAdd(&st[1], 1ull);
      if (bd.superko) atomicAdd(&st[2], 1ull);
      atomicAdd(&st[3], (unsigned long long)steps);
    }
  }
};

// Ownership (elfgo_own_run*): OwnTally over playout_pairs.  `pol` comes last so that the arguments before it are elfgo_own_run's.
template <int N, class Policy>
__global__ __launch_bounds__(OWN_WAVE * OWN_WAVES) void k_playout_own(Pool<N> pool, int capacity, u64* scratch, const int32_t* ids,
                                                                       const u64* seeds, int n, int K, int max_steps, float komi,
                                                                       int32_t* counts, unsigned long long* stats, Policy pol) {
  using G = Geo<N>;
  __shared__ Slot<N> lds_all[OWN_WAVES];
  __shared__ u64 zlds[G::P];
  __shared__ u32 mlds[G::NP + 2];
  __shared__ int acc[2 * G::NP];
  playout_tables<N, OWN_WAVE * OWN_WAVES>(pool.zob, zlds, mlds);
  for (int j = threadIdx.x; j < 2 * G::NP; j += OWN_WAVE * OWN_WAVES) acc[j] = 0;
  __syncthreads();
  OwnTally<N, Policy> t{acc, seeds, max_steps, komi, counts, stats, pol};
  playout_pairs<N>(pool, capacity, scratch, ids, n, K, lds_all, zlds, mlds, t);
}
