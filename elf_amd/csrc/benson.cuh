// Benson's unconditional life (k_pass_alive): the chains of a colour that cannot be captured even if their owner passes for ever,
// and the regions those chains enclose.  For a colour X: the chains are the groups pt[] labels; the regions are the 4-connected
// components of the points without an X stone (empty points and opponent stones); a region is VITAL to a chain if it has an empty
// point and every empty point of it is adjacent to a stone of the chain.  Repeat until nothing changes: remove every chain with
// fewer than two surviving vital regions, then every region that borders a removed chain.  What survives is pass-alive; a
// surviving region that is vital to a surviving chain is safe (its opponent stones are unconditionally dead).
// One wave64 = one board, as everywhere else; Board<N> is used through its public members only, and the slot is only read.  Both
// colours are read in one launch, one after the other, over the same tables in LDS beside the slot -- no global scratch:
//   lab[PP]  u32, per point (LDS index): the region label of a point without an X stone, else NONE.  A label is the LDS index of a
//            point of the region, so region ids and chain roots (indices of X stones) never collide and every table below is
//            indexed by point.
//   aux[PP]  u32: first the smallest empty point of each region (at the region's label), then, in the removal rounds, the number
//            of surviving vital regions of each chain (at the chain's root).
//   cand[PP][4] u16, per region label: the chains the region is vital to (roots, 0 = none).
//   live[PP] u8, per region label: 1 while the region survives.
//   labels:  all components at once by min-label propagation with hooking.  An empty point starts with its own index, an opponent
//            stone with its chain's root -- opponent chains are already connected through pt[].  A pass: every lane takes, for each
//            of its points, the minimum m of its label and its four neighbours' labels, follows it once (m = lab[m], the pointer
//            jump) and, if that is smaller than its label cur, lowers both lab[point] and lab[cur] to it (ds_min_u32): lowering
//            the old label's own entry drags everything that pointed there along at its next jump.  Labels only fall and never
//            leave their component, every label v keeps lab[v] <= v, and a pass without a change is a fixed point at which a
//            component shares one label; it is never slower than plain propagation, so N*N passes bound it (a handful in practice).
//   vital:   a chain to which R is vital touches R's smallest empty point, so the <= 4 distinct chains next to that point are the
//            only candidates; every other empty point of R clears the candidates it does not touch.  Lane-parallel over points.
//   rounds:  recount aux over region labels (one ds_add per candidate), then every point of a surviving region that touches a
//            stone of a chain with aux < 2 clears its region's live byte.  A round that changes something removes a chain, so
//            chains + 1 rounds bound the loop.
// If a bound is hit (never expected) the colour's rounds word carries BENSON_BOUND_HIT, its other answers are 0 and the kernel
// goes on to the next colour.
#pragma once
#include "go_board.cuh"
#include "engine_host.h"

#define BENSON_WAVE 64   // k_pass_alive: one board per workgroup
#define BENSON_SUMMARY_WORDS 8
#define BENSON_BOUND_HIT 0x80000000u
#define BENSON_NONE 0xFFFFu   // lab[] of X stones and border points, aux[] of a region without an empty point: above every index

// the roots of the X chains on the four neighbours of point p (LDS index), 0 where the neighbour is no X stone
template <int N>
__device__ __forceinline__ void benson_roots4(const Slot<N>* L, int p, u32 xb, u32 (&r)[4]) {
  constexpr int S = Geo<N>::S;
  const u32 g[4] = {L->pt[p - S], L->pt[p - 1], L->pt[p + S], L->pt[p + 1]};
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = (is_stone(g[j]) && (g[j] & 0x8000u) == xb) ? (g[j] & 0x7FFFu) : 0u;
}

// map [n][NP] uint8: bit 0 / 1 a Black / White stone of a pass-alive chain, bit 2 / 3 a safe point of Black / White.
// summary [n][8] int32: per colour, Black first: pass-alive chains, pass-alive stones, safe points, removal rounds run (top bit:
// a loop bound was hit).  A row whose slot id lies outside the pool reads nothing: map 0, summary -1.
template <int N>
__global__ __launch_bounds__(BENSON_WAVE) void k_pass_alive(Pool<N> pool, int capacity, const int32_t* ids, int n, uint8_t* map, int32_t* summary) {
  using G = Geo<N>;
  constexpr int R = G::R, NP = G::NP, S = G::S, PP = G::PP;
  __shared__ Slot<N> lds;
  __shared__ u32 lab[PP];
  __shared__ u32 aux[PP];
  __shared__ __attribute__((aligned(8))) u16 cand[PP * 4];
  __shared__ unsigned char live[PP];
  const int row = blockIdx.x;
  const int b = rfl(ids ? ids[row] : row);
  const int lane = threadIdx.x;
  uint8_t* const mrow = map ? map + (size_t)row * NP : nullptr;
  int32_t* const srow = summary ? summary + (size_t)row * BENSON_SUMMARY_WORDS : nullptr;
  if (b < 0 || b >= capacity) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int a = k * 64 + lane;
      if (mrow && a < NP) mrow[a] = 0;
    }
    if (srow && lane < BENSON_SUMMARY_WORDS) srow[lane] = -1;
    return;
  }
  Board<N> bd;
  bd.init(&lds, pool.zob, pool.skr(b));
  bd.load(&pool.slots[b]);
  const Slot<N>* const L = bd.L;
  const u64 E = ~(bd.Bw | bd.Ww) & bd.mValid;
  u32 mv[R];
#pragma unroll
  for (int k = 0; k < R; ++k) mv[k] = 0;

#pragma unroll 1
  for (int c = 0; c < 2; ++c) {
    const u32 xb = c ? 0x8000u : 0u;
    const u64 X = c ? bd.Ww : bd.Bw;
    const u64 NX = ~X & bd.mValid;   // empty points and opponent stones
    int chains = 0, alive = 0, stones = 0, safe = 0, rounds = 0;
    bool done = false;

    // ---- tables
    for (int j = lane; j < PP; j += BENSON_WAVE) { lab[j] = BENSON_NONE; aux[j] = BENSON_NONE; live[j] = 1; }
    for (int j = lane; j < PP * 2; j += BENSON_WAVE) reinterpret_cast<u32*>(cand)[j] = 0;
    Board<N>::wsync();
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (lane_bit(rl64(NX, k))) {
        const int p = bd.idx[k];
        const u32 v = L->pt[p];
        lab[p] = v ? (v & 0x7FFFu) : (u32)p;
      }
    }
    Board<N>::wsync();

    // ---- region labels: at most NP passes
    bool labelled = false;
#pragma unroll 1
    for (int pass = 0; pass < NP; ++pass) {
      bool ch = false;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        if (lane_bit(rl64(NX, k))) {
          const int p = bd.idx[k];
          const u32 cur = lab[p];
          u32 m = min(min(lab[p - S], lab[p - 1]), min(lab[p + S], lab[p + 1]));
          m = lab[min(m, cur)];
          if (m < cur) { atomicMin(&lab[p], m); atomicMin(&lab[cur], m); ch = true; }
        }
        Board<N>::wsync();
      }
      if (__ballot(ch) == 0) { labelled = true; break; }
    }

    if (labelled) {
      // ---- the smallest empty point of each region, its neighbour chains, and what the other empty points leave of them
#pragma unroll
      for (int k = 0; k < R; ++k)
        if (lane_bit(rl64(E, k))) atomicMin(&aux[lab[bd.idx[k]]], (u32)bd.idx[k]);
      Board<N>::wsync();
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int p = bd.idx[k];
        const u32 lr = lab[p];
        if (lane_bit(rl64(E, k)) && aux[lr] == (u32)p) {
          u32 r[4];
          benson_roots4<N>(L, p, xb, r);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            bool first = r[j] != 0;
#pragma unroll
            for (int i = 0; i < j; ++i) first = first && r[i] != r[j];
            if (first) cand[lr * 4 + j] = (u16)r[j];
          }
        }
      }
      Board<N>::wsync();
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int p = bd.idx[k];
        const u32 lr = lab[p];
        if (lane_bit(rl64(E, k)) && aux[lr] != (u32)p) {
          u32 r[4];
          benson_roots4<N>(L, p, xb, r);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const u32 cj = cand[lr * 4 + j];
            if (cj != 0 && cj != r[0] && cj != r[1] && cj != r[2] && cj != r[3]) cand[lr * 4 + j] = 0;
          }
        }
      }
      Board<N>::wsync();

      // ---- the removal rounds: at most chains + 1
      u64 rootm = 0;   // the chains' root stones, lane-distributed
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const u64 m = __ballot(lane_bit(rl64(X, k)) && (L->pt[bd.idx[k]] & 0x7FFFu) == (u32)bd.idx[k]);
        set_lane64(rootm, k, m);
        chains += __popcll(m);
      }
      alive = chains;
#pragma unroll 1
      for (int t = 0; t <= chains; ++t) {
        for (int j = lane; j < PP; j += BENSON_WAVE) aux[j] = 0;
        Board<N>::wsync();
        for (int j = lane; j < PP; j += BENSON_WAVE) {
          if (lab[j] == (u32)j && live[j]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const u32 cq = cand[j * 4 + q];
              if (cq) atomicAdd(&aux[cq], 1u);
            }
          }
        }
        Board<N>::wsync();
        int now = 0;
        bool rem = false;
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const int p = bd.idx[k];
          now += __popcll(__ballot(lane_bit(rl64(rootm, k)) && aux[p] >= 2u));
          if (lane_bit(rl64(NX, k))) {
            const u32 lr = lab[p];
            if (live[lr]) {
              u32 r[4];
              benson_roots4<N>(L, p, xb, r);
              bool dead = false;
#pragma unroll
              for (int j = 0; j < 4; ++j) dead = dead || (r[j] != 0 && aux[r[j]] < 2u);
              if (dead) { live[lr] = 0; rem = true; }
            }
          }
        }
        Board<N>::wsync();
        ++rounds;
        const bool changed = __ballot(rem) != 0 || now != alive;
        alive = now;
        if (!changed) { done = true; break; }
      }
    }

    // ---- the colour's bits and counts
    if (done) {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int p = bd.idx[k];
        const bool al = lane_bit(rl64(X, k)) && aux[L->pt[p] & 0x7FFFu] >= 2u;
        bool sf = false;
        if (lane_bit(rl64(NX, k))) {
          const u32 lr = lab[p];
          if (live[lr]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const u32 cq = cand[lr * 4 + q];
              sf = sf || (cq != 0 && aux[cq] >= 2u);
            }
          }
        }
        stones += __popcll(__ballot(al));
        safe += __popcll(__ballot(sf));
        mv[k] |= (al ? 1u << c : 0u) | (sf ? 4u << c : 0u);
      }
    }
    if (srow && lane < 4) {
      const u32 rw = (u32)rounds | (done ? 0u : BENSON_BOUND_HIT);
      srow[c * 4 + lane] = lane == 3 ? (int32_t)rw : !done ? 0 : lane == 0 ? alive : lane == 1 ? stones : safe;
    }
    Board<N>::wsync();   // the next colour refills the tables
  }
  if (mrow) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int a = k * 64 + lane;
      if (a < NP) mrow[a] = (uint8_t)mv[k];
    }
  }
}
