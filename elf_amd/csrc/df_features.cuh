// BoardFeature::extract (base/board_feature.cc:43-237): the reference's 25 DarkForest planes of a board slot, and the upkeep of
// the one piece of state they need that a slot does not carry -- Info::last_placed, the ply at which the stone on a point was
// placed (board.cc:680, :1379) -- in a side table uint16 [capacity][N*N] in action order (a = x*N + y) that only callers who
// ask for these planes pay for.
//
// Planes (board_feature.h:18-36; "ours" = the side to move), fp32 [25][N][N] under Transform (board_feature.h:97-113):
//   0-2 / 3-5  our / the opponent's stones of groups with 1, 2, >= 3 liberties     getLibertyMap3binary
//   6          the simple-ko point (ko_age == 0 && ko_pt != M_PASS)                getSimpleKo
//   7 / 8 / 9  our stones / the opponent's / empty points                          getStones
//   10 / 11    on our / the opponent's stones (float)exp((last_placed - ply) / 10.0): looked up in a host-made table, the
//              device never evaluates exp                                           getHistoryExp
//   14 / 15    Manhattan distance to our / the opponent's nearest stone, 10000 everywhere without one (what the two separable
//              passes of DistanceTransform compute)                                 getDistanceMap
//   16 / 17    all 1.0 when Black / White is to move
//   12, 13, 18-24 zero
//
// One wave per row, DF_WAVES rows in flight per workgroup, rows looped grid-stride (as k_extract_agz).  The planes themselves are
// df_planes_row (df_planes.cuh), the text k_replay_extract_df shares: a wave stages, per OUTPUT point o, one class word (bits 0-9 =
// planes 0-9, bits 10-17 / 18-25 = the two distances, 255 = no stone) and the history value in LDS; the store pass then walks
// the flat row 16 bytes per lane, 1 KiB per instruction, and derives every element from those two arrays, so the row's
// alignment (25*N*N*4 is no multiple of 16) only moves the peeled head and tail.
#pragma once
#include "df_planes.cuh"

namespace elfgo {

constexpr int DF_WAVES = 4;

// LDS of one wave: the staged slot prefix, then what df_planes_row works in -- per OUTPUT point one class word and the history
// value, per SOURCE point (action order) the placement ply
template <int N>
struct alignas(16) DfLds {
  using G = Geo<N>;
  static constexpr int IMG = df_img_bytes<N>();
  uint4 img[IMG / 16];
  u32 cls[G::NP];
  float hx[G::NP];
  u16 placed[(G::NP + 7) & ~7];
};

// placed: the table (row = slot id) when by_slot, else the caller's rows (row = r)
template <int N>
__global__ __launch_bounds__(DF_WAVE * DF_WAVES) void k_extract_df(const Slot<N>* __restrict__ slots, int capacity, const int32_t* ids,
                                                                    const int32_t* d4s, int n, const u16* __restrict__ placed, int by_slot,
                                                                    const float* __restrict__ exptab, float* dst, int64_t stride) {
  constexpr int NP = Geo<N>::NP;
  __shared__ DfLds<N> lds_all[DF_WAVES];
  const int lane = threadIdx.x & 63, wv = rfl((int)(threadIdx.x >> 6));
  DfLds<N>& L = lds_all[wv];
  const Hdr* hdr = reinterpret_cast<const Hdr*>(L.img);
  const int nw = (int)gridDim.x * DF_WAVES;
  for (int r = (int)blockIdx.x * DF_WAVES + wv; r < n; r += nw) {
    const int b = rfl(ids ? ids[r] : r);
    float* row = dst + (size_t)r * stride;
    // an opaque copy of the lane index: the per-point geometry of df_planes_row does not depend on the row, and hoisted out of
    // this loop it would cost a hundred registers
    int ln = lane;
    asm volatile("" : "+v"(ln));
    if (b < 0 || b >= capacity) {   // wave-uniform
      df_store<N>(row, lane, [](int, int) { return 0.0f; });
      continue;
    }
    const uint4* g4 = reinterpret_cast<const uint4*>(&slots[b]);
    for (int j = lane; j < DfLds<N>::IMG / 16; j += DF_WAVE) L.img[j] = g4[j];
    const u16* prow = placed + (size_t)(by_slot ? b : r) * NP;
    for (int j = lane; j < NP; j += DF_WAVE) L.placed[j] = prow[j];
    const int d4 = rfl(d4s ? d4s[r] : 0);
    agz_wave_sync();
    const int ply = rfl((int)hdr->ply), player = rfl((int)hdr->next_player);
    const int ko_pt = rfl((int)hdr->ko_pt), ko_age = rfl((int)hdr->ko_age);
    df_planes_row<N>(L.img, L.placed, L.cls, L.hx, ply, player, ko_pt, ko_age, d4, exptab, row, lane, ln);
  }
}

// ---- the table's upkeep: one thread per point or per row; a slot id outside the pool is skipped (reads as a zero row) ----------
__device__ __forceinline__ int df_slot(const int32_t* ids, int i) { return ids ? ids[i] : i; }

// rows of the listed slots to 0 (elfgo_reset's part)
__global__ void k_df_clear(u16* table, int np, int capacity, const int32_t* ids, int n) {
  const int b = df_slot(ids, blockIdx.x);
  if (b < 0 || b >= capacity) return;
  for (int a = threadIdx.x; a < np; a += blockDim.x) table[(size_t)b * np + a] = 0;
}

// row dst[i] <- row src[i] (elfgo_copy's part)
__global__ void k_df_copy(u16* table, int np, int capacity, const int32_t* dst, const int32_t* src, int n) {
  const int d = dst[blockIdx.x], s = src[blockIdx.x];
  if (d == s || d < 0 || d >= capacity || s < 0 || s >= capacity) return;
  for (int a = threadIdx.x; a < np; a += blockDim.x) table[(size_t)d * np + a] = table[(size_t)s * np + a];
}

// after elfgo_forward: an accepted placement at ply p wrote p (board.cc:680, :1379; _ply is incremented afterwards, :1237), so
// p is the slot's ply now minus one.  A pass, a resignation and a refused move change nothing.
template <int N>
__global__ void k_df_note(const Slot<N>* slots, u16* table, int capacity, const int32_t* ids, const int32_t* moves, const uint8_t* ok, int n) {
  constexpr int S = N + 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || ok[i] != 1) return;
  const int b = df_slot(ids, i), c = moves[i];
  if (b < 0 || b >= capacity || c < 0 || c >= S * S) return;
  const int x = c % S - 1, y = c / S - 1;
  if (x < 0 || x >= N || y < 0 || y >= N) return;
  table[(size_t)b * (N * N) + x * N + y] = (u16)(slots[b].h.ply - 1);
}

// after elfgo_setup: accepted rows carry 1 under every stone and 0 elsewhere (PlaceHandicap plays at ply 1 and puts the ply
// back, board.cc:109-126); refused rows are untouched
__global__ void k_df_setup(u16* table, int np, int capacity, const int32_t* ids, const uint8_t* stones, const uint8_t* ok, int n) {
  const int i = blockIdx.x;
  if (ok[i] != 1) return;
  const int b = df_slot(ids, i);
  if (b < 0 || b >= capacity) return;
  for (int a = threadIdx.x; a < np; a += blockDim.x) table[(size_t)b * np + a] = stones[(size_t)i * np + a] ? 1 : 0;
}

// out[i] <- row ids[i]
__global__ void k_df_placed(const u16* table, int np, int capacity, const int32_t* ids, int n, u16* out) {
  const int b = df_slot(ids, blockIdx.x);
  const bool in = b >= 0 && b < capacity;
  for (int a = threadIdx.x; a < np; a += blockDim.x) out[(size_t)blockIdx.x * np + a] = in ? table[(size_t)b * np + a] : (u16)0;
}

}  // namespace elfgo
