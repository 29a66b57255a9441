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
// One wave per row, DF_WAVES rows in flight per workgroup, rows looped grid-stride (as k_extract_agz).  A wave stages, per
// OUTPUT point o, one class word (bits 0-9 = planes 0-9, bits 10-17 / 18-25 = the two distances, 255 = no stone) and the
// history value in LDS; the store pass then walks the flat row 16 bytes per lane, 1 KiB per instruction, and derives every
// element from those two arrays, so the row's alignment (25*N*N*4 is no multiple of 16) only moves the peeled head and tail.
#pragma once
#include "go_board.cuh"

namespace elfgo {

constexpr int DF_PLANES = 25;   // base/board_feature.h:18 MAX_NUM_FEATURE
constexpr int DF_WAVES = 4;
constexpr int DF_WAVE = 64;
constexpr u32 DF_FAR = 255;     // "no stone of that colour": stored as 10000.0f

// LDS of one wave
template <int N>
struct alignas(16) DfLds {
  using G = Geo<N>;
  static constexpr int IMG = 64 + 4 * G::PP;   // the slot's prefix: header, pt, libs
  uint4 img[IMG / 16];
  u32 cls[G::NP];
  float hx[G::NP];
  u16 placed[(G::NP + 7) & ~7];
};
static_assert(DfLds<19>::IMG % 16 == 0 && DfLds<9>::IMG % 16 == 0, "the slot prefix is copied 16 B per lane");
static_assert(offsetof(Slot<19>, hist) == DfLds<19>::IMG && offsetof(Slot<9>, hist) == DfLds<9>::IMG, "header, pt and libs are the slot's first bytes");

// the flat row, element f = plane * N*N + o: head up to the first 16-byte boundary, 16 B per lane, tail
template <int N, class F>
__device__ __forceinline__ void df_store(float* __restrict__ out, int lane, F value) {
  constexpr int NP = Geo<N>::NP, TOTAL = DF_PLANES * NP;
  const int head = (int)(((16 - ((uintptr_t)out & 15)) & 15) >> 2);
  if (lane < head) out[lane] = value(0, lane);
  const int body = (TOTAL - head) >> 2;
  float4* o4 = (float4*)(out + head);
  for (int j = lane; j < body; j += DF_WAVE) {
    const int f = head + 4 * j;
    int p = f / NP, o = f - p * NP;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = value(p, o);
      if (++o == NP) { o = 0; ++p; }
    }
    o4[j] = make_float4(v[0], v[1], v[2], v[3]);
  }
  const int f = head + 4 * body + lane;
  if (f < TOTAL) out[f] = value(f / NP, f % NP);
}

// distance from position y to the nearest set bit of the non-zero row mask m (bits 0..N-1)
__device__ __forceinline__ u32 df_row_dist(u32 m, u32 y) {
  const u32 lo = m & ((2u << y) - 1u), hi = m >> y;
  const u32 dl = lo ? y - (31u - (u32)__builtin_clz(lo)) : DF_FAR;
  const u32 dr = hi ? (u32)__builtin_ctz(hi) : DF_FAR;
  return dl < dr ? dl : dr;
}

// placed: the table (row = slot id) when by_slot, else the caller's rows (row = r)
template <int N>
__global__ __launch_bounds__(DF_WAVE * DF_WAVES) void k_extract_df(const Slot<N>* __restrict__ slots, int capacity, const int32_t* ids,
                                                                    const int32_t* d4s, int n, const u16* __restrict__ placed, int by_slot,
                                                                    const float* __restrict__ exptab, float* dst, int64_t stride) {
  using G = Geo<N>;
  constexpr int R = G::R, NP = G::NP, S = G::S;
  __shared__ DfLds<N> lds_all[DF_WAVES];
  const int lane = threadIdx.x & 63, wv = rfl((int)(threadIdx.x >> 6));
  DfLds<N>& L = lds_all[wv];
  const Hdr* hdr = reinterpret_cast<const Hdr*>(L.img);
  const u16* pt = reinterpret_cast<const u16*>(L.img) + 32;
  const u16* libs = pt + G::PP;
  const int nw = (int)gridDim.x * DF_WAVES;
  for (int r = (int)blockIdx.x * DF_WAVES + wv; r < n; r += nw) {
    const int b = rfl(ids ? ids[r] : r);
    float* row = dst + (size_t)r * stride;
    // an opaque copy of the lane index: the per-point geometry below (19 x R row offsets among it) does not depend on the row,
    // and hoisted out of this loop it would cost a hundred registers
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
    // board.cc:466-474; ko_pt is a reference Coord c = (y+1)*S + (x+1)
    const int ko_a = (ko_age == 0 && ko_pt != M_PASS) ? (ko_pt % S - 1) * N + (ko_pt / S - 1) : -1;
    const bool white_moves = player == S_WHITE;
    const int rot = d4 & 3;
    const bool flip = ((d4 >> 2) & 1) != 0;
    u32 xo_[R], yo_[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const u32 o = (u32)(k * 64 + ln);
      const bool valid = (k + 1) * 64 <= NP || o < (u32)NP;
      // Transform (board_feature.h:97-113): output point o = (xo, yo) shows source point (x, y)
      const u32 xo = __umul24(o, (u32)G::DN_M) >> G::DN_S, yo = o - __umul24(xo, (u32)N);
      xo_[k] = xo; yo_[k] = yo;
      u32 xf = xo, yf = yo;
      if (flip) { xf = yo; yf = xo; }
      u32 x = xf, y = yf;
      if (rot == 1) { x = N - 1 - yf; y = xf; }
      else if (rot == 2) { x = N - 1 - xf; y = N - 1 - yf; }
      else if (rot == 3) { x = yf; y = N - 1 - xf; }
      if (valid) {
        const u32 a = __umul24(x, (u32)N) + y;
        const u32 v = pt[a + S + 1 + 2 * x];   // Board::a2i
        const u32 lb = libs[v & 0x7FFFu];
        const bool stone = (v & 0x7FFFu) != 0;
        const bool ours = stone && ((v >> 15) != 0) == white_moves;
        const u32 lc = lb == 1 ? 0u : (lb == 2 ? 1u : 2u);
        u32 c = 0;
        if (stone) c = (1u << (lc + (ours ? 0u : 3u))) | (ours ? 1u << 7 : 1u << 8);
        if (v == 0) c = 1u << 9;
        if ((int)a == ko_a) c |= 1u << 6;
        int d = ply - (int)L.placed[a];
        d = d < 0 ? 0 : (d > 2 * NP ? 2 * NP : d);
        L.cls[o] = c;
        L.hx[o] = stone ? exptab[d] : 0.0f;
      }
    }
    agz_wave_sync();
    // output row xo as a bit mask over yo, per colour, in lane xo
    u32 row_ours = 0, row_theirs = 0;
    if (ln < N) {
      for (int y = 0; y < N; ++y) {
        const u32 c = L.cls[ln * N + y];
        row_ours |= ((c >> 7) & 1u) << y;
        row_theirs |= ((c >> 8) & 1u) << y;
      }
    }
    // distance of (xo, yo) = min over rows r with a stone of |xo - r| + distance to the nearest set bit of row r from yo
    u32 dm[2][R];
#pragma unroll
    for (int k = 0; k < R; ++k) dm[0][k] = dm[1][k] = DF_FAR;
#pragma unroll
    for (int rr = 0; rr < N; ++rr) {
#pragma unroll
      for (int col = 0; col < 2; ++col) {
        const u32 m = (u32)rl((int)(col ? row_theirs : row_ours), rr);   // wave-uniform
        if (m != 0) {
#pragma unroll
          for (int k = 0; k < R; ++k) {
            const int dx = (int)xo_[k] - rr;
            const u32 d = df_row_dist(m, yo_[k]) + (u32)(dx < 0 ? -dx : dx);
            dm[col][k] = d < dm[col][k] ? d : dm[col][k];
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const u32 o = (u32)(k * 64 + ln);
      if ((k + 1) * 64 <= NP || o < (u32)NP) L.cls[o] |= (dm[0][k] << 10) | (dm[1][k] << 18);
    }
    agz_wave_sync();
    const u32* cls = L.cls;
    const float* hx = L.hx;
    df_store<N>(row, lane, [=](int p, int o) -> float {
      const u32 c = cls[o];
      if (p < 10) return (float)((c >> p) & 1u);
      if (p == 10 || p == 11) return ((c >> (p - 3)) & 1u) ? hx[o] : 0.0f;
      if (p == 14 || p == 15) {
        const u32 d = (c >> (p == 14 ? 10 : 18)) & 0xFFu;
        return d == DF_FAR ? 10000.0f : (float)d;
      }
      if (p == 16) return white_moves ? 0.0f : 1.0f;
      if (p == 17) return white_moves ? 1.0f : 0.0f;
      return 0.0f;
    });
    agz_wave_sync();
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
