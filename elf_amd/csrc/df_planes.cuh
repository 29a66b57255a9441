// The one text of the 25 DarkForest planes (BoardFeature::extract, base/board_feature.cc:43-237; plane list in df_features.cuh):
// df_planes_row turns the LDS image of a slot's prefix plus a row of placement plies into one fp32 [25][N][N] row.  Its callers
// are k_extract_df (df_features.cuh: a board slot and a row of the side table, staged from HBM) and k_replay_extract_df
// (train_df.cuh: the replayed position where it already lies, placement plies rebuilt from the move list).
// Only templates and inline device functions here: this header is included by more than one translation unit.
#pragma once
#include "go_board.cuh"

namespace elfgo {

constexpr int DF_PLANES = 25;   // base/board_feature.h:18 MAX_NUM_FEATURE
constexpr int DF_WAVE = 64;
constexpr u32 DF_FAR = 255;     // "no stone of that colour": stored as 10000.0f

template <int N>
constexpr int df_img_bytes() { return 64 + 4 * Geo<N>::PP; }   // the slot's prefix: header, pt, libs
static_assert(df_img_bytes<19>() % 16 == 0 && df_img_bytes<9>() % 16 == 0, "the slot prefix is copied 16 B per lane");
static_assert(offsetof(Slot<19>, hist) == df_img_bytes<19>() && offsetof(Slot<9>, hist) == df_img_bytes<9>(), "header, pt and libs are the slot's first bytes");

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

// One wave, one row: classification, distance pass, store.  All of img, placed, cls, hx are LDS of this wave:
//   img     image of the slot prefix; only pt and libs are read -- the header fields arrive as arguments, because a caller that
//           replayed the position holds them in registers and its LDS header is stale
//   placed  the placement plies, action order, NP entries, visible to the wave on entry
//   cls, hx NP words each, written here (a caller short of LDS may lay them over whatever it no longer needs)
// ply / player / ko_pt / ko_age / d4 are wave-uniform.  ln = the lane index, which the caller may pass as an opaque copy to keep
// the per-point geometry (19 x R row offsets among it) from being hoisted over its own loops.  Ends with a wave fence: the LDS
// may be reused on return.
template <int N>
__device__ __forceinline__ void df_planes_row(const uint4* img, const u16* placed, u32* cls, float* hx, int ply, int player, int ko_pt, int ko_age,
                                              int d4, const float* __restrict__ exptab, float* row, int lane, int ln) {
  using G = Geo<N>;
  constexpr int R = G::R, NP = G::NP, S = G::S;
  const u16* pt = reinterpret_cast<const u16*>(img) + 32;
  const u16* libs = pt + G::PP;
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
      int d = ply - (int)placed[a];
      d = d < 0 ? 0 : (d > 2 * NP ? 2 * NP : d);
      cls[o] = c;
      hx[o] = stone ? exptab[d] : 0.0f;
    }
  }
  agz_wave_sync();
  // output row xo as a bit mask over yo, per colour, in lane xo
  u32 row_ours = 0, row_theirs = 0;
  if (ln < N) {
    for (int y = 0; y < N; ++y) {
      const u32 c = cls[ln * N + y];
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
    if ((k + 1) * 64 <= NP || o < (u32)NP) cls[o] |= (dm[0][k] << 10) | (dm[1][k] << 18);
  }
  agz_wave_sync();
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

}  // namespace elfgo
