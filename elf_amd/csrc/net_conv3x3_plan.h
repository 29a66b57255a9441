// What of elfnet_conv3x3_f16's algo 1 (net_conv3x3.hip) the host can plan: the work ids of a launch and what each computes, the
// two row orders and how their ids are dealt to the workgroups, the rule that chooses between the orders, the division by a launch
// constant and the byte offsets the buffer-addressed staging goes by.  The kernel and its host entry (net_conv3x3.hip) and the
// exported host arithmetic (net_conv3x3_plan.hip) call the same functions.
#pragma once
#include "net_common.h"

namespace {

constexpr int kTileM = 256;                      // positions per workgroup
constexpr int kTileN = 256;                      // output channels per workgroup

// ---- buffer-addressed staging.  x and w are read through one raw buffer descriptor each (stride 0, offen), made in scalar
// registers at kernel entry; a staged piece is buffer_load_dwordx4 v, s[rsrc], s offen lds: the lane's 32-bit byte offset (made
// once per item, decode_rows) in the vector register, everything wave-uniform about the piece (tap, channel chunk) in the scalar
// offset.  The sum the instruction addresses by is unsigned, and a tap's offset from a row's own position is negative for ky = 0
// and kx = 0, so x's descriptor starts bias = (W + 1) Cin 2 bytes in front of x and every scalar offset of x carries + bias.
// Zeros come from the descriptor's range check: a lane whose vector offset is at or above num_records reads nothing and its
// 16 bytes of LDS are written with zeros.  Such a lane carries kSentinel, whatever the tensor's size: 16-byte aligned, at or above
// every num_records the entry accepts, and with every scalar offset still below 2^32.  The arithmetic, shared with the host entry
// elfnet_conv3x3_f16_bufstage and its test:
//   x  bytes < 2^31 (net_conv.hip), bias and every scalar offset (at most (2 W + 3) Cin 2) below 2^30 (the native entry refuses a
//      wider board): num_records = bytes + bias < 2^31 + 2^30 = kSentinel; a valid row's offset + scalar offset < 2^31 + 2^30;
//      kSentinel + scalar offset < 2^32: no sum wraps.  A tap that is on the board addresses bytes of x only: offset + scalar
//      offset - bias is that neighbour's chunk.
//   w  bytes < 2^31, the scalar offset stays inside a weight row: below the tensor's size.
constexpr uint32_t kSentinel = 0xC0000000u;
__host__ __device__ inline uint32_t x_bias(int W, int Cin) { return (uint32_t)(W + 1) * (uint32_t)(Cin * 2); }
// the scalar byte offset of K tile (tap, kc): from a row's own position in x (bias included), and from the start of a weight row
__host__ __device__ inline uint32_t x_soffset(int W, int Cin, int tap, int kc) {
  const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
  return (uint32_t)((dy * W + dx) * Cin * 2 + kc * 128) + x_bias(W, Cin);
}
__host__ __device__ inline uint32_t w_soffset(int Cin, int tap, int kc) { return (uint32_t)(tap * Cin * 2 + kc * 128); }
// does the buffer form take the shape?  (every scalar offset of x below 2^30)
inline bool bufstage_takes(int wd, int c) { return (2 * (int64_t)wd + 3) * c * 2 < ((int64_t)1 << 30); }

// Work id -> work.  Work items are numbered tiles fastest, then channel column; ids below nfull are one full item each, and
// every item from nfull on is two consecutive ids: channel half 0, then half 1.  half < 0: the full 256 channels.
struct WorkItem { int tile, col, half; };
__host__ __device__ inline WorkItem work_item(int id, int tiles, int nfull) {
  int half = -1;
  if (id >= nfull) {
    const int e = id - nfull;
    id = nfull + (e >> 1);
    half = e & 1;
  }
  const int col = id / tiles;
  return WorkItem{id - col * tiles, col, half};
}
// How many of `total` work items stay full when they run `width` at a time: the items of a last round that is at most half full
// are split (each half then has a CU of its own in that round); a fuller last round, none, or less than one round is left alone.
__host__ __device__ inline int full_items(int64_t total, int64_t width) {
  const int64_t r = total % width;
  return (int)(total >= width && r > 0 && 2 * r <= width ? total - r : total);
}

// floor(n / d) for every 0 <= n < 2^31 as one multiply and one shift: with l = ceil(log2 d), s = max(32, 31 + l) and
// mul = floor((2^s - 1) / d), which is below 2^32, e = 2^s - mul d lies in [1, d] and (n + 1) mul / 2^s = (n + 1) / d -
// (n + 1) e / (d 2^s); (n + 1) e <= 2^31 2^l <= 2^s, so the second term is above 0 and at most 1 / d: the floor is floor(n / d)
// whether d divides n + 1 or not.  The rounded-up multiplier would need 33 bits at d = 1.  The host makes (mul, shift = s - 32)
// once per launch; a launch's divisors are H W and W.
struct Recip { uint32_t mul, shift; };
inline Recip recip_of(uint32_t d) {   // 1 <= d <= 2^31
  int l = 0;
  while (((uint64_t)1 << l) < d) ++l;
  const int s = l == 0 ? 32 : 31 + l;
  return Recip{(uint32_t)((((uint64_t)1 << s) - 1) / d), (uint32_t)(s - 32)};
}
// the quotient where the host plans with it too (the deal below); on the device n is wave-uniform there (per lane: the kernel's div_by)
__host__ __device__ inline uint32_t udiv_by(uint32_t n, Recip r) { return (uint32_t)(((uint64_t)(n + 1) * r.mul) >> 32) >> r.shift; }

// ---- the two row orders.  A work item is 256 rows x a channel column; row r of it is position base + r * stride, valid for
// r < limit, and the item visits the taps of `mask` (bit 3 ky + kx), ascending, Cin / 64 K tiles each.
//   linear  tile t is the positions 256 t .. 256 t + 255: base = 256 t, stride 1, limit = M - base, every tap (0x1FF); what is off
//           the board is decided per row (decode_rows).  Ids, split last round and deal are work_item's and full_items' above.
//   board   with B = ceil(rows / 256) blocks of 256 consecutive boards, an item is (block b, board position hw, column): row r is
//           board 256 b + r at hw, base = 256 b H W + hw, stride H W, limit = rows - 256 b.  Every row has the same taps on the
//           board, so the item visits only those: 4 for a corner, 6 for an edge, 9 inside.  No half tiles.
//           id = (rank(hw) * columns + column) * B + b, the block fastest; rank lists the inner positions, then the edges, then
//           the corners, each class row-major (a board with H or W below 3 has no such classes: rank = hw), so the long items
//           come first.  With G workgroups and F = ids / G, workgroup g runs g, g + G, ... in the F full rounds and, in the last,
//           partial round, id F G + (G - 1 - g) if there is one: the last round's items, the shortest, go to the workgroups that
//           got the shorter items of the round where the classes change.  Static, no workgroup depends on another.
struct Deal {
  int board;                 // the row order: 0 linear, 1 board
  int ids, fullids;          // work ids; board: F G, the ids of the full rounds (linear: never reached)
  int tiles, nfull;          // linear: work_item's arguments
  int nblk, per_rank, boards, stride;   // board: B, B * columns, rows, H W (linear: stride 1)
  Recip dpr, dblk, din, dw;  // board: the divisions by per_rank, B, W - 2 and W
};
struct Item { int base, limit, kbase, mask, half; };
__host__ __device__ inline int tap_mask(int hh, int ww, int H, int W) {
  const int rowm = (hh > 0 ? 1 : 0) | 8 | (hh + 1 < H ? 64 : 0), colm = (ww > 0 ? 1 : 0) | 2 | (ww + 1 < W ? 4 : 0);
  return rowm * colm;   // decode_rows has why this is the mask
}
// rank -> board position (h, w)
__host__ __device__ inline void pos_of_rank(int k, int H, int W, Recip din, Recip dw, int& hh, int& ww) {
  if (H < 3 || W < 3) { hh = (int)udiv_by((uint32_t)k, dw); ww = k - hh * W; return; }
  const int a = W - 2, inner = (H - 2) * a, side = 2 * (H - 2);
  if (k < inner) { hh = (int)udiv_by((uint32_t)k, din); ww = k - hh * a + 1; hh += 1; }
  else if ((k -= inner) < a) { hh = 0; ww = k + 1; }
  else if ((k -= a) < side) { hh = (k >> 1) + 1; ww = (k & 1) * (W - 1); }
  else if ((k -= side) < a) { hh = H - 1; ww = k + 1; }
  else { k -= a; hh = (k >> 1) * (H - 1); ww = (k & 1) * (W - 1); }
}
__host__ __device__ inline Item item_of(const Deal& d, int id, int M, int H, int W, int* block = nullptr, int* pos = nullptr) {
  if (!d.board) {
    const WorkItem wi = work_item(id, d.tiles, d.nfull);
    return Item{wi.tile * kTileM, M - wi.tile * kTileM, wi.col * kTileN + (wi.half > 0 ? kTileN / 2 : 0), 0x1FF, wi.half};
  }
  const int rank = (int)udiv_by((uint32_t)id, d.dpr), rem = id - rank * d.per_rank;
  const int col = (int)udiv_by((uint32_t)rem, d.dblk), b = rem - col * d.nblk;
  int hh, ww;
  pos_of_rank(rank, H, W, d.din, d.dw, hh, ww);
  const int hw = hh * W + ww;
  if (block) *block = b;
  if (pos) *pos = hw;
  return Item{b * kTileM * d.stride + hw, d.boards - b * kTileM, col * kTileN, tap_mask(hh, ww, H, W), -1};
}
// the id behind `id` on workgroup g of G; at or beyond d.ids: none
__host__ __device__ inline int next_id(const Deal& d, int id, int g, int G) {
  if (id >= d.fullids) return d.ids;
  const int nid = id + G;
  return nid >= d.fullids ? d.fullids + (G - 1 - g) : nid;
}
// the K-tile taps of a mask: the lowest, and the next above t (9 or more: none)
__host__ __device__ inline int first_tap(int mask) { return __builtin_ctz((unsigned)mask | 0x200u); }
__host__ __device__ inline int next_tap(int mask, int t) { return t + 1 + __builtin_ctz(((unsigned)mask >> (t + 1)) | 0x200u); }

// ---- host: the two plans
// the linear order's deal for `width` items at a time (0: one id per workgroup)
inline Deal linear_deal(int64_t m, int k, int width, int* G) {
  Deal d{};
  d.tiles = (int)((m + kTileM - 1) / kTileM);
  const int64_t total = (int64_t)d.tiles * (k / kTileN);       // below 2^31: m * k is below 2^30
  d.nfull = width > 0 ? full_items(total, width) : (int)total;
  d.ids = (int)(2 * total - d.nfull);
  d.fullids = 1 << 30;
  d.stride = 1;
  *G = width > 0 && width < d.ids ? width : d.ids;
  return d;
}
// Does board order take the shape?  Not an item of one K tile (a 1 x 1 board at 64 input channels: the loop's first K tile is at
// the latest its last but one), and its ids stay below 2^30.
inline bool board_takes(int64_t rows, int h, int wd, int c, int k) {
  const int64_t nblk = (rows + kTileM - 1) / kTileM;
  return rows > 0 && !((int64_t)h * wd == 1 && c < 128) && nblk * h * wd * (k / kTileN) < ((int64_t)1 << 30);
}
inline Deal board_deal(int64_t rows, int h, int wd, int k, int width, int* G) {
  Deal d{};
  d.board = 1;
  d.nblk = (int)((rows + kTileM - 1) / kTileM);
  d.per_rank = d.nblk * (k / kTileN);
  d.boards = (int)rows;
  d.stride = h * wd;
  d.ids = d.per_rank * d.stride;
  *G = width > 0 && width < d.ids ? width : d.ids;
  d.fullids = d.ids / *G * *G;
  d.nfull = d.ids;
  d.dpr = recip_of((uint32_t)d.per_rank);
  d.dblk = recip_of((uint32_t)d.nblk);
  d.din = recip_of((uint32_t)(wd > 2 ? wd - 2 : 1));
  d.dw = recip_of((uint32_t)wd);
  return d;
}
// the K tiles of workgroup g of G, in chunks-per-tap units of `kchunks`: board order
inline int64_t board_load(const Deal& d, int g, int G, int h, int wd, int kchunks) {
  int64_t sum = 0;
  for (int id = g; id < d.ids; id = next_id(d, id, g, G))
    sum += (int64_t)__builtin_popcount((unsigned)item_of(d, id, 0, h, wd).mask) * kchunks;
  return sum;
}
// The order the plain entry takes for a shape at `width` items a round: board order iff there are at least 256 rows and its most
// loaded workgroup has strictly fewer K tiles than the linear order's, which is its full rounds x 9 kchunks plus a last round of
// 9 kchunks, or of 3/4 of that where it is split (a half tile takes 0.75 of a tile's time: profiles/conv_tail_probe.json).
// Compared in quarters of a K tile.  Host arithmetic, the same on every call of a shape; the last answer is kept per thread.
inline int order_of(int64_t rows, int h, int wd, int c, int k, int width) {
  if (rows < kTileM || width <= 0 || !board_takes(rows, h, wd, c, k)) return 0;
  struct Key { int64_t rows; int h, wd, c, k, width, order; };
  static thread_local Key last{-1, 0, 0, 0, 0, 0, 0};
  if (last.rows == rows && last.h == h && last.wd == wd && last.c == c && last.k == k && last.width == width) return last.order;
  const int kchunks = c >> 6;
  int G = 0;
  const Deal l = linear_deal(rows * h * wd, k, width, &G);
  const int64_t total = (int64_t)l.tiles * (k / kTileN), r = total % width;
  const int64_t lin4 = (total / width * 4 + (r == 0 ? 0 : l.nfull < total ? 3 : 4)) * 9 * kchunks;
  const Deal b = board_deal(rows, h, wd, k, width, &G);
  int64_t most = 0;
  for (int g = 0; g < G && 4 * most < lin4; ++g) {
    const int64_t v = board_load(b, g, G, h, wd, kchunks);
    if (v > most) most = v;
  }
  last = Key{rows, h, wd, c, k, width, 4 * most < lin4 ? 1 : 0};
  return last.order;
}

}  // namespace

// the CU count of the current device, asked for once per device; 0: unknown.  Defined in net_conv3x3.hip, for both units.
__attribute__((visibility("hidden"))) int round_width_of_device();
