// elfnet_conv3x3_f16's algo 1: the trunk convolution y = relu?(conv3x3_same(x, w) + bias (+ res)) as a hand-written implicit GEMM,
// fp16 NHWC in and out, w as [K,3,3,C], fp32 accumulation in v_mfma_f32_32x32x16_f16.  Nothing is unfolded, no workspace.
//
// Why beside CK's kernel (net_conv.hip, algo 0): that one is a 256 x 128 x 32 tile with one LDS stage and two barriers per 32-deep
// K step, and sits on that structure's ceiling.  Here:
//   tile      256 positions x 256 output channels x BK 64 (one tap, 64 consecutive input channels); all of N in one tile, so an
//             activation byte is staged once for every output channel.  512 threads, 8 waves as 2 (positions) x 4 (channels), each
//             owning 128 positions x 64 channels = 4 x 2 MFMA tiles = 128 accumulator registers.  One workgroup per CU.
//   staging   LDS-DMA (buffer_load_dwordx4 ... offen lds through one raw buffer descriptor per operand: the row's offset in a vector
//             register, the K tile's in a scalar; the comment at kSentinel) straight into two 64-KiB LDS buffers (activation tile, weight tile: 256 rows of
//             128 B each), in half-tiles of 128 rows of one operand, two 8-row pieces per wave, issued one at a time between the
//             MFMAs of the MFMA segments; three or four half-tiles stay in flight across the loop's barriers, which are bare
//             s_barriers behind counted vmcnt waits (the comment at the main loop has the slots and the counts).  vmcnt(0) only
//             once the last half-tile is on its way.  Every staged piece is a full aligned 128-B line: 8 lanes per row.
//   halo      a staging lane decodes its four rows once (position -> n, h, w: two divisions by launch constants, each a multiply
//             by a multiplier the host entry made and a shift) and keeps a 9-bit tap mask (a 3-bit row mask times a 3-bit column
//             mask) and a byte offset; for an off-board tap, and for a row at or beyond its item's limit (M; in board order the
//             last board), its offset is one the descriptor's range check refuses, and the load writes zeros to LDS without
//             reading memory.  LDS is never zeroed by a second path.  Board order keeps no mask: its items visit on-board taps only.
//   LDS image lane-linear, as the DMA writes it; the 16-B slot s of row r holds the row's chunk s ^ ((r >> 1) & 7): the XOR is on
//             the source address when staging and on the read address of the fragment ds_read_b128s, which are then conflict-free
//             (rows r and r + 1 share a 256-B bank row, so the swizzle steps every second row; checked against the 16-lane groups
//             ds_read_b128 is served in).
//   K order   tap-major (ky, kx, then c ascending); inside a 32-channel block the two MFMAs take channels {0..7, 16..23} and
//             {8..15, 24..31}, as CK's blockwise GEMM hands them out: algo 0's accumulation chain per output element, bit for bit.
//   epilogue  accumulators -> fp16 -> LDS (4 KiB of the wave's own behind the staging buffers, 32 positions at a time) -> 16 B of
//             consecutive channels per lane; bias and res are read in that shape, and the values are BiasResAct's of
//             net_conv.hip: float(half(acc)) + bias (+ res), max(., 0), one rounding to fp16, computed as one v_fma_mix_f32 per
//             addition (it converts its fp16 operands itself), the rounding, and the ReLU on the packed fp16 pair behind it under
//             a uniform branch (max and a monotone rounding commute; NaN gives +0 either way).  Rows at or beyond the limit are not
//             stored.  No workgroup barrier: a wave reads back what it wrote itself.
//   tail      the work items of a launch (position tiles x channel columns of 256) run in rounds of one per CU.  Where the last
//             round is at most half full, each of its items runs as two work ids of 256 positions x 128 channels (the half
//             tile: the same waves at 128 x 32 each, three staged half-tiles per K tile instead of four), so that round takes
//             a half tile's time.  Same kernel, same launch, same K chain per output element: the bits do not change.  The host
//             entry decides (full_items below).
//   orders    the 256 rows of a tile are, in linear order, 256 consecutive positions (n, h, w), about 13.5 rows of a 19 x 19
//             board: every tile has positions on every edge, runs all nine taps and multiplies staged zeros wherever a tap is
//             off the board, 6.9 % of all K tiles on 19 x 19.  In board order they are one board position (h, w) of 256 consecutive
//             boards, H W positions apart: every row has the same taps on the board, the item carries that 9-bit mask in a scalar
//             and its K loop visits only the set taps, ascending (first_tap, next_tap; popcount x Cin / 64 K tiles: 4 taps in a
//             corner, 6 on an edge, 9 inside; 3025 taps per block of boards on 19 x 19 instead of 3249).  One kernel body: row r of an
//             item is position base + r stride, valid below limit (decode_rows, load_skip and the epilogue's stores share that one
//             mapping), and linear order is the mask 0x1FF with the per-row masks below.  The comment at Deal has the ids and how
//             they are dealt; the host entry chooses the order by shape (order_of).
//   bits      for finite operands both orders give the same bits, algo 0's: every accumulator takes the same non-zero products in
//             the same order; what linear order adds is MFMAs whose B operand is all zeros, that is products +-0 added to an
//             accumulator that started at +0 and can never be -0 (an fp16 product is exact in fp32, and a sum that cancels exactly
//             is +0 in round-to-nearest), and x + (+-0) = x.  What differs: a non-finite weight at a tap that is off the board for a
//             position reaches that position in linear order (0 x Inf = NaN) and not in board order.
//   items     a launch is G = min(round width, work ids) workgroups; workgroup g runs the ids g, g + G, ... in ascending order
//             (board order: the last, partial round from workgroup G - 1 downwards), statically, depending on no other workgroup.
//             A full item with a full item behind it stages that item's first seven
//             half-tiles from its own last two K tiles, in the slots that would stage nothing, so the staging stream does not
//             stop between two main loops and only the wave-private epilogue lies between them (main_loop, `chained`).  The
//             workgroup's last full item ends drained: behind its last barrier it decodes the half item's rows, if one follows,
//             issues that item's whole prologue and only then runs its own epilogue (finish_item has the order and the counts).
//
// The operands are swapped in the MFMA (A = weights, B = activations) so that a lane's accumulator registers run along the
// channels: four consecutive channels of one position per register group, one ds_write_b64 each.
//
// This translation unit includes nothing from CK and nothing of the project but the C header: it is its own object (GNUmakefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/elf_amd.h"


namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kTileM = 256;                      // positions per workgroup
constexpr int kTileN = 256;                      // output channels per workgroup
constexpr int kThreads = 512;
constexpr int kOperandBytes = 256 * 128;         // one operand of one K tile: 256 rows x 64 fp16
constexpr int kBufBytes = 2 * kOperandBytes;     // activations, then weights
constexpr int kWaveCBytes = 4096;                // a wave's own piece of the epilogue: 32 positions x 64 channels fp16
constexpr int kLdsBytes = 2 * kBufBytes + 8 * kWaveCBytes;   // two K tiles and the eight waves' epilogue pieces: 160 KiB, all a CU has

typedef __attribute__((address_space(3))) void* lptr_t;
typedef __amdgpu_buffer_rsrc_t rsrc_t;

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
constexpr uint32_t kRsrcWord3 = 0x00020000u;   // a raw buffer of dwords on gfx9: DATA_FORMAT 32, no swizzle, no index
__host__ __device__ inline uint32_t x_bias(int W, int Cin) { return (uint32_t)(W + 1) * (uint32_t)(Cin * 2); }
// the scalar byte offset of K tile (tap, kc): from a row's own position in x (bias included), and from the start of a weight row
__host__ __device__ inline uint32_t x_soffset(int W, int Cin, int tap, int kc) {
  const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
  return (uint32_t)((dy * W + dx) * Cin * 2 + kc * 128) + x_bias(W, Cin);
}
__host__ __device__ inline uint32_t w_soffset(int Cin, int tap, int kc) { return (uint32_t)(tap * Cin * 2 + kc * 128); }
// does the buffer form take the shape?  (every scalar offset of x below 2^30)
inline bool bufstage_takes(int wd, int c) { return (2 * (int64_t)wd + 3) * c * 2 < ((int64_t)1 << 30); }

// 64 lanes x 16 B: lane l's 16 bytes land at lds_base + 16 * l (the destination is wave-uniform, the source offset per lane)
__device__ __forceinline__ void stage16(rsrc_t r, uint32_t voff, uint32_t soff, char* lds_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lptr_t)lds_base, 16, (int)voff, (int)soff, 0, 0);
}

// the counted wait of the main loop: at most kN of this wave's LDS-DMA loads (two per staged half-tile, in issue order) are
// still in flight behind it; with kLgkm the wave's own ds_reads have retired too
template <int kN, bool kLgkm>
__device__ __forceinline__ void wait_staged() {
  if constexpr (kLgkm) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(kN) : "memory");
  else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kN) : "memory");
}
// the loop's barrier is the bare instruction: __syncthreads() would fence, and the fence waits for every LDS-DMA in flight
__device__ __forceinline__ void raw_barrier() {
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int kV> struct Mode { static constexpr int v = kV; };
// s_setprio in the main loop.  0: every wave raises its priority for its MFMA segments (shipped); the other two are what the probe
// timed against it: 1 none, 2 the static form, waves 4..7 at priority 1 for the whole loop.
#ifndef ELFNET_CONV3X3_PRIO
#define ELFNET_CONV3X3_PRIO 0
#endif
// The lane id, made opaque: what is derived from it (fragment and epilogue addresses) is then computed where it is used, per item,
// and not hoisted out of the loop over a workgroup's items to be kept in registers across its main loops.
__device__ __forceinline__ int fresh(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
// The same for a wave-uniform value
__device__ __forceinline__ int fresh_uniform(int v) {
  asm volatile("" : "+s"(v));
  return v;
}

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
__device__ __forceinline__ uint32_t div_by(uint32_t n, Recip r) { return __umulhi(n + 1, r.mul) >> r.shift; }
// the same quotient where the host plans with it too (the deal below); on the device n is wave-uniform there
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

// What a wave knows about itself and the launch: everything the staging and the epilogue address by.
struct Ctx {
  char* lds;
  rsrc_t xr, wr;                 // the raw buffer descriptors of x (starting bias bytes in front of it) and w
  uint32_t bias;                 // x_bias(W, Cin)
  int M, H, W, Cin, K, relu;
  int stride;                    // positions between two rows of an item: 1 (linear order) or H W (board order)
  Recip dhw, dw;                 // the decode's divisions by H W and by W
  int lane, wv;                  // wv through readfirstlane: what depends on the wave alone stays in scalar registers
};
// The rows a staging lane feeds, decoded once per work item: the vector offsets of its four activation rows (kSentinel for a row at
// or beyond the item's limit) and four weight rows, and, in linear order, the 9-bit tap masks of the activation rows.
struct Rows { uint32_t xoff[4], woff[4], xmask[4]; };

// ---- staging.  A K tile is staged as four half-tiles of 128 rows, in the order the fragment reads need them:
//   Xa  activation rows of the waves' position sub-tiles 0 and 1 (rows wm * 128 + 0..63)      Wa  weight rows of channel
//   Xb  ... of sub-tiles 2 and 3 (rows wm * 128 + 64..127)                                    sub-tile 0 (wn * 64 + 0..31)
//                                                                                             Wb  ... of sub-tile 1 (+ 32..63)
// Every wave issues two 8-row pieces of each half-tile (i = 0, 1): a lane is row (lane >> 3) of its piece and LDS slot
// (lane & 7) of that row.  Index hf * 2 + i below.
// The half tile (kNT == 1) has one weight half-tile per K tile, Wh: its 128 weight rows, LDS row = channel - kbase, wave (wm, wn)
// reads rows wn * 32 + fr; piece i of wave wv is rows i * 64 + wv * 8 .. + 7 (woff[0..1]).
template <int kNT, bool kBoard>
__device__ __forceinline__ void decode_rows(const Ctx& c, Rows& rw, const Item& it) {
  const int lane = c.lane, wv = c.wv, kbase = it.kbase;
  const uint32_t hw = (uint32_t)(c.H * c.W), wd = (uint32_t)c.W;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int hf = j >> 1, i = j & 1;
    const int r = i * 128 + hf * 64 + wv * 8 + (lane >> 3);
    const int p = it.base + r * c.stride;   // the one mapping of (item, row) to a position; load_skip and epilogue have it too
    // tap 3 ky + kx is on the board iff row hh + ky - 1 and column ww + kx - 1 are: the rows' three bits stand at 0, 3 and 6, the
    // columns' at 0, 1 and 2, and their product has bit 3 ky + kx set iff both are (no carries: the column mask is below 8)
    // (board order: every tap the item visits is on the board for all its rows, no mask)
    if constexpr (!kBoard) {
      const uint32_t rem = (uint32_t)p - div_by((uint32_t)p, c.dhw) * hw, hh = div_by(rem, c.dw), ww = rem - hh * wd;
      const uint32_t rowm = (hh > 0 ? 1u : 0u) | 8u | ((int)hh + 1 < c.H ? 64u : 0u);
      const uint32_t colm = (ww > 0 ? 1u : 0u) | 2u | ((int)ww + 1 < c.W ? 4u : 0u);
      uint32_t m = __umul24(rowm, colm);
      asm("" : "+v"(m));   // made for every row and selected, with no branch around the arithmetic for the rows at or beyond the limit
      rw.xmask[j] = r < it.limit ? m : 0u;
    } else {
      rw.xmask[j] = 0u;
    }
    uint32_t off = (uint32_t)p * (uint32_t)(c.Cin * 2) + (((lane & 7) ^ ((r >> 1) & 7)) << 4);   // below 2^31 for a valid row
    asm("" : "+v"(off));   // as the mask: made for every row, then selected
    rw.xoff[j] = r < it.limit ? off : kSentinel;
    const int rwt = kNT == 2 ? (i * 2 + (wv >> 2)) * 64 + hf * 32 + (wv & 3) * 8 + (lane >> 3) : i * 64 + wv * 8 + (lane >> 3);
    rw.woff[j] = (uint32_t)(kbase + rwt) * (uint32_t)(9 * c.Cin * 2) + (((lane & 7) ^ ((rwt >> 1) & 7)) << 4);
  }
}
// the scalar offset of K tile (tap, kc) in x (bias included) and in w: wave-uniform
__device__ __forceinline__ uint32_t x_delta(const Ctx& c, int tap, int kc) {
  const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
  return (uint32_t)((dy * c.W + dx) * c.Cin * 2 + kc * 128) + c.bias;   // x_soffset(c.W, c.Cin, tap, kc)
}
__device__ __forceinline__ uint32_t w_delta(const Ctx& c, int tap, int kc) { return w_soffset(c.Cin, tap, kc); }
// piece i of one half-tile of the K tile at tap `tap` and scalar offset d (x_delta, w_delta) into buffer buf; the two pieces of a
// half-tile are issued in the order i = 0, 1.  Board order: the row's offset as it is.  Linear order: the sentinel where the tap is
// off the board for the row (one select).
template <bool kBoard>
__device__ __forceinline__ void stage_x_piece(const Ctx& c, const Rows& rw, int hf, int i, int tap, uint32_t d, int buf) {
  uint32_t v = rw.xoff[hf * 2 + i];
  if constexpr (!kBoard) v = ((rw.xmask[hf * 2 + i] >> tap) & 1) ? v : kSentinel;
  stage16(c.xr, v, d, c.lds + buf * kBufBytes + (i * 128 + hf * 64 + c.wv * 8) * 128);
}
template <int kNT>
__device__ __forceinline__ void stage_w_piece(const Ctx& c, const Rows& rw, int hf, int i, uint32_t d, int buf) {
  stage16(c.wr, rw.woff[hf * 2 + i], d,
          c.lds + buf * kBufBytes + kOperandBytes +
              (kNT == 2 ? (i * 2 + (c.wv >> 2)) * 64 + hf * 32 + (c.wv & 3) * 8 : i * 64 + c.wv * 8) * 128);
}
// both pieces of a half-tile, back to back: the prologue's form
template <bool kBoard>
__device__ __forceinline__ void stage_x(const Ctx& c, const Rows& rw, int hf, int tap, int kc, int buf) {
  const uint32_t d = x_delta(c, tap, kc);
#pragma unroll
  for (int i = 0; i < 2; ++i) stage_x_piece<kBoard>(c, rw, hf, i, tap, d, buf);
}
template <int kNT>
__device__ __forceinline__ void stage_w(const Ctx& c, const Rows& rw, int hf, int tap, int kc, int buf) {
  const uint32_t d = w_delta(c, tap, kc);
#pragma unroll
  for (int i = 0; i < 2; ++i) stage_w_piece<kNT>(c, rw, hf, i, d, buf);
}
// K tiles t + 1 and t + 2 of a work item, carried in scalars through its loop
struct KPos { int tap0, tap1, kc1, tap2, kc2; };
__device__ __forceinline__ KPos first_kpos(int kchunks, int mask) {
  const int t0 = first_tap(mask);
  KPos k{t0, t0, 1, t0, 2};
  if (kchunks == 1) { k.tap1 = next_tap(mask, t0); k.kc1 = 0; k.tap2 = next_tap(mask, k.tap1); k.kc2 = 0; }
  else if (kchunks == 2) { k.tap2 = next_tap(mask, t0); k.kc2 = 0; }
  return k;
}
// An item's prologue, issue only: Xa Wa Wb Xb of K tile 0 and Xa Wa Wb of K tile 1 (seven half-tiles, 14 loads per wave; the half
// tile: Xa Wh Xb, Xa Wh, five and 10).  Its wait is wait_staged<kFly> (+ what was issued behind it) and a barrier.
template <int kNT, bool kBoard>
__device__ __forceinline__ void issue_prologue(const Ctx& c, const Rows& rw, int kchunks, int mask) {
  const KPos k = first_kpos(fresh_uniform(kchunks), mask);   // K tile 1's tap and chunk are made here, per item, not kept
  stage_x<kBoard>(c, rw, 0, k.tap0, 0, 0); stage_w<kNT>(c, rw, 0, k.tap0, 0, 0);
  if constexpr (kNT == 2) stage_w<kNT>(c, rw, 1, k.tap0, 0, 0);
  stage_x<kBoard>(c, rw, 1, k.tap0, 0, 0);
  stage_x<kBoard>(c, rw, 0, k.tap1, k.kc1, 1); stage_w<kNT>(c, rw, 0, k.tap1, k.kc1, 1);
  if constexpr (kNT == 2) stage_w<kNT>(c, rw, 1, k.tap1, k.kc1, 1);
}

// The main loop of one work item: 256 positions x kNT * 128 output channels (kNT = 2: the full tile, 1: the half tile) over all
// of K, into acc.  Entered with the item's prologue issued, waited for and behind its barrier.  Comments are written for the full
// tile; the half tile's differences stand at the `kNT == 1` branches.
// The full tile's loop also takes what the chain needs (the comment at `chained` below): par, the LDS buffer of the item's K tile
// 0; stores, whether the item before it on this workgroup left 16 stores per lane behind its carried pieces; and, with kChain (a
// full item follows this full item on the workgroup), that item's tile and first channel: it decodes that item's rows, stages its
// first seven half-tiles and leaves its rows in rw.  The two kinds of full item are two copies of the loop, and the kernel runs
// its chained items in a loop of their own: with both ends behind one steady loop this compiler allocates the accumulators twice
// and spills some 400 registers.
template <int kNT, bool kChain, bool kBoard>
__device__ __forceinline__ void main_loop(const Ctx& c, Rows& rw, floatx16 (&acc)[4][kNT], int par, bool stores, int mask,
                                          const Item& nit) {
  static_assert(kNT == 2 || !kChain, "only a full item is chained");
  Rows rn;   // the next item's rows (kChain)
  char* const lds = c.lds;
  const int lane = c.lane, wv = c.wv;
  // ---- fragments: lane (fr = lane & 31, fh = lane >> 5) holds row fr of a 32-row MFMA tile and 8 of the 16 k of one MFMA
  const int wm = wv >> 2, wn = wv & 3;
  const int fr = lane & 31, fh = lane >> 5;
  const int sw = (fr >> 1) & 7;                  // the tiles start at multiples of 32 rows: (row >> 1) & 7 is the lane's own
  const int xrow = (wm * 128 + fr) * 128;                      // + mt * 4096
  const int wrow = kOperandBytes + (wn * 32 * kNT + fr) * 128;   // + nt * 4096
  // Which 8 channels a lane half feeds to which MFMA is algo 0's: CK gives half fh of the wave the channels 16 fh .. 16 fh + 15 of
  // a 32-channel block and spends them in two MFMAs, so MFMA s of block j sums channels 32 j + 8 s + {0..7} and + {16..23}.
  int cs[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) cs[kk] = (((kk >> 1) * 4 + fh * 2 + (kk & 1)) ^ sw) << 4;
  auto ldx = [&](const char* b, int mt, int kk) { return *(const half8*)(b + xrow + mt * 4096 + cs[kk]); };
  auto ldw = [&](const char* b, int nt, int kk) { return *(const half8*)(b + wrow + nt * 4096 + cs[kk]); };

  // The full tile's K tile 0 is a copy of its own in front of the loop, and there the compiler folds these zeros into the first MFMA
  // of every accumulator as its C operand (C = 0: +0 plus the products, the same bits): no v_mov_b32 is left of them.  The half
  // tile's stay 64 v_mov_b32.
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mt][nt][e] = 0.0f;

  // K tile t lives in LDS buffer t & 1 and is spent in two halves of the wave's 128 x 64, each a load segment and
  // an MFMA segment with a bare s_barrier behind every segment:
  //   L1  reads Xa, Wa, Wb of K tile t (16 ds_read_b128)                                    ends: vmcnt(6) lgkmcnt(0) barrier
  //   M1  16 MFMAs: acc[0..1][0..1] over the whole BK = 64; stages Xb(t + 1) among them     ends: barrier
  //   L2  reads Xb(t) over Xa (8 ds_read_b128)                                              ends: vmcnt(2) lgkmcnt(0) barrier
  //   M2  16 MFMAs: acc[2..3][0..1]; stages Xa, Wa, Wb of t + 2 among them                  ends: barrier
  // Every accumulator still takes its K in ascending order.  Waves 4..7 (the second wave of every SIMD) pass one barrier more
  // before the loop and waves 0..3 one more behind it, so the two waves of a SIMD run one segment apart: one issues its MFMAs while
  // the other reads and waits, and the matrix pipe does not stand still while both fetch.
  // The LDS-DMA pieces are issued from the MFMA segments, one at a time between two MFMAs (kM1At, kM2At: after which MFMA of the
  // segment; a sched_barrier on both sides keeps each where it is written): an issue costs the wave far less among MFMAs than in
  // a segment that also carries the fragment reads, and there it is in the MFMAs' shadow, while in a load segment it made the
  // slot longer for all eight waves.  The issue order is what it was: Xa Wa Wb Xb of a K tile.
  // Slots (a slot is what lies between two barriers; early = waves 0..3, late = waves 4..7, one slot behind):
  //   slot      4t          4t+1        4t+2        4t+3        4t+4        4t+5
  //   early     L1(t)       M1(t)       L2(t)       M2(t)       L1(t+1)     M1(t+1)
  //             r XaWaWb(t) s Xb(t+1)   r Xb(t)     s XaWaWb(t+2)
  //   late      M2(t-1)     L1(t)       M1(t)       L2(t)       M2(t)       L1(t+1)
  //             s XaWaWb(t+1) r XaWaWb(t) s Xb(t+1) r Xb(t)     s XaWaWb(t+2)
  // By the counts (a wave's loads retire in issue order, two per half-tile), for waves that may be one barrier apart:
  //   landed   what a load segment reads was waited for, by every wave, in its load segment before: there are two barriers
  //            between a wave's wait and its own next load segment, so at least one between anybody's wait and anybody's read.
  //            L1(t)'s wait is for Xb(t), read in L2(t): the wave has issued up to Wb(t+1) (in M2(t-1), or in the prologue), that
  //            is Xa, Wa, Wb of t + 1 behind it: 3 half-tiles, vmcnt(6).  L2(t)'s wait is for Xa, Wa, Wb of t + 1, read in
  //            L1(t+1): issued up to Xb(t+1) (in M1(t)), one half-tile behind them: vmcnt(2).  A half-tile has three slots to land in.
  //   free     a half-tile is restaged from the second segment after the load segment that read it (lgkmcnt(0) in front of that
  //            one's barrier): Xb(t-1), read in L2(t-1) (slots 4t-2 and 4t-1), is restaged in M1(t) (slots 4t+1 and 4t+2);
  //            Xa, Wa, Wb of t, read in L1(t) (slots 4t and 4t+1), are restaged in M2(t) (slots 4t+3 and 4t+4).  The closest pair
  //            is the late half's read and the early half's restaging: two barriers apart.
  // So the loop never drains the queue.  The last but one K tile stages Xb of the last in its M1 and nothing in its M2, the last
  // nothing: the last but one waits as every tile before it (6, 2), the last for everything in its L1 (0; nothing is left for L2).
  // The half tile (kNT == 1) is the same loop with one weight half-tile, issue order Xa Wh Xb per K tile:
  //   L1  reads Xa, Wh of K tile t (12 ds_read_b128)   M1  8 MFMAs: acc[0..1][0]; stages Xb(t + 1)
  //   L2  reads Xb(t) over Xa (8)                      M2  8 MFMAs: acc[2..3][0]; stages Xa, Wh of t + 2
  // The segments, their barriers and the stagger are those above, so landed and free hold by the same barrier counts: neither
  // depends on how long an MFMA segment is.  The counts: L1(t) waits for Xb(t) with Xa, Wh of t + 1 behind it, vmcnt(4); L2(t)
  // waits for Xa, Wh of t + 1 with Xb(t+1) behind them, vmcnt(2); the last K tile 0.
  // The prologue's issue (Xa Wa Wb Xb of K tile 0, Xa Wa Wb of K tile 1) is what M1 and M2 of K tiles -2 and -1 would have issued,
  // and its wait (kernel entry, finish_item) is for the first three with four behind them, as before.
  constexpr int kWaitL1 = 2 * (1 + kNT), kWaitL2 = 2;   // loads in flight behind the counted waits: 6 (4), and 2
  constexpr int kM1At[2] = {4 * kNT - 1, 6 * kNT - 1};                                        // 7, 11 (3, 5)
  constexpr int kM2At[6] = {2 * kNT - 1, 2 * kNT + 1, 2 * kNT + 3, kNT == 2 ? 9 : 6, 11, 13};   // 3, 5, 7, 9, 11, 13 (1, 3, 5, 6)
  // the item's K tiles: its mask's taps, ascending, kchunks each; 9 kchunks in linear order, down to 2 in board order (the host
  // entry refuses a shape with an item of one K tile)
  const int kchunks = c.Cin >> 6, ktiles = __builtin_popcount((unsigned)mask) * kchunks;
  half8 xf[2][4], wa[4], wb[kNT == 2 ? 4 : 1];
  KPos k = first_kpos(kchunks, mask);
  auto wfrag = [&](int nt, int kk) -> half8 {
    if constexpr (kNT == 2) return nt ? wb[kk] : wa[kk];
    else return wa[kk];
  };

  // An MFMA segment: the 8 kNT MFMAs of acc[2 kSeg .. 2 kSeg + 1][..] with that segment's kP staging pieces between them
  auto mseg = [&](auto seg, auto pieces, int cur, int tap, uint32_t dx, uint32_t dw) {
    constexpr int kSeg = decltype(seg)::v, kP = decltype(pieces)::v;
#if ELFNET_CONV3X3_PRIO == 0
    __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          acc[2 * kSeg + m][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wfrag(nt, kk), xf[m][kk], acc[2 * kSeg + m][nt], 0, 0, 0);
          const int at = (kk * kNT + nt) * 2 + m;
#pragma unroll
          for (int p = 0; p < kP; ++p)
            if (at == (kSeg == 0 ? kM1At[p] : kM2At[p])) {
              __builtin_amdgcn_sched_barrier(0);
              if constexpr (kSeg == 0) stage_x_piece<kBoard>(c, rw, 1, p, tap, dx, cur ^ 1);
              else if (p < 2) stage_x_piece<kBoard>(c, rw, 0, p, tap, dx, cur);
              else stage_w_piece<kNT>(c, rw, (p - 2) >> 1, p & 1, dw, cur);
              __builtin_amdgcn_sched_barrier(0);
            }
        }
#if ELFNET_CONV3X3_PRIO == 0
    __builtin_amdgcn_s_setprio(0);
#endif
    __builtin_amdgcn_sched_barrier(0);
    raw_barrier();
  };

  // One K tile.  kP1, kP2: the pieces M1 and M2 stage (2 or 0; 2 + 2 kNT or 0), from rw at (tap1, kc1) and (tap2, kc2); kW1, kW2:
  // the counts of its two waits; first = 1: K tile 0 of a full item (the waits below, the next item's decode), 2: the last but one
  // K tile of a chained item (the turn below).  tc is the tile's index in the workgroup's chain of K tiles: its buffer is tc & 1.
  auto ktile = [&](auto p1, auto p2, auto w1, auto w2, auto first, int tc, int tap1, int kc1, int tap2, int kc2) {
    constexpr int kP1 = decltype(p1)::v, kP2 = decltype(p2)::v, kW1 = decltype(w1)::v, kW2 = decltype(w2)::v;
    constexpr bool kFirst = (decltype(first)::v & 1) != 0, kTurn = (decltype(first)::v & 2) != 0;
    const int cur = tc & 1;
    const char* b = lds + cur * kBufBytes;
    // the pieces' scalar offsets are made here, in a load segment, so that among the MFMAs a piece is the m0 write and the load
    // (linear order: and the select of the row's offset or the sentinel)
    uint32_t dx1 = 0, dx2 = 0, dw2 = 0;
    if constexpr (kP1 != 0) dx1 = x_delta(c, tap1, kc1);
    if constexpr (kP2 != 0) { dx2 = x_delta(c, tap2, kc2); dw2 = w_delta(c, tap2, kc2); }
    asm volatile("" : "+s"(dx1), "+s"(dx2), "+s"(dw2));
    // L1
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      wa[kk] = ldw(b, 0, kk);
      xf[0][kk] = ldx(b, 0, kk);
      xf[1][kk] = ldx(b, 1, kk);
      if constexpr (kNT == 2) wb[kk] = ldw(b, 1, kk);
    }
    // The fragment registers pass through an empty statement in front of the segment's wait.  A buffer load counts on vmcnt alone
    // (the flat form it replaces counted on lgkmcnt too, out of order, and the compiler answered that with one lgkmcnt(0) per MFMA
    // segment), so the compiler now counts the ds_reads exactly and would put a counted lgkmcnt wait in front of every MFMA that
    // takes a new fragment, fourteen more per K tile, each satisfied long before by the wait below.  This way its one wait stands
    // here, and the registers are the statement's results behind it.
    asm volatile("" : "+v"(xf[0][0]), "+v"(xf[0][1]), "+v"(xf[0][2]), "+v"(xf[0][3]), "+v"(xf[1][0]), "+v"(xf[1][1]), "+v"(xf[1][2]),
                      "+v"(xf[1][3]), "+v"(wa[0]), "+v"(wa[1]), "+v"(wa[2]), "+v"(wa[3]));
    if constexpr (kNT == 2) asm volatile("" : "+v"(wb[0]), "+v"(wb[1]), "+v"(wb[2]), "+v"(wb[3]));
    // K tile 0 behind a carried transition: the 16 stores of the item before are younger than the pieces this wait leaves in
    // flight and older than nothing it waits for, so they are added to the count; a lane may have issued fewer where that item's
    // tile had rows at or beyond M, and then the steady count, which is right for no store at all and stronger otherwise
    if (kFirst && stores) wait_staged<kW1 + 8 * kNT, true>();
    else wait_staged<kW1, true>();
    raw_barrier();
    // M1
    mseg(Mode<0>{}, p1, cur, tap1, dx1, 0);
    // L2
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      xf[0][kk] = ldx(b, 2, kk);
      xf[1][kk] = ldx(b, 3, kk);
    }
    // the next item's rows, decoded here once per item, in the load segment with the longest wait at its barrier; nothing is
    // staged from them before M2 of the item's last but one K tile
    if constexpr (kFirst && kChain) decode_rows<2, kBoard>(c, rn, nit);
    // the turn: M1 of the item's last but one K tile was the last to stage from the item's own rows, and everything from this
    // tile's M2 on is staged from the next item's, which become rw here
    if constexpr (kTurn) rw = rn;
    asm volatile("" : "+v"(xf[0][0]), "+v"(xf[0][1]), "+v"(xf[0][2]), "+v"(xf[0][3]), "+v"(xf[1][0]), "+v"(xf[1][1]), "+v"(xf[1][2]),
                      "+v"(xf[1][3]));   // as in L1
    if (kFirst && stores) wait_staged<kW2 + 8 * kNT, true>();
    else wait_staged<kW2, true>();
    raw_barrier();
    // M2
    mseg(Mode<1>{}, p2, cur, tap2, dx2, dw2);
  };
  auto next_k = [&]() {
    k.tap1 = k.tap2; k.kc1 = k.kc2;
    if (++k.kc2 == kchunks) { k.kc2 = 0; k.tap2 = next_tap(mask, k.tap2); }
  };
  const Mode<2> kX{};                 // M1's pieces: Xb
  const Mode<2 + 2 * kNT> kXW{};      // M2's: Xa, Wa, Wb (Xa, Wh)
  const Mode<0> kNone{};
  const Mode<kWaitL1> kL1{};
  const Mode<kWaitL2> kL2{};
  const int late = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8);   // waves 4..7: the second wave of every SIMD
  auto leave = [&]() {
#if ELFNET_CONV3X3_PRIO == 2
    __builtin_amdgcn_s_setprio(0);
#endif
    if (!late) raw_barrier();
  };
  if (late) raw_barrier();
#if ELFNET_CONV3X3_PRIO == 2
  if (late) __builtin_amdgcn_s_setprio(1);
#endif
  if constexpr (kNT == 1) {
    for (int t = 0; t < ktiles - 2; ++t) {
      ktile(kX, kXW, kL1, kL2, kNone, t, k.tap1, k.kc1, k.tap2, k.kc2);
      next_k();
    }
    ktile(kX, kNone, kL1, kL2, kNone, ktiles - 2, k.tap1, k.kc1, 0, 0);   // the last but one: waits as every tile before it
    ktile(kNone, kNone, kNone, kNone, kNone, ktiles - 1, 0, 0, 0, 0);     // the last: for everything, in its L1
  } else {
    // chained: a full item follows this one on the workgroup.  The staging stream then runs on into it: with T = ktiles, K tile
    // T + j of this item is K tile j of the next, staged from the next item's rows (rn, decoded in L2(0); they become rw in
    // L2(T-2), behind the last piece of the item's own), and the slots that would stage nothing get their pieces back, in the
    // prologue's issue order:
    //   M2(T-2)  Xa Wa Wb of the next item's K tile 0      M1(T-1)  Xb of its K tile 0      M2(T-1)  Xa Wa Wb of its K tile 1
    // So K tiles T - 2 and T - 1 are steady tiles: they wait with 6 and 2, and the queue is never empty between two main loops.
    // The buffer of a K tile is the parity of its index in the chain (tc = par + t): with an odd T the next item starts in the
    // other buffer, and the kernel carries par from item to item.
    //   landed   the steady rule, continued: L2(T-1)'s wait is for Xa, Wa, Wb of tile T (the next item's 0), with Xb(T) of M1(T-1)
    //            behind them: vmcnt(2), by every wave, in front of a barrier; they are read in the next item's L1(0), behind at
    //            least three more barriers (M2(T-1)'s, the stagger's one, the transition's).  The next L1(0)'s wait is for Xb(T),
    //            read in its L2(0): behind it Xa, Wa, Wb of T + 1 (6) and the epilogue's stores (16): vmcnt(22); its L2(0)'s is for
    //            Xa, Wa, Wb of T + 1, read in L1(1): behind them the 16 stores and Xb(T+1) of M1(0): vmcnt(18).  From the next K
    //            tile 1 on the stores are older than whatever is waited for and the steady counts hold.  (The epilogue's own wait
    //            for its bias and skip registers is the compiler's vmcnt(0), which also retires the eight carried loads: these
    //            counts do not rely on it.)
    //   free     M2(T-2), M1(T-1) and M2(T-1) restage what the steady M2, M1, M2 of those tiles restage, read in L1(T-2), L2(T-2)
    //            and L1(T-1): two barriers between the late half's read and the early half's restaging, as above.  The next item's
    //            M1(0) and M2(0) restage Xb of tile T - 1's buffer (read in L2(T-1)) and Xa, Wa, Wb of tile T - 2's (last read
    //            in L1(T-2); as tile T's, in its own L1(0)): the steady distances plus the transition's two barriers.  The
    //            epilogue between them touches only the wave's own 4 KiB behind the K-tile buffers.
    // A full item that is its workgroup's last, or has a half item behind it, ends drained as before: its last but one K tile
    // stages Xb of the last in M1 and nothing in M2, its last nothing and waits with 0.
    // An item of two K tiles (board order, an end of a board one position wide at 64 input channels) has its first K tile for
    // its last but one: that tile is both, and decodes the next item's rows and turns to them in the same L2.
    if (ktiles > 2) {
      ktile(kX, kXW, kL1, kL2, Mode<1>{}, par, k.tap1, k.kc1, k.tap2, k.kc2);
      next_k();
      for (int t = 1; t < ktiles - 2; ++t) {
        ktile(kX, kXW, kL1, kL2, kNone, par + t, k.tap1, k.kc1, k.tap2, k.kc2);
        next_k();
      }
      if constexpr (kChain) {
        const KPos kn = first_kpos(fresh_uniform(kchunks), nit.mask);
        ktile(kX, kXW, kL1, kL2, Mode<2>{}, par + ktiles - 2, k.tap1, k.kc1, kn.tap0, 0);
        ktile(kX, kXW, kL1, kL2, kNone, par + ktiles - 1, kn.tap0, 0, kn.tap1, kn.kc1);
      } else {
        ktile(kX, kNone, kL1, kL2, kNone, par + ktiles - 2, k.tap1, k.kc1, 0, 0);
        ktile(kNone, kNone, kNone, kNone, kNone, par + ktiles - 1, 0, 0, 0, 0);
      }
    } else if constexpr (kChain) {
      const KPos kn = first_kpos(fresh_uniform(kchunks), nit.mask);
      ktile(kX, kXW, kL1, kL2, Mode<3>{}, par, k.tap1, k.kc1, kn.tap0, 0);
      ktile(kX, kXW, kL1, kL2, kNone, par + 1, kn.tap0, 0, kn.tap1, kn.kc1);
    } else {
      ktile(kX, kNone, kL1, kL2, Mode<1>{}, par, k.tap1, k.kc1, 0, 0);
      ktile(kNone, kNone, kNone, kNone, kNone, par + 1, 0, 0, 0, 0);
    }
  }
  leave();
  // Barriers of one item, per wave: the prologue's, 4 per K tile, and the stagger's one (in front of the loop for waves 4..7,
  // behind it for waves 0..3): 4 ktiles + 2 for every wave, so the items of a workgroup stay paired whatever their kind.  Behind
  // the last of them every wave is past its last fragment read: a wave 4..7 arrives there from its last M2, with the lgkmcnt(0) of
  // L2 behind it, and a wave 0..3 has nothing left.  So whoever passes it may stage the next item into both K-tile buffers.
}

// ---- epilogue.  D = W X^T: the lane's column is position fr of an MFMA tile, its register e is channel (e & 3) + 8 (e >> 2) + 4 fh.
// It is wave-private: the wave's own 4 KiB behind the K-tile buffers, no barrier, so it runs while the next item's prologue lands
// in the K-tile buffers.  Four passes, one per mt: 32 positions x 64 channels of this wave (the half tile: x 32) as rows of kC = 8
// (4) chunks of 16 B, the chunk q of position p at chunk q ^ ((p >> 1) & 7) (the half tile: q ^ ((p >> 2) & 3)); written as
// ds_write_b64 by the lane that holds the four channels, lgkmcnt(0), read back as 16 B of consecutive channels per lane, kC lanes
// per position, so a store instruction writes whole 128-B (64-B) runs of y.  Banks, by the lane groups each instruction is served
// in and the 64 banks of 4 B (enumerated on the host from the two formulas below): a ds_write_b64 group is 16
// consecutive positions writing the same half of the same chunk number: the 256-B bank row holds two (four) positions and the XOR
// steps every second (fourth), so the 16 lanes land in 16 different 16-B slots; a ds_read_b128 group is four runs of 4 lanes (or two
// of 8), each run a different position of a different slot quarter: all 64 banks once.
// The epilogue's arithmetic on two fp16 values per register.  BiasResAct's sequence is float(half(acc)) + float(bias), + float(res),
// max(., 0), one rounding to fp16; v_fma_mix_f32 converts its fp16 sources exactly and rounds the fp32 fused multiply-add once, and
// float(h) * 1.0 + c rounded once is float(h) + c rounded once, so one instruction is the conversion (of both operands, for the
// bias) and the addition: the same fp32 value, NaN, infinities, zeros' signs and subnormals included.  kHi: the upper half.
typedef uint32_t uint32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
template <int kHi>
__device__ __forceinline__ float add_h_h(uint32_t a, uint32_t b, Mode<kHi>) {   // float(a.half) + float(b.half)
  float d;
  if constexpr (kHi) asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "v"(b));
  else asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
template <int kHi>
__device__ __forceinline__ float add_h_f(uint32_t a, float c, Mode<kHi>) {      // float(a.half) + c
  float d;
  if constexpr (kHi) asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(a), "v"(c));
  else asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(a), "v"(c));
  return d;
}
// ReLU behind the last rounding, on both halves: rounding to fp16 is monotone and keeps zero, so max(round(v), 0) is
// round(max(v, 0)) for every v that is not NaN, and for NaN both give +0 (the maximum returns the operand that is a number).
// The instruction itself: the compiler's own maximum first canonicalises its operand with a second v_pk_max_f16; volatile, so
// that the uniform branch around it stays a branch and is not turned back into selects.
__device__ __forceinline__ uint32_t relu_h2(uint32_t v) {
  asm volatile("v_pk_max_f16 %0, %0, 0" : "+v"(v));
  return v;
}

template <bool kHasRes, int kNT>
struct Skip { half8 bv; half8 rv[kHasRes ? 8 * kNT : 1]; };

template <int kNT>
struct EpiLane {
  static constexpr int kC = 4 * kNT;           // chunks per row = lanes per position in the read-back
  static constexpr int kPos = 64 / kC;         // positions per read-back instruction
  static constexpr int kR = 32 / kPos;         // read-backs per pass
  int pr, q, chan;                             // the lane's position in a read-back, its chunk, its first channel of the item
  int row0;                                    // the wave's first row of the item
  __device__ __forceinline__ EpiLane(const Ctx& c, int kbase)
      : pr(c.lane / kC), q(c.lane % kC), chan(kbase + (c.wv & 3) * 32 * kNT + (c.lane % kC) * 8), row0((c.wv >> 2) * 128) {}
  static __device__ __forceinline__ int swz(int p) { return kNT == 2 ? (p >> 1) & 7 : (p >> 2) & 3; }
};

// bias and the skip's 16 B per (position, chunk), in the shape the read-back has.  A row at or beyond the item's limit reads the
// tensor's last row instead (no branch around a load) and is not stored.
template <bool kHasRes, int kNT>
__device__ __forceinline__ void load_bias(const Ctx& c, Skip<kHasRes, kNT>& s, const _Float16* __restrict__ bias, const Item& it) {
  const EpiLane<kNT> e(c, it.kbase);
  s.bv = *(const half8*)(bias + e.chan);
}
template <bool kHasRes, int kNT>
__device__ __forceinline__ void load_skip(const Ctx& c, Skip<kHasRes, kNT>& s, const _Float16* __restrict__ res, const Item& it) {
  using E = EpiLane<kNT>;
  const E e(c, it.kbase);
  if constexpr (kHasRes) {
#pragma unroll
    for (int i = 0; i < 4 * E::kR; ++i) {
      const int r = e.row0 + (i / E::kR) * 32 + (i % E::kR) * E::kPos + e.pr;
      s.rv[i] = *(const half8*)(res + (size_t)(r < it.limit ? it.base + r * c.stride : c.M - 1) * c.K + e.chan);
    }
  }
}

// kAll: every row of the item is valid, and every lane issues all its 8 kNT stores (the count the next item's first wait uses).
template <bool kHasRes, int kNT, bool kAll>
__device__ __forceinline__ void epilogue(const Ctx& c, const half4 (&hacc)[4][kNT][4], const Skip<kHasRes, kNT>& s,
                                         _Float16* __restrict__ y, const Item& it) {
  using E = EpiLane<kNT>;
  const E e(c, it.kbase);
  char* const cl = c.lds + 2 * kBufBytes + c.wv * kWaveCBytes;
  const int fr = c.lane & 31, fh = c.lane >> 5;
  constexpr int kRowB = 16 * E::kC;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) *(half4*)(cl + fr * kRowB + (((nt * 4 + g) ^ E::swz(fr)) << 4) + fh * 8) = hacc[mt][nt][g];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own writes; nobody else's are read
    auto readback = [&](int j) {
      const int pos = j * E::kPos + e.pr;
      return *(const uint32x4*)(cl + pos * kRowB + ((e.q ^ E::swz(pos)) << 4));
    };
    // The branch below ends the compiler's own look-ahead, so the next read-back is issued in front of this one's arithmetic by
    // hand: four registers more, which the kernel with the skip does not have (at 254 it spills with them, in any pass).
    constexpr bool ahead = !kHasRes;
    uint32x4 nv;
    if (ahead) nv = readback(0);
#pragma unroll
    for (int j = 0; j < E::kR; ++j) {
      const uint32x4 cv = ahead ? nv : readback(j);
      if (ahead && j + 1 < E::kR) nv = readback(j + 1);
      uint32x4 ov;
      const uint32x4 bv = __builtin_bit_cast(uint32x4, s.bv);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float lo = add_h_h(cv[i], bv[i], Mode<0>{}), hi = add_h_h(cv[i], bv[i], Mode<1>{});
        if constexpr (kHasRes) {
          const uint32_t rv = __builtin_bit_cast(uint32x4, s.rv[mt * E::kR + j])[i];
          lo = add_h_f(rv, lo, Mode<0>{});
          hi = add_h_f(rv, hi, Mode<1>{});
        }
        ov[i] = __builtin_bit_cast(uint32_t, h2_t{(_Float16)lo, (_Float16)hi});
      }
      // a uniform branch around four instructions (the comparison is made here, on the scalar argument: a flag kept across the
      // passes ends up in a VGPR), not a select per element: relu = 0 executes nothing and passes NaN, -0 and negative values
      if (fresh_uniform(c.relu)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ov[i] = relu_h2(ov[i]);
      }
      const int r = e.row0 + mt * 32 + j * E::kPos + e.pr;
      if (kAll || r < it.limit) *(uint32x4*)(y + (size_t)(it.base + r * c.stride) * c.K + e.chan) = ov;
    }
    __builtin_amdgcn_wave_barrier();   // the next pass's writes stay behind this pass's read-backs
  }
}

// The drained end of one item and the start of the next (kNext = 1: a half item follows, 0: nothing; 2, a full item, is written
// out too but no longer used: a full item in front of a full item ends in finish_chained below).  Order:
//   bias and skip loads of this item (1 + 16 plain loads with the skip, 1 without)
//   the next item's rows decoded over this item's (dead since its last staging), its whole prologue issued (14 or 10 LDS-DMA loads)
//   this item's epilogue: four passes, 4 stores each (the half tile: 2)
//   the next item's first wait and barrier
// vmcnt counts loads, LDS-DMA loads and stores together, in issue order.  The waits on this path:
//   the epilogue's passes wait for bias / skip registers only, with counts the compiler places: the loads they wait for are older
//   than the prologue, so nothing of the prologue is waited for (pass mt of a full item with the skip: its four skip loads have
//   the later 12 - 4 mt skip loads, the 14 prologue loads and 4 mt stores behind them: vmcnt(26) every pass);
//   the first wait needs Xa, Wa, Wb of K tile 0: behind them kFly = 8 loads of the prologue (6 for a half item next) and this
//   item's 16 stores: vmcnt(24) (22).  Where the tile has rows at or beyond M a lane may issue fewer stores, and a count that is
//   too high waits for too little: that tile waits with kFly alone, which is right for no store at all and stronger otherwise.
template <bool kHasRes, int kNT, int kNext, bool kBoard>
__device__ __forceinline__ void finish_item(Ctx& c, int lane, Rows& rw, const floatx16 (&acc)[4][kNT], const _Float16* __restrict__ bias,
                                            const _Float16* __restrict__ res, _Float16* __restrict__ y, const Item& it,
                                            const Item& nit) {
  Skip<kHasRes, kNT> s;
  load_bias<kHasRes, kNT>(c, s, bias, it);
  __builtin_amdgcn_sched_barrier(0);
  // the accumulators' first rounding, at once: 64 registers instead of 128 under the skip's 64 and the prologue's addresses
  half4 hacc[4][kNT][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int i = 0; i < 4; ++i) hacc[mt][nt][g][i] = (_Float16)acc[mt][nt][g * 4 + i];
        asm volatile("" : "+v"(hacc[mt][nt][g]));   // converted here, not where it is written out
      }
  c.lane = fresh(lane);   // behind the conversions: no address of what follows is made while all 192 registers are in use
  __builtin_amdgcn_sched_barrier(0);
  load_skip<kHasRes, kNT>(c, s, res, it);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (kNext != 0) {
    decode_rows<kNext, kBoard>(c, rw, nit);
    __builtin_amdgcn_sched_barrier(0);
  }
  // The compiler's wait for the bias and skip registers is made to stand here, in front of the prologue: once LDS-DMA loads are
  // pending it counts nothing and waits with vmcnt(0) for any register a plain load returns, which behind the prologue would be
  // a wait for the prologue.  The conversions and the decode above are what these loads have to return in.  (Nothing is pending
  // here, the item ended drained, so with buffer loads the compiler counts these registers down one by one, vmcnt(16) .. vmcnt(0)
  // with the skip: the same last wait, in the same place.)
  asm volatile("" ::"v"(s.bv));
  if constexpr (kHasRes) {
#pragma unroll
    for (int i = 0; i < 8 * kNT; ++i) asm volatile("" ::"v"(s.rv[i]));
  }
  if constexpr (kNext != 0) {
    issue_prologue<kNext, kBoard>(c, rw, c.Cin >> 6, nit.mask);
    __builtin_amdgcn_sched_barrier(0);
  }
  const bool all = __builtin_amdgcn_readfirstlane(it.limit >= kTileM);
  if (all) epilogue<kHasRes, kNT, true>(c, hacc, s, y, it);
  else epilogue<kHasRes, kNT, false>(c, hacc, s, y, it);
  if constexpr (kNext != 0) {
    constexpr int kFly = 2 * (2 + kNext);
    if (all) wait_staged<kFly + 8 * kNT, false>();
    else wait_staged<kFly, false>();
    raw_barrier();
  }
}

// The end of a full item whose staging stream has run on into the next full item (main_loop, `chained`): nothing of the next item
// is left to do here, its rows are decoded and its first seven half-tiles are issued, eight loads of them still in flight.  Order:
//   the 16 skip loads, directly behind the item's last barrier: the fragment registers are dead, and the skip's miss latency
//   is what this path still exposes; then the bias load, and the conversions, which the loads return under
//   the compiler's wait for the bias and skip registers, made to stand behind the conversions as finish_item does (left to their
//   first uses inside the passes' branches, it comes back as a vmcnt(0) in the next item's first load segment, behind the stores):
//   with LDS-DMA loads pending it is a vmcnt(0), which also retires the eight carried loads, all older than the skip loads
//   the epilogue: four passes, 4 stores each, no wait on vmcnt
//   the transition's barrier, with no wait in front of it: what the next L1(0) reads was waited for in L2 of this item's last K tile
// Returns whether every lane issued all its 16 stores (the next item's first K tile counts them).
template <bool kHasRes>
__device__ __forceinline__ bool finish_chained(Ctx& c, int lane, const floatx16 (&acc)[4][2], const _Float16* __restrict__ bias,
                                               const _Float16* __restrict__ res, _Float16* __restrict__ y, const Item& it) {
  Skip<kHasRes, 2> s;
  c.lane = fresh(lane);
  load_skip<kHasRes, 2>(c, s, res, it);
  __builtin_amdgcn_sched_barrier(0);
  load_bias<kHasRes, 2>(c, s, bias, it);
  __builtin_amdgcn_sched_barrier(0);
  half4 hacc[4][2][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int i = 0; i < 4; ++i) hacc[mt][nt][g][i] = (_Float16)acc[mt][nt][g * 4 + i];
        asm volatile("" : "+v"(hacc[mt][nt][g]));   // converted here, not where it is written out
      }
  c.lane = fresh(lane);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::"v"(s.bv));
  if constexpr (kHasRes) {
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("" ::"v"(s.rv[i]));
  }
  const bool all = __builtin_amdgcn_readfirstlane(it.limit >= kTileM);
  if (all) epilogue<kHasRes, 2, true>(c, hacc, s, y, it);
  else epilogue<kHasRes, 2, false>(c, hacc, s, y, it);
  raw_barrier();
  return all;
}

// One workgroup runs its work ids of the launch one after the other (G = gridDim.x): g, g + G, g + 2 G, ... in ascending order and,
// in board order, the last round from workgroup G - 1 downwards (next_id).  The host entry makes G = min(round width, ids), so
// where the last round is split the full ids are a multiple of G: a workgroup's first item is a full one and a half item, if it
// has one, is its last (at most one: there are at most G half ids; board order has none).
template <bool kHasRes, bool kBoard>
__device__ __forceinline__ void conv_body(const char* __restrict__ x, const char* __restrict__ w, const _Float16* __restrict__ bias,
                                          const _Float16* __restrict__ res, _Float16* __restrict__ y, int M, int H, int W, int Cin,
                                          int K, int relu, const Deal& d, Recip dhw, Recip dw) {
  __shared__ __attribute__((aligned(128))) char lds[kLdsBytes];   // ALL of the kernel's LDS: one array
  const int tid = threadIdx.x;
  Ctx c;
  c.lds = lds; c.M = M; c.H = H; c.W = W; c.Cin = Cin; c.K = K; c.relu = relu; c.dhw = dhw; c.dw = dw;
  c.stride = d.stride;
  c.lane = tid & 63;
  c.wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the two descriptors, from kernel arguments alone: scalar registers.  x's starts bias bytes in front of x and is bias bytes
  // longer (the comment at kSentinel); both sizes are below 2^31 + 2^30
  c.bias = x_bias(W, Cin);
  c.xr = __builtin_amdgcn_make_buffer_rsrc((void*)(x - c.bias), 0, (int)((uint32_t)M * (uint32_t)(Cin * 2) + c.bias), (int)kRsrcWord3);
  c.wr = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, (int)((uint32_t)K * (uint32_t)(9 * Cin * 2)), (int)kRsrcWord3);
  const int G = (int)gridDim.x, g = (int)blockIdx.x, kchunks = Cin >> 6;
  int id = g;
  Item it = item_of(d, id, M, H, W);   // a full item: see above
  Rows rw;
  decode_rows<2, kBoard>(c, rw, it);
  issue_prologue<2, kBoard>(c, rw, kchunks, it.mask);
  wait_staged<8, false>();   // Xa, Wa, Wb of K tile 0; behind them Xb(0), Xa(1), Wa(1), Wb(1)
  raw_barrier();
  // What follows an item is known before its main loop, and is the same for every wave.  While it is a full item the staging
  // stream runs on into it and the item ends in finish_chained; the workgroup's last full item ends drained, in finish_item, with
  // a half item or nothing behind it.  The three ends are uniform branches that do not meet again: each has its own epilogue, so
  // the compiler's counts for the bias and skip registers are those of one path (joined, it would take the path without a
  // prologue and wait for the other paths' prologues).
  const int lane = c.lane;
  int par = 0, nid;
  bool stores = false;
  Item nit = it;
  for (;;) {
    nid = next_id(d, id, g, G);
    if (nid >= d.ids) break;
    nit = item_of(d, nid, M, H, W);
    if constexpr (!kBoard) {   // board order has no half items
      if (__builtin_amdgcn_readfirstlane(nit.half) >= 0) break;
    }
    floatx16 acc[4][2];
    c.lane = fresh(lane);
    main_loop<2, true, kBoard>(c, rw, acc, par, stores, it.mask, nit);
    stores = finish_chained<kHasRes>(c, lane, acc, bias, res, y, it);
    par = (par + __builtin_popcount((unsigned)it.mask) * kchunks) & 1;   // the item's own K tiles
    id = nid;
    it = nit;
  }
  floatx16 acc[4][2];
  c.lane = fresh(lane);
  main_loop<2, false, kBoard>(c, rw, acc, par, stores, it.mask, it);
  if (kBoard || nid >= d.ids) {
    finish_item<kHasRes, 2, 0, kBoard>(c, lane, rw, acc, bias, res, y, it, it);
    return;
  }
  if constexpr (!kBoard) {
    finish_item<kHasRes, 2, 1, kBoard>(c, lane, rw, acc, bias, res, y, it, nit);
    floatx16 acch[4][1];
    c.lane = fresh(lane);
    main_loop<1, false, kBoard>(c, rw, acch, 0, false, nit.mask, nit);
    finish_item<kHasRes, 1, 0, kBoard>(c, lane, rw, acch, bias, res, y, nit, nit);
  }
}
// The two row orders are two kernels of the one body: board order stages every activation piece from its row's offset as it is,
// linear order keeps the rows' tap masks and one select per piece, and only linear order has half items.
template <bool kHasRes>
__global__ __launch_bounds__(kThreads, 2) void k_conv3x3_f16(const char* __restrict__ x, const char* __restrict__ w,
                                                             const _Float16* __restrict__ bias, const _Float16* __restrict__ res,
                                                             _Float16* __restrict__ y, int M, int H, int W, int Cin, int K, int relu,
                                                             Deal d, Recip dhw, Recip dw) {
  conv_body<kHasRes, false>(x, w, bias, res, y, M, H, W, Cin, K, relu, d, dhw, dw);
}
template <bool kHasRes>
__global__ __launch_bounds__(kThreads, 2) void k_conv3x3_f16_boards(const char* __restrict__ x, const char* __restrict__ w,
                                                                    const _Float16* __restrict__ bias, const _Float16* __restrict__ res,
                                                                    _Float16* __restrict__ y, int M, int H, int W, int Cin, int K,
                                                                    int relu, Deal d, Recip dhw, Recip dw) {
  conv_body<kHasRes, true>(x, w, bias, res, y, M, H, W, Cin, K, relu, d, dhw, dw);
}

// The zero-fill probe of elfnet_conv3x3_f16_bufstage_probe: one wave, one staged piece.  1 KiB of LDS at lds_off is filled with
// 0xFF by ds_write, then lane l stages 16 B from voff[l] + soff through a descriptor of `records` bytes at src, and the KiB is
// copied out.
__global__ __launch_bounds__(64) void k_bufstage_probe(const char* __restrict__ src, uint32_t records, const uint32_t* __restrict__ voff,
                                                       uint32_t soff, uint32_t lds_off, uint32x4* __restrict__ out) {
  __shared__ __attribute__((aligned(128))) char lds[kLdsBytes];
  const int lane = threadIdx.x;
  char* const dst = lds + lds_off;   // the host entry keeps it a multiple of 1024 and the KiB inside the array
  *(uint32x4*)(dst + lane * 16) = uint32x4{~0u, ~0u, ~0u, ~0u};
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)records, (int)kRsrcWord3);
  stage16(r, voff[lane], soff, dst);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  out[lane] = *(const uint32x4*)(dst + lane * 16);
}

// the CU count of the current device, asked for once per device
int round_width_of_device() {
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 0; }
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); return 0; }
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// ---- host: the two plans
// the linear order's deal for `width` items at a time (0: one id per workgroup)
Deal linear_deal(int64_t m, int k, int width, int* G) {
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
bool board_takes(int64_t rows, int h, int wd, int c, int k) {
  const int64_t nblk = (rows + kTileM - 1) / kTileM;
  return rows > 0 && !((int64_t)h * wd == 1 && c < 128) && nblk * h * wd * (k / kTileN) < ((int64_t)1 << 30);
}
Deal board_deal(int64_t rows, int h, int wd, int k, int width, int* G) {
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
int64_t board_load(const Deal& d, int g, int G, int h, int wd, int kchunks) {
  int64_t sum = 0;
  for (int id = g; id < d.ids; id = next_id(d, id, g, G))
    sum += (int64_t)__builtin_popcount((unsigned)item_of(d, id, 0, h, wd).mask) * kchunks;
  return sum;
}
// The order the plain entry takes for a shape at `width` items a round: board order iff there are at least 256 rows and its most
// loaded workgroup has strictly fewer K tiles than the linear order's, which is its full rounds x 9 kchunks plus a last round of
// 9 kchunks, or of 3/4 of that where it is split (a half tile takes 0.75 of a tile's time: profiles/conv_tail_probe.json).
// Compared in quarters of a K tile.  Host arithmetic, the same on every call of a shape; the last answer is kept per thread.
int order_of(int64_t rows, int h, int wd, int c, int k, int width) {
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

// The entry point behind elfnet_conv3x3_f16_width(algo = 1) and elfnet_conv3x3_f16_boards; net_conv.hip has checked pointers,
// alignment and the size limits (every tensor below 2^31 bytes) and set the device.  One launch on `stream`: no allocation, no
// memset, no synchronisation, no copy.  Shapes the kernel does not take are refused with nothing launched.
// round_width is how many work items run at a time, 0 for the device's CU count (one workgroup per CU).
// order: 0 the linear order, 1 board order, -1 whichever order_of names for the shape (the comment at Deal has both).
// Linear: with total = tiles x columns and r = total % width, the last round is split iff total >= width and 0 < 2 r <= width:
// total + r work ids, the last r items as two half tiles each (work_item); otherwise total ids.  The launch is a 1-D grid of
// min(width, ids) workgroups, each running every width-th id (a width above the ids, or an unknown CU count: one id per workgroup).
// Board: B x H W x columns ids, no half tiles, the same grid.
extern "C" __attribute__((visibility("hidden"))) int elfnet_conv3x3_native_f16(const void* x, const void* w, const void* bias,
                                                                               const void* res, void* y, int64_t rows, int h, int wd,
                                                                               int c, int k, int relu, int round_width, int order,
                                                                               hipStream_t stream) {
  if ((c & 63) != 0 || (k & 255) != 0 || round_width < 0 || order < -1 || order > 1) return ELFGO_E_BADARG;
  if (order == 1 && !board_takes(rows, h, wd, c, k)) return ELFGO_E_BADARG;
  if (!bufstage_takes(wd, c)) return ELFGO_E_BADARG;   // a board some 2^27 / c positions wide: the comment at kSentinel
  const int64_t m = rows * h * wd;
  const int width = round_width > 0 ? round_width : round_width_of_device();
  if (order < 0) order = order_of(rows, h, wd, c, k, width);
  int G = 0;
  const Deal d = order ? board_deal(rows, h, wd, k, width, &G) : linear_deal(m, k, width, &G);
  const dim3 grid((unsigned)G);
  const Recip dhw = recip_of((uint32_t)(h * wd)), dw = recip_of((uint32_t)wd);   // h * wd <= m, below 2^31
  const auto kern = order ? (res ? k_conv3x3_f16_boards<true> : k_conv3x3_f16_boards<false>)
                          : (res ? k_conv3x3_f16<true> : k_conv3x3_f16<false>);
  hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, stream, (const char*)x, (const char*)w, (const _Float16*)bias,
                     (const _Float16*)res, (_Float16*)y, (int)m, h, wd, c, k, relu, d, dhw, dw);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// Host arithmetic only: the board-order launch of elfnet_conv3x3_f16_boards for a shape and round_width > 0.  Returns its work
// ids; with id >= 0 also what that id computes: its block of 256 boards, its board position h * W + w, its channel column and its
// 9-bit tap mask (bit 3 ky + kx: the tap is on the board).
extern "C" int64_t elfnet_conv3x3_f16_boards_plan(int64_t rows, int h, int wd, int k, int round_width, int64_t id, int* block,
                                                  int* position, int* column, int* mask) {
  if (rows <= 0 || h <= 0 || wd <= 0 || k <= 0 || (k & 255) != 0 || round_width <= 0 || !board_takes(rows, h, wd, 128, k))
    return ELFGO_E_BADARG;
  int G = 0;
  const Deal d = board_deal(rows, h, wd, k, round_width, &G);
  if (id >= 0) {
    if (id >= d.ids) return ELFGO_E_BADARG;
    int b = 0, hw = 0;
    const Item it = item_of(d, (int)id, 0, h, wd, &b, &hw);
    if (block) *block = b;
    if (position) *position = hw;
    if (column) *column = it.kbase / kTileN;
    if (mask) *mask = it.mask;
  }
  return d.ids;
}

// Host arithmetic only: the deal of that launch.  g < 0: the number of workgroups G.  Otherwise the work id that workgroup g runs
// as its j-th item (j from 0), or -1 where it has fewer.
extern "C" int64_t elfnet_conv3x3_f16_boards_deal(int64_t rows, int h, int wd, int k, int round_width, int g, int j) {
  const int64_t ids = elfnet_conv3x3_f16_boards_plan(rows, h, wd, k, round_width, -1, nullptr, nullptr, nullptr, nullptr);
  if (ids < 0) return ids;
  int G = 0;
  const Deal d = board_deal(rows, h, wd, k, round_width, &G);
  if (g < 0) return G;
  if (g >= G || j < 0) return ELFGO_E_BADARG;
  int id = g;
  for (; j > 0 && id < d.ids; --j) id = next_id(d, id, g, G);
  return id < d.ids ? id : -1;
}

// Host arithmetic only: the K tiles (one tap x 64 input channels of one item) workgroup g of that launch runs through, at c input
// channels: the sum of popcount(mask) * c / 64 over its items.
extern "C" int64_t elfnet_conv3x3_f16_boards_load(int64_t rows, int h, int wd, int c, int k, int round_width, int g) {
  const int64_t G = elfnet_conv3x3_f16_boards_deal(rows, h, wd, k, round_width, -1, 0);
  if (G < 0) return G;
  if (c <= 0 || (c & 63) != 0 || g < 0 || g >= G || !board_takes(rows, h, wd, c, k)) return ELFGO_E_BADARG;
  int G2 = 0;
  const Deal d = board_deal(rows, h, wd, k, round_width, &G2);
  return board_load(d, g, G2, h, wd, c >> 6);
}

// The order elfnet_conv3x3_f16(algo 1) takes for a shape: 0 linear, 1 board (order_of).  round_width 0: at the current device's
// CU count, as the plain entry (an unknown count: linear); above 0: host arithmetic only, at that width.
extern "C" int elfnet_conv3x3_f16_order(int64_t rows, int h, int wd, int c, int k, int round_width) {
  if (rows < 0 || h <= 0 || wd <= 0 || c <= 0 || k <= 0 || (c & 63) != 0 || (k & 255) != 0 || round_width < 0) return ELFGO_E_BADARG;
  if (rows * h * wd * (int64_t)(c > k ? c : k) >= ((int64_t)1 << 30)) return ELFGO_E_BADARG;
  return order_of(rows, h, wd, c, k, round_width > 0 ? round_width : round_width_of_device());
}

// Host arithmetic only: how elfnet_conv3x3_f16_width lays a launch of tiles x columns work items out for round_width > 0.
extern "C" int64_t elfnet_conv3x3_f16_plan(int64_t tiles, int columns, int round_width, int64_t id, int* tile, int* column, int* half) {
  if (tiles <= 0 || columns <= 0 || round_width <= 0 || tiles * columns >= ((int64_t)1 << 30)) return ELFGO_E_BADARG;
  const int64_t total = tiles * columns;
  const int nfull = full_items(total, round_width);
  const int64_t groups = 2 * total - nfull;
  if (tile || column || half) {
    if (id < 0 || id >= groups) return ELFGO_E_BADARG;
    const WorkItem wi = work_item((int)id, (int)tiles, nfull);
    if (tile) *tile = wi.tile;
    if (column) *column = wi.col;
    if (half) *half = wi.half;
  }
  return groups;
}

// Host arithmetic only: the multiplier and the shift the kernel divides a position by `divisor` with (recip_of): for every
// 0 <= n < 2^31, n / divisor == (((n + 1) * mul) >> 32) >> shift, the product in 64 bits.
extern "C" int elfnet_conv3x3_f16_recip(int64_t divisor, uint32_t* mul, uint32_t* shift) {
  if (divisor < 1 || divisor > ((int64_t)1 << 31) || !mul || !shift) return ELFGO_E_BADARG;
  const Recip r = recip_of((uint32_t)divisor);
  *mul = r.mul;
  *shift = r.shift;
  return 0;
}

// Host arithmetic only: what the kernel's buffer-addressed staging addresses a shape by (the comment at kSentinel; the kernel calls
// the same functions).  bias: how far x's descriptor starts in front of x; x_records, w_records: the two descriptors' num_records;
// sentinel: the vector offset of a lane that stages zeros.  With 0 <= tap < 9 and 0 <= kc < c / 64 also the scalar offsets of K
// tile (tap, kc); tap < 0: the shape's values alone.  The vector offset of position p's 16-byte chunk q is p * c * 2 + 16 q in x,
// that of output channel n's is n * 9 * c * 2 + 16 q in w.  Refuses what the launch refuses.
extern "C" int elfnet_conv3x3_f16_bufstage(int64_t rows, int h, int wd, int c, int k, int tap, int kc, uint32_t* bias,
                                           uint32_t* x_records, uint32_t* w_records, uint32_t* sentinel, uint32_t* x_soff,
                                           uint32_t* w_soff) {
  if (rows <= 0 || h <= 0 || wd <= 0 || c <= 0 || k <= 0 || (c & 63) != 0 || (k & 255) != 0 || tap >= 9) return ELFGO_E_BADARG;
  if (rows * h * wd * (int64_t)(c > k ? c : k) >= ((int64_t)1 << 30) || (int64_t)k * 9 * c >= ((int64_t)1 << 30)) return ELFGO_E_BADARG;
  if (!bufstage_takes(wd, c) || (tap >= 0 && (kc < 0 || kc >= (c >> 6)))) return ELFGO_E_BADARG;
  const uint32_t b = x_bias(wd, c);
  if (bias) *bias = b;
  if (x_records) *x_records = (uint32_t)(rows * h * wd) * (uint32_t)(c * 2) + b;
  if (w_records) *w_records = (uint32_t)k * (uint32_t)(9 * c * 2);
  if (sentinel) *sentinel = kSentinel;
  if (tap >= 0) {
    if (x_soff) *x_soff = x_soffset(wd, c, tap, kc);
    if (w_soff) *w_soff = w_soffset(c, tap, kc);
  }
  return 0;
}

// One staged piece of one wave, for the test of what the hardware does with a lane that is out of range: 1 KiB of LDS at byte
// lds_offset (a multiple of 1024, below 160 KiB) is filled with 0xFF, lane l stages 16 bytes from voffset[l] + soffset through a
// raw buffer descriptor of `records` bytes at src with the kernel's own instruction, and the KiB is copied to out.  src, voffset
// (64 x uint32) and out (1 KiB) are device memory; every voffset[l] + soffset + 16 that is at most `records` must lie inside src's
// allocation.  One launch on `stream`, nothing else.
extern "C" int elfnet_conv3x3_f16_bufstage_probe(const void* src, uint32_t records, const void* voffset, uint32_t soffset,
                                                 uint32_t lds_offset, void* out, void* stream) {
  if (!src || !voffset || !out || (lds_offset & 1023u) != 0 || lds_offset > (uint32_t)(kLdsBytes - 1024)) return ELFGO_E_BADARG;
  if ((((uintptr_t)src | (uintptr_t)out) & 15) != 0 || ((uintptr_t)voffset & 3) != 0) return ELFGO_E_BADARG;
  hipLaunchKernelGGL(k_bufstage_probe, dim3(1), dim3(64), 0, (hipStream_t)stream, (const char*)src, records,
                     (const uint32_t*)voffset, soffset, lds_offset, (uint32x4*)out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// Host arithmetic only: the workgroups of that launch.  Workgroup g runs the work ids g, g + G, g + 2 G, ... of the plan.
extern "C" int64_t elfnet_conv3x3_f16_grid(int64_t tiles, int columns, int round_width) {
  const int64_t ids = elfnet_conv3x3_f16_plan(tiles, columns, round_width, 0, nullptr, nullptr, nullptr);
  return ids < 0 ? ids : round_width < ids ? round_width : ids;
}
