// The host arithmetic of elfnet_conv3x3_f16's algo 1 as the C ABI exports it: how a launch is laid out in either row order, the
// rule that chooses the order, the division multipliers and the staging's byte offsets, over the functions of net_conv3x3_plan.h
// that the kernel and its host entry (net_conv3x3.hip) go by.  No kernel is defined here and nothing is launched; the CPU tests
// enumerate these.  Its own object (GNUmakefile).
#include "net_conv3x3_plan.h"

namespace {

// The board-order launch of elfnet_conv3x3_f16_boards for a shape and round_width > 0: its deal and its workgroups, or false for
// a shape the three entries below refuse.
bool boards_launch(int64_t rows, int h, int wd, int k, int round_width, Deal* d, int* G) {
  if (rows <= 0 || h <= 0 || wd <= 0 || k <= 0 || (k & 255) != 0 || round_width <= 0 || !board_takes(rows, h, wd, 128, k))
    return false;
  *d = board_deal(rows, h, wd, k, round_width, G);
  return true;
}

}  // namespace

// Host arithmetic only: the board-order launch of elfnet_conv3x3_f16_boards for a shape and round_width > 0.  Returns its work
// ids; with id >= 0 also what that id computes: its block of 256 boards, its board position h * W + w, its channel column and its
// 9-bit tap mask (bit 3 ky + kx: the tap is on the board).
extern "C" int64_t elfnet_conv3x3_f16_boards_plan(int64_t rows, int h, int wd, int k, int round_width, int64_t id, int* block,
                                                  int* position, int* column, int* mask) {
  Deal d;
  int G = 0;
  if (!boards_launch(rows, h, wd, k, round_width, &d, &G)) return ELFGO_E_BADARG;
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
  Deal d;
  int G = 0;
  if (!boards_launch(rows, h, wd, k, round_width, &d, &G)) return ELFGO_E_BADARG;
  if (g < 0) return G;
  if (g >= G || j < 0) return ELFGO_E_BADARG;
  int id = g;
  for (; j > 0 && id < d.ids; --j) id = next_id(d, id, g, G);
  return id < d.ids ? id : -1;
}

// Host arithmetic only: the K tiles (one tap x 64 input channels of one item) workgroup g of that launch runs through, at c input
// channels: the sum of popcount(mask) * c / 64 over its items.
extern "C" int64_t elfnet_conv3x3_f16_boards_load(int64_t rows, int h, int wd, int c, int k, int round_width, int g) {
  Deal d;
  int G = 0;
  if (!boards_launch(rows, h, wd, k, round_width, &d, &G)) return ELFGO_E_BADARG;
  if (c <= 0 || (c & 63) != 0 || g < 0 || g >= G || !board_takes(rows, h, wd, c, k)) return ELFGO_E_BADARG;
  return board_load(d, g, G, h, wd, c >> 6);
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

// Host arithmetic only: the workgroups of that launch.  Workgroup g runs the work ids g, g + G, g + 2 G, ... of the plan.
extern "C" int64_t elfnet_conv3x3_f16_grid(int64_t tiles, int columns, int round_width) {
  const int64_t ids = elfnet_conv3x3_f16_plan(tiles, columns, round_width, 0, nullptr, nullptr, nullptr);
  return ids < 0 ? ids : round_width < ids ? round_width : ids;
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
