// elfnet_conv3x3_f16's algo 1: the trunk convolution y = relu?(conv3x3_same(x, w) + bias (+ res)) as a hand-written implicit GEMM,
// fp16 NHWC in and out, w as [K,3,3,C], fp32 accumulation in v_mfma_f32_32x32x16_f16.  Nothing is unfolded, no workspace.
//
// Why beside CK's kernel (net_conv.hip, algo 0): that one is a 256 x 128 x 32 tile with one LDS stage and two barriers per 32-deep
// K step, and sits on that structure's ceiling.  Here:
//   tile      256 positions x 256 output channels x BK 64 (one tap, 64 consecutive input channels); all of N in one tile, so an
//             activation byte is staged once for every output channel.  512 threads, 8 waves as 2 (positions) x 4 (channels), each
//             owning 128 positions x 64 channels = 4 x 2 MFMA tiles = 128 accumulator registers.  One workgroup per CU.
//   staging   LDS-DMA (global_load_lds_dwordx4) straight into two 64-KiB LDS buffers (activation tile, weight tile: 256 rows of
//             128 B each), in half-tiles of 128 rows of one operand, two 8-row pieces per wave; four half-tiles stay in flight
//             across the loop's barriers, which are bare s_barriers behind counted vmcnt waits (the comment at the main loop has
//             the counts).  vmcnt(0) only once the last half-tile is on its way.  Every staged piece is a full aligned 128-B
//             line: 8 lanes per row.
//   halo      a staging lane decodes its four rows once (position -> n, h, w) and keeps a 9-bit tap mask and a byte offset; for an
//             off-board tap, and for a row at or beyond M, its source address is a zero-filled line in global memory.  LDS is never
//             zeroed by a second path.
//   LDS image lane-linear, as the DMA writes it; the 16-B slot s of row r holds the row's chunk s ^ ((r >> 1) & 7): the XOR is on
//             the source address when staging and on the read address of the fragment ds_read_b128s, which are then conflict-free
//             (rows r and r + 1 share a 256-B bank row, so the swizzle steps every second row; checked against the 16-lane groups
//             ds_read_b128 is served in).
//   K order   tap-major (ky, kx, then c ascending); inside a 32-channel block the two MFMAs take channels {0..7, 16..23} and
//             {8..15, 24..31}, as CK's blockwise GEMM hands them out: algo 0's accumulation chain per output element, bit for bit.
//   epilogue  accumulators -> fp16 -> LDS (the staging buffers, reused) -> 16 B of consecutive channels per lane; bias and res are
//             read in that shape, and the sequence is BiasResAct's of net_conv.hip: float(half(acc)) + bias (+ res), max(., 0), one
//             rounding to fp16.  Rows at or beyond M are not stored.
//   tail      the work items of a launch (position tiles x channel columns of 256) run in rounds of one per CU.  Where the last
//             round is at most half full, each of its items is launched as two workgroups of 256 positions x 128 channels (the
//             half tile: the same waves at 128 x 32 each, three staged half-tiles per K tile instead of four), so that round takes
//             a half tile's time.  Same kernel, same launch, same K chain per output element: the bits do not change.  The host
//             entry decides (full_items below); a launch that is not split is the 2-D grid it always was.
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
constexpr int kLdsBytes = 2 * kBufBytes;         // two K tiles: 128 KiB, and exactly the 256 x 256 fp16 C tile of the epilogue

// the line every off-board tap and every row beyond M is staged from
__device__ __attribute__((aligned(128))) unsigned char g_zero_line[128] = {0};

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// 64 lanes x 16 B: lane l's 16 bytes land at lds_base + 16 * l (the destination is wave-uniform, the source per lane)
__device__ __forceinline__ void stage16(const char* src, char* lds_base) {
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)lds_base, 16, 0, 0);
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

// Workgroup id -> work.  Work items are numbered tiles fastest, then channel column; ids below nfull are one full item each, and
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

// One work item: 256 positions from tile * 256 on, x kNT * 128 output channels from kbase on (kNT = 2: the full tile, 1: the half
// tile).  Comments are written for the full tile; the half tile's differences stand at the `kNT == 1` branches.
template <bool kHasRes, int kNT>
__device__ __forceinline__ void conv_tile(char* lds, const char* __restrict__ x, const char* __restrict__ w,
                                          const _Float16* __restrict__ bias, const _Float16* __restrict__ res,
                                          _Float16* __restrict__ y, int M, int H, int W, int Cin, int K, int relu, int tile,
                                          int kbase) {
  // wv through readfirstlane: the compiler then keeps everything that depends on the wave alone (LDS destinations, weight rows)
  // in scalar registers, off the vector pipe the MFMAs issue through
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- staging.  A K tile is staged as four half-tiles of 128 rows, in the order the fragment reads need them:
  //   Xa  activation rows of the waves' position sub-tiles 0 and 1 (rows wm * 128 + 0..63)      Wa  weight rows of channel
  //   Xb  ... of sub-tiles 2 and 3 (rows wm * 128 + 64..127)                                    sub-tile 0 (wn * 64 + 0..31)
  //                                                                                             Wb  ... of sub-tile 1 (+ 32..63)
  // Every wave issues two 8-row pieces of each half-tile (i = 0, 1): a lane is row (lane >> 3) of its piece and LDS slot
  // (lane & 7) of that row.  Index hf * 2 + i below.
  // The half tile has one weight half-tile per K tile, Wh: its 128 weight rows, LDS row = channel - kbase, wave (wm, wn) reads rows
  // wn * 32 + fr; piece i of wave wv is rows i * 64 + wv * 8 .. + 7 (woff[0..1]).
  uint32_t xoff[4], woff[4], xmask[4];
  const unsigned char* zsrc = g_zero_line + (lane & 7) * 16;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int hf = j >> 1, i = j & 1;
    const int r = i * 128 + hf * 64 + wv * 8 + (lane >> 3);
    const int p = tile * kTileM + r;
    uint32_t m = 0;
    if (p < M) {
      const int rem = p % (H * W), hh = rem / W, ww = rem - hh * W;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        if ((unsigned)(hh + dy) < (unsigned)H && (unsigned)(ww + dx) < (unsigned)W) m |= 1u << tap;
      }
    }
    xmask[j] = m;
    xoff[j] = (uint32_t)p * (uint32_t)(Cin * 2) + (((lane & 7) ^ ((r >> 1) & 7)) << 4);   // below 2^31 wherever it is used (p < M)
    const int rw = kNT == 2 ? (i * 2 + (wv >> 2)) * 64 + hf * 32 + (wv & 3) * 8 + (lane >> 3) : i * 64 + wv * 8 + (lane >> 3);
    woff[j] = (uint32_t)(kbase + rw) * (uint32_t)(9 * Cin * 2) + (((lane & 7) ^ ((rw >> 1) & 7)) << 4);
  }
  // the two pieces of one half-tile of K tile (tap, kc) into buffer buf
  auto stage_x = [&](int hf, int tap, int kc, int buf) {
    const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
    const uint32_t d = (uint32_t)((dy * W + dx) * Cin * 2 + kc * 128);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      stage16(((xmask[hf * 2 + i] >> tap) & 1) ? x + (uint32_t)(xoff[hf * 2 + i] + d) : (const char*)zsrc,
              lds + buf * kBufBytes + (i * 128 + hf * 64 + wv * 8) * 128);
  };
  auto stage_w = [&](int hf, int tap, int kc, int buf) {
    const uint32_t d = (uint32_t)(tap * Cin * 2 + kc * 128);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      stage16(w + (uint32_t)(woff[hf * 2 + i] + d),
              lds + buf * kBufBytes + kOperandBytes +
                  (kNT == 2 ? (i * 2 + (wv >> 2)) * 64 + hf * 32 + (wv & 3) * 8 : i * 64 + wv * 8) * 128);
  };

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

  floatx16 acc[4][kNT];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mt][nt][e] = 0.0f;

  // ---- main loop.  K tile t lives in LDS buffer t & 1 and is spent in two halves of the wave's 128 x 64, each a load segment and
  // an MFMA segment with a bare s_barrier behind every segment:
  //   L1  reads Xa, Wa, Wb of K tile t (16 ds_read_b128)   stages Xb(t + 1)                 ends: vmcnt(8) lgkmcnt(0) barrier
  //   M1  16 MFMAs: acc[0..1][0..1] over the whole BK = 64                                  ends: barrier
  //   L2  reads Xb(t) over Xa (8 ds_read_b128)             stages Xa, Wa, Wb of t + 2       ends: vmcnt(8) lgkmcnt(0) barrier
  //   M2  16 MFMAs: acc[2..3][0..1]                                                         ends: barrier
  // Every accumulator still takes its K in ascending order.  Waves 4..7 (the second wave of every SIMD) pass one barrier more
  // before the loop and waves 0..3 one more behind it, so the two waves of a SIMD run one segment apart: one issues its MFMAs while
  // the other reads, stages and waits, and the matrix pipe does not stand still while both fetch.
  // By the counts (a wave's loads retire in issue order, two per half-tile, half-tiles in the order Xa Wa Wb Xb of a K tile), for
  // waves that may be one barrier apart:
  //   landed   what a load segment reads was waited for, by every wave, in its load segment before: there are two barriers
  //            between a wave's wait and its own next load segment, so at least one between anybody's wait and anybody's read.
  //            L1(t)'s wait is for Xb(t), read in L2(t): the wave has issued up to Xb(t+1), that is Xa, Wa, Wb, Xb of t + 1 behind
  //            it: 4 half-tiles, vmcnt(8).  L2(t)'s wait is for Xa, Wa, Wb of t + 1, read in L1(t+1): issued up to Wb(t+2), that
  //            is Xb(t+1), Xa, Wa, Wb of t + 2 behind them: vmcnt(8) again.
  //   free     a half-tile is restaged one load segment after the one that read it (lgkmcnt(0) in front of that one's barrier), two
  //            barriers later for the wave itself and at least one for a wave that runs behind: Xb(t-1), read in L2(t-1), is
  //            restaged in L1(t); Xa, Wa, Wb of t, read in L1(t), are restaged in L2(t).
  // So four half-tiles (64 KiB) are in flight across every barrier, each for a whole K tile of MFMAs, and the loop never drains
  // the queue; the last two K tiles issue nothing new and count it down (8, 2, then 0 in the last K tile's L1).
  // The half tile (kNT == 1) is the same loop with one weight half-tile, issue order Xa Wh Xb per K tile:
  //   L1  reads Xa, Wh of K tile t (12 ds_read_b128)   stages Xb(t + 1)          M1  8 MFMAs: acc[0..1][0]
  //   L2  reads Xb(t) over Xa (8)                      stages Xa, Wh of t + 2    M2  8 MFMAs: acc[2..3][0]
  // The segments, their barriers and the stagger are those above, so landed and free hold by the same barrier counts: neither
  // depends on how long an MFMA segment is.  The counts: L1(t) waits for Xb(t) with Xa, Wh, Xb of t + 1 issued behind it, three
  // half-tiles, vmcnt(6); L2(t) waits for Xa, Wh of t + 1 with Xb(t+1), Xa, Wh of t + 2 behind them, vmcnt(6) again; the prologue
  // issues Xa Wh Xb of tile 0 and Xa Wh of tile 1 and waits for the first two: vmcnt(6).  The last but one K tile: 6 in L1 (it
  // still stages Xb of the last tile), 2 in L2 (only that Xb is behind Xa, Wh of the last tile); the last: 0 in L1.
  constexpr int kFly = 2 * (2 + kNT);   // two loads per half-tile x half-tiles in flight behind a counted wait: 8, or 6
  const int kchunks = Cin >> 6, ktiles = 9 * kchunks;   // at least 9
  half8 xf[2][4], wa[4], wb[kNT == 2 ? 4 : 1];
  int tap1 = 0, kc1 = 1, tap2 = 0, kc2 = 2;             // K tiles t + 1 and t + 2
  if (kchunks == 1) { tap1 = 1; kc1 = 0; tap2 = 2; kc2 = 0; }
  else if (kchunks == 2) { tap2 = 1; kc2 = 0; }
  stage_x(0, 0, 0, 0); stage_w(0, 0, 0, 0);
  if constexpr (kNT == 2) stage_w(1, 0, 0, 0);
  stage_x(1, 0, 0, 0);
  stage_x(0, tap1, kc1, 1); stage_w(0, tap1, kc1, 1);
  if constexpr (kNT == 2) stage_w(1, tap1, kc1, 1);
  wait_staged<kFly, false>();   // Xa, Wa, Wb of K tile 0; behind them Xb(0), Xa(1), Wa(1), Wb(1)
  raw_barrier();

  // mode 0: a K tile with two more behind it; 1: the last but one; 2: the last
  auto ktile = [&](auto mode, int t) {
    constexpr int kMode = decltype(mode)::v;
    const int cur = t & 1, nxt = cur ^ 1;
    const char* b = lds + cur * kBufBytes;
    // L1
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      wa[kk] = ldw(b, 0, kk);
      xf[0][kk] = ldx(b, 0, kk);
      xf[1][kk] = ldx(b, 1, kk);
      if constexpr (kNT == 2) wb[kk] = ldw(b, 1, kk);
    }
    if constexpr (kMode <= 1) stage_x(1, tap1, kc1, nxt);
    wait_staged<kMode == 2 ? 0 : kFly, true>();
    raw_barrier();
    // M1
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa[kk], xf[0][kk], acc[0][0], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa[kk], xf[1][kk], acc[1][0], 0, 0, 0);
      if constexpr (kNT == 2) {
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wb[kk], xf[0][kk], acc[0][1], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wb[kk], xf[1][kk], acc[1][1], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    raw_barrier();
    // L2
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      xf[0][kk] = ldx(b, 2, kk);
      xf[1][kk] = ldx(b, 3, kk);
    }
    if constexpr (kMode == 0) {
      stage_x(0, tap2, kc2, cur); stage_w(0, tap2, kc2, cur);
      if constexpr (kNT == 2) stage_w(1, tap2, kc2, cur);
    }
    wait_staged<kMode == 0 ? kFly : kMode == 1 ? 2 : 0, true>();
    raw_barrier();
    // M2
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      acc[2][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa[kk], xf[0][kk], acc[2][0], 0, 0, 0);
      acc[3][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa[kk], xf[1][kk], acc[3][0], 0, 0, 0);
      if constexpr (kNT == 2) {
        acc[2][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wb[kk], xf[0][kk], acc[2][1], 0, 0, 0);
        acc[3][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wb[kk], xf[1][kk], acc[3][1], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    raw_barrier();
  };
  const int late = __builtin_amdgcn_readfirstlane(tid >> 8);   // waves 4..7: the second wave of every SIMD
  if (late) raw_barrier();
  for (int t = 0; t < ktiles - 2; ++t) {
    ktile(Mode<0>{}, t);
    tap1 = tap2; kc1 = kc2;
    if (++kc2 == kchunks) { kc2 = 0; ++tap2; }
  }
  ktile(Mode<1>{}, ktiles - 2);
  ktile(Mode<2>{}, ktiles - 1);
  if (!late) raw_barrier();

  // ---- epilogue.  D = W X^T: the lane's column is position fr of the tile, its register e is channel (e & 3) + 8 (e >> 2) + 4 fh.
  // C tile in LDS: [256 positions][256 channels] fp16, the 16-B chunk q of position p at chunk q ^ (p & 31).
  __syncthreads();   // the last K tile's fragment reads are done in every wave
  // The half tile's C tile is [256][128]: 256-B rows, the chunk q of position p at chunk q ^ (p & 15), in the first 64 KiB.
  // Banks (the lane groups and bank widths each instruction is served in): a ds_read_b128 group of 16 lanes is 16 chunks of one
  // position (full tile) or 8 + 8 chunks of positions p, p + 1 with p even (half tile: q ^ p and q ^ (p + 1) differ in bit 0 only,
  // and both lane sets are closed under that flip), so it covers all 64 banks once; a ds_write_b64 group is 16 consecutive
  // positions writing the same half of the same chunk number, which the XOR spreads over 16 chunks: every one of the 16 banks
  // that half can reach is used twice, in the half tile as in the full one (enumerated on the host from the two formulas below).
  constexpr int kRowB = kNT * 256, kCm = kNT * 16 - 1;          // bytes per C row; chunk mask
  constexpr int kQs = kNT == 2 ? 5 : 4, kIts = kNT * 8;         // lanes per row = 1 << kQs; passes of 512 >> kQs rows
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) {
      const int pos = wm * 128 + mt * 32 + fr;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ch = wn * 32 * kNT + nt * 32 + g * 8 + fh * 4;
        half4 hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) hv[e] = (_Float16)acc[mt][nt][g * 4 + e];
        *(half4*)(lds + pos * kRowB + (((ch >> 3) ^ (pos & kCm)) << 4) + ((ch >> 2) & 1) * 8) = hv;
      }
    }
  const int q = tid & kCm;
  const half8 bv = *(const half8*)(bias + kbase + q * 8);
  if constexpr (kHasRes) {
    // the skip's 16 B per (position, chunk) are requested before the barrier, now that the accumulators' registers are free: they
    // arrive while the waves meet.  A row beyond M reads the last valid row instead (no branch around a load) and is not stored.
    half8 rv[kIts];
#pragma unroll
    for (int it = 0; it < kIts; ++it) {
      const int p = tile * kTileM + (it << (9 - kQs)) + (tid >> kQs);
      rv[it] = *(const half8*)(res + (size_t)(p < M ? p : M - 1) * K + kbase + q * 8);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kIts; ++it) {
      const int pos = (it << (9 - kQs)) + (tid >> kQs);
      const int p = tile * kTileM + pos;
      const half8 cv = *(const half8*)(lds + pos * kRowB + ((q ^ (pos & kCm)) << 4));
      half8 ov;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = (float)cv[e];
        v += (float)bv[e];
        v += (float)rv[it][e];
        if (relu) v = fmaxf(v, 0.0f);
        ov[e] = (_Float16)v;
      }
      if (p < M) *(half8*)(y + (size_t)p * K + kbase + q * 8) = ov;
    }
  } else {
    __syncthreads();
#pragma unroll 4
    for (int it = 0; it < kIts; ++it) {
      const int pos = (it << (9 - kQs)) + (tid >> kQs);
      const int p = tile * kTileM + pos;
      if (p < M) {
        const half8 cv = *(const half8*)(lds + pos * kRowB + ((q ^ (pos & kCm)) << 4));
        half8 ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = (float)cv[e];
          v += (float)bv[e];
          if (relu) v = fmaxf(v, 0.0f);
          ov[e] = (_Float16)v;
        }
        *(half8*)(y + (size_t)p * K + kbase + q * 8) = ov;
      }
    }
  }
}

template <bool kHasRes>
__global__ __launch_bounds__(kThreads, 2) void k_conv3x3_f16(const char* __restrict__ x, const char* __restrict__ w,
                                                             const _Float16* __restrict__ bias, const _Float16* __restrict__ res,
                                                             _Float16* __restrict__ y, int M, int H, int W, int Cin, int K, int relu,
                                                             int tiles, int nfull) {
  __shared__ __attribute__((aligned(128))) char lds[kLdsBytes];   // ALL of the kernel's LDS: one array
  // The workgroup's id is in scalar registers, so this branch is uniform; an unsplit launch (nfull = every item) is the 2-D grid
  // of tiles x columns, whose linear id is the item.  The half tile leaves by a return of its own: as if / else the two bodies met
  // in one exit block, and the compiler, which then sees a path from the half tile's epilogue into the full tile, put an
  // s_waitcnt vmcnt(0) between the full tile's prologue and its loop (with res), draining the four half-tiles in flight there.
  const WorkItem wi = work_item((int)(blockIdx.y * gridDim.x + blockIdx.x), tiles, nfull);
  if (__builtin_amdgcn_readfirstlane(wi.half) >= 0) {
    conv_tile<kHasRes, 1>(lds, x, w, bias, res, y, M, H, W, Cin, K, relu, wi.tile, wi.col * kTileN + wi.half * (kTileN / 2));
    return;
  }
  conv_tile<kHasRes, 2>(lds, x, w, bias, res, y, M, H, W, Cin, K, relu, wi.tile, wi.col * kTileN);
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

}  // namespace

// The entry point behind elfnet_conv3x3_f16_width(algo = 1); net_conv.hip has checked pointers, alignment and the size limits (every
// tensor below 2^31 bytes) and set the device.  One launch on `stream`: no allocation, no memset, no synchronisation, no copy.
// Shapes the kernel does not take are refused with nothing launched.
// round_width is how many work items run at a time, 0 for the device's CU count (one workgroup per CU).  With total = tiles x
// columns and r = total % width, the last round is split iff total >= width and 0 < 2 r <= width: a 1-D grid of total + r
// workgroups, the last r items as two half tiles each (work_item).  Otherwise the launch is the 2-D grid of tiles x columns.
extern "C" __attribute__((visibility("hidden"))) int elfnet_conv3x3_native_f16(const void* x, const void* w, const void* bias,
                                                                               const void* res, void* y, int64_t rows, int h, int wd,
                                                                               int c, int k, int relu, int round_width,
                                                                               hipStream_t stream) {
  if ((c & 63) != 0 || (k & 255) != 0 || round_width < 0) return ELFGO_E_BADARG;
  const int64_t m = rows * h * wd;
  const int tiles = (int)((m + kTileM - 1) / kTileM), cols = k / kTileN;
  const int64_t total = (int64_t)tiles * cols;       // below 2^31: m * k is below 2^30
  const int width = round_width > 0 ? round_width : round_width_of_device();
  const int nfull = width > 0 ? full_items(total, width) : (int)total;
  const dim3 grid = nfull < total ? dim3((unsigned)(2 * total - nfull)) : dim3((unsigned)tiles, (unsigned)cols);
  if (res)
    hipLaunchKernelGGL(k_conv3x3_f16<true>, grid, dim3(kThreads), 0, stream, (const char*)x, (const char*)w, (const _Float16*)bias,
                       (const _Float16*)res, (_Float16*)y, (int)m, h, wd, c, k, relu, tiles, nfull);
  else
    hipLaunchKernelGGL(k_conv3x3_f16<false>, grid, dim3(kThreads), 0, stream, (const char*)x, (const char*)w, (const _Float16*)bias,
                       (const _Float16*)nullptr, (_Float16*)y, (int)m, h, wd, c, k, relu, tiles, nfull);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
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
