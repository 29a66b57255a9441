// elfnet_conv3x3_bf16_big: the bf16 trunk convolution y = relu?(conv3x3_same(x, w) + bias (+ res)) of net_conv3x3_bf16.hip on a
// workgroup tile of 256 positions x 256 output channels, for calls large enough to give every CU such a tile: x, res and y bf16
// NHWC, w bf16 [K,3,3,C], bias bf16 [K], fp32 accumulation in v_mfma_f32_32x32x16_bf16.
//
// Why beside the 64- and 128-tiles of net_conv3x3_bf16.hip: with K = 256 the 128-tile stages every activation byte twice, once
// per channel column, a wave owns only 64 x 64, and each K tile costs it 16 ds_read_b128 for 16 MFMAs.  Here all of K = 256 is in
// one tile, an activation byte is staged once for every output channel, and a wave reads 24 ds_read_b128 for 32 MFMAs.  This is
// the geometry of the fp16 kernel's first step (net_conv3x3.hip) with the arithmetic of the bf16 file; none of algo 1's later
// rounds (work plans, board order, chained items, half tiles) is here.
//
//   tile      256 positions x 256 output channels x BK 64 (a K tile is one tap and 64 consecutive input channels).  512 threads =
//             8 waves as 2 (positions) x 4 (channels); a wave owns 128 x 64 = 4 x 2 MFMA tiles = 128 accumulator registers of the
//             256 it has.  The grid is ceil(M / 256) x K / 256: one work item per workgroup, one workgroup per CU.
//   staging   LDS-DMA (global_load_lds_dwordx4), 16 B per lane.  A stage is the activation tile, then the weight tile, 256 rows of
//             128 B each: 64 KiB; the ring has TWO, 128 KiB.  A K tile is pieces of 8 rows, every piece a full aligned 128-B line
//             per 8 lanes; a wave issues four pieces of each operand.  K tile t + 1 is staged right behind the barrier of K tile t,
//             behind the first fragment reads, and lands while t's MFMAs run.  The loop has ONE bare s_barrier per K tile behind a
//             counted vmcnt wait (the comment at the main loop has the count), and no __syncthreads().
//   halo      a staging lane decodes its four rows once (position -> h, w) and keeps a 9-bit tap mask and a byte offset per row;
//             for an off-board tap, and for a row at or beyond M, its source address is this file's zero-filled 128-B line in
//             global memory.  LDS is never zeroed by a second path.
//   LDS image lane-linear, as the DMA writes it; the 16-B slot s of row r holds the row's chunk s ^ ((r >> 1) & 7), the XOR on the
//             source address when staging and on the address of the fragment ds_read_b128s.
//   K order   tap-major (ky, kx, then c ascending: MFMA kk of a K tile sums channels 16 kk .. 16 kk + 15); one fp32 accumulator
//             per output from zero; no split-K, no atomics.  That is the chain of the 64- and 128-tiles, and the epilogue's
//             arithmetic is theirs: for finite operands the output is BIT-EQUAL to elfnet_conv3x3_bf16_tile(..., 128, ...).
//   epilogue  ONE rounding: acc + bias (+ res) in fp32, fmaxf(., 0) when relu is set (a NaN becomes 0), one round-to-nearest-even
//             to bf16.  The accumulators go as fp32, one MFMA tile (4 KiB) at a time, through the wave's own region of the stage
//             that the last K tile is NOT in, and come back as 8 consecutive channels per lane, so a store instruction writes
//             64-B runs of y.  Rows at or beyond M are not stored.  No workgroup barrier: a wave reads back what it wrote itself.
//   skip      loaded PER MFMA TILE, one tile ahead: the two 16-B loads of MFMA tile i + 1 are issued in front of tile i's trip
//             through LDS, and those of tile 0 inside the last K tile, in front of its MFMAs.  A row beyond M reads row M - 1.
//             Why not at kernel entry, as the 128-tile does: the whole skip of a wave is 8 tiles x 2 x 4 = 64 registers, which
//             with 128 accumulators, 48 of fragments and the staging's offsets does not fit 256 through the main loop.  Why not
//             all of it behind the main loop: the first tile would wait a whole miss with nothing to run under it, while one
//             tile ahead keeps 8 to 16 registers live and every load but the first has a tile's conversions and stores in front
//             of its use.  bias is 8 registers and is loaded at kernel entry, in front of the first LDS-DMA.
//
// The operands are swapped in the MFMA (A = weights, B = activations): a lane's accumulator registers run along the channels,
// four consecutive channels of one position per register group.
//
// This translation unit includes nothing from CK and nothing of the project but net_common.h: it is its own object (GNUmakefile).
#include "net_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512;
constexpr int kTile = 256;                       // positions, and output channels, per workgroup
constexpr int kSubM = 4, kSubN = 2;              // MFMA tiles per wave along the positions and along the channels
constexpr int kPieces = kTile / 64;              // pieces of 8 rows one wave stages per operand and K tile: 8 waves x 8 rows x 4
constexpr int kOperandBytes = kTile * 128;       // one operand of one K tile: 256 rows x 64 bf16
constexpr int kBufBytes = 2 * kOperandBytes;     // activations, then weights
constexpr int kLoads = 2 * kPieces;              // LDS-DMA loads one wave issues per K tile
constexpr int kAhead = 1;                        // K tiles staged ahead of the one being spent: the ring has two stages
constexpr int kWaveCBytes = 4096;                // a wave's own piece of the epilogue: 32 positions x 32 channels fp32
static_assert(8 * kWaveCBytes <= kBufBytes, "the epilogue's eight wave regions fit one stage");

// the line every off-board tap and every row beyond M is staged from
__device__ __attribute__((aligned(128))) unsigned char g_zero_line_bf16_big[128] = {0};

typedef const __attribute__((address_space(1))) void* gptr_t;

// 64 lanes x 16 B: lane l's 16 bytes land at lds_base + 16 * l (the destination is wave-uniform, the source per lane)
__device__ __forceinline__ void stage16(const char* src, char* lds_base) {
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)lds_base, 16, 0, 0);
}
// at most kN of this wave's loads (in issue order) are still in flight behind it, and its own ds_reads have retired
template <int kN>
__device__ __forceinline__ void wait_staged() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(kN) : "memory");
}
// the loop's barrier is the bare instruction: __syncthreads() would fence, and the fence waits for every LDS-DMA in flight
__device__ __forceinline__ void raw_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

template <bool kHasRes>
__global__ __launch_bounds__(kThreads) void k_conv3x3_bf16_big(const char* __restrict__ x, const char* __restrict__ w,
                                                               const __bf16* __restrict__ bias, const __bf16* __restrict__ res,
                                                               __bf16* __restrict__ y, int M, int H, int W, int Cin, int K, int relu) {
  __shared__ __attribute__((aligned(128))) char lds[2 * kBufBytes];   // ALL of the kernel's LDS: one array, 128 KiB
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wv >> 2, wn = wv & 3;
  const int tile = blockIdx.x, kbase = blockIdx.y * kTile;

  // ---- epilogue geometry, and the bias: in the read-back of MFMA tile (im, in) a lane is position pr (+ 16 j) of the tile's 32
  // and chunk q of its four 8-channel chunks.
  const int pr = lane >> 2, q = lane & 3;
  const int chan = kbase + wn * (32 * kSubN) + q * 8;
  const int row0 = tile * kTile + wm * (32 * kSubM);
  bf16x8 bv[kSubN];
#pragma unroll
  for (int in = 0; in < kSubN; ++in) bv[in] = *(const bf16x8*)(bias + chan + in * 32);
  __builtin_amdgcn_sched_barrier(0);   // these loads are the oldest: the loop's vmcnt counts stand for LDS-DMA loads alone
  // the skip of MFMA tile i = im * kSubN + in, positions j = 0, 1.  A row beyond M reads the last valid row instead (no branch
  // around a load) and is not stored.
  auto load_skip = [&](int i, bf16x8* rv) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = row0 + (i / kSubN) * 32 + j * 16 + pr;
      rv[j] = *(const bf16x8*)(res + (size_t)(p < M ? p : M - 1) * K + chan + (i % kSubN) * 32);
    }
  };

  // ---- the rows a staging lane feeds.  Wave wv issues pieces i = 0 .. 3 of each operand: rows i * 64 + wv * 8 .. + 7.  A lane is
  // row (lane >> 3) of its piece and LDS slot (lane & 7) of that row.
  const unsigned char* const zsrc = g_zero_line_bf16_big + (lane & 7) * 16;
  uint32_t xoff[kPieces], woff[kPieces], xmask[kPieces];
  {
    const int hw = H * W;
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int r = i * 64 + wv * 8 + (lane >> 3);
      const int p = tile * kTile + r;
      uint32_t m = 0;
      if (p < M) {
        const int rem = p % hw, hh = rem / W, ww = rem - hh * W;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int dy = tap / 3 - 1, dx = tap % 3 - 1;
          if ((unsigned)(hh + dy) < (unsigned)H && (unsigned)(ww + dx) < (unsigned)W) m |= 1u << tap;
        }
      }
      const uint32_t sl = (uint32_t)(((lane & 7) ^ ((r >> 1) & 7)) << 4);
      xmask[i] = m;
      xoff[i] = (uint32_t)p * (uint32_t)(Cin * 2) + sl;                  // below 2^31 wherever it is used (p < M)
      woff[i] = (uint32_t)(kbase + r) * (uint32_t)(9 * Cin * 2) + sl;    // kbase + r < K: K is a multiple of 256
    }
  }
  // K tile (tap, kc) into ring buffer buf: this wave's pieces, the activations' and then the weights'
  auto stage = [&](int tap, int kc, int buf) {
    const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
    const uint32_t dxb = (uint32_t)((dy * W + dx) * Cin * 2 + kc * 128);
    const uint32_t dwb = (uint32_t)(tap * Cin * 2 + kc * 128);
    char* const b = lds + buf * kBufBytes + wv * 1024;
#pragma unroll
    for (int i = 0; i < kPieces; ++i)
      stage16(((xmask[i] >> tap) & 1) ? x + (uint32_t)(xoff[i] + dxb) : (const char*)zsrc, b + i * 8192);
#pragma unroll
    for (int i = 0; i < kPieces; ++i) stage16(w + (uint32_t)(woff[i] + dwb), b + kOperandBytes + i * 8192);
  };

  // ---- fragments: lane (fr = lane & 31, fh = lane >> 5) holds row fr of a 32-row MFMA tile and 8 of the 16 k of one MFMA: MFMA kk
  // of a K tile takes the 16-B chunk 2 kk + fh of the row, channels 16 kk + 8 fh .. + 7.
  const int fr = lane & 31, fh = lane >> 5;
  const int sw = (fr >> 1) & 7;                  // the MFMA tiles start at multiples of 32 rows: (row >> 1) & 7 is the lane's own
  const int xrow = (wm * (32 * kSubM) + fr) * 128;
  const int wrow = kOperandBytes + (wn * (32 * kSubN) + fr) * 128;
  int cs[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) cs[kk] = ((kk * 2 + fh) ^ sw) << 4;

  floatx16 acc[kSubN][kSubM];   // [channels][positions]
#pragma unroll
  for (int in = 0; in < kSubN; ++in)
#pragma unroll
    for (int im = 0; im < kSubM; ++im)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[in][im][e] = 0.0f;

  // K tile t lives in ring buffer t & 1; one K tile is staged ahead.  Iteration t:
  //   wait     vmcnt(kLoads * (kAhead - 1)) lgkmcnt(0): this wave's loads of K tile t have landed, and its fragment reads of t - 1 have
  //            retired.  The count is the 128-tile's kLoads * (kAhead - 1) at kAhead = 1: in a ring of two every load a wave has
  //            in flight here is one of K tile t's own eight (t + 1 goes into the buffer t - 1 is being read from, so it cannot
  //            be issued before this iteration's barrier), and all eight are needed.  Nothing younger exists to leave in flight;
  //            the bias loads are older.  In the last K tile the same count stands for "everything".
  //   barrier  so every wave's loads of t have landed, and every wave is done reading t - 1
  //   read     the fragments of MFMA 0 from buffer t & 1 (those of MFMA kk + 1 are read in front of the MFMAs of kk)
  //   stage    K tile t + 1 into buffer (t + 1) & 1, which is (t - 1) & 1: free since the barrier
  //   spend    the MFMAs, 8 per kk
  // landed: a read of K tile t stands behind the barrier that stands behind every wave's wait for it.  free: the restaging of a
  // buffer stands behind the barrier that stands behind the lgkmcnt(0) of every wave's last read of it; the reads of t that come
  // behind the staging of t + 1 are of the other buffer.  Neither depends on how far apart the waves run: a wave is at most one
  // barrier ahead of another.  The last K tile stages nothing.  The prologue is K tile 0.
  const int kchunks = Cin >> 6, ktiles = 9 * kchunks;   // at least 9
  bf16x8 rv[2], rvn[2];                                 // the skip of the MFMA tile in the epilogue, and of the one behind it
  stage(0, 0, 0);
  int tapn = 1 / kchunks, kcn = 1 % kchunks;            // K tile t + 1
  int cur = 0;
  auto ktile = [&](auto mode) {
    constexpr bool kStage = decltype(mode)::v == 1;     // this iteration stages one more behind its first reads
    wait_staged<kLoads * (kAhead - 1)>();
    raw_barrier();
    const char* b = lds + cur * kBufBytes;
    bf16x8 wf[2][kSubN], xf[2][kSubM];
    auto read = [&](int kk) {
#pragma unroll
      for (int s = 0; s < kSubN; ++s) wf[kk & 1][s] = *(const bf16x8*)(b + wrow + s * 4096 + cs[kk]);
#pragma unroll
      for (int s = 0; s < kSubM; ++s) xf[kk & 1][s] = *(const bf16x8*)(b + xrow + s * 4096 + cs[kk]);
    };
    read(0);
    __builtin_amdgcn_sched_barrier(0);   // the first reads are on their way before the staging's address arithmetic and issue
    if constexpr (kStage) {
      stage(tapn, kcn, cur ^ 1);
    } else if constexpr (kHasRes) {
      load_skip(0, rv);                  // the last K tile: the first MFMA tile's skip arrives under its MFMAs
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (kk < 3) {
        read(kk + 1);
        __builtin_amdgcn_sched_barrier(0);   // issued in front of kk's MFMAs and returning under them, not sunk behind them
      }
#pragma unroll
      for (int in = 0; in < kSubN; ++in)
#pragma unroll
        for (int im = 0; im < kSubM; ++im)
          acc[in][im] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[kk & 1][in], xf[kk & 1][im], acc[in][im], 0, 0, 0);
    }
    cur ^= 1;
  };
  for (int t = 0; t < ktiles - 1; ++t) {
    ktile(Mode<1>{});
    if (++kcn == kchunks) { kcn = 0; ++tapn; }
  }
  ktile(Mode<0>{});

  // ---- epilogue.  D = W X^T: the lane's column is position fr of the MFMA tile, its register e is channel (e & 3) + 8 (e >> 2)
  // + 4 fh.  An MFMA tile's 32 positions x 32 channels go as fp32 rows of eight 16-B chunks, chunk g of position p at chunk
  // g ^ (p & 7), into the wave's own 4 KiB of stage ktiles & 1: the last K tile was read from stage (ktiles - 1) & 1, and every
  // wave has passed the last barrier, behind its last read of the other stage; no LDS-DMA is in flight (the last wait).  So no
  // barrier: a wave reads back what it wrote itself, and its LDS instructions run in order, one MFMA tile after the other.
  char* const cl = lds + (ktiles & 1) * kBufBytes + wv * kWaveCBytes;
#pragma unroll
  for (int im = 0; im < kSubM; ++im)
#pragma unroll
    for (int in = 0; in < kSubN; ++in) {
      const int i = im * kSubN + in;
      if constexpr (kHasRes)
        if (i + 1 < kSubM * kSubN) load_skip(i + 1, rvn);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        floatx4 fv;
#pragma unroll
        for (int e = 0; e < 4; ++e) fv[e] = acc[in][im][g * 4 + e];
        *(floatx4*)(cl + fr * 128 + (((g * 2 + fh) ^ (fr & 7)) << 4)) = fv;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own writes; nobody else's are read
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int pos = j * 16 + pr;
        const int p = row0 + im * 32 + pos;
        const floatx4 c0 = *(const floatx4*)(cl + pos * 128 + (((q * 2) ^ (pos & 7)) << 4));
        const floatx4 c1 = *(const floatx4*)(cl + pos * 128 + (((q * 2 + 1) ^ (pos & 7)) << 4));
        bf16x8 ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = e < 4 ? c0[e & 3] : c1[e & 3];
          v += (float)bv[in][e];
          if constexpr (kHasRes) v += (float)rv[j][e];
          if (relu) v = fmaxf(v, 0.0f);
          ov[e] = (__bf16)v;   // the one rounding: round-to-nearest-even
        }
        if (p < M) *(bf16x8*)(y + (size_t)p * K + chan + in * 32) = ov;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the read-back has retired before the next MFMA tile overwrites it
      __builtin_amdgcn_wave_barrier();
      if constexpr (kHasRes)
        if (i + 1 < kSubM * kSubN) { rv[0] = rvn[0]; rv[1] = rvn[1]; }
    }
}

}  // namespace

// The convolution entries' argument checks (conv_args), C a multiple of 64 and K of 256.  One launch on `stream`: no allocation,
// no memset, no workspace, no synchronisation, no copy; every refusal comes before it.
extern "C" int elfnet_conv3x3_bf16_big(const void* x, const void* w, const void* bias, const void* res, void* y, int64_t rows, int h,
                                       int wd, int c, int k, int relu, void* stream) {
  if ((c & 63) != 0 || (k & 255) != 0) return ELFGO_E_BADARG;
  int dev = 0;
  const int go = conv_args(x, 16, w, bias, res, y, rows, h, wd, c, k, &dev);
  if (go <= 0) return go;
  DevGuard _dg(dev);
  const int64_t m = rows * h * wd;
  const dim3 grid((unsigned)((m + kTile - 1) / kTile), (unsigned)(k / kTile));   // below 2^14 x below 2^13 by conv_args' limits
  hipStream_t st = (hipStream_t)stream;
  if (res)
    hipLaunchKernelGGL((k_conv3x3_bf16_big<true>), grid, dim3(kThreads), 0, st, (const char*)x, (const char*)w, (const __bf16*)bias,
                       (const __bf16*)res, (__bf16*)y, (int)m, h, wd, c, k, relu);
  else
    hipLaunchKernelGGL((k_conv3x3_bf16_big<false>), grid, dim3(kThreads), 0, st, (const char*)x, (const char*)w, (const __bf16*)bias,
                       (const __bf16*)nullptr, (__bf16*)y, (int)m, h, wd, c, k, relu);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
