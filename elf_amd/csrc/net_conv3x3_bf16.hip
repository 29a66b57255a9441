// elfnet_conv3x3_bf16: the trunk convolution y = relu?(conv3x3_same(x, w) + bias (+ res)) of a bf16 net: x, res and y bf16 NHWC,
// w bf16 [K,3,3,C], bias bf16 [K], fp32 accumulation in v_mfma_f32_32x32x16_bf16.  Before it a bf16 net's trunk convolution was
// a bias-free MIOpen convolution and a second pass over the activation (elfnet_bias_act_bf16): two kernels and two roundings.
//
// ONE ROUNDING.  The epilogue computes acc + bias (+ res) in fp32, takes fmaxf(., 0) when relu is set (a NaN becomes 0, as in the
// fp16 kernels) and rounds ONCE to bf16, round-to-nearest-even, with the hardware convert (v_cvt_pk_bf16_f32).  The fp16 kernels
// round the accumulator to fp16 first because they reproduce CK's chain bit for bit; nothing ties bf16 to that chain.
//
// One kernel template, two workgroup tiles, 256 threads = 4 waves as 2 (positions) x 2 (channels) in both, BK = 64 in both (a K
// tile is one tap and 64 consecutive input channels):
//   narrow    64 positions x 64 output channels: a wave owns 32 x 32 = one MFMA tile = 16 accumulator registers; 8 ds_read_b128
//             for 4 MFMAs per K tile.  A ring of three 16-KiB stages (48 KiB, three workgroups per CU).  The geometry of
//             net_conv3x3_small.hip: a single game's 16-row call (5 776 positions, K = 256) is 364 workgroups.
//   wide      128 positions x 128 output channels: a wave owns 64 x 64 = 2 x 2 MFMA tiles = 64 accumulator registers; 16
//             ds_read_b128 for 16 MFMAs per K tile, half the LDS traffic per MFMA.  A stage is 32 KiB; the ring has TWO (64 KiB,
//             two workgroups per CU, one's epilogue under the other's main loop): K tile t + 1 is staged right behind the
//             barrier of K tile t.  A ring of three (96 KiB, one workgroup per CU) is the same template with kStages = 3; it is
//             not instantiated and was not measured.
//   staging   LDS-DMA (global_load_lds_dwordx4).  A stage is the activation tile, then the weight tile, rows of 128 B.  A K tile
//             is pieces of 8 rows, every piece a full aligned 128-B line per 8 lanes; a wave issues kTile / 32 pieces of each
//             operand (2 + 2 narrow, 4 + 4 wide).  The loop has ONE bare s_barrier per K tile behind a counted vmcnt wait.
//   halo      a staging lane decodes its rows once (position -> h, w) and keeps a 9-bit tap mask and a byte offset per row; for
//             an off-board tap, and for a row at or beyond M, its source address is this file's zero-filled 128-B line in global
//             memory.  LDS is never zeroed by a second path.
//   LDS image lane-linear, as the DMA writes it; the 16-B slot s of row r holds the row's chunk s ^ ((r >> 1) & 7), the XOR on the
//             source address when staging and on the address of the fragment ds_read_b128s.
//   K order   tap-major (ky, kx, then c ascending: MFMA kk of a K tile sums channels 16 kk .. 16 kk + 15); one fp32 accumulator
//             per output from zero; no split-K, no atomics.
//   epilogue  the accumulators go as fp32, one MFMA tile (4 KiB) at a time, through the wave's own region of the stage that the last
//             K tile is NOT in, and come back as 8 consecutive channels per lane, so a store instruction writes 64-B runs of y.
//             Rows at or beyond M are not stored.  bias and the skip are loaded in that shape at kernel entry, in front of the first
//             LDS-DMA, and used behind the last.
//
// The operands are swapped in the MFMA (A = weights, B = activations): a lane's accumulator registers run along the channels,
// four consecutive channels of one position per register group.
//
// elfnet_conv3x3_bf16 picks the tile with elfnet_conv3x3_bf16_pick at the device's CU count; elfnet_conv3x3_bf16_tile pins it.
// This translation unit includes nothing from CK and nothing of the project but net_common.h: it is its own object (GNUmakefile).
#include "net_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaveCBytes = 4096;                // a wave's own piece of the epilogue: 32 positions x 32 channels fp32

// the line every off-board tap and every row beyond M is staged from
__device__ __attribute__((aligned(128))) unsigned char g_zero_line_bf16[128] = {0};

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

// kTile: positions and output channels per workgroup (64 or 128).  kStages: the depth of the LDS ring, 2 or 3.
template <int kTile, int kStages, bool kHasRes>
__global__ __launch_bounds__(kThreads) void k_conv3x3_bf16(const char* __restrict__ x, const char* __restrict__ w,
                                                           const __bf16* __restrict__ bias, const __bf16* __restrict__ res,
                                                           __bf16* __restrict__ y, int M, int H, int W, int Cin, int K, int relu) {
  constexpr int kSub = kTile / 64;                 // MFMA tiles per wave along either axis
  constexpr int kWave = 32 * kSub;                 // positions, and channels, per wave
  constexpr int kPieces = kTile / 32;              // pieces of 8 rows one wave stages per operand and K tile
  constexpr int kOperandBytes = kTile * 128;       // one operand of one K tile: kTile rows x 64 bf16
  constexpr int kBufBytes = 2 * kOperandBytes;     // activations, then weights
  constexpr int kLoads = 2 * kPieces;              // LDS-DMA loads one wave issues per K tile
  constexpr int kAhead = kStages - 1;              // K tiles staged ahead of the one being spent
  static_assert((kTile == 64 || kTile == 128) && (kStages == 2 || kStages == 3), "tiles of 64 or 128, rings of 2 or 3");
  static_assert(4 * kWaveCBytes <= kBufBytes, "the epilogue's four wave regions fit one stage");
  __shared__ __attribute__((aligned(128))) char lds[kStages * kBufBytes];   // ALL of the kernel's LDS: one array
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wv >> 1, wn = wv & 1;
  const int tile = blockIdx.x, kbase = blockIdx.y * kTile;

  // ---- epilogue operands, loaded first: in the read-back of MFMA tile (im, in) a lane is position pr (+ 16 j) of the tile's 32
  // and chunk q of its four 8-channel chunks.  A row beyond M reads the last valid row instead (no branch around a load) and is
  // not stored.
  const int pr = lane >> 2, q = lane & 3;
  const int chan = kbase + wn * kWave + q * 8;
  const int row0 = tile * kTile + wm * kWave;
  bf16x8 bv[kSub];
  bf16x8 rv[kHasRes ? kSub * kSub * 2 : 1];
#pragma unroll
  for (int in = 0; in < kSub; ++in) bv[in] = *(const bf16x8*)(bias + chan + in * 32);
  if constexpr (kHasRes) {
#pragma unroll
    for (int im = 0; im < kSub; ++im)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int p = row0 + im * 32 + j * 16 + pr;
        const __bf16* rp = res + (size_t)(p < M ? p : M - 1) * K + chan;
#pragma unroll
        for (int in = 0; in < kSub; ++in) rv[(im * kSub + in) * 2 + j] = *(const bf16x8*)(rp + in * 32);
      }
  }
  __builtin_amdgcn_sched_barrier(0);   // these loads are the oldest: the loop's vmcnt counts stand for LDS-DMA loads alone

  // ---- the rows a staging lane feeds.  Wave wv issues pieces i = 0 .. kPieces - 1 of each operand: rows i * 32 + wv * 8 .. + 7.
  // A lane is row (lane >> 3) of its piece and LDS slot (lane & 7) of that row.
  const unsigned char* const zsrc = g_zero_line_bf16 + (lane & 7) * 16;
  uint32_t xoff[kPieces], woff[kPieces], xmask[kPieces];
  {
    const int hw = H * W;
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int r = i * 32 + wv * 8 + (lane >> 3);
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
      woff[i] = (uint32_t)(kbase + r) * (uint32_t)(9 * Cin * 2) + sl;    // kbase + r < K: K is a multiple of kTile
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
      stage16(((xmask[i] >> tap) & 1) ? x + (uint32_t)(xoff[i] + dxb) : (const char*)zsrc, b + i * 4096);
#pragma unroll
    for (int i = 0; i < kPieces; ++i) stage16(w + (uint32_t)(woff[i] + dwb), b + kOperandBytes + i * 4096);
  };

  // ---- fragments: lane (fr = lane & 31, fh = lane >> 5) holds row fr of a 32-row MFMA tile and 8 of the 16 k of one MFMA: MFMA kk
  // of a K tile takes the 16-B chunk 2 kk + fh of the row, channels 16 kk + 8 fh .. + 7.
  const int fr = lane & 31, fh = lane >> 5;
  const int sw = (fr >> 1) & 7;                  // the MFMA tiles start at multiples of 32 rows: (row >> 1) & 7 is the lane's own
  const int xrow = (wm * kWave + fr) * 128;
  const int wrow = kOperandBytes + (wn * kWave + fr) * 128;
  int cs[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) cs[kk] = ((kk * 2 + fh) ^ sw) << 4;

  floatx16 acc[kSub][kSub];   // [channels][positions]
#pragma unroll
  for (int in = 0; in < kSub; ++in)
#pragma unroll
    for (int im = 0; im < kSub; ++im)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[in][im][e] = 0.0f;

  // K tile t lives in ring buffer t % kStages; kAhead = kStages - 1 K tiles are staged ahead.  Iteration t:
  //   wait     vmcnt(kLoads * (kAhead - 1)) lgkmcnt(0): this wave's loads of K tile t have landed (those of t + 1 .. t + kAhead - 1
  //            may still fly), and its fragment reads of t - 1 have retired
  //   barrier  so every wave's loads of t have landed, and every wave is done reading t - 1
  //   read     the fragments from buffer t % kStages
  //   stage    K tile t + kAhead into buffer (t + kAhead) % kStages, which is (t - 1) % kStages: free since the barrier
  //   spend    the MFMAs
  // landed: a read of K tile t stands behind the barrier that stands behind every wave's wait for it.  free: the restaging of a
  // buffer stands behind the barrier that stands behind the lgkmcnt(0) of every wave's last read of it.  Neither depends on how
  // far apart the waves run: a wave is at most one barrier ahead of another.
  // The last kAhead K tiles stage nothing, and the last waits for everything.  The prologue is K tiles 0 .. kAhead - 1.
  const int kchunks = Cin >> 6, ktiles = 9 * kchunks;   // at least 9
#pragma unroll
  for (int t = 0; t < kAhead; ++t) stage(t / kchunks, t % kchunks, t);
  int tapn = kAhead / kchunks, kcn = kAhead % kchunks;   // K tile t + kAhead
  int cur = 0, nxt = kAhead;
  auto ktile = [&](auto mode) {
    constexpr int kBehind = decltype(mode)::v;   // how many K tiles of this wave's are staged and not yet waited for
    constexpr bool kStage = kBehind == kAhead;   // this iteration stages one more behind its reads
    wait_staged<kLoads * (kStage ? kAhead - 1 : kBehind)>();
    raw_barrier();
    const char* b = lds + cur * kBufBytes;
    bf16x8 xf[kSub][4], wf[kSub][4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int s = 0; s < kSub; ++s) {
        wf[s][kk] = *(const bf16x8*)(b + wrow + s * 4096 + cs[kk]);
        xf[s][kk] = *(const bf16x8*)(b + xrow + s * 4096 + cs[kk]);
      }
    __builtin_amdgcn_sched_barrier(0);   // all reads are on their way before anything else: the staging's address arithmetic and
    if constexpr (kStage) {              // issue run while they return
      stage(tapn, kcn, nxt);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int in = 0; in < kSub; ++in)
#pragma unroll
        for (int im = 0; im < kSub; ++im)
          acc[in][im] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[in][kk], xf[im][kk], acc[in][im], 0, 0, 0);
    cur = cur == kStages - 1 ? 0 : cur + 1;
    nxt = nxt == kStages - 1 ? 0 : nxt + 1;
  };
  for (int t = 0; t < ktiles - kAhead; ++t) {
    ktile(Mode<kAhead>{});
    if (++kcn == kchunks) { kcn = 0; ++tapn; }
  }
  if constexpr (kAhead == 2) ktile(Mode<1>{});
  ktile(Mode<0>{});

  // ---- epilogue.  D = W X^T: the lane's column is position fr of the MFMA tile, its register e is channel (e & 3) + 8 (e >> 2)
  // + 4 fh.  An MFMA tile's 32 positions x 32 channels go as fp32 rows of eight 16-B chunks, chunk g of position p at chunk
  // g ^ (p & 7), into the wave's own 4 KiB of stage ktiles % kStages: the last K tile was read from stage (ktiles - 1) % kStages,
  // and every wave has passed the last barrier, behind its last read of every other stage; nothing is in flight (vmcnt(0)).  So
  // no barrier: a wave reads back what it wrote itself, and its LDS instructions run in order, one MFMA tile after the other.
  char* const cl = lds + (ktiles % kStages) * kBufBytes + wv * kWaveCBytes;
#pragma unroll
  for (int im = 0; im < kSub; ++im)
#pragma unroll
    for (int in = 0; in < kSub; ++in) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        floatx4 fv;
#pragma unroll
        for (int i = 0; i < 4; ++i) fv[i] = acc[in][im][g * 4 + i];
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
        for (int i = 0; i < 8; ++i) {
          float v = i < 4 ? c0[i & 3] : c1[i & 3];
          v += (float)bv[in][i];
          if constexpr (kHasRes) v += (float)rv[(im * kSub + in) * 2 + j][i];
          if (relu) v = fmaxf(v, 0.0f);
          ov[i] = (__bf16)v;   // the one rounding: round-to-nearest-even
        }
        if (p < M) *(bf16x8*)(y + (size_t)p * K + chan + in * 32) = ov;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the read-back has retired before the next MFMA tile overwrites it
      __builtin_amdgcn_wave_barrier();
    }
}

template <int kTile, int kStages>
int launch(const void* x, const void* w, const void* bias, const void* res, void* y, int64_t m, int h, int wd, int c, int k, int relu,
           hipStream_t st) {
  const dim3 grid((unsigned)((m + kTile - 1) / kTile), (unsigned)(k / kTile));   // below 2^24 x below 2^24 by conv_args' limits
  if (res)
    hipLaunchKernelGGL((k_conv3x3_bf16<kTile, kStages, true>), grid, dim3(kThreads), 0, st, (const char*)x, (const char*)w,
                       (const __bf16*)bias, (const __bf16*)res, (__bf16*)y, (int)m, h, wd, c, k, relu);
  else
    hipLaunchKernelGGL((k_conv3x3_bf16<kTile, kStages, false>), grid, dim3(kThreads), 0, st, (const char*)x, (const char*)w,
                       (const __bf16*)bias, (const __bf16*)nullptr, (__bf16*)y, (int)m, h, wd, c, k, relu);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

// The wide tile where it exists (K a multiple of 128) and the wide tiles alone fill the chip once, ceil(positions / 128) * (K / 128)
// >= cus; the narrow tile otherwise.  A derived rule -- below it some CUs would have no wide workgroup at all while the narrow
// tiles, four times as many, still spread over all of them -- that the probed sizes bear out, though they do not locate the
// crossover.  Measured on MI355X (256 CUs) at 19 x 19 x 256 -> 256, us without / with skip, tile 64 against tile 128
// (profiles/conv_bf16_probe.json): 1 row (6 wide workgroups) 11.2 / 11.2 against 23.6 / 23.8; 16 rows (92) 15.9 / 15.6 against
// 24.2 / 25.3; 64 rows (362) 45.3 / 45.1 against 41.9 / 38.3, beyond the spread with skip only; 128 rows (722) 86.6 / 87.5 against
// 72.5 / 72.5; 2048 rows 1448.1 / 1508.5 against 980.1 / 1027.6.  Nothing between 16 and 64 rows was probed.
extern "C" int elfnet_conv3x3_bf16_pick(int64_t positions, int k, int cus) {
  if (positions <= 0 || k <= 0 || (k & 127) != 0) return 64;
  return ((positions + 127) / 128) * (k / 128) >= (int64_t)cus ? 128 : 64;
}

// The convolution entries' argument checks (conv_args), C and K multiples of 64, and a tile that exists.  One launch on `stream`:
// no allocation, no memset, no workspace, no synchronisation, no copy; every refusal comes before it.
extern "C" int elfnet_conv3x3_bf16_tile(const void* x, const void* w, const void* bias, const void* res, void* y, int64_t rows, int h,
                                        int wd, int c, int k, int relu, int tile, void* stream) {
  if ((c & 63) != 0 || (k & 63) != 0) return ELFGO_E_BADARG;
  if ((tile != 0 && tile != 64 && tile != 128) || (tile == 128 && (k & 127) != 0)) return ELFGO_E_BADARG;
  int dev = 0;
  const int go = conv_args(x, 16, w, bias, res, y, rows, h, wd, c, k, &dev);
  if (go <= 0) return go;
  DevGuard _dg(dev);
  const int64_t m = rows * h * wd;
  if (tile == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
      const hipError_t e = hipGetLastError();
      return e == hipSuccess ? (int)hipErrorUnknown : (int)e;
    }
    tile = elfnet_conv3x3_bf16_pick(m, k, cus);
  }
  hipStream_t st = (hipStream_t)stream;
  return tile == 128 ? launch<128, 2>(x, w, bias, res, y, m, h, wd, c, k, relu, st)
                     : launch<64, 3>(x, w, bias, res, y, m, h, wd, c, k, relu, st);
}

extern "C" int elfnet_conv3x3_bf16(const void* x, const void* w, const void* bias, const void* res, void* y, int64_t rows, int h,
                                   int wd, int c, int k, int relu, void* stream) {
  return elfnet_conv3x3_bf16_tile(x, w, bias, res, y, rows, h, wd, c, k, relu, 0, stream);
}
