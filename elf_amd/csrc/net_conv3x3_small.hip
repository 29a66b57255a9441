// elfnet_conv3x3_small_f16: the trunk convolution y = relu?(conv3x3_same(x, w) + bias (+ res)) for calls of a few thousand positions
// (a single game's 16-row net call is 5 776), fp16 NHWC in and out, w as [K,3,3,C], fp32 accumulation in v_mfma_f32_32x32x16_f16.
//
// Why a third main loop beside algo 0 (CK, net_conv.hip) and algo 1 (net_conv3x3.hip): both cut the positions into tiles of 256,
// so a 16-row call is 46 (algo 0) or 23 (algo 1) workgroups on 256 CUs, each walking all of K alone: the call takes one
// workgroup's serial K loop with four fifths of the chip idle.  Here the tile is small enough that the
// same call is 364 workgroups, all resident at once:
//   tile      64 positions x 64 output channels x BK 64 (one tap, 64 consecutive input channels).  256 threads, 4 waves as
//             2 (positions) x 2 (channels), each owning 32 x 32 = one MFMA tile = 16 accumulator registers.  The launch is a plain
//             grid of tiles x (K / 64) workgroups, none depending on another.
//   staging   LDS-DMA (global_load_lds_dwordx4) into a ring of three 16-KiB LDS buffers (activation tile, then weight tile: 64 rows
//             of 128 B each): 48 KiB, three workgroups per CU.  A K tile is 16 pieces of 8 rows, four per wave (two of each
//             operand), every piece a full aligned 128-B line per 8 lanes.  Two K tiles are in flight while one is spent; the loop
//             has ONE bare s_barrier per K tile behind a counted vmcnt wait (the comment at the loop has the counts).
//   halo      as algo 1: a staging lane decodes its two rows once (position -> n, h, w) and keeps a 9-bit tap mask and a byte
//             offset; for an off-board tap, and for a row at or beyond M, its source address is a zero-filled line in global
//             memory.  LDS is never zeroed by a second path.
//   LDS image as algo 1: lane-linear, as the DMA writes it; the 16-B slot s of row r holds the row's chunk s ^ ((r >> 1) & 7), the
//             XOR on the source address when staging and on the address of the fragment ds_read_b128s.
//   K order   algo 0's accumulation chain per output element, bit for bit: tap-major (ky, kx, then c ascending); inside a
//             32-channel block the two MFMAs take channels {0..7, 16..23} and {8..15, 24..31}; one fp32 accumulator per output
//             from zero; no split-K, no atomics.
//   epilogue  BiasResAct's sequence (net_conv.hip): float(half(acc)) + bias (+ res), max(., 0), one rounding to fp16.  The
//             accumulators go through 2 KiB of the wave's own in LDS buffer 0 (free by then, see the loop) and come back as 16 B of
//             consecutive channels per lane, so a store instruction writes 64-B runs of y.  Rows at or beyond M are not stored.
//             bias and the skip are loaded in that shape at kernel entry, in front of the first LDS-DMA, and used behind the last.
//
// The operands are swapped in the MFMA (A = weights, B = activations), as in algo 1: a lane's accumulator registers run along the
// channels, four consecutive channels of one position per register group.
//
// This translation unit includes nothing from CK and nothing of the project but the C header: it is its own object (GNUmakefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/elf_amd.h"


namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kTileM = 64;                       // positions per workgroup
constexpr int kTileN = 64;                       // output channels per workgroup
constexpr int kThreads = 256;
constexpr int kOperandBytes = 64 * 128;          // one operand of one K tile: 64 rows x 64 fp16
constexpr int kBufBytes = 2 * kOperandBytes;     // activations, then weights
constexpr int kStages = 3;
constexpr int kLdsBytes = kStages * kBufBytes;   // 48 KiB
constexpr int kWaveCBytes = 2048;                // a wave's own piece of the epilogue: 32 positions x 32 channels fp16
constexpr int kLoadsPerTile = 4;                 // LDS-DMA loads one wave issues per K tile

// the line every off-board tap and every row beyond M is staged from
__device__ __attribute__((aligned(128))) unsigned char g_zero_line_small[128] = {0};

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

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
template <int kV> struct Mode { static constexpr int v = kV; };

template <bool kHasRes>
__global__ __launch_bounds__(kThreads) void k_conv3x3_small_f16(const char* __restrict__ x, const char* __restrict__ w,
                                                                const _Float16* __restrict__ bias, const _Float16* __restrict__ res,
                                                                _Float16* __restrict__ y, int M, int H, int W, int Cin, int K,
                                                                int relu) {
  __shared__ __attribute__((aligned(128))) char lds[kLdsBytes];   // ALL of the kernel's LDS: one array
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wv >> 1, wn = wv & 1;
  const int tile = blockIdx.x, kbase = blockIdx.y * kTileN;

  // ---- epilogue operands, loaded first: in the read-back a lane is position pr (+ 16 j) of the wave's 32 and chunk q of its four
  // 16-B chunks of channels.  A row beyond M reads the last valid row instead (no branch around a load) and is not stored.
  const int pr = lane >> 2, q = lane & 3;
  const int chan = kbase + wn * 32 + q * 8;
  const int row0 = tile * kTileM + wm * 32;
  const half8 bv = *(const half8*)(bias + chan);
  half8 rv[kHasRes ? 2 : 1];
  if constexpr (kHasRes) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = row0 + j * 16 + pr;
      rv[j] = *(const half8*)(res + (size_t)(p < M ? p : M - 1) * K + chan);
    }
  }

  // ---- the rows a staging lane feeds.  A K tile is 8 + 8 pieces of 8 rows; wave wv issues pieces i = 0, 1 of each operand: rows
  // i * 32 + wv * 8 .. + 7.  A lane is row (lane >> 3) of its piece and LDS slot (lane & 7) of that row.
  const unsigned char* const zsrc = g_zero_line_small + (lane & 7) * 16;
  uint32_t xoff[2], woff[2], xmask[2];
  {
    const int hw = H * W;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = i * 32 + wv * 8 + (lane >> 3);
      const int p = tile * kTileM + r;
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
      woff[i] = (uint32_t)(kbase + r) * (uint32_t)(9 * Cin * 2) + sl;    // kbase + r < K: K is a multiple of 64
    }
  }
  // K tile (tap, kc) into ring buffer buf: this wave's four pieces, X X W W
  auto stage = [&](int tap, int kc, int buf) {
    const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
    const uint32_t dxb = (uint32_t)((dy * W + dx) * Cin * 2 + kc * 128);
    const uint32_t dwb = (uint32_t)(tap * Cin * 2 + kc * 128);
    char* const b = lds + buf * kBufBytes + wv * 1024;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      stage16(((xmask[i] >> tap) & 1) ? x + (uint32_t)(xoff[i] + dxb) : (const char*)zsrc, b + i * 4096);
#pragma unroll
    for (int i = 0; i < 2; ++i) stage16(w + (uint32_t)(woff[i] + dwb), b + kOperandBytes + i * 4096);
  };

  // ---- fragments: lane (fr = lane & 31, fh = lane >> 5) holds row fr of a 32-row MFMA tile and 8 of the 16 k of one MFMA.
  // Which 8 channels a lane half feeds to which MFMA is algo 0's: CK gives half fh of the wave the channels 16 fh .. 16 fh + 15 of
  // a 32-channel block and spends them in two MFMAs, so MFMA s of block j sums channels 32 j + 8 s + {0..7} and + {16..23}.
  const int fr = lane & 31, fh = lane >> 5;
  const int sw = (fr >> 1) & 7;                  // the tiles start at multiples of 32 rows: (row >> 1) & 7 is the lane's own
  const int xrow = (wm * 32 + fr) * 128;
  const int wrow = kOperandBytes + (wn * 32 + fr) * 128;
  int cs[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) cs[kk] = (((kk >> 1) * 4 + fh * 2 + (kk & 1)) ^ sw) << 4;

  floatx16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0f;

  // K tile t lives in ring buffer t % 3.  Iteration t:
  //   wait     vmcnt(4) lgkmcnt(0): this wave's four loads of K tile t have landed (the four of t + 1 may still fly), and its
  //            fragment reads of t - 1 have retired
  //   barrier  so every wave's loads of t have landed, and every wave is done reading t - 1
  //   read     8 ds_read_b128 from buffer t % 3
  //   stage    K tile t + 2 into buffer (t + 2) % 3, which is (t - 1) % 3: free since the barrier
  //   spend    4 MFMAs
  // landed: a read of K tile t stands behind the barrier that stands behind every wave's wait for it.  free: the restaging of a
  // buffer stands behind the barrier that stands behind the lgkmcnt(0) of every wave's last read of it.  Neither depends on how
  // far apart the waves run: a wave is at most one barrier ahead of another.
  // The last two K tiles stage nothing, and the last waits for everything.  The prologue is K tiles 0 and 1.
  const int kchunks = Cin >> 6, ktiles = 9 * kchunks;   // at least 9, and a multiple of 3: the last K tile is in buffer 2
  int tap2 = kchunks > 2 ? 0 : kchunks == 2 ? 1 : 2, kc2 = kchunks > 2 ? 2 : 0;   // K tile t + 2
  stage(0, 0, 0);
  if (kchunks > 1) stage(0, 1, 1);
  else stage(1, 0, 1);
  int cur = 0, nxt = 2;
  auto ktile = [&](auto mode) {
    constexpr int kMode = decltype(mode)::v;   // 0: a K tile with two more behind it; 1: the last but one; 2: the last
    wait_staged<kMode == 2 ? 0 : kLoadsPerTile>();
    raw_barrier();
    const char* b = lds + cur * kBufBytes;
    half8 xf[4], wf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      wf[kk] = *(const half8*)(b + wrow + cs[kk]);
      xf[kk] = *(const half8*)(b + xrow + cs[kk]);
    }
    __builtin_amdgcn_sched_barrier(0);   // all eight reads are on their way before anything else: the staging's address
    if constexpr (kMode == 0) {          // arithmetic and issue run while they return (-14 % at one row)
      stage(tap2, kc2, nxt);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[kk], xf[kk], acc, 0, 0, 0);
    cur = cur == kStages - 1 ? 0 : cur + 1;
    nxt = nxt == kStages - 1 ? 0 : nxt + 1;
  };
  for (int t = 0; t < ktiles - 2; ++t) {
    ktile(Mode<0>{});
    if (++kc2 == kchunks) { kc2 = 0; ++tap2; }
  }
  ktile(Mode<1>{});
  ktile(Mode<2>{});

  // ---- epilogue.  D = W X^T: the lane's column is position fr of the MFMA tile, its register e is channel (e & 3) + 8 (e >> 2)
  // + 4 fh.  The wave's 32 positions x 32 channels go as rows of four 16-B chunks, chunk g of position p at chunk g ^ ((p >> 2) & 3),
  // into its own 2 KiB of buffer 0: the last K tile is read from buffer 2, and every wave has passed the last barrier, behind
  // its last read of buffers 0 and 1; nothing is in flight (vmcnt(0)).  So no barrier: a wave reads back what it wrote itself.
  char* const cl = lds + wv * kWaveCBytes;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    half4 hv;
#pragma unroll
    for (int i = 0; i < 4; ++i) hv[i] = (_Float16)acc[g * 4 + i];
    *(half4*)(cl + fr * 64 + ((g ^ ((fr >> 2) & 3)) << 4) + fh * 8) = hv;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own writes; nobody else's are read
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int pos = j * 16 + pr;
    const int p = row0 + pos;
    const half8 cv = *(const half8*)(cl + pos * 64 + ((q ^ ((pos >> 2) & 3)) << 4));
    half8 ov;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float v = (float)cv[i];
      v += (float)bv[i];
      if constexpr (kHasRes) v += (float)rv[j][i];
      if (relu) v = fmaxf(v, 0.0f);
      ov[i] = (_Float16)v;
    }
    if (p < M) *(half8*)(y + (size_t)p * K + chan) = ov;
  }
}

// net_conv.hip's DevGuard
struct DevGuard {
  int prev = -1;
  explicit DevGuard(int dev) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
  }
  ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};

}  // namespace

// elfnet_conv3x3_f16_width's argument checks, and C and K multiples of 64.  One launch on `stream`: no allocation, no memset, no
// workspace, no synchronisation, no copy; every refusal comes before it.
extern "C" int elfnet_conv3x3_small_f16(const void* x, const void* w, const void* bias, const void* res, void* y, int64_t rows, int h,
                                        int wd, int c, int k, int relu, void* stream) {
  if (!x || !w || !bias || !y || rows < 0 || h <= 0 || wd <= 0 || c <= 0 || k <= 0) return ELFGO_E_BADARG;
  if ((c & 63) != 0 || (k & 63) != 0) return ELFGO_E_BADARG;
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)y) & 15) != 0) return ELFGO_E_BADARG;
  if (y == x || y == res) return ELFGO_E_BADARG;
  // byte offsets are 32-bit in the kernel: every tensor stays below 2^31 bytes
  const int64_t cmax = c > k ? c : k;
  if (rows * h * wd * cmax >= ((int64_t)1 << 30) || (int64_t)k * 9 * c >= ((int64_t)1 << 30)) return ELFGO_E_BADARG;
  if (rows == 0) return 0;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, x) != hipSuccess) { (void)hipGetLastError(); return ELFGO_E_BADARG; }
  DevGuard _dg(at.device);
  const int64_t m = rows * h * wd;
  const dim3 grid((unsigned)((m + kTileM - 1) / kTileM), (unsigned)(k / kTileN));   // below 2^18 x below 2^15 by the limits above
  hipStream_t st = (hipStream_t)stream;
  if (res)
    hipLaunchKernelGGL(k_conv3x3_small_f16<true>, grid, dim3(kThreads), 0, st, (const char*)x, (const char*)w, (const _Float16*)bias,
                       (const _Float16*)res, (_Float16*)y, (int)m, h, wd, c, k, relu);
  else
    hipLaunchKernelGGL(k_conv3x3_small_f16<false>, grid, dim3(kThreads), 0, st, (const char*)x, (const char*)w, (const _Float16*)bias,
                       (const _Float16*)nullptr, (_Float16*)y, (int)m, h, wd, c, k, relu);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
