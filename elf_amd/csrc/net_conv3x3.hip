// elfnet_conv3x3_f16's algo 1: the trunk convolution y = relu?(conv3x3_same(x, w) + bias (+ res)) as a hand-written implicit GEMM,
// fp16 NHWC in and out, w as [K,3,3,C], fp32 accumulation in v_mfma_f32_32x32x16_f16.  Nothing is unfolded, no workspace.
//
// Why beside CK's kernel (net_conv.hip, algo 0): that one is a 256 x 128 x 32 tile with one LDS stage and two barriers per 32-deep
// K step, and sits on that structure's ceiling.  Here:
//   tile      256 positions x 256 output channels x BK 64 (one tap, 64 consecutive input channels); all of N in one tile, so an
//             activation byte is staged once for every output channel.  512 threads, 8 waves as 2 (positions) x 4 (channels), each
//             owning 128 positions x 64 channels = 4 x 2 MFMA tiles = 128 accumulator registers.  One workgroup per CU.
//   staging   LDS-DMA (global_load_lds_dwordx4) straight into two 64-KiB LDS buffers (activation tile, weight tile: 256 rows of
//             128 B each); the eight pieces of K tile t+1 go out behind the one barrier of K tile t, between the MFMAs of its first
//             two 16-deep steps (their execution hides the issue), and land behind the rest.  One vmcnt(0) + barrier per K tile.
//             Every staged piece is a full aligned 128-B line: 8 lanes per row.
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
//
// The operands are swapped in the MFMA (A = weights, B = activations) so that a lane's accumulator registers run along the
// channels: four consecutive channels of one position per register group, one ds_write_b64 each.
//
// This translation unit includes nothing from CK and nothing of the project but the C header: it is its own object (GNUmakefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

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

template <bool kHasRes>
__global__ __launch_bounds__(kThreads, 2) void k_conv3x3_f16(const char* __restrict__ x, const char* __restrict__ w,
                                                             const _Float16* __restrict__ bias, const _Float16* __restrict__ res,
                                                             _Float16* __restrict__ y, int M, int H, int W, int Cin, int K, int relu) {
  __shared__ __attribute__((aligned(128))) char lds[kLdsBytes];   // ALL of the kernel's LDS: one array
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tile = blockIdx.x, kbase = blockIdx.y * kTileN;

  // ---- staging: wave wv writes the 8-row pieces i * 8 + wv (i = 0..3) of both operands; a lane is row (lane >> 3) of its
  // piece and LDS slot (lane & 7) of that row
  uint32_t xoff[4], woff[4], xmask[4];
  const unsigned char* zsrc = g_zero_line + (lane & 7) * 16;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (i * 8 + wv) * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((r >> 1) & 7);
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
    xmask[i] = m;
    xoff[i] = (uint32_t)p * (uint32_t)(Cin * 2) + chunk * 16;            // below 2^31 wherever it is used (p < M)
    woff[i] = (uint32_t)(kbase + r) * (uint32_t)(9 * Cin * 2) + chunk * 16;
  }
  // piece j of K tile (tap, kc) into buffer buf: j = 0..3 the activation rows, 4..7 the weight rows
  auto piece = [&](int j, int tap, int kc, int buf) {
    char* dst = lds + buf * kBufBytes + wv * 1024;
    if (j < 4) {
      const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
      const uint32_t d = (uint32_t)((dy * W + dx) * Cin * 2 + kc * 128);
      stage16(((xmask[j] >> tap) & 1) ? x + (uint32_t)(xoff[j] + d) : (const char*)zsrc, dst + j * 8192);
    } else {
      stage16(w + (uint32_t)(woff[j - 4] + (uint32_t)(tap * Cin * 2 + kc * 128)), dst + kOperandBytes + (j - 4) * 8192);
    }
  };

  // ---- fragments: lane (fr = lane & 31, fh = lane >> 5) holds row fr of a 32-row MFMA tile and 8 of the 16 k of one MFMA
  const int wm = wv >> 2, wn = wv & 3;
  const int fr = lane & 31, fh = lane >> 5;
  const int sw = (fr >> 1) & 7;                  // the tiles start at multiples of 32 rows: (row >> 1) & 7 is the lane's own
  const int xrow = (wm * 128 + fr) * 128;                      // + mt * 4096
  const int wrow = kOperandBytes + (wn * 64 + fr) * 128;       // + nt * 4096
  // Which 8 channels a lane half feeds to which MFMA is algo 0's: CK gives half fh of the wave the channels 16 fh .. 16 fh + 15 of
  // a 32-channel block and spends them in two MFMAs, so MFMA s of block j sums channels 32 j + 8 s + {0..7} and + {16..23}.
  int cs[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) cs[kk] = (((kk >> 1) * 4 + fh * 2 + (kk & 1)) ^ sw) << 4;

  floatx16 acc[4][2];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mt][nt][e] = 0.0f;

  const int kchunks = Cin >> 6, ktiles = 9 * kchunks;
#pragma unroll
  for (int j = 0; j < 8; ++j) piece(j, 0, 0, 0);
  int tap = 0, kc = 0;
  for (int t = 0; t < ktiles; ++t) {
    // K tile t has landed (this wave's pieces by the count, the others' by the barrier), and every wave is done reading the
    // other buffer (K tile t - 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int ntap = tap, nkc = kc + 1;
    if (nkc == kchunks) { nkc = 0; ++ntap; }
    const bool more = t + 1 < ktiles;
    // K tile t + 1: its eight pieces go out in the first two 16-deep steps, two behind every four MFMAs
    const int nbuf = (t + 1) & 1;
    tap = ntap; kc = nkc;
    const char* b = lds + (t & 1) * kBufBytes;
    // the six fragments of 16-deep step kk + 1 are issued in front of the eight MFMAs of step kk and arrive behind them
    half8 xf[2][4], wf[2][2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) wf[0][nt] = *(const half8*)(b + wrow + nt * 4096 + cs[0]);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) xf[0][mt] = *(const half8*)(b + xrow + mt * 4096 + cs[0]);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int cur = kk & 1, nxt = cur ^ 1;
      if (kk < 3) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) wf[nxt][nt] = *(const half8*)(b + wrow + nt * 4096 + cs[kk + 1]);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) xf[nxt][mt] = *(const half8*)(b + xrow + mt * 4096 + cs[kk + 1]);
      }
      __builtin_amdgcn_sched_barrier(0);   // the reads stay in front of the MFMAs they hide behind (the wait is a counted lgkmcnt)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[cur][nt], xf[cur][mt], acc[mt][nt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (more && kk < 2) { piece(4 * kk, ntap, nkc, nbuf); piece(4 * kk + 1, ntap, nkc, nbuf); }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mt = 2; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[cur][nt], xf[cur][mt], acc[mt][nt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (more && kk < 2) { piece(4 * kk + 2, ntap, nkc, nbuf); piece(4 * kk + 3, ntap, nkc, nbuf); }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue.  D = W X^T: the lane's column is position fr of the tile, its register e is channel (e & 3) + 8 (e >> 2) + 4 fh.
  // C tile in LDS: [256 positions][256 channels] fp16, the 16-B chunk q of position p at chunk q ^ (p & 31).
  __syncthreads();   // the last K tile's fragment reads are done in every wave
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int pos = wm * 128 + mt * 32 + fr;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ch = wn * 64 + nt * 32 + g * 8 + fh * 4;
        half4 hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) hv[e] = (_Float16)acc[mt][nt][g * 4 + e];
        *(half4*)(lds + pos * 512 + (((ch >> 3) ^ (pos & 31)) << 4) + ((ch >> 2) & 1) * 8) = hv;
      }
    }
  const int q = tid & 31;
  const half8 bv = *(const half8*)(bias + kbase + q * 8);
  if constexpr (kHasRes) {
    // the skip's 16 B per (position, chunk) are requested before the barrier, now that the accumulators' registers are free: they
    // arrive while the waves meet.  A row beyond M reads the last valid row instead (no branch around a load) and is not stored.
    half8 rv[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int p = tile * kTileM + it * 16 + (tid >> 5);
      rv[it] = *(const half8*)(res + (size_t)(p < M ? p : M - 1) * K + kbase + q * 8);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int pos = it * 16 + (tid >> 5);
      const int p = tile * kTileM + pos;
      const half8 cv = *(const half8*)(lds + pos * 512 + ((q ^ (pos & 31)) << 4));
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
    for (int it = 0; it < 16; ++it) {
      const int pos = it * 16 + (tid >> 5);
      const int p = tile * kTileM + pos;
      if (p < M) {
        const half8 cv = *(const half8*)(lds + pos * 512 + ((q ^ (pos & 31)) << 4));
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

}  // namespace

// The entry point behind elfnet_conv3x3_f16(algo = 1); net_conv.hip has checked pointers, alignment and the size limits (every
// tensor below 2^31 bytes) and set the device.  One launch on `stream`: no allocation, no memset, no synchronisation, no copy.
// Shapes the kernel does not take are refused with nothing launched.
extern "C" __attribute__((visibility("hidden"))) int elfnet_conv3x3_native_f16(const void* x, const void* w, const void* bias,
                                                                               const void* res, void* y, int64_t rows, int h, int wd,
                                                                               int c, int k, int relu, hipStream_t stream) {
  if ((c & 63) != 0 || (k & 255) != 0) return ELFGO_E_BADARG;
  const int64_t m = rows * h * wd;
  const dim3 grid((unsigned)((m + kTileM - 1) / kTileM), (unsigned)(k / kTileN));
  if (res)
    hipLaunchKernelGGL(k_conv3x3_f16<true>, grid, dim3(kThreads), 0, stream, (const char*)x, (const char*)w, (const _Float16*)bias,
                       (const _Float16*)res, (_Float16*)y, (int)m, h, wd, c, k, relu);
  else
    hipLaunchKernelGGL(k_conv3x3_f16<false>, grid, dim3(kThreads), 0, stream, (const char*)x, (const char*)w, (const _Float16*)bias,
                       (const _Float16*)nullptr, (_Float16*)y, (int)m, h, wd, c, k, relu);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
