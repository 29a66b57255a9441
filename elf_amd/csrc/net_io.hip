// The two ends of the fp16 policy/value net on this library's own kernels, so that a BN-folded net runs from feature rows to pi / V
// as  elfnet_conv3x3_in_f16 -> N x elfnet_conv3x3_f16 -> elfnet_heads_f16  with no MIOpen and no BLAS call in between.
//
// elfnet_conv3x3_in_f16   the input convolution: y = relu?(conv3x3_same(x, w) + bias), x fp16 [rows,H,W,C] with a small even C
//   (18 planes: 36 B per position), w [K,3,3,C], fp32 accumulation in v_mfma_f32_32x32x16_f16.  An implicit GEMM whose K axis is
//   the FLATTENED (tap, channel) index, 9 C long, padded with zeros to a multiple of 16: 11 MFMA steps for C = 18 where a per-tap
//   padding of C to 32 would take 18.
//     tile      64 positions x up to 256 output channels, 512 threads.  Wave v owns the 32 output channels kbase + 32 v .. + 31 for
//               all 64 positions: 2 MFMA tiles, 32 accumulator registers.  A wave whose channels lie beyond K only helps staging.
//               Small on purpose: with the weights below it stays within 128 VGPRs, so two workgroups share a CU and one stages
//               or stores while the other multiplies; there is no pipeline inside a workgroup.
//     weights   in REGISTERS for the whole workgroup: a wave's 32 x Kp weights are its A fragments (4 VGPRs per MFMA step), loaded
//               once; the workgroup then walks over position tiles (grid-stride), so the weights are read once per workgroup.
//     staging   plain 4-B vector loads (C is even, so a channel pair is one aligned dword) build the im2col tile
//               [64 positions][Kp halves] in LDS: eight lanes per position, one dword per lane and MFMA step; an off-board tap
//               and a position at or beyond M store zeros; so do the columns between 9 C and Kp.
//     halo      per position one 9-bit tap mask (position -> h, w), as in net_conv3x3.hip.
//     epilogue  net_conv3x3.hip's: accumulators -> fp16 -> LDS (the staging buffer, reused) -> 16 B of consecutive channels per lane;
//               float(half(acc)) + bias, max(., 0), one rounding to fp16.  Rows at or beyond M are not stored.
//   The operands are swapped (A = weights, B = activations) so that a lane's accumulator registers run along the channels.
//
// elfnet_heads_f16   both heads from the trunk activation, all in fp32:
//     k_head_convs  reads act [rows*d][C] ONCE: per position the three 1x1-convolution outputs (policy 0, policy 1, value) with bias
//                   and ReLU, written to the workspace as P [rows][2][d] (torch's flattening of [B,2,H,W]: c * d + pos) and
//                   V0 [rows][d].  A group of 8 / 16 / 32 lanes shares a position, 16 B per lane, a fixed shuffle tree sums them.
//     k_head_fc     a workgroup takes up to 8 rows: P and V0 into LDS, then one wave per output neuron (pi_linear's d + 1 and
//                   value_linear1's vh), the lanes striding along the weight row, a fixed shuffle tree; softmax and the value's
//                   last layer + tanh from LDS.  No atomics anywhere: repeated launches return the same bits.
//
// This translation unit includes nothing of the project but the C header: it is its own object (GNUmakefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/elf_amd.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// net_conv.hip's device guard (that file is CK's translation unit; engine_host.h pulls the board kernels in)
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

// ------------------------------------------------------------------------------------------------ the input convolution

constexpr int kInTileM = 64;                     // positions per tile
constexpr int kInTileN = 256;                    // output channels per workgroup: 8 waves x 32
constexpr int kInThreads = 512;
constexpr int kInMaxC = 32;
constexpr int kInRowPad = 8;                     // halves behind a row of the im2col tile: rows 16 B apart in the banks
// the im2col tile of the largest C (9 * 32 = 288 halves a row) and the 64 x 256 fp16 C tile of the epilogue share the array
constexpr int kInLdsBytes = kInTileM * (9 * kInMaxC + kInRowPad) * 2 > kInTileM * kInTileN * 2 ? kInTileM * (9 * kInMaxC + kInRowPad) * 2
                                                                                                 : kInTileM * kInTileN * 2;

// what an off-board tap, a position beyond M and the K padding are staged from
__device__ uint32_t g_zero_word = 0;

// kSteps: MFMA steps of 16 along the padded K axis (11 covers C <= 18, 18 covers C <= 32)
template <int kSteps>
__global__ __launch_bounds__(kInThreads, kSteps <= 11 ? 4 : 2) void k_conv3x3_in_f16(   // second bound: waves per SIMD
    const uint32_t* __restrict__ x, const _Float16* __restrict__ w, const _Float16* __restrict__ bias, _Float16* __restrict__ y, int M,
    int H, int W, int Cin, int K, int relu) {
  __shared__ __attribute__((aligned(16))) char lds[kInLdsBytes];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kbase = blockIdx.y * kInTileN;
  const int c2 = Cin >> 1;                        // dwords per tap
  const int kreal = 9 * Cin;                      // halves of the flattened K axis
  // every instance runs all of its kSteps steps, whatever C: the columns from 9 C on are zeros in LDS and in the weight fragments, and
  // nothing in the loops below branches on C
  constexpr int rowb = (kSteps * 16 + kInRowPad) * 2;   // bytes per row of the im2col tile: a multiple of 16
  const int c2inv = (65536 + c2 - 1) / c2;
  const int fr = lane & 31, fh = lane >> 5;

  // ---- the wave's weights: A fragment of step s = row (channel) fr, k = 16 s + 8 fh .. + 7 of the flattened [9 C] weight row;
  // zeros beyond 9 C (9 C is even: a pair is inside or outside as a whole)
  const bool has_n = kbase + wv * 32 < K;         // wave-uniform
  u32x4 wf[kSteps];                               // four packed pairs = the half8 of one MFMA step
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const uint32_t* wr = (const uint32_t*)(w + (size_t)(has_n ? kbase + wv * 32 + fr : 0) * kreal);   // 9 C is even: rows are 4-B aligned
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = s * 16 + fh * 8 + 2 * e;
      wf[s][e] = *(has_n && k < kreal ? wr + (k >> 1) : &g_zero_word);
    }
  }
  const int q = tid & 31;                         // the epilogue's 16-B chunk of the channel axis
  const bool has_q = kbase + q * 8 < K;
  half8 bv;
#pragma unroll
  for (int e = 0; e < 8; ++e) bv[e] = (_Float16)0.0f;
  if (has_q) bv = *(const half8*)(bias + kbase + q * 8);

  const int ntiles = (M + kInTileM - 1) / kInTileM;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // ---- staging: lanes 8 r .. 8 r + 7 build row r, lane `sub` its dwords sub, sub + 8, ...: exactly one per MFMA step.  Dword j of a
    // row is channel pair j % (C/2) of tap j / (C/2); the columns from 9 C on (up to the instance's 16 kSteps) are the K padding.
    {
      const int r = tid >> 3;
      int sub = tid & 7;
      // opaque per tile: the per-step offsets below would otherwise be hoisted out of the tile loop and held in 2 x kSteps registers
      asm volatile("" : "+v"(sub));
      const int p = tile * kInTileM + r;
      uint32_t m = 0;
      if (p < M) {
        const int rem = p % (H * W), hh = rem / W, ww = rem - hh * W;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int dy = tap / 3 - 1, dx = tap % 3 - 1;
          if ((unsigned)(hh + dy) < (unsigned)H && (unsigned)(ww + dx) < (unsigned)W) m |= 1u << tap;
        }
      }
      uint32_t* row = (uint32_t*)(lds + r * rowb);
      const uint32_t pc = (uint32_t)p * (uint32_t)c2;   // x is below 2^31 bytes: a dword index fits 32 bits wherever it is used
      uint32_t v[kSteps];
#pragma unroll
      for (int i = 0; i < kSteps; ++i) {
        const int j = sub + 8 * i;
        const int tap = (j * c2inv) >> 16;         // j / c2, exact for j < 144 (c2inv = ceil(65536 / c2), c2 <= 16)
        const int ty = (tap * 11) >> 5;            // tap / 3 for tap < 9
        const int off = ((ty - 1) * W + (tap - 3 * ty - 1)) * c2 + (j - tap * c2);
        // in bounds wherever the mask bit is set; tap >= 9 (the padding) has no bit.  The load is unconditional (no branch
        // around it, no select behind it): where the bit is clear its source is a zero word in global memory.
        const bool ok = tap < 9 && ((m >> (tap & 31)) & 1);
        v[i] = *(ok ? x + (uint32_t)(pc + (uint32_t)off) : &g_zero_word);
      }
#pragma unroll
      for (int i = 0; i < kSteps; ++i) row[sub + 8 * i] = v[i];
    }
    __syncthreads();

    // ---- MFMA: D = W X^T, 32 channels x 32 positions per tile, K ascending
    floatx16 acc[kInTileM / 32];
#pragma unroll
    for (int mt = 0; mt < kInTileM / 32; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mt][e] = 0.0f;
    if (has_n) {
      // the fragments of step s + 1 are requested in front of step s's MFMAs; the scheduling barrier keeps the compiler from
      // hoisting every step's reads to the top (two fragments in flight are enough with four waves on a SIMD, and the registers
      // are what lets two workgroups share a CU)
      const char* xb = lds + fr * rowb + fh * 16;
      half8 xf[kInTileM / 32], xn[kInTileM / 32];
#pragma unroll
      for (int mt = 0; mt < kInTileM / 32; ++mt) xf[mt] = *(const half8*)(xb + mt * 32 * rowb);
#pragma unroll
      for (int s = 0; s < kSteps; ++s) {
        if (s + 1 < kSteps) {
#pragma unroll
          for (int mt = 0; mt < kInTileM / 32; ++mt) xn[mt] = *(const half8*)(xb + mt * 32 * rowb + (s + 1) * 32);
        }
#pragma unroll
        for (int mt = 0; mt < kInTileM / 32; ++mt)
          acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, wf[s]), xf[mt], acc[mt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < kInTileM / 32; ++mt) xf[mt] = xn[mt];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();   // every wave has read its fragments: the array becomes the C tile

    // ---- epilogue.  The lane's column is position fr of the MFMA tile, its register e is channel (e & 3) + 8 (e >> 2) + 4 fh.
    // C tile: [64 positions][256 channels] fp16, the 16-B chunk c of position p at chunk c ^ (p & 31).
    if (has_n) {
#pragma unroll
      for (int mt = 0; mt < kInTileM / 32; ++mt) {
        const int pos = mt * 32 + fr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ch = wv * 32 + g * 8 + fh * 4;
          half4 hv;
#pragma unroll
          for (int e = 0; e < 4; ++e) hv[e] = (_Float16)acc[mt][g * 4 + e];
          *(half4*)(lds + pos * 512 + (((ch >> 3) ^ (pos & 31)) << 4) + ((ch >> 2) & 1) * 8) = hv;
        }
      }
    }
    __syncthreads();
    if (has_q) {
#pragma unroll
      for (int it = 0; it < kInTileM / 16; ++it) {
        const int pos = it * 16 + (tid >> 5);
        const int p = tile * kInTileM + pos;
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
    __syncthreads();   // the C tile is read: the next tile's staging may overwrite it
  }
}

// ------------------------------------------------------------------------------------------------ the heads

constexpr int kHcThreads = 256;
constexpr int kHcUnroll = 4;                     // positions a lane group has in flight

// kG lanes share a position: lane l of the group takes the 16-B chunks l, l + kG, ... of its C channels
template <int kG>
__global__ __launch_bounds__(kHcThreads) void k_head_convs(const _Float16* __restrict__ act, const _Float16* __restrict__ pw,
                                                           const _Float16* __restrict__ pb, const _Float16* __restrict__ vw,
                                                           const _Float16* __restrict__ vb, float* __restrict__ P, float* __restrict__ V0,
                                                           int M, int d, int C) {
  const int l = threadIdx.x & (kG - 1);
  const int c8 = C >> 3;
  const int groups = gridDim.x * (kHcThreads / kG);
  const int gid = blockIdx.x * (kHcThreads / kG) + threadIdx.x / kG;
  // the group's first chunk of the three weight rows stays in registers (C <= 8 kG: all of them)
  float w0[8], w1[8], w2[8];
  {
    half8 a, b, c;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = b[e] = c[e] = (_Float16)0.0f;
    if (l < c8) {
      a = *(const half8*)(pw + l * 8);
      b = *(const half8*)(pw + C + l * 8);
      c = *(const half8*)(vw + l * 8);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { w0[e] = (float)a[e]; w1[e] = (float)b[e]; w2[e] = (float)c[e]; }
  }
  const float b0 = (float)pb[0], b1 = (float)pb[1], b2 = (float)vb[0];

  for (int base = gid; base < M; base += groups * kHcUnroll) {
    half8 av[kHcUnroll];
#pragma unroll
    for (int u = 0; u < kHcUnroll; ++u) {
      const int p = base + u * groups;
#pragma unroll
      for (int e = 0; e < 8; ++e) av[u][e] = (_Float16)0.0f;
      if (p < M && l < c8) av[u] = *(const half8*)(act + (size_t)p * C + l * 8);
    }
#pragma unroll
    for (int u = 0; u < kHcUnroll; ++u) {
      const int p = base + u * groups;   // uniform over the group
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float a = (float)av[u][e];
        s0 += a * w0[e]; s1 += a * w1[e]; s2 += a * w2[e];
      }
      if (p < M)
        for (int qq = l + kG; qq < c8; qq += kG) {   // C above 8 kG: the further chunks' weights come from memory
          const half8 a8 = *(const half8*)(act + (size_t)p * C + qq * 8);
          const half8 x0 = *(const half8*)(pw + qq * 8), x1 = *(const half8*)(pw + C + qq * 8), x2 = *(const half8*)(vw + qq * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float a = (float)a8[e];
            s0 += a * (float)x0[e]; s1 += a * (float)x1[e]; s2 += a * (float)x2[e];
          }
        }
#pragma unroll
      for (int o = kG >> 1; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o);
      }
      if (p < M && l == 0) {
        const int row = p / d, pos = p - row * d;
        P[(size_t)row * 2 * d + pos] = fmaxf(s0 + b0, 0.0f);
        P[(size_t)row * 2 * d + d + pos] = fmaxf(s1 + b1, 0.0f);
        V0[(size_t)row * d + pos] = fmaxf(s2 + b2, 0.0f);
      }
    }
  }
}

constexpr int kFcThreads = 256;
constexpr int kFcRows = 8;                       // rows a workgroup takes at most

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// dynamic LDS, floats: P [rpb][2 d] | V0 [rpb][d] | logits [rpb][d + 1] | v1 [rpb][vh]
__global__ __launch_bounds__(kFcThreads) void k_head_fc(const float* __restrict__ P, const float* __restrict__ V0,
                                                        const _Float16* __restrict__ piw, const _Float16* __restrict__ pib,
                                                        const _Float16* __restrict__ v1w, const _Float16* __restrict__ v1b,
                                                        const _Float16* __restrict__ v2w, const _Float16* __restrict__ v2b,
                                                        float* __restrict__ pi, int64_t pi_stride, float* __restrict__ value,
                                                        float* __restrict__ logits, int rows, int d, int vh, int rpb) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r0 = blockIdx.x * rpb;
  const int nr = min(rpb, rows - r0);
  float* sP = sm;
  float* sV = sP + rpb * 2 * d;
  float* sL = sV + rpb * d;
  float* s1 = sL + rpb * (d + 1);
  for (int i = tid; i < nr * 2 * d; i += kFcThreads) sP[i] = P[(size_t)r0 * 2 * d + i];
  for (int i = tid; i < nr * d; i += kFcThreads) sV[i] = V0[(size_t)r0 * d + i];
  __syncthreads();

  // one wave per output neuron: j < d + 1 is a logit (weight row of 2 d halves: d aligned pairs), the others value_linear1's
  const int nout = d + 1 + vh;
  for (int j = wv; j < nout; j += kFcThreads / 64) {
    float acc[kFcRows];
#pragma unroll
    for (int r = 0; r < kFcRows; ++r) acc[r] = 0.0f;
    if (j <= d) {
      const half2v* wr = (const half2v*)(piw + (size_t)j * 2 * d);
      for (int t = lane; t < d; t += 64) {
        const half2v w2 = wr[t];
        const float wl = (float)w2[0], wh = (float)w2[1];
#pragma unroll
        for (int r = 0; r < kFcRows; ++r)
          if (r < nr) {
            const float2 pv = *(const float2*)(sP + r * 2 * d + 2 * t);
            acc[r] += wl * pv.x;
            acc[r] += wh * pv.y;
          }
      }
    } else {
      const _Float16* wr = v1w + (size_t)(j - d - 1) * d;   // d may be odd: rows are 2-B aligned only
      for (int t = lane; t < d; t += 64) {
        const float wl = (float)wr[t];
#pragma unroll
        for (int r = 0; r < kFcRows; ++r)
          if (r < nr) acc[r] += wl * sV[r * d + t];
      }
    }
#pragma unroll
    for (int r = 0; r < kFcRows; ++r)
      if (r < nr) acc[r] = wave_sum(acc[r]);
    if (lane == 0) {
      if (j <= d) {
        const float b = (float)pib[j];
#pragma unroll
        for (int r = 0; r < kFcRows; ++r)
          if (r < nr) sL[r * (d + 1) + j] = acc[r] + b;
      } else {
        const float b = (float)v1b[j - d - 1];
#pragma unroll
        for (int r = 0; r < kFcRows; ++r)
          if (r < nr) s1[r * vh + (j - d - 1)] = fmaxf(acc[r] + b, 0.0f);
      }
    }
  }
  __syncthreads();

  // one wave per row: softmax over the d + 1 logits, and tanh(v2_w . v1 + v2_b)
  for (int r = wv; r < nr; r += kFcThreads / 64) {
    const float* lg = sL + r * (d + 1);
    float mx = -INFINITY;
    for (int t = lane; t <= d; t += 64) mx = fmaxf(mx, lg[t]);
    mx = wave_max(mx);
    float sum = 0.0f;
    for (int t = lane; t <= d; t += 64) sum += expf(lg[t] - mx);
    sum = wave_sum(sum);
    float* po = pi + (size_t)(r0 + r) * pi_stride;
    for (int t = lane; t <= d; t += 64) po[t] = expf(lg[t] - mx) / sum;
    if (logits) {
      float* lo = logits + (size_t)(r0 + r) * pi_stride;
      for (int t = lane; t <= d; t += 64) lo[t] = lg[t];
    }
    float v = 0.0f;
    for (int t = lane; t < vh; t += 64) v += (float)v2w[t] * s1[r * vh + t];
    v = wave_sum(v);
    if (lane == 0) value[r0 + r] = tanhf(v + (float)v2b[0]);
  }
}

inline size_t heads_ws_bytes(int64_t rows, int64_t d) { return (size_t)rows * 3 * (size_t)d * sizeof(float); }

}  // namespace

extern "C" int elfnet_conv3x3_in_f16(const void* x, const void* w, const void* bias, void* y, int64_t rows, int h, int wd, int c, int k,
                                     int relu, void* stream) {
  if (!x || !w || !bias || !y || rows < 0 || h <= 0 || wd <= 0) return ELFGO_E_BADARG;
  if (c < 2 || c > kInMaxC || (c & 1) != 0 || k <= 0 || (k & 31) != 0) return ELFGO_E_BADARG;
  if ((((uintptr_t)w | (uintptr_t)bias | (uintptr_t)y) & 15) != 0 || ((uintptr_t)x & 3) != 0) return ELFGO_E_BADARG;
  if (y == x) return ELFGO_E_BADARG;
  // every tensor below 2^31 bytes, as for elfnet_conv3x3_f16 (k >= c here)
  if (rows * h * wd * k >= ((int64_t)1 << 30) || (int64_t)k * 9 * c >= ((int64_t)1 << 30)) return ELFGO_E_BADARG;
  if (rows == 0) return 0;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, x) != hipSuccess) { (void)hipGetLastError(); return ELFGO_E_BADARG; }
  DevGuard _dg(at.device);
  const int m = (int)(rows * h * wd);
  const int tiles = (m + kInTileM - 1) / kInTileM;
  const int gy = (k + kInTileN - 1) / kInTileN;
  // two workgroups (16 waves of at most 128 VGPRs, 37 KiB of LDS each) share a CU: 512 of them fill 256 CUs, and each walks over
  // its share of the tiles
  const int gx = tiles < 512 / gy ? tiles : (512 / gy > 0 ? 512 / gy : 1);
  const dim3 grid((unsigned)gx, (unsigned)gy);
  hipStream_t st = (hipStream_t)stream;
  if (9 * c <= 11 * 16)
    hipLaunchKernelGGL(k_conv3x3_in_f16<11>, grid, dim3(kInThreads), 0, st, (const uint32_t*)x, (const _Float16*)w, (const _Float16*)bias,
                       (_Float16*)y, m, h, wd, c, k, relu);
  else
    hipLaunchKernelGGL(k_conv3x3_in_f16<18>, grid, dim3(kInThreads), 0, st, (const uint32_t*)x, (const _Float16*)w, (const _Float16*)bias,
                       (_Float16*)y, m, h, wd, c, k, relu);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" size_t elfnet_heads_workspace(int64_t rows, int h, int wd) {
  if (rows < 0 || h <= 0 || wd <= 0) return 0;
  // never 0 for a valid shape: a caller may allocate it as it is
  return (heads_ws_bytes(rows > 0 ? rows : 1, (int64_t)h * wd) + 255) & ~(size_t)255;
}

extern "C" int elfnet_heads_f16(const void* act, const ElfNetHeads* hd, int64_t rows, int h, int wd, float* pi, int64_t pi_stride,
                                float* value, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
  if (!act || !hd || !pi || !value || !workspace || rows < 0 || h <= 0 || wd <= 0) return ELFGO_E_BADARG;
  if (!hd->pconv_w || !hd->pconv_b || !hd->vconv_w || !hd->vconv_b || !hd->pi_w || !hd->pi_b || !hd->v1_w || !hd->v1_b || !hd->v2_w ||
      !hd->v2_b)
    return ELFGO_E_BADARG;
  const int C = hd->channels, vh = hd->value_hidden;
  const int64_t d = (int64_t)h * wd;
  if (C <= 0 || (C & 7) != 0 || vh <= 0 || pi_stride < d + 1) return ELFGO_E_BADARG;
  if (rows * d >= ((int64_t)1 << 31) || d > (1 << 20) || vh > (1 << 20)) return ELFGO_E_BADARG;
  if (workspace_bytes < heads_ws_bytes(rows, d)) return ELFGO_E_BADARG;
  // 16-B loads of act and the head-conv weights, 4-B pairs of pi_w, floats in the workspace and the outputs
  if ((((uintptr_t)act | (uintptr_t)hd->pconv_w | (uintptr_t)hd->vconv_w) & 15) != 0) return ELFGO_E_BADARG;
  if ((((uintptr_t)hd->pi_w | (uintptr_t)workspace | (uintptr_t)pi | (uintptr_t)value | (uintptr_t)logits) & 3) != 0) return ELFGO_E_BADARG;
  // rows per workgroup of k_head_fc: enough workgroups for the chip first, then fewer passes over the weights; within 64 KiB of LDS
  int rpb = (int)(rows / 256);
  rpb = rpb < 1 ? 1 : rpb > kFcRows ? kFcRows : rpb;
  const size_t per_row = (size_t)(2 * d + d + d + 1 + vh) * sizeof(float);
  while (rpb > 1 && rpb * per_row > 65536) --rpb;
  if (per_row > 65536) return ELFGO_E_BADARG;
  if (rows == 0) return 0;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, act) != hipSuccess) { (void)hipGetLastError(); return ELFGO_E_BADARG; }
  DevGuard _dg(at.device);
  hipStream_t st = (hipStream_t)stream;
  const int m = (int)(rows * d);
  float* P = (float*)workspace;
  float* V0 = P + (size_t)rows * 2 * d;
  const _Float16 *pw = (const _Float16*)hd->pconv_w, *pb = (const _Float16*)hd->pconv_b, *vw = (const _Float16*)hd->vconv_w,
                 *vb = (const _Float16*)hd->vconv_b;
  const int c8 = C >> 3;
  const int g = c8 <= 8 ? 8 : c8 <= 16 ? 16 : 32;
  const int per_block = kHcThreads / g * kHcUnroll;
  int blocks = (m + per_block - 1) / per_block;
  if (blocks > 2048) blocks = 2048;
  if (g == 8)
    hipLaunchKernelGGL(k_head_convs<8>, dim3(blocks), dim3(kHcThreads), 0, st, (const _Float16*)act, pw, pb, vw, vb, P, V0, m, (int)d, C);
  else if (g == 16)
    hipLaunchKernelGGL(k_head_convs<16>, dim3(blocks), dim3(kHcThreads), 0, st, (const _Float16*)act, pw, pb, vw, vb, P, V0, m, (int)d, C);
  else
    hipLaunchKernelGGL(k_head_convs<32>, dim3(blocks), dim3(kHcThreads), 0, st, (const _Float16*)act, pw, pb, vw, vb, P, V0, m, (int)d, C);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_head_fc, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(kFcThreads), rpb * per_row, st, P, V0,
                     (const _Float16*)hd->pi_w, (const _Float16*)hd->pi_b, (const _Float16*)hd->v1_w, (const _Float16*)hd->v1_b,
                     (const _Float16*)hd->v2_w, (const _Float16*)hd->v2_b, pi, pi_stride, value, logits, (int)rows, (int)d, vh, rpb);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
