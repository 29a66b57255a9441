// The two ends of the policy/value net on this library's own kernels, for fp16 and for bf16, so that a BN-folded net runs from
// feature rows to pi / V as  elfnet_conv3x3_in_<t> -> N x elfnet_conv3x3_<t> -> elfnet_heads_<t>  with no MIOpen and no BLAS call in
// between.  Every kernel and every host check is written once and takes the element type as a trait (F16, Bf16 below), which
// carries only what differs: the MFMA, how a dword becomes two floats, the heads' 16-byte dot product and the input convolution's
// epilogue.  The launch geometry, the refusals and their order are the same for both types.
//
// elfnet_conv3x3_in_f16 / _bf16   the input convolution: y = relu?(conv3x3_same(x, w) + bias), x [rows,H,W,C] with a small even C
//   (18 planes: 36 B per position), w [K,3,3,C], fp32 accumulation in v_mfma_f32_32x32x16_f16 / _bf16.  An implicit GEMM whose K
//   axis is the FLATTENED (tap, channel) index, 9 C long, padded with zeros to a multiple of 16: 11 MFMA steps for C = 18 where a
//   per-tap padding of C to 32 would take 18 (the 18-step instance covers C <= 32).
//     tile      64 positions x up to 256 output channels, 512 threads.  Wave v owns the 32 output channels kbase + 32 v .. + 31 for
//               all 64 positions: 2 MFMA tiles, 32 accumulator registers.  A wave whose channels lie beyond K only helps staging
//               (K = 288: the second workgroup along k has one wave with channels, 256 .. 287, and seven that stage).
//     weights   in REGISTERS for the whole workgroup: a wave's 32 x Kp weights are its A fragments (4 VGPRs per MFMA step), loaded
//               once.  The 11-step instances stay within 128 VGPRs with no scratch, so two workgroups of 8 waves share a CU and one
//               stages or stores while the other multiplies; there is no pipeline inside a workgroup.  The 18-step ones take 160:
//               one workgroup per CU.
//     staging   plain 4-B vector loads (C is even, so a channel pair is one aligned dword) build the im2col tile
//               [64 positions][Kp elements] in LDS: eight lanes per position, one dword per lane and MFMA step.  The bf16 entry
//               with x_is_f16 converts the dword on its way, fp16 -> fp32 (exact) -> bf16, round to nearest even: bit for bit what
//               it computes on x.bfloat16().
//     zeros     an off-board tap, a position at or beyond M and the columns between 9 C and Kp are loaded from one zero word in
//               global memory (no branch around a load, no second path that clears LDS).  Per position one 9-bit tap mask
//               (position -> h, w), as in net_conv3x3.hip; rows at or beyond M have an empty mask and are not stored.
//     epilogue  through LDS (the staging array, reused as the C tile [64 positions][256 channels], chunk c of position p at chunk
//               c ^ (p & 31)), which turns four channels per lane into 16 B of consecutive channels per lane for the stores:
//                 fp16   net_conv3x3.hip's: the accumulator is rounded to fp16 on its way into LDS; behind it
//                        float(half(acc)) + bias, max(., 0), a second rounding to fp16.
//                 bf16   in registers, before the transposition: acc + bias in fp32, fmaxf(., 0), ONE round-to-nearest-even to
//                        bf16 (the trunk's rule, net_conv3x3_bf16.hip); what goes through LDS is the finished value.
//     grid      (min(tiles, 512 / gy), gy) workgroups, tiles = ceil(M / 64), gy = ceil(K / 256): two workgroups per CU on 256
//               CUs; workgroup bx takes the position tiles bx, bx + gridDim.x, ..., so the weights are read once per workgroup.
//   The operands are swapped (A = weights, B = activations) so that a lane's accumulator registers run along the channels.
//
// elfnet_heads_f16 / _bf16   both heads from the trunk activation, all in fp32, nothing rounded on the way:
//     k_head_convs  reads act [rows*d][C] ONCE: per position the three 1x1-convolution outputs (policy 0, policy 1, value) with bias
//                   and ReLU, written to the workspace as P [rows][2][d] (torch's flattening of [B,2,H,W]: c * d + pos) and
//                   V0 [rows][d].  A group of 8 / 16 / 32 lanes shares a position, 16 B per lane and chunk; the type's dot3 sums a
//                   chunk, a fixed shuffle tree sums the group:
//                     fp16   one chain per output over the chunk's eight channels in order (hardware converts);
//                     bf16   per output one chain over the dwords' low halves (even channels) and one over their high halves,
//                            low + high at the end: a bf16 value IS the upper half of its fp32 (v << 16, v & 0xffff0000), so
//                            there is no convert anywhere, and the six chains are independent.
//     k_head_fc     a workgroup (1024 threads) takes up to 8 rows: P and V0 into LDS, then one wave per output neuron (pi_linear's
//                   d + 1 and value_linear1's vh), the lanes striding along the weight row; the 8 rows' partial sums are reduced
//                   together by one transposed shuffle tree (10 shuffles, not 8 x 6) that gives every row the plain butterfly's
//                   order; softmax and the value's last layer + tanh from LDS.
//   No atomics anywhere, and every sum's order is fixed by the shape of one row: repeated launches return the same bits, and a
//   row's bits do not depend on the rows around it.
//
// This translation unit includes nothing of the project but net_common.h: it is its own object (GNUmakefile).
#include <type_traits>

#include "net_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef uint32_t uint32x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------ what differs between the types

struct F16 {
  typedef _Float16 elem;
  typedef half8 vec8;
  typedef half4 vec4;
  static constexpr bool kEpilogueInRegs = false;
  static __device__ __forceinline__ floatx16 mfma(vec8 a, vec8 b, floatx16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  // the two values of a dword as fp32
  static __device__ __forceinline__ float low(uint32_t v) { return (float)__builtin_bit_cast(half2v, v)[0]; }
  static __device__ __forceinline__ float high(uint32_t v) { return (float)__builtin_bit_cast(half2v, v)[1]; }
  // dot3: one 16-B chunk of a position against the same chunk of the three weight rows, added to the lane's partial sums, which
  // live in the caller as lo[3] and hi[3] (zero at first); total() is output i's sum.  Here one chain per output over the eight
  // channels in order: hi is left alone and total() does not add it, so no + 0.0f enters the chain.
  static __device__ __forceinline__ void dot3(const uint32x4 a, const uint32x4 w0, const uint32x4 w1, const uint32x4 w2, float lo[3], float hi[3]) {
    const half8 ah = __builtin_bit_cast(half8, a), x0 = __builtin_bit_cast(half8, w0), x1 = __builtin_bit_cast(half8, w1),
                x2 = __builtin_bit_cast(half8, w2);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = (float)ah[e];
      lo[0] += v * (float)x0[e]; lo[1] += v * (float)x1[e]; lo[2] += v * (float)x2[e];
    }
  }
  static __device__ __forceinline__ float total(const float lo[3], const float hi[3], int i) { return lo[i]; }
};

struct Bf16 {
  typedef __bf16 elem;
  typedef bf16x8 vec8;
  typedef bf16x4 vec4;
  static constexpr bool kEpilogueInRegs = true;
  static __device__ __forceinline__ floatx16 mfma(vec8 a, vec8 b, floatx16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  // the value's 16 bits are the upper 16 of its fp32
  static __device__ __forceinline__ float low(uint32_t v) { return __uint_as_float(v << 16); }
  static __device__ __forceinline__ float high(uint32_t v) { return __uint_as_float(v & 0xffff0000u); }
  // two chains per output: lo[] sums the even channels (the dwords' low halves), hi[] the odd ones; lo + hi at the end
  static __device__ __forceinline__ void dot3(const uint32x4 a, const uint32x4 w0, const uint32x4 w1, const uint32x4 w2, float lo[3], float hi[3]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float al = low(a[i]), ah = high(a[i]);
      lo[0] += al * low(w0[i]); hi[0] += ah * high(w0[i]);
      lo[1] += al * low(w1[i]); hi[1] += ah * high(w1[i]);
      lo[2] += al * low(w2[i]); hi[2] += ah * high(w2[i]);
    }
  }
  static __device__ __forceinline__ float total(const float lo[3], const float hi[3], int i) { return lo[i] + hi[i]; }
};

// element i of an array of T's 2-byte elements as fp32
template <typename T>
__device__ __forceinline__ float elem_at(const void* p, int i) { return T::low(((const uint16_t*)p)[i]); }

// ------------------------------------------------------------------------------------------------ the input convolution

constexpr int kInTileM = 64;                     // positions per tile
constexpr int kInTileN = 256;                    // output channels per workgroup: 8 waves x 32
constexpr int kInThreads = 512;
constexpr int kInMaxC = 32;
constexpr int kInRowPad = 8;                     // elements behind a row of the im2col tile: rows 16 B apart in the banks
// the im2col tile of the largest C (9 * 32 = 288 elements a row) and the 64 x 256 C tile of the epilogue share the array
constexpr int kInCTileBytes = kInTileM * kInTileN * 2;
constexpr int kInStageBytes = kInTileM * (9 * kInMaxC + kInRowPad) * 2;
constexpr int kInLdsBytes = kInStageBytes > kInCTileBytes ? kInStageBytes : kInCTileBytes;

// what an off-board tap, a position beyond M and the K padding are staged from
__device__ uint32_t g_zero_word = 0;

// two fp16 -> two bf16 through fp32, round to nearest even
__device__ __forceinline__ uint32_t f16x2_to_bf16x2(uint32_t u) {
  const half2v h = __builtin_bit_cast(half2v, u);
  bf16x2 o;
  o[0] = (__bf16)(float)h[0];
  o[1] = (__bf16)(float)h[1];
  return __builtin_bit_cast(uint32_t, o);
}

// kSteps: MFMA steps of 16 along the padded K axis (11 covers C <= 18, 18 covers C <= 32).  kCvtX: x holds fp16, T is Bf16
template <int kSteps, typename T, bool kCvtX>
__global__ __launch_bounds__(kInThreads, kSteps <= 11 ? 4 : 2) void k_conv3x3_in(   // second bound: waves per SIMD
    const uint32_t* __restrict__ x, const uint16_t* __restrict__ w, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int M,
    int H, int W, int Cin, int K, int relu) {
  typedef typename T::vec8 vec8;
  typedef typename T::vec4 vec4;
  __shared__ __attribute__((aligned(16))) char lds[kInLdsBytes];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kbase = blockIdx.y * kInTileN;
  const int c2 = Cin >> 1;                        // dwords per tap
  const int kreal = 9 * Cin;                      // elements of the flattened K axis
  // every instance runs all of its kSteps steps, whatever C: the columns from 9 C on are zeros in LDS and in the weight fragments, and
  // nothing in the loops below branches on C
  constexpr int rowb = (kSteps * 16 + kInRowPad) * 2;   // bytes per row of the im2col tile: a multiple of 16
  const int c2inv = (65536 + c2 - 1) / c2;
  const int fr = lane & 31, fh = lane >> 5;

  // ---- the wave's weights: A fragment of step s = row (channel) fr, k = 16 s + 8 fh .. + 7 of the flattened [9 C] weight row;
  // zeros beyond 9 C (9 C is even: a pair is inside or outside as a whole)
  const bool has_n = kbase + wv * 32 < K;         // wave-uniform; K is a multiple of 32: all 32 channels or none
  uint32x4 wf[kSteps];                              // four packed pairs = the vec8 of one MFMA step
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const uint32_t* wr = (const uint32_t*)(w + (size_t)(has_n ? kbase + wv * 32 + fr : 0) * kreal);   // 9 C is even: rows are 4-B aligned
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = s * 16 + fh * 8 + 2 * e;
      wf[s][e] = *(has_n && k < kreal ? wr + (k >> 1) : &g_zero_word);
    }
  }
  // ---- the biases, where the type's epilogue adds them.  In registers (bq): the lane's accumulator register 4 g + e is channel
  // 8 g + 4 fh + e of the wave's 32, its four biases are two dwords.  Behind LDS (bv): the eight of the store's 16-B chunk q.
  uint32x2 bq[4];
  vec8 bv;
  if constexpr (T::kEpilogueInRegs) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bq[g][0] = bq[g][1] = 0;
      if (has_n) bq[g] = *(const uint32x2*)(bias + kbase + wv * 32 + g * 8 + fh * 4);
    }
  }
  const int q = tid & 31;                         // the store's 16-B chunk of the channel axis
  const bool has_q = kbase + q * 8 < K;
  if constexpr (!T::kEpilogueInRegs) {
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = (typename T::elem)0.0f;
    if (has_q) bv = *(const vec8*)(bias + kbase + q * 8);
  }

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
        // in bounds wherever the mask bit is set (p < M and the tap's cell is on p's own board); tap >= 9 (the padding) has no
        // bit.  The load is unconditional (no branch around it, no select behind it): where the bit is clear its source is the
        // zero word.
        const bool ok = tap < 9 && ((m >> (tap & 31)) & 1);
        v[i] = *(ok ? x + (uint32_t)(pc + (uint32_t)off) : &g_zero_word);
      }
#pragma unroll
      for (int i = 0; i < kSteps; ++i) row[sub + 8 * i] = kCvtX ? f16x2_to_bf16x2(v[i]) : v[i];
    }
    __syncthreads();

    // ---- MFMA: D = W X^T, 32 channels x 32 positions per tile, K ascending, one accumulator per output from zero
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
      vec8 xf[kInTileM / 32], xn[kInTileM / 32];
#pragma unroll
      for (int mt = 0; mt < kInTileM / 32; ++mt) xf[mt] = *(const vec8*)(xb + mt * 32 * rowb);
#pragma unroll
      for (int s = 0; s < kSteps; ++s) {
        if (s + 1 < kSteps) {
#pragma unroll
          for (int mt = 0; mt < kInTileM / 32; ++mt) xn[mt] = *(const vec8*)(xb + mt * 32 * rowb + (s + 1) * 32);
        }
#pragma unroll
        for (int mt = 0; mt < kInTileM / 32; ++mt) acc[mt] = T::mfma(__builtin_bit_cast(vec8, wf[s]), xf[mt], acc[mt]);
#pragma unroll
        for (int mt = 0; mt < kInTileM / 32; ++mt) xf[mt] = xn[mt];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();   // every wave has read its fragments: the array becomes the C tile

    // ---- epilogue.  The lane's column is position fr of the MFMA tile, its register 4 g + e is channel 8 g + 4 fh + e: 8 B per
    // (position, g) into the C tile.  In registers: acc + bias, fmaxf, the ONE rounding.  Otherwise: the accumulator, rounded.
    if (has_n) {
#pragma unroll
      for (int mt = 0; mt < kInTileM / 32; ++mt) {
        const int pos = mt * 32 + fr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ch = wv * 32 + g * 8 + fh * 4;
          vec4 ov;
          if constexpr (T::kEpilogueInRegs) {
            const float b4[4] = {T::low(bq[g][0]), T::high(bq[g][0]), T::low(bq[g][1]), T::high(bq[g][1])};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float v = acc[mt][g * 4 + e] + b4[e];
              if (relu) v = fmaxf(v, 0.0f);
              ov[e] = (typename T::elem)v;   // the one rounding: round-to-nearest-even
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) ov[e] = (typename T::elem)acc[mt][g * 4 + e];
          }
          *(vec4*)(lds + pos * 512 + (((ch >> 3) ^ (pos & 31)) << 4) + ((ch >> 2) & 1) * 8) = ov;
        }
      }
    }
    __syncthreads();
    if (has_q) {   // chunk q's channels kbase + 8 q .. + 7 are below K (a multiple of 32), and a wave with channels wrote them
#pragma unroll
      for (int it = 0; it < kInTileM / 16; ++it) {
        const int pos = it * 16 + (tid >> 5);
        const int p = tile * kInTileM + pos;
        if (p < M) {
          vec8 ov = *(const vec8*)(lds + pos * 512 + ((q ^ (pos & 31)) << 4));
          if constexpr (!T::kEpilogueInRegs) {   // float(rounded acc) + bias, max(., 0), the second rounding
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              float v = (float)ov[e];
              v += (float)bv[e];
              if (relu) v = fmaxf(v, 0.0f);
              ov[e] = (typename T::elem)v;
            }
          }
          *(vec8*)(y + (size_t)p * K + kbase + q * 8) = ov;
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
template <int kG, typename T>
__global__ __launch_bounds__(kHcThreads) void k_head_convs(const uint32x4* __restrict__ act, const uint32x4* __restrict__ pw,
                                                           const void* __restrict__ pb, const uint32x4* __restrict__ vw,
                                                           const void* __restrict__ vb, float* __restrict__ P, float* __restrict__ V0,
                                                           int M, int d, int C) {
  const int l = threadIdx.x & (kG - 1);
  const int c8 = C >> 3;                         // 16-B chunks per position, and per weight row
  const int groups = gridDim.x * (kHcThreads / kG);
  const int gid = blockIdx.x * (kHcThreads / kG) + threadIdx.x / kG;
  // the group's first chunk of the three weight rows stays in registers (C <= 8 kG: all of them); a lane without a chunk holds
  // zeros and adds zeros
  uint32x4 w0 = {0, 0, 0, 0}, w1 = w0, w2 = w0;
  if (l < c8) { w0 = pw[l]; w1 = pw[c8 + l]; w2 = vw[l]; }
  const float b0 = elem_at<T>(pb, 0), b1 = elem_at<T>(pb, 1), b2 = elem_at<T>(vb, 0);

  for (int base = gid; base < M; base += groups * kHcUnroll) {
    uint32x4 av[kHcUnroll];
#pragma unroll
    for (int u = 0; u < kHcUnroll; ++u) {
      const int p = base + u * groups;
      av[u] = uint32x4{0, 0, 0, 0};
      if (p < M && l < c8) av[u] = act[(size_t)p * c8 + l];
    }
#pragma unroll
    for (int u = 0; u < kHcUnroll; ++u) {
      const int p = base + u * groups;   // uniform over the group
      float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
      T::dot3(av[u], w0, w1, w2, lo, hi);
      if (p < M)
        for (int qq = l + kG; qq < c8; qq += kG)   // C above 8 kG: the further chunks' weights come from memory
          T::dot3(act[(size_t)p * c8 + qq], pw[qq], pw[c8 + qq], vw[qq], lo, hi);
      float s0 = T::total(lo, hi, 0), s1 = T::total(lo, hi, 1), s2 = T::total(lo, hi, 2);
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

constexpr int kFcThreads = 1024;                 // 16 waves: a neuron's weight row is a few dependent loads, one neuron per wave in flight
constexpr int kFcRows = 8;                       // rows a workgroup takes at most; rows_sum is written for 8

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
// The wave's sums of kFcRows = 8 values per lane at once.  Offsets 32, 16 and 8 each halve the values a lane carries: a lane keeps
// the half its bit of the offset selects and adds the partner's copy of it, so behind them lane l holds row 4 b5 + 2 b4 + b3 (the
// bits of l) summed over its 8-lane-strided class; offsets 4, 2, 1 finish it.  Every row's tree is wave_sum's, level by level (an
// fp32 add commutes), whichever slot the row sits in: its bits do not depend on the rows beside it.
__device__ __forceinline__ float rows_sum(const float (&a)[8], int lane) {
  float b[4], c[2];
  const bool u5 = lane & 32, u4 = lane & 16, u3 = lane & 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = (u5 ? a[i + 4] : a[i]) + __shfl_xor(u5 ? a[i] : a[i + 4], 32);
#pragma unroll
  for (int i = 0; i < 2; ++i) c[i] = (u4 ? b[i + 2] : b[i]) + __shfl_xor(u4 ? b[i] : b[i + 2], 16);
  float v = (u3 ? c[1] : c[0]) + __shfl_xor(u3 ? c[0] : c[1], 8);
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// dynamic LDS, floats: P [rpb][2 d] | V0 [rpb][d] | logits [rpb][d + 1] | v1 [rpb][vh]
template <typename T>
__global__ __launch_bounds__(kFcThreads) void k_head_fc(const float* __restrict__ P, const float* __restrict__ V0,
                                                        const uint32_t* __restrict__ piw, const void* __restrict__ pib,
                                                        const uint16_t* __restrict__ v1w, const void* __restrict__ v1b,
                                                        const void* __restrict__ v2w, const void* __restrict__ v2b,
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

  // one wave per output neuron: j < d + 1 is a logit (a weight row of 2 d elements = d aligned dwords), the others value_linear1's
  const int nout = d + 1 + vh;
  for (int j = wv; j < nout; j += kFcThreads / 64) {
    float acc[kFcRows];
#pragma unroll
    for (int r = 0; r < kFcRows; ++r) acc[r] = 0.0f;
    if (j <= d) {
      const uint32_t* wr = piw + (size_t)j * d;
      for (int t = lane; t < d; t += 64) {
        const uint32_t w2 = wr[t];
        const float wl = T::low(w2), wh = T::high(w2);
#pragma unroll
        for (int r = 0; r < kFcRows; ++r)
          if (r < nr) {
            const float2 pv = *(const float2*)(sP + r * 2 * d + 2 * t);
            acc[r] += wl * pv.x;
            acc[r] += wh * pv.y;
          }
      }
    } else {
      const uint16_t* wr = v1w + (size_t)(j - d - 1) * d;   // d may be odd: rows are 2-B aligned only
      for (int t = lane; t < d; t += 64) {
        const float wl = T::low(wr[t]);
#pragma unroll
        for (int r = 0; r < kFcRows; ++r)
          if (r < nr) acc[r] += wl * sV[r * d + t];
      }
    }
    // the eight rows' sums in 10 shuffles, not 48: lane l is left with the total of row 4 b5 + 2 b4 + b3 of its bits
    const float tot = rows_sum(acc, lane);
    const int r = ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);
    if ((lane & 7) == 0 && r < nr) {
      if (j <= d)
        sL[r * (d + 1) + j] = tot + elem_at<T>(pib, j);
      else
        s1[r * vh + (j - d - 1)] = fmaxf(tot + elem_at<T>(v1b, j - d - 1), 0.0f);
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
    for (int t = lane; t < vh; t += 64) v += elem_at<T>(v2w, t) * s1[r * vh + t];
    v = wave_sum(v);
    if (lane == 0) value[r0 + r] = tanhf(v + elem_at<T>(v2b, 0));
  }
}

// ------------------------------------------------------------------------------------------------ the host entries

// P [rows][2][d] and V0 [rows][d]
inline size_t heads_ws_bytes(int64_t rows, int64_t d) { return (size_t)rows * 3 * (size_t)d * sizeof(float); }

// x_is_f16: only Bf16 converts; the fp16 entry passes 0
template <typename T>
int conv_in_entry(const void* x, int x_is_f16, const void* w, const void* bias, void* y, int64_t rows, int h, int wd, int c, int k,
                  int relu, void* stream) {
  if (x_is_f16 != 0 && x_is_f16 != 1) return ELFGO_E_BADARG;
  if (c < 2 || c > kInMaxC || (c & 1) != 0 || k <= 0 || (k & 31) != 0) return ELFGO_E_BADARG;
  // the convolution entries' checks with no skip; x is read in channel pairs of either type, so 4-byte aligned is enough for it
  int dev = 0;
  const int go = conv_args(x, 4, w, bias, nullptr, y, rows, h, wd, c, k, &dev);
  if (go <= 0) return go;
  DevGuard _dg(dev);
  const int m = (int)(rows * h * wd);
  const int tiles = (m + kInTileM - 1) / kInTileM;
  const int gy = (k + kInTileN - 1) / kInTileN;
  // two workgroups (16 waves of at most 128 VGPRs, 37 KiB of LDS each) share a CU: 512 of them fill 256 CUs, and each walks over
  // its share of the tiles
  const int gx = tiles < 512 / gy ? tiles : (512 / gy > 0 ? 512 / gy : 1);
  const dim3 grid((unsigned)gx, (unsigned)gy);
  const auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kInThreads), 0, (hipStream_t)stream, (const uint32_t*)x, (const uint16_t*)w,
                       (const uint16_t*)bias, (uint16_t*)y, m, h, wd, c, k, relu);
  };
  const bool small = 9 * c <= 11 * 16;
  if (!x_is_f16)
    small ? launch(k_conv3x3_in<11, T, false>) : launch(k_conv3x3_in<18, T, false>);
  else if constexpr (std::is_same<T, Bf16>::value)
    small ? launch(k_conv3x3_in<11, T, true>) : launch(k_conv3x3_in<18, T, true>);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

template <typename T>
int heads_entry(const void* act, const ElfNetHeads* hd, int64_t rows, int h, int wd, float* pi, int64_t pi_stride, float* value,
                float* logits, void* workspace, size_t workspace_bytes, void* stream) {
  if (!act || !hd || !pi || !value || !workspace || rows < 0 || h <= 0 || wd <= 0) return ELFGO_E_BADARG;
  if (!hd->pconv_w || !hd->pconv_b || !hd->vconv_w || !hd->vconv_b || !hd->pi_w || !hd->pi_b || !hd->v1_w || !hd->v1_b || !hd->v2_w ||
      !hd->v2_b)
    return ELFGO_E_BADARG;
  const int C = hd->channels, vh = hd->value_hidden;
  const int64_t d = (int64_t)h * wd;
  if (C <= 0 || (C & 7) != 0 || vh <= 0 || pi_stride < d + 1) return ELFGO_E_BADARG;
  if (rows * d >= ((int64_t)1 << 31) || d > (1 << 20) || vh > (1 << 20)) return ELFGO_E_BADARG;
  if (workspace_bytes < heads_ws_bytes(rows, d)) return ELFGO_E_BADARG;
  // 16-B loads of act and the head-conv weights, dwords of pi_w, floats in the workspace and the outputs
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
  const int c8 = C >> 3;
  const int g = c8 <= 8 ? 8 : c8 <= 16 ? 16 : 32;
  const int per_block = kHcThreads / g * kHcUnroll;
  int blocks = (m + per_block - 1) / per_block;
  if (blocks > 2048) blocks = 2048;
  const auto convs = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kHcThreads), 0, st, (const uint32x4*)act, (const uint32x4*)hd->pconv_w, hd->pconv_b,
                       (const uint32x4*)hd->vconv_w, hd->vconv_b, P, V0, m, (int)d, C);
  };
  if (g == 8)
    convs(k_head_convs<8, T>);
  else if (g == 16)
    convs(k_head_convs<16, T>);
  else
    convs(k_head_convs<32, T>);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_head_fc<T>, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(kFcThreads), rpb * per_row, st, P, V0,
                     (const uint32_t*)hd->pi_w, hd->pi_b, (const uint16_t*)hd->v1_w, hd->v1_b, hd->v2_w, hd->v2_b, pi, pi_stride, value,
                     logits, (int)rows, (int)d, vh, rpb);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" int elfnet_conv3x3_in_f16(const void* x, const void* w, const void* bias, void* y, int64_t rows, int h, int wd, int c, int k,
                                     int relu, void* stream) {
  return conv_in_entry<F16>(x, 0, w, bias, y, rows, h, wd, c, k, relu, stream);
}

extern "C" int elfnet_conv3x3_in_bf16(const void* x, int x_is_f16, const void* w, const void* bias, void* y, int64_t rows, int h, int wd,
                                      int c, int k, int relu, void* stream) {
  return conv_in_entry<Bf16>(x, x_is_f16, w, bias, y, rows, h, wd, c, k, relu, stream);
}

extern "C" size_t elfnet_heads_workspace(int64_t rows, int h, int wd) {
  if (rows < 0 || h <= 0 || wd <= 0) return 0;
  // never 0 for a valid shape: a caller may allocate it as it is
  return (heads_ws_bytes(rows > 0 ? rows : 1, (int64_t)h * wd) + 255) & ~(size_t)255;
}

extern "C" int elfnet_heads_f16(const void* act, const ElfNetHeads* hd, int64_t rows, int h, int wd, float* pi, int64_t pi_stride,
                                float* value, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
  return heads_entry<F16>(act, hd, rows, h, wd, pi, pi_stride, value, logits, workspace, workspace_bytes, stream);
}

extern "C" int elfnet_heads_bf16(const void* act, const ElfNetHeads* hd, int64_t rows, int h, int wd, float* pi, int64_t pi_stride,
                                 float* value, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
  return heads_entry<Bf16>(act, hd, rows, h, wd, pi, pi_stride, value, logits, workspace, workspace_bytes, stream);
}
