// The trunk convolution of the policy/value net with its epilogue inside: y = relu?(conv3x3_same(x, w) + bias (+ res)) in ONE
// kernel, fp16 NHWC in and out, fp32 accumulation.  Before this file a trunk conv was MIOpen's implicit GEMM followed by one
// k_bias_act pass (net_epilogue.hip) that read and rewrote the activation the conv had just stored: 14 % of a self-play step.
//
// The main loop is not ours: it is Composable Kernel's GridwiseGemmMultipleD_xdl_cshuffle, instantiated here from the headers that
// ship with ROCm, with the tile parameters of the instance MIOpen's tuned database picks for the 2048 x 19 x 19 x 256 -> 256 shape
// (elf_amd/data/miopen_db/*.udb.txt: <256, 256, 128, 32, Default, 32, 32, 4, 2, 8, 8, 8, 1, 1>).  What is ours is the element-wise
// functor CK applies in its C-shuffle epilogue, on the values it is about to store (BiasResAct below).
//
// algo 0  DeviceGroupedConvFwdMultipleABD_Xdl_CShuffle with those parameters.  MIOpen runs them inside the *_Large_Tensor device
//         op; that op cannot take a bias: it indexes every D tensor with E's descriptor and its IsSupportedArgument refuses a D
//         whose strides differ from E's, so a [K] bias would have to be expanded to a whole activation.  The ABD op builds the same
//         gridwise GEMM (same K order y, x, c; same pipeline v1) and gives each D its own descriptor (G_K layout for the bias).
// algo 1  not CK: the hand-written 256 x 256 x 64 LDS-DMA kernel of net_conv3x3.hip, an object of its own that this file only
//         calls (elfnet_conv3x3_native_f16, hidden; that object exports only host arithmetic: the plans of its two row orders
//         and the rule that chooses between them).  Same K order and MFMA as algo 0.  elfnet_conv3x3_f16_width hands algo 1 the
//         round width its split of the last round goes by and keeps it on the linear order, elfnet_conv3x3_f16_boards forces
//         board order, and the plain entry lets that object choose by shape.
//
// This translation unit is its own object (GNUmakefile): the CK templates take ~40 s each to compile and depend on none of the
// project's .cuh files, which is also why it carries its own small device guard instead of including engine_host.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>

#if !__has_include("ck/ck.hpp")
#error "net_conv.hip needs Composable Kernel's headers (ck/ck.hpp, shipped with ROCm under <rocm>/include/ck): there is no build of libelf_amd.so without the fused trunk convolution"
#endif
#include "ck/ck.hpp"
#include "ck/tensor_operation/gpu/device/convolution_forward_specialization.hpp"
#include "ck/tensor_operation/gpu/device/gemm_specialization.hpp"
#include "ck/tensor_operation/gpu/device/impl/device_grouped_conv_fwd_multiple_abd_xdl_cshuffle.hpp"
#include "ck/tensor_operation/gpu/device/tensor_layout.hpp"
#include "ck/tensor_operation/gpu/element/element_wise_operation.hpp"

#include "../../include/elf_amd.h"

namespace {

using F16 = ck::half_t;
using F32 = float;
template <ck::index_t... Is>
using S = ck::Sequence<Is...>;
using PassThrough = ck::tensor_operation::element_wise::PassThrough;
namespace lay = ck::tensor_layout::convolution;

// The epilogue, on the values of the C-shuffle tile (c arrives in CShuffleDataType = fp16: the rounding MIOpen's conv applies
// when it stores y; the explicit conversion keeps that true whatever CShuffleDataType is).  Then k_bias_act's sequence, in its
// order: fp32 + bias, + res, max(., 0), one rounding to fp16.  With algo 0 the result is the old two-kernel result bit for bit.
struct BiasResAct {
  int relu;
  template <typename E, typename C, typename D0>
  __host__ __device__ void operator()(E& e, const C& c, const D0& bias) const {
    float v = ck::type_convert<float>(ck::type_convert<F16>(c));
    v += ck::type_convert<float>(bias);
    if (relu) v = fmaxf(v, 0.0f);
    e = ck::type_convert<E>(v);
  }
  template <typename E, typename C, typename D0, typename D1>
  __host__ __device__ void operator()(E& e, const C& c, const D0& bias, const D1& res) const {
    float v = ck::type_convert<float>(ck::type_convert<F16>(c));
    v += ck::type_convert<float>(bias);
    v += ck::type_convert<float>(res);
    if (relu) v = fmaxf(v, 0.0f);
    e = ck::type_convert<E>(v);
  }
};

constexpr auto kConvDefault = ck::tensor_operation::device::ConvolutionForwardSpecialization::Default;
constexpr auto kMNKPadding = ck::tensor_operation::device::GemmSpecialization::MNKPadding;

// clang-format off
template <typename DsLayout, typename DsTypes>
using ConvA = ck::tensor_operation::device::DeviceGroupedConvFwdMultipleABD_Xdl_CShuffle<
    2, lay::NHWGC, lay::GKYXC, DsLayout, lay::NHWGK, F16, F16, F32, F16, DsTypes, F16, PassThrough, PassThrough, BiasResAct,
    kConvDefault, kMNKPadding, 1, 256, 256, 128, 32, 8, 8, 32, 32, 4, 2,
    S<4, 64, 1>, S<1, 0, 2>, S<1, 0, 2>, 2, 8, 8, 1,
    S<4, 64, 1>, S<1, 0, 2>, S<1, 0, 2>, 2, 8, 8, 1,
    1, 1, S<1, 32, 1, 8>, 8>;
// clang-format on

using DsBias = ck::Tuple<lay::G_K>;
using DsBiasRes = ck::Tuple<lay::G_K, lay::NHWGK>;
using T1 = ck::Tuple<F16>;
using T2 = ck::Tuple<F16, F16>;

// engine_host.h's DevGuard (that header pulls the board kernels in, see the top of this file)
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

struct Shape { int n, h, w, c, k; };

// host-side argument object and CK's own support check; with `launch`, one launch on `stream`: no allocation, no
// synchronisation, no copy
template <typename Op, int ND>
int run(const void* x, const void* w, const std::array<const void*, ND>& ds, void* y, const Shape& s, int relu, hipStream_t stream,
        bool launch) {
  using A5 = std::array<ck::index_t, 5>;
  using A2 = std::array<ck::index_t, 2>;
  const int n = s.n, h = s.h, wd = s.w, c = s.c, k = s.k;
  // logical order G, N, C|K, H, W over NHWGC / GKYXC / NHWGK memory with G = 1
  const A5 xl{1, n, c, h, wd}, xs{c, h * wd * c, 1, wd * c, c};
  const A5 wl{1, k, c, 3, 3}, ws{k * 9 * c, 9 * c, 1, 3 * c, c};
  const A5 yl{1, n, k, h, wd}, ys{k, h * wd * k, 1, wd * k, k};
  const A5 bs{k, 0, 1, 0, 0};   // the bias, G_K: broadcast over N, H, W
  std::array<A5, ND> dl, dst;
  dl[0] = yl; dst[0] = bs;
  if (ND == 2) { dl[ND - 1] = yl; dst[ND - 1] = ys; }
  const A2 one{1, 1};
  try {
    auto arg = Op::MakeArgument(x, w, ds, y, xl, xs, wl, ws, dl, dst, yl, ys, one, one, one, one, PassThrough{}, PassThrough{},
                                BiasResAct{relu});
    if (!Op::IsSupportedArgument(arg)) return ELFGO_E_BADARG;
    if (!launch) return 0;
    auto inv = Op::MakeInvoker();
    (void)inv.Run(arg, StreamConfig{stream, false});
  } catch (...) {   // CK reports a failed launch by throwing; nothing is thrown across the C ABI
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? (int)hipErrorLaunchFailure : (int)e;
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

// net_conv3x3.hip
extern "C" __attribute__((visibility("hidden"))) int elfnet_conv3x3_native_f16(const void* x, const void* w, const void* bias,
                                                                               const void* res, void* y, int64_t rows, int h, int wd,
                                                                               int c, int k, int relu, int round_width, int order,
                                                                               hipStream_t stream);

namespace {

// order is algo 1's row order: 0 linear, 1 board, -1 the one net_conv3x3.hip chooses for the shape
int conv3x3_f16(const void* x, const void* w, const void* bias, const void* res, void* y, int64_t rows, int h, int wd, int c, int k,
                int relu, int algo, int round_width, int order, void* stream) {
  if (!x || !w || !bias || !y || rows < 0 || h <= 0 || wd <= 0 || c <= 0 || k <= 0) return ELFGO_E_BADARG;
  if ((c & 7) != 0 || (k & 7) != 0 || (algo != 0 && algo != 1) || round_width < 0) return ELFGO_E_BADARG;
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)y) & 15) != 0) return ELFGO_E_BADARG;
  if (y == x || y == res) return ELFGO_E_BADARG;
  // CK's descriptors are 32-bit: every tensor stays below 2^31 bytes (2048 rows of 19 x 19 x 256 are 0.38 GB)
  const int64_t cmax = c > k ? c : k;
  if (rows * h * wd * cmax >= ((int64_t)1 << 30) || (int64_t)k * 9 * c >= ((int64_t)1 << 30)) return ELFGO_E_BADARG;
  if (rows == 0) return 0;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, x) != hipSuccess) { (void)hipGetLastError(); return ELFGO_E_BADARG; }
  DevGuard _dg(at.device);
  const Shape s{(int)rows, h, wd, c, k};
  hipStream_t st = (hipStream_t)stream;
  if (algo == 1) return elfnet_conv3x3_native_f16(x, w, bias, res, y, rows, h, wd, c, k, relu, round_width, order, st);
  // one launch whatever the size: the device op splits N itself
  if (res) return run<ConvA<DsBiasRes, T2>, 2>(x, w, {bias, res}, y, s, relu, st, true);
  return run<ConvA<DsBias, T1>, 1>(x, w, {bias}, y, s, relu, st, true);
}

}  // namespace

extern "C" int elfnet_conv3x3_f16(const void* x, const void* w, const void* bias, const void* res, void* y, int64_t rows, int h, int wd,
                                  int c, int k, int relu, int algo, void* stream) {
  return conv3x3_f16(x, w, bias, res, y, rows, h, wd, c, k, relu, algo, 0, -1, stream);
}

// a named round width keeps algo 1 on the linear order; 0 is the plain entry
extern "C" int elfnet_conv3x3_f16_width(const void* x, const void* w, const void* bias, const void* res, void* y, int64_t rows, int h,
                                        int wd, int c, int k, int relu, int algo, int round_width, void* stream) {
  return conv3x3_f16(x, w, bias, res, y, rows, h, wd, c, k, relu, algo, round_width, round_width > 0 ? 0 : -1, stream);
}

// algo 1 in board order, whatever the shape and the width
extern "C" int elfnet_conv3x3_f16_boards(const void* x, const void* w, const void* bias, const void* res, void* y, int64_t rows, int h,
                                         int wd, int c, int k, int relu, int round_width, void* stream) {
  return conv3x3_f16(x, w, bias, res, y, rows, h, wd, c, k, relu, 1, round_width, 1, stream);
}
