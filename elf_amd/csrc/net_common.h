// What the net translation units (net_conv.hip, net_conv3x3.hip, net_conv3x3_plan.hip, net_conv3x3_small.hip, net_conv3x3_bf16.hip,
// net_conv3x3_bf16_big.hip, net_io.hip) share:
// the vector types of the MFMA kernels, the host entries' device guard and the argument checks of the convolution entries.  It
// includes nothing from CK and nothing of the project but the C header, so that each of those files stays an object of its own
// (GNUmakefile); engine_host.h, which has a DevGuard too, pulls the board kernels in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/elf_amd.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef uint32_t uint32x4 __attribute__((ext_vector_type(4)));

typedef __attribute__((address_space(3))) void* lptr_t;

template <int kV> struct Mode { static constexpr int v = kV; };

// engine_host.h's DevGuard: the device of an entry's tensors for the entry's duration, then the caller's again
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

// The checks the convolution entries make alike, in the order they share: no null x / w / bias / y and no size below 1 (rows may be
// 0), w / bias / res / y 16-byte aligned and x to x_align bytes, y neither x nor res, and every tensor below 2^31 bytes (CK's
// descriptors and the kernels' byte offsets are 32-bit; 2048 rows of 19 x 19 x 256 are 0.38 GB); then, for a call that has rows,
// the device x lives on.  Returns ELFGO_E_BADARG for a call to refuse, 0 for one with nothing to do (rows == 0: accepted behind
// every check above and before the first call into the GPU runtime), and 1 with *dev for one to launch under DevGuard(*dev).
// What only one entry asks of c, k and its other arguments that entry checks itself, in front of this call where it refuses
// before rows == 0 is accepted and behind it where it does not.
inline int conv_args(const void* x, uintptr_t x_align, const void* w, const void* bias, const void* res, const void* y, int64_t rows,
                     int h, int wd, int c, int k, int* dev) {
  if (!x || !w || !bias || !y || rows < 0 || h <= 0 || wd <= 0 || c <= 0 || k <= 0) return ELFGO_E_BADARG;
  if ((((uintptr_t)w | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)y) & 15) != 0 || ((uintptr_t)x & (x_align - 1)) != 0)
    return ELFGO_E_BADARG;
  if (y == x || y == res) return ELFGO_E_BADARG;
  const int64_t cmax = c > k ? c : k;
  if (rows * h * wd * cmax >= ((int64_t)1 << 30) || (int64_t)k * 9 * c >= ((int64_t)1 << 30)) return ELFGO_E_BADARG;
  if (rows == 0) return 0;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, x) != hipSuccess) { (void)hipGetLastError(); return ELFGO_E_BADARG; }
  *dev = at.device;
  return 1;
}

}  // namespace
