// Host side of elfgo_ladder_map (include/elf_amd.h): argument checks and the launch of k_ladder_map (ladder.cuh).  Included by
// exactly one HIP translation unit of libelf_amd.so.
#pragma once
#include "ladder.cuh"

extern "C" {

int elfgo_ladder_map(ElfGoEngine* e, const int32_t* ids, int n, int16_t* depth, int16_t* calls, void* stream) {
  if (!e || n < 0 || (!ids && n > e->capacity)) return ELFGO_E_BADARG;
  if (n == 0) return 0;
  if (!depth) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  DISPATCH(e, hipLaunchKernelGGL(k_ladder_map<N>, dim3(n), dim3(LADDER_WAVE), 0, (hipStream_t)stream, pool_of<N>(e), e->capacity, ids, n,
                                 depth, calls));
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
