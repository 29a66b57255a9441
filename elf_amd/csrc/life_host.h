// Host side of elfgo_life_map (include/elf_amd.h): argument checks and the launch of k_life_map (life.cuh).  Included by exactly
// one HIP translation unit of libelf_amd.so.
#pragma once
#include "life.cuh"

extern "C" {

int elfgo_life_map(ElfGoEngine* e, const int32_t* ids, int n, const int32_t* regions, uint8_t* eye, int16_t* semi_move, uint8_t* alive,
                   int32_t* summary, void* stream) {
  if (!e || n <= 0 || (!ids && n > e->capacity) || (!eye && !semi_move && !alive && !summary)) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  DISPATCH(e, hipLaunchKernelGGL(k_life_map<N>, dim3(n), dim3(LIFE_WAVE), 0, (hipStream_t)stream, pool_of<N>(e), e->capacity, ids, n, regions,
                                 eye, semi_move, alive, summary));
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
