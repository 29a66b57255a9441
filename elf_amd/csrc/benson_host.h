// Host side of elfgo_pass_alive (include/elf_amd.h): argument checks and the launch of k_pass_alive (benson.cuh).  Included by
// exactly one HIP translation unit of libelf_amd.so.
#pragma once
#include "benson.cuh"

extern "C" {

int elfgo_pass_alive(ElfGoEngine* e, const int32_t* ids, int n, uint8_t* map, int32_t* summary, void* stream) {
  if (!e || n <= 0 || (!ids && n > e->capacity) || (!map && !summary)) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  DISPATCH(e, hipLaunchKernelGGL(k_pass_alive<N>, dim3(n), dim3(BENSON_WAVE), 0, (hipStream_t)stream, pool_of<N>(e), e->capacity, ids, n, map,
                                 summary));
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
