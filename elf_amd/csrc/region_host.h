// Host side of elfgo_region_moves / elfgo_ld_run (include/elf_amd.h): argument checks and the launches of the kernels in
// region.cuh.  Included by exactly one HIP translation unit of libelf_amd.so, after ownership_host.h (ElfGoOwnership).
#pragma once
#include "region.cuh"
#include "ownership_host.h"

extern "C" {

int elfgo_region_moves(ElfGoEngine* e, const int32_t* ids, int n, const int32_t* regions, int self_atari_thres, uint8_t* cand,
                       uint8_t* valid, uint8_t* groups, void* stream) {
  if (!e || n <= 0 || (!ids && n > e->capacity) || (!cand && !valid && !groups)) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  DISPATCH(e, hipLaunchKernelGGL(k_region_moves<N>, dim3(n), dim3(REGION_WAVE), 0, (hipStream_t)stream, pool_of<N>(e), e->capacity, ids, n,
                                 regions, self_atari_thres, cand, valid, groups));
  HIPCHK(hipGetLastError());
  return 0;
}

int elfgo_ld_run(ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts, int max_steps,
                 int self_atari_thres, const int32_t* regions, const uint8_t* attackers, int32_t* info, int64_t* stats, int32_t* first,
                 void* stream) {
  const int wgs = own_plan(o, ids, seeds, n, playouts);
  if (!wgs || !info || !stats || !first) return ELFGO_E_BADARG;
  ElfGoEngine* e = o->e;
  DevGuard _dg(e->device);
  const size_t na = (size_t)e->n * e->n + 1;
  HIPCHK(hipMemsetAsync(info, 0, (size_t)n * LD_INFO_WORDS * sizeof(int32_t), (hipStream_t)stream));
  HIPCHK(hipMemsetAsync(stats, 0, (size_t)n * LD_STAT_WORDS * sizeof(int64_t), (hipStream_t)stream));
  HIPCHK(hipMemsetAsync(first, 0, (size_t)n * 3 * na * sizeof(int32_t), (hipStream_t)stream));
  DISPATCH(e, hipLaunchKernelGGL(k_playout_ld<N>, dim3(wgs), dim3(OWN_WAVE * OWN_WAVES), 0, (hipStream_t)stream, pool_of<N>(e), e->capacity,
                                 o->scratch, ids, (const u64*)seeds, n, playouts, max_steps, self_atari_thres, regions, attackers, info,
                                 (unsigned long long*)stats, first));
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
