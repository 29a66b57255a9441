// Host side of elfgo_candidates / elfgo_playout_cand / elfgo_own_run_cand (include/elf_amd.h): argument checks and the launches
// of the kernels in candidates.cuh.  Included by exactly one HIP translation unit of libelf_amd.so, after ownership_host.h
// (ElfGoOwnership).
#pragma once
#include "candidates.cuh"
#include "ownership_host.h"

extern "C" {

int elfgo_candidates(ElfGoEngine* e, const int32_t* ids, int n, int self_atari_thres, uint8_t* mask, int16_t* stones, void* stream) {
  if (!e || n <= 0 || (!ids && n > e->capacity) || (!mask && !stones)) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  DISPATCH(e, hipLaunchKernelGGL(k_candidates<N>, dim3(n), dim3(CAND_WAVE), 0, (hipStream_t)stream, pool_of<N>(e), e->capacity, ids, n,
                                 self_atari_thres, mask, stones));
  HIPCHK(hipGetLastError());
  return 0;
}

int elfgo_playout_cand(ElfGoEngine* e, const int32_t* ids, const uint64_t* seeds, int n, int max_steps, int self_atari_thres,
                       uint32_t* out, void* stream) {
  if (!e || n < 0 || (!ids && n > e->capacity)) return ELFGO_E_BADARG;
  if (n == 0) return 0;
  if (!seeds || !out) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  DISPATCH(e, hipLaunchKernelGGL(k_playout_cand<N>, dim3((n + PLAYOUT_WAVES - 1) / PLAYOUT_WAVES), dim3(PLAYOUT_WAVE * PLAYOUT_WAVES), 0,
                                 (hipStream_t)stream, pool_of<N>(e), ids, (const u64*)seeds, n, max_steps, self_atari_thres, out));
  HIPCHK(hipGetLastError());
  return 0;
}

int elfgo_own_run_cand(ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts, int max_steps, float komi,
                       int self_atari_thres, int32_t* counts, int64_t* stats, void* stream) {
  return own_run(o, ids, seeds, n, playouts, max_steps, komi, counts, stats, stream, CandPolicy{self_atari_thres});
}

}  // extern "C"
