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
  DISPATCH(e, hipLaunchKernelGGL(k_playout_cand<N>, dim3((n + CAND_WAVES - 1) / CAND_WAVES), dim3(CAND_WAVE * CAND_WAVES), 0, (hipStream_t)stream,
                                 pool_of<N>(e), ids, (const u64*)seeds, n, max_steps, self_atari_thres, out));
  HIPCHK(hipGetLastError());
  return 0;
}

int elfgo_own_run_cand(ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts, int max_steps, float komi,
                       int self_atari_thres, int32_t* counts, int64_t* stats, void* stream) {
  if (!o || !seeds || !counts || !stats || n <= 0 || playouts <= 0) return ELFGO_E_BADARG;
  ElfGoEngine* e = o->e;
  if (!ids && n > e->capacity) return ELFGO_E_BADARG;
  if ((long long)n * playouts > 0x7FFFFFF0ll) return ELFGO_E_BADARG;   // the kernel counts (row, playout) pairs in 32 bits
  DevGuard _dg(e->device);
  const size_t np = (size_t)e->n * e->n;
  HIPCHK(hipMemsetAsync(counts, 0, (size_t)n * 2 * np * sizeof(int32_t), (hipStream_t)stream));
  HIPCHK(hipMemsetAsync(stats, 0, (size_t)n * 4 * sizeof(int64_t), (hipStream_t)stream));
  const int groups = (n * playouts + CAND_WAVES - 1) / CAND_WAVES;
  const int wgs = groups < o->lanes / CAND_WAVES ? groups : o->lanes / CAND_WAVES;
  DISPATCH(e, hipLaunchKernelGGL(k_playout_own_cand<N>, dim3(wgs), dim3(CAND_WAVE * CAND_WAVES), 0, (hipStream_t)stream, pool_of<N>(e), o->scratch,
                                 ids, (const u64*)seeds, n, playouts, max_steps, komi, self_atari_thres, counts,
                                 (unsigned long long*)stats));
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
