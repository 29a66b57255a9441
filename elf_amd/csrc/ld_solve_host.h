// Host side of elfgo_ld_solve (include/elf_amd.h): argument checks and the launches of k_ld_solve (ld_solve.cuh).  Included by
// exactly one HIP translation unit of libelf_amd.so, after region_host.h.
#pragma once
#include "ld_solve.cuh"

extern "C" {

int elfgo_ld_solve_max_depth(void) { return LD_SOLVE_MAX_DEPTH; }

int elfgo_ld_solve(ElfGoEngine* e, const int32_t* ids, int n, const int32_t* regions, const uint8_t* attackers, int max_depth,
                   int max_nodes, int self_atari_thres, int32_t* info, int8_t* value, int32_t* nodes, void* stream) {
  if (!e || n <= 0 || (!ids && n > e->capacity) || !value || max_depth < 0 || max_depth > LD_SOLVE_MAX_DEPTH || max_nodes <= 0)
    return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  // one wave per (root move, row); the grid's second dimension holds 65 535 rows, so a larger call goes out in slices
  constexpr int ROWS = 65535;
  for (int row0 = 0; row0 < n; row0 += ROWS) {
    const int rows = n - row0 < ROWS ? n - row0 : ROWS;
    DISPATCH(e, hipLaunchKernelGGL(k_ld_solve<N>, dim3(Geo<N>::NP, rows), dim3(LD_SOLVE_WAVE), ld_solve_stack_bytes<N>(max_depth),
                                   (hipStream_t)stream, pool_of<N>(e), e->capacity, ids, row0, regions, attackers, max_depth, max_nodes,
                                   self_atari_thres, info, value, nodes));
    HIPCHK(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
