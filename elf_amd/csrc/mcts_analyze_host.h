// Host side of elfmcts_analyze (include/elf_amd.h): argument checks and the launch of k_mcts_analyze (mcts_analyze.cuh).
// `struct ElfMcts` and tree_of<N>() are private to mcts_capi.hip, so this header is compiled in that translation unit: it is
// included by mcts_analyze.hip, after mcts_capi.hip, and by nothing else.
#pragma once
#include "mcts_analyze.cuh"

extern "C" {

int elfmcts_analyze(ElfMcts* m, int max_moves, int max_pv, int32_t* info, int32_t* coord, int32_t* orig, int32_t* visits,
                    float* reward, float* prior, int32_t* pv_len, int32_t* pv, void* stream) {
  if (!m || !info || max_moves < 1 || max_moves > AN_MAX_MOVES || max_pv < 1 || max_pv > AN_MAX_PV) return ELFGO_E_BADARG;
  static_assert(AN_INFO_WORDS == ELFMCTS_ANALYZE_WORDS && AN_MAX_MOVES == ELFMCTS_ANALYZE_MAX_MOVES &&
                AN_MAX_PV == ELFMCTS_ANALYZE_MAX_PV, "the header's limits are the kernel's");
  DevGuard _dg(m->eng->device);
  const int waves = max_moves < AN_WAVES ? max_moves : AN_WAVES;
  const AnalyzeOut out{info, coord, orig, visits, reward, prior, pv_len, pv};
  DISPATCH(m->eng, hipLaunchKernelGGL(k_mcts_analyze<N>, dim3(m->G), dim3(64 * waves), 0, (hipStream_t)stream, tree_of<N>(m),
                                      max_moves, max_pv, out));
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
