// Host side of elfgo_area_map / elfgo_own_* (include/elf_amd.h): argument checks, the ownership handle and the launches of
// the kernels in ownership.cuh.  Included by exactly one HIP translation unit of libelf_amd.so.
#pragma once
#include <new>

#include "ownership.cuh"

// Scratch + launch geometry over an engine.  The record areas of the playout copies live here and not in ElfGoEngine: a copy
// never touches the records of the slot it was taken from.
struct ElfGoOwnership {
  ElfGoEngine* e = nullptr;
  int lanes = 0;            // waves in flight, a multiple of OWN_WAVES; one record area each
  u64* scratch = nullptr;   // [lanes][MAXMOVE+2][SKW]
  size_t scratch_bytes = 0;
};

template <int N>
static size_t own_record_bytes() { return (size_t)(Geo<N>::MAXMOVE + 2) * Geo<N>::SKW * sizeof(u64); }

// The launch plan of a playout_pairs kernel (elfgo_own_run*, elfgo_ld_run): checks the arguments they share and returns the workgroups
// of the persistent launch, one per group of OWN_WAVES pairs up to the handle's record areas; 0 = an argument is refused.
static int own_plan(const ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts) {
  if (!o || !seeds || n <= 0 || playouts <= 0) return 0;
  if (!ids && n > o->e->capacity) return 0;
  if ((long long)n * playouts > 0x7FFFFFF0ll) return 0;   // the kernel counts (row, playout) pairs in 32 bits
  const int groups = (n * playouts + OWN_WAVES - 1) / OWN_WAVES;
  return groups < o->lanes / OWN_WAVES ? groups : o->lanes / OWN_WAVES;
}

// elfgo_own_run under the given playout policy: checks, zeroed sums, one persistent launch.
template <class Policy>
static int own_run(ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts, int max_steps, float komi,
                   int32_t* counts, int64_t* stats, void* stream, Policy pol) {
  const int wgs = own_plan(o, ids, seeds, n, playouts);
  if (!wgs || !counts || !stats) return ELFGO_E_BADARG;
  ElfGoEngine* e = o->e;
  DevGuard _dg(e->device);
  const size_t np = (size_t)e->n * e->n;
  HIPCHK(hipMemsetAsync(counts, 0, (size_t)n * 2 * np * sizeof(int32_t), (hipStream_t)stream));
  HIPCHK(hipMemsetAsync(stats, 0, (size_t)n * 4 * sizeof(int64_t), (hipStream_t)stream));
  DISPATCH(e, hipLaunchKernelGGL((k_playout_own<N, Policy>), dim3(wgs), dim3(OWN_WAVE * OWN_WAVES), 0, (hipStream_t)stream, pool_of<N>(e),
                                 e->capacity, o->scratch, ids, (const u64*)seeds, n, playouts, max_steps, komi, counts,
                                 (unsigned long long*)stats, pol));
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" {

int elfgo_area_map(ElfGoEngine* e, const int32_t* ids, int n, uint8_t* out, void* stream) {
  if (!e || n < 0 || (!ids && n > e->capacity)) return ELFGO_E_BADARG;
  if (n == 0) return 0;
  if (!out) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  DISPATCH(e, hipLaunchKernelGGL(k_area_map<N>, dim3(n), dim3(OWN_WAVE), 0, (hipStream_t)stream, pool_of<N>(e), ids, n, out));
  HIPCHK(hipGetLastError());
  return 0;
}

int elfgo_own_create(ElfGoEngine* e, int max_lanes, ElfGoOwnership** out) {
  if (!e || !out) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  if (max_lanes <= 0) {
    // 7 workgroups of k_playout_own fit a CU's LDS at 19x19 (8 at 9x9 would not change the picture): 28 waves per CU
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
    max_lanes = cus * 7 * OWN_WAVES;
  }
  ElfGoOwnership* o = new (std::nothrow) ElfGoOwnership();
  if (!o) return ELFGO_E_NOMEM;
  o->e = e;
  o->lanes = (max_lanes + OWN_WAVES - 1) / OWN_WAVES * OWN_WAVES;
  o->scratch_bytes = (size_t)o->lanes * (e->n == 19 ? own_record_bytes<19>() : own_record_bytes<9>());
  const hipError_t rc = hipMalloc((void**)&o->scratch, o->scratch_bytes);
  if (rc != hipSuccess) { delete o; return (int)rc; }
  *out = o;
  return 0;
}

int elfgo_own_destroy(ElfGoOwnership* o) {
  if (!o) return ELFGO_E_BADARG;
  DevGuard _dg(o->e->device);
  if (o->scratch) (void)hipFree(o->scratch);
  delete o;
  return 0;
}

size_t elfgo_own_scratch_bytes(const ElfGoOwnership* o) { return o ? o->scratch_bytes : 0; }

int elfgo_own_run(ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts, int max_steps, float komi,
                  int32_t* counts, int64_t* stats, void* stream) {
  return own_run(o, ids, seeds, n, playouts, max_steps, komi, counts, stats, stream, EyePolicy{});
}

}  // extern "C"
