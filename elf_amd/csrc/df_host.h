// Host side of elfgo_df_* / elfgo_extract_df (include/elf_amd.h): argument checks, the placement-ply table's handle and the
// launches of the kernels in df_features.cuh.  Included by exactly one HIP translation unit of libelf_amd.so.
#pragma once
#include <math.h>

#include <new>
#include <vector>

#include "df_features.cuh"

// The side table over an engine: Info::last_placed of every slot, the exponent table of planes 10 / 11 and an `ok` row for
// callers of elfgo_df_forward / elfgo_df_setup that pass none.
struct ElfGoDf {
  ElfGoEngine* e = nullptr;
  u16* table = nullptr;      // [capacity][N*N], action order
  float* exp_d = nullptr;    // [2 N*N + 1]
  uint8_t* ok = nullptr;     // [capacity]
};

// entry d = what getHistoryExp (board_feature.cc:166-167) stores for last_placed - _ply = -d: the double exp of the C library,
// narrowed on assignment
static void df_fill_exp(int n, float* out) {
  const int len = 2 * n * n + 1;
  for (int d = 0; d < len; ++d) {
    const int last_placed = 0, ply = d;
    out[d] = exp((last_placed - ply) / 10.0);
  }
}

static int df_extract(ElfGoDf* df, const int32_t* ids, const int32_t* d4, int n, const uint16_t* rows, float* dst, int64_t stride_floats,
                      void* stream) {
  if (!df || n < 0) return ELFGO_E_BADARG;
  ElfGoEngine* e = df->e;
  if (!ids && n > e->capacity) return ELFGO_E_BADARG;
  if (n == 0) return 0;
  if (!dst || stride_floats < (int64_t)DF_PLANES * e->n * e->n || ((uintptr_t)dst & 3) != 0) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  // enough workgroups to fill 256 CUs, then rows loop inside the waves (as elfgo_extract_agz)
  const int want = (n + DF_WAVES - 1) / DF_WAVES, wgs = want < 4096 ? want : 4096;
  DISPATCH(e, hipLaunchKernelGGL(k_extract_df<N>, dim3(wgs), dim3(DF_WAVE * DF_WAVES), 0, (hipStream_t)stream,
                                 reinterpret_cast<const Slot<N>*>(e->slots), e->capacity, ids, d4, n, rows ? rows : df->table, rows ? 0 : 1,
                                 df->exp_d, dst, stride_floats));
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" {

int elfgo_df_exp_table(int board_size, float* out_host) {
  if (!out_host) return ELFGO_E_BADARG;
  if (board_size != 19 && board_size != 9) return ELFGO_E_BADSIZE;
  df_fill_exp(board_size, out_host);
  return 0;
}

int elfgo_df_destroy(ElfGoDf* df) {
  if (!df) return ELFGO_E_BADARG;
  DevGuard _dg(df->e->device);
  if (df->table) (void)hipFree(df->table);
  if (df->exp_d) (void)hipFree(df->exp_d);
  if (df->ok) (void)hipFree(df->ok);
  delete df;
  return 0;
}

int elfgo_df_create(ElfGoEngine* e, ElfGoDf** out) {
  if (!e || !out) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  ElfGoDf* df = new (std::nothrow) ElfGoDf();
  if (!df) return ELFGO_E_NOMEM;
  df->e = e;
  const size_t np = (size_t)e->n * e->n, bytes = (size_t)e->capacity * np * sizeof(u16);
  std::vector<float> tab(2 * np + 1);
  df_fill_exp(e->n, tab.data());
  hipError_t rc = hipMalloc((void**)&df->table, bytes);
  if (rc == hipSuccess) rc = hipMemset(df->table, 0, bytes);
  if (rc == hipSuccess) rc = hipMalloc((void**)&df->exp_d, tab.size() * sizeof(float));
  if (rc == hipSuccess) rc = hipMemcpy(df->exp_d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
  if (rc == hipSuccess) rc = hipMalloc((void**)&df->ok, (size_t)e->capacity);
  if (rc != hipSuccess) { elfgo_df_destroy(df); return (int)rc; }
  *out = df;
  return 0;
}

int elfgo_df_reset(ElfGoDf* df, const int32_t* ids, int n, void* stream) {
  if (!df) return ELFGO_E_BADARG;
  ElfGoEngine* e = df->e;
  const int rc = elfgo_reset(e, ids, n, stream);
  if (rc || n == 0) return rc;
  DevGuard _dg(e->device);
  hipLaunchKernelGGL(k_df_clear, dim3(n), dim3(128), 0, (hipStream_t)stream, df->table, e->n * e->n, e->capacity, ids, n);
  HIPCHK(hipGetLastError());
  return 0;
}

int elfgo_df_copy(ElfGoDf* df, const int32_t* dst_ids, const int32_t* src_ids, int n, void* stream) {
  if (!df) return ELFGO_E_BADARG;
  ElfGoEngine* e = df->e;
  const int rc = elfgo_copy(e, dst_ids, src_ids, n, stream);
  if (rc || n == 0) return rc;
  DevGuard _dg(e->device);
  hipLaunchKernelGGL(k_df_copy, dim3(n), dim3(128), 0, (hipStream_t)stream, df->table, e->n * e->n, e->capacity, dst_ids, src_ids, n);
  HIPCHK(hipGetLastError());
  return 0;
}

int elfgo_df_forward(ElfGoDf* df, const int32_t* ids, const int32_t* moves, int n, uint8_t* ok, void* stream) {
  if (!df || (!ok && n > df->e->capacity)) return ELFGO_E_BADARG;
  ElfGoEngine* e = df->e;
  if (!ok) ok = df->ok;
  const int rc = elfgo_forward(e, ids, moves, n, ok, stream);
  if (rc || n == 0) return rc;
  DevGuard _dg(e->device);
  DISPATCH(e, hipLaunchKernelGGL(k_df_note<N>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                                 reinterpret_cast<const Slot<N>*>(e->slots), df->table, e->capacity, ids, moves, ok, n));
  HIPCHK(hipGetLastError());
  return 0;
}

int elfgo_df_setup(ElfGoDf* df, const int32_t* ids, const uint8_t* stones, const uint8_t* next_player, int n, uint8_t* ok, void* stream) {
  if (!df || (!ok && n > df->e->capacity)) return ELFGO_E_BADARG;
  ElfGoEngine* e = df->e;
  if (!ok) ok = df->ok;
  const int rc = elfgo_setup(e, ids, stones, next_player, n, ok, stream);
  if (rc || n == 0) return rc;
  DevGuard _dg(e->device);
  hipLaunchKernelGGL(k_df_setup, dim3(n), dim3(128), 0, (hipStream_t)stream, df->table, e->n * e->n, e->capacity, ids, stones, ok, n);
  HIPCHK(hipGetLastError());
  return 0;
}

int elfgo_df_placed(ElfGoDf* df, const int32_t* ids, int n, uint16_t* out, void* stream) {
  if (!df || n < 0 || (!ids && n > df->e->capacity)) return ELFGO_E_BADARG;
  if (n == 0) return 0;
  if (!out) return ELFGO_E_BADARG;
  ElfGoEngine* e = df->e;
  DevGuard _dg(e->device);
  hipLaunchKernelGGL(k_df_placed, dim3(n), dim3(128), 0, (hipStream_t)stream, df->table, e->n * e->n, e->capacity, ids, n, out);
  HIPCHK(hipGetLastError());
  return 0;
}

int elfgo_df_extract(ElfGoDf* df, const int32_t* ids, const int32_t* d4, int n, float* dst, int64_t stride_floats, void* stream) {
  return df_extract(df, ids, d4, n, nullptr, dst, stride_floats, stream);
}

int elfgo_extract_df(ElfGoDf* df, const int32_t* ids, const int32_t* d4, int n, const uint16_t* placed_rows, float* dst,
                     int64_t stride_floats, void* stream) {
  if (!placed_rows) return ELFGO_E_BADARG;
  return df_extract(df, ids, d4, n, placed_rows, dst, stride_floats, stream);
}

}  // extern "C"
