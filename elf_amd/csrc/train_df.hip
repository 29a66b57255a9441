// The trainer's translation unit of libelf_amd.so: train_capi.hip as it stands, plus the DarkForest row format of
// elftrain_extract (ELFGO_FEAT_DF_F32_NCHW, kernels in train_df.cuh).  train_capi.hip is one of elf_amd._lib.KERNEL_SOURCES -- the
// committed PMC profiles are only priced while its bytes stand -- so GNUmakefile compiles this file in its place (as
// mcts_analyze.hip for the search).  Three of its entry points gain something and are therefore compiled under other names and
// wrapped here: create / destroy (the store's DarkForest share) and extract (the new format, and the per-put replay that now
// also notes the placement plies).  Every other elftrain_* function is train_capi.hip's own.
#include "../../include/elf_amd.h"   // the public declarations, under the public names

extern "C" {   // train_capi.hip's own three, under the names they are compiled to here
int elftrain_create_agz_(ElfGoEngine* e, int capacity, int max_moves, int with_policies, uint32_t seed, ElfReplay** out);
int elftrain_destroy_agz_(ElfReplay* r);
int elftrain_extract_agz_(ElfReplay* r, const int32_t* rec, const int32_t* move_to, const int32_t* d4, int n, const ElfTrainBatch* b, void* stream);
}
#define elftrain_create elftrain_create_agz_
#define elftrain_destroy elftrain_destroy_agz_
#define elftrain_extract elftrain_extract_agz_
#include "train_capi.hip"
#undef elftrain_create
#undef elftrain_destroy
#undef elftrain_extract

#include <mutex>
#include <unordered_map>

#include "train_df.cuh"

// The DarkForest share of a store: 2 B per move (a 19x19 record holds about 248 KB in checkpointed mode) and the exponent table
// of planes 10 / 11.  ElfReplay has no room for them, so they hang beside it, keyed by the handle.
namespace {
std::mutex g_df_mu;
std::unordered_map<const ElfReplay*, ReplayDf> g_df;

bool df_of(const ElfReplay* r, ReplayDf* out) {
  std::lock_guard<std::mutex> lk(g_df_mu);
  const auto it = g_df.find(r);
  if (it == g_df.end()) return false;
  *out = it->second;
  return true;
}
}  // namespace

extern "C" {

int elftrain_destroy(ElfReplay* r) {
  if (!r) return ELFGO_E_BADARG;
  ReplayDf df{};
  {
    std::lock_guard<std::mutex> lk(g_df_mu);
    const auto it = g_df.find(r);
    if (it != g_df.end()) { df = it->second; g_df.erase(it); }
  }
  {
    DevGuard _dg(r->eng->device);
    if (df.place_ply) (void)hipFree(df.place_ply);
    if (df.exp) (void)hipFree(const_cast<float*>(df.exp));
  }
  return elftrain_destroy_agz_(r);
}

int elftrain_create(ElfGoEngine* e, int capacity, int max_moves, int with_policies, uint32_t seed, ElfReplay** out) {
  ElfReplay* r = nullptr;
  const int rc = elftrain_create_agz_(e, capacity, max_moves, with_policies, seed, &r);
  if (rc) return rc;
  DevGuard _dg(e->device);
  // always there, used or not: the exponents are made once, on the host, by the expression elfgo_df_exp_table exports
  std::vector<float> tab((size_t)2 * e->n * e->n + 1);
  ReplayDf df{};
  float* exp_d = nullptr;
  const size_t pbytes = (size_t)capacity * max_moves * sizeof(u16);
  hipError_t he = elfgo_df_exp_table(e->n, tab.data()) == 0 ? hipSuccess : hipErrorInvalidValue;
  if (he == hipSuccess) he = hipMalloc((void**)&df.place_ply, pbytes);
  if (he == hipSuccess) he = hipMemset(df.place_ply, 0, pbytes);
  if (he == hipSuccess) he = hipMalloc((void**)&exp_d, tab.size() * sizeof(float));
  if (he == hipSuccess) he = hipMemcpy(exp_d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
  if (he != hipSuccess) {
    if (df.place_ply) (void)hipFree(df.place_ply);
    if (exp_d) (void)hipFree(exp_d);
    (void)elftrain_destroy_agz_(r);
    return (int)he;
  }
  df.exp = exp_d;
  {
    std::lock_guard<std::mutex> lk(g_df_mu);
    g_df[r] = df;
  }
  *out = r;
  return 0;
}

int elftrain_extract(ElfReplay* r, const int32_t* rec, const int32_t* move_to, const int32_t* d4, int n, const ElfTrainBatch* b, void* stream) {
  if (!r || !rec || !move_to || !b || n < 0 || (r->keep_states && n > r->eng->capacity)) return ELFGO_E_BADARG;
  if (n == 0) return 0;
  const bool is_df = b->s_format == ELFGO_FEAT_DF_F32_NCHW;
  const int nn = r->eng->n;
  // nothing is queued for a call that will be refused: the AGZ formats' own checks, repeated ahead of the per-put replay below
  if (!is_df && b->s_format != ELFGO_FEAT_F32_NCHW && b->s_format != ELFGO_FEAT_F16_NHWC) return ELFGO_E_BADARG;
  if (!b->s || b->s_stride < (int64_t)(is_df ? DF_PLANES : 18) * nn * nn || (is_df && ((uintptr_t)b->s & 3) != 0)) return ELFGO_E_BADARG;
  if (b->offline_a && b->num_future_actions < 1) return ELFGO_E_BADARG;
  ReplayDf df{};
  if (!df_of(r, &df)) return ELFGO_E_BADARG;
  DevGuard _dg(r->eng->device);
  hipStream_t s = (hipStream_t)stream;
  if (!r->dirty.empty() && !r->keep_states) {
    // train_capi.hip's dirty-list step with k_replay_checkpoint_df in k_replay_checkpoint's place: the records put since the last
    // extraction get their checkpoints, superko records and placement plies now, ahead of the samples that use them.  The list is
    // empty afterwards, so the AGZ path below finds nothing left to do.  (With keep_states on nothing reads any of the three: the
    // slots stay on the list for a later switch of the mode.)
    const int nd = (int)r->dirty.size();
    HIPCHK(hipMemcpyAsync(r->d_dirty, r->dirty.data(), sizeof(int32_t) * nd, hipMemcpyHostToDevice, s));
    DISPATCH(r->eng, hipLaunchKernelGGL((k_replay_checkpoint_df<N, Pool<N>>), dim3((nd + REPLAY_WAVES_CK - 1) / REPLAY_WAVES_CK), dim3(64 * REPLAY_WAVES_CK), 0, s,
                                        pool_of<N>(r->eng), r->st, df, r->d_dirty, nd));
    HIPCHK(hipGetLastError());
    for (int32_t sl : r->dirty) r->is_dirty[sl] = 0;
    r->dirty.clear();
  }
  if (!is_df) return elftrain_extract_agz_(r, rec, move_to, d4, n, b, stream);
  TrainBatch o;
  o.s = b->s; o.s_stride = b->s_stride; o.fmt = FEAT_F32_NCHW;
  o.offline_a = b->offline_a; o.nfa = b->num_future_actions;
  o.winner = b->winner; o.mcts_scores = b->mcts_scores; o.predicted_value = b->predicted_value;
  o.move_idx = b->move_idx; o.num_move = b->num_move; o.aug_code = b->aug_code; o.selfplay_ver = b->selfplay_ver;
  const dim3 grid((n + REPLAY_WAVES - 1) / REPLAY_WAVES), block(64 * REPLAY_WAVES);
  if (r->keep_states) {
    DISPATCH(r->eng, hipLaunchKernelGGL((k_replay_extract_df<N, Pool<N>, true>), grid, block, 0, s, pool_of<N>(r->eng), r->st, df, rec, move_to, d4, n, o));
  } else {
    DISPATCH(r->eng, hipLaunchKernelGGL((k_replay_extract_df<N, Pool<N>, false>), grid, block, 0, s, pool_of<N>(r->eng), r->st, df, rec, move_to, d4, n, o));
  }
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
