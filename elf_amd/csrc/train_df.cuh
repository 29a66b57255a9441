// DarkForest rows from the replay loader: with GameOptions.use_df_feature the reference binds the "train" batch's "s" to
// extractState / extractStateExt (common/game_feature.h:98-102, :159-170) -- BoardFeature::extract, the 25 planes of
// df_planes.cuh -- and GoGameTrain::act sends them beside offline_a [num_future_actions]: what the DarkForest policy nets
// (df_model.py) train on.  k_replay_extract_df is k_replay_extract (train.cuh) with that row in place of the AGZ one.
//
// The planes read Info::last_placed (the ply at which the stone on a point was placed, board.cc:680, :1379), which a slot does not
// carry.  For a recorded game it is a pure function of the move list, so the checkpoint trick of train.cuh survives: the store
// keeps, per record, uint16 place_ply[max_moves] -- the ply every accepted placement wrote, 0 for everything else, written by the
// one replay per put that also writes the checkpoints -- and a sample rebuilds the table of its position in LDS from
// place_ply[0 .. move_to) and the move list.  Plies grow with t, so a maximum per point gives the last writer; entries under points
// whose stone has been captured since differ from the reference's (equally stale) ones, and no plane reads them.
//
// Why siblings and not template parameters of the kernels in train.cuh: train.cuh and train_capi.hip are among
// elf_amd._lib.KERNEL_SOURCES -- the committed PMC profiles are only priced while their bytes stand (tests/test_abi.py) -- so, as
// mcts_analyze.hip does for the search, the additions live in files of their own and the AGZ kernels are not even recompiled
// differently.  The price is the replay prologue and the batch's other fields stated twice; tests/test_gpu_train_df.py holds the
// two statements together field by field.
#pragma once
#include "df_planes.cuh"
#include "train.cuh"

namespace elfgo {

struct ReplayDf {
  u16* place_ply;     // [capacity][max_moves] beside ReplayStore.moves: the board's ply before move t (_ply starts at 1) if move t was
                      // an accepted placement, else 0 (pass, resignation, refused move, M_INVALID)
  const float* exp;   // [2 N*N + 1] elfgo_df_exp_table's values: the device never evaluates exp
};

// k_replay_checkpoint (train.cuh) that also notes the placement plies: launched in its place for every record put since the
// last extraction, so a record is still replayed once per put.
template <int N, class PoolT>
__global__ __launch_bounds__(64 * REPLAY_WAVES_CK) void k_replay_checkpoint_df(PoolT pool, ReplayStore st, ReplayDf df, const int32_t* slots, int n) {
  using G = Geo<N>;
  __shared__ Slot<N> lds_all[REPLAY_WAVES_CK];
  __shared__ u64 zlds[G::P];
  for (int j = threadIdx.x; j < G::P; j += 64 * REPLAY_WAVES_CK) zlds[j] = pool.zob[j];
  __syncthreads();
  const int wv = rfl((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int i = blockIdx.x * REPLAY_WAVES_CK + wv;
  if (i >= n) return;
  const int r = rfl(slots[i]);
  const int nm = rfl(st.num_moves[r]);
  const u16* mv = st.moves + (size_t)r * st.max_moves;
  u16* pp = df.place_ply + (size_t)r * st.max_moves;
  Board<N> bd;
  bd.init(&lds_all[wv], pool.zob, st.skrec + (size_t)r * (st.max_moves + 2) * G::SKW);
  bd.reset();
  bd.playout_begin(zlds);
  Slot<N>* ck = reinterpret_cast<Slot<N>*>(st.ckpt) + (size_t)r * st.nck;
  for (int t = 0; t < nm; ++t) {
    const int c = rfl((int)mv[t]);
    const int ply = bd.ply;
    int played = 0;
    if (c != M_INVALID) played = bd.forward(c);  // a refused move is skipped like any other (see k_replay_extract)
    if (lane == 0) pp[t] = (u16)(played && c != M_PASS && c != M_RESIGN ? ply : 0);
    if ((t + 1) % CK_INTERVAL == 0 && (t + 1) / CK_INTERVAL <= st.nck) bd.store(&ck[(t + 1) / CK_INTERVAL - 1]);
  }
}

// Info::last_placed of the position after the first `mt` moves of a record: placed[point of move t] = max over t < mt of
// place_ply[t].  The maximum is taken by LDS atomics on the 32-bit words of `acc` (NP words, free until the classification) and
// narrowed into `placed`.
template <int N>
__device__ __forceinline__ void df_placed_from_record(u16* placed, u32* acc, const u16* __restrict__ place_ply, const u16* __restrict__ mv, int mt,
                                                      int lane) {
  using G = Geo<N>;
  for (int j = lane; j < G::NP; j += 64) acc[j] = 0;
  agz_wave_sync();
  for (int t = lane; t < mt; t += 64) {
    const u32 p = place_ply[t];
    const u32 c = mv[t];
    // Board::c2a_u; an accepted placement is on the board, and whatever else the two arrays might hold must not leave `acc`
    const u32 y1 = (c * (u32)G::DS_M) >> G::DS_S, a = (c - y1 * G::S - 1) * N + (y1 - 1);
    if (p != 0 && c < (u32)G::P && a < (u32)G::NP)
      __hip_atomic_fetch_max((__attribute__((address_space(3))) u32*)&acc[a], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  agz_wave_sync();
  for (int j = lane; j < G::NP; j += 64) placed[j] = (u16)acc[j];
  agz_wave_sync();
}

// what a wave of k_replay_extract_df owns in LDS beside its slot
template <int N>
struct alignas(16) ReplayDfLds {
  float hx[Geo<N>::NP];
  u16 placed[(Geo<N>::NP + 7) & ~7];
};

// k_replay_extract with "s" = fp32 [25][N][N]: same launch geometry (REPLAY_WAVES samples per workgroup, one wave each, no
// synchronisation after the prologue), same replay (KEEP as there), every other field of the batch the same text.  o.fmt is not
// read.  LDS: the class words of df_planes_row take the slot's history ring and Bloom words, which are dead once the position is
// replayed (and stored, with KEEP) -- 1984 B >= 4 * 361; the history values and the placement plies (2176 B per wave at 19x19) are
// this kernel's own, which leaves 5 workgroups = 20 waves per CU where the AGZ kernel has 8 = 32.
template <int N, class PoolT, bool KEEP>
__global__ __launch_bounds__(64 * REPLAY_WAVES) void k_replay_extract_df(PoolT pool, ReplayStore st, ReplayDf df, const int32_t* rec, const int32_t* move_to,
                                                                          const int32_t* d4s, int n, TrainBatch o) {
  using G = Geo<N>;
  static_assert(sizeof(Slot<N>) - offsetof(Slot<N>, hist) >= sizeof(u32) * G::NP, "the class words fit behind the slot's prefix");
  __shared__ Slot<N> lds_all[REPLAY_WAVES];
  __shared__ ReplayDfLds<N> own_all[REPLAY_WAVES];
  __shared__ u64 zlds[G::P];   // Zobrist constants: forward reads them from LDS, not behind its own superko record stores (Board::zob_v)
  for (int j = threadIdx.x; j < G::P; j += 64 * REPLAY_WAVES) zlds[j] = pool.zob[j];
  __syncthreads();
  const int wv = rfl((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int i = blockIdx.x * REPLAY_WAVES + wv;
  if (i >= n) return;
  Slot<N>& lds = lds_all[wv];
  ReplayDfLds<N>& own = own_all[wv];
  u32* cls = reinterpret_cast<u32*>(&lds.hist[0][0][0]);
  int r = rfl(rec[i]);
  r = r < 0 ? 0 : (r >= st.capacity ? st.capacity - 1 : r);   // an out-of-range record id must not read outside the store
  const int d4 = rfl(d4s ? d4s[i] : 0) & 7;
  const int nm = rfl(st.num_moves[r]);
  int mt = rfl(move_to[i]);
  if (mt > nm) mt = nm;   // the reference asserts move_to < size (go_state_ext.h:284)
  const u16* mv = st.moves + (size_t)r * st.max_moves;
  Board<N> bd;
  if (KEEP) {
    bd.init(&lds, pool.zob, pool.skr(i));
    bd.reset();                                   // _state.reset()
    bd.playout_begin(zlds);
    for (int j = lane; j < G::NP; j += 64) own.placed[j] = 0;   // Info::last_placed, noted as the replay goes
    Board<N>::wsync();
    for (int t = 0; t < mt; ++t) {                // switchBeforeMove: for (i < move_to) _state.forward(moves[i])
      const int c = rfl((int)mv[t]);
      if (c == M_INVALID) continue;               // the reference throws here (go_state.cc:75-77); a refused move is skipped like any other
      const int ply = bd.ply;
      const int played = bd.forward(c);
      if (played && c != M_PASS && c != M_RESIGN && lane == 0) own.placed[Board<N>::c2a_u(c)] = (u16)ply;
    }
    bd.store(&pool.slots[i]);                     // the replayed GoState stays inspectable through elfgo_* (slot i)
    Board<N>::wsync();                            // the store's LDS reads are issued before the ring is overwritten
  } else {
    const u64* skr = st.skrec + (size_t)r * (st.max_moves + 2) * G::SKW;
    bd.init(&lds, pool.zob, const_cast<u64*>(skr));
    int ck = mt / CK_INTERVAL;                    // checkpoints at or below move_to
    if (ck > st.nck) ck = st.nck;
    if (ck > 0) bd.load(reinterpret_cast<const Slot<N>*>(st.ckpt) + (size_t)r * st.nck + (ck - 1));
    else bd.reset();
    bd.playout_begin(zlds);
    const ReplaySK<N> sk{skr};
    for (int t = ck * CK_INTERVAL; t < mt; ++t) {
      const int c = rfl((int)mv[t]);
      if (c == M_INVALID) continue;
      bd.forward(c, sk);
    }
    Board<N>::wsync();
    df_placed_from_record<N>(own.placed, cls, df.place_ply + (size_t)r * st.max_moves, mv, mt, lane);
  }
  // "s": extractState -> BoardFeature::extract under the sample's D4 code.  pt and libs of the LDS image are the replayed
  // position's (what store() writes); ply, player and ko state come from the Board object -- the LDS header is stale
  {
    int ln = lane;                                // opaque: the row's per-point geometry is not to be computed above the replay
    asm volatile("" : "+v"(ln));
    df_planes_row<N>(reinterpret_cast<const uint4*>(&lds), own.placed, cls, own.hx, bd.ply, bd.next_player, bd.ko_pt, bd.ko_age, d4, df.exp,
                     (float*)o.s + (size_t)i * o.s_stride, lane, ln);
  }
  const int idx = bd.ply - 1;                   // every extractor's move_to = _state.getPly() - 1
  if (lane == 0) {
    if (o.move_idx) o.move_idx[i] = idx;
    if (o.num_move) o.num_move[i] = nm;
    if (o.aug_code) o.aug_code[i] = d4;
    if (o.winner) o.winner[i] = st.winner[r];
    if (o.selfplay_ver) o.selfplay_ver[i] = st.black_ver[r];
    if (o.predicted_value) o.predicted_value[i] = idx < st.num_values[r] ? st.values[(size_t)r * st.max_moves + idx] : 0.0f;
  }
  if (o.offline_a) {                            // extractOfflineAction :129-139
    for (int j = lane; j < o.nfa; j += 64) {
      const int t = idx + j;
      o.offline_a[(size_t)i * o.nfa + j] = t < nm ? (int64_t)coord_to_action<N>(mv[t], d4) : 0;
    }
  }
  if (o.mcts_scores) {                          // extractMCTSPi :107-127
    float* ms = o.mcts_scores + (size_t)i * G::NA;
    const bool have = st.pol != nullptr && idx < rfl(st.num_pol[r]);
    if (have) {
      const unsigned char* pr = st.pol + ((size_t)r * st.max_moves + idx) * G::P;
      static_assert(G::NA <= G::R * 64, "one action per lane per round");
      float v[G::R];
      float sum = 0.0f;                         // integers <= 255 * 362 < 2^24: the fp32 sum is exact in any order
#pragma unroll
      for (int k = 0; k < G::R; ++k) {
        const int a = k * 64 + lane;
        v[k] = 0.0f;
        if (a < G::NA) {
          int coord, a0;
          action_to_coord<N>(a, d4, coord, a0);
          v[k] = (float)pr[coord];
          sum += v[k];
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
#pragma unroll
      for (int k = 0; k < G::R; ++k) {
        const int a = k * 64 + lane;
        if (a < G::NA) ms[a] = __fdiv_rn(v[k], sum);
      }
    } else {
      const int hot = idx < nm ? coord_to_action<N>(mv[idx], d4) : -1;
      for (int a = lane; a < G::NA; a += 64) ms[a] = a == hot ? 1.0f : 0.0f;
    }
  }
}

}  // namespace elfgo
