// Search analysis (include/elf_amd.h, elfmcts_analyze): the candidate moves of every game's root and the principal variation the
// search expects below each of them.  What the reference shows with
//   src_cpp/elf/ai/tree_search/tree_search_node.h   SearchTreeT::printTree :479-528 (reached from MCTSAI_T, mcts.h:105)
//   src_cpp/elf/ai/tree_search/tree_search_base.h   MCTSResultT::addActions :248-292 (MOST_VISITED: strict '>', first in iteration order)
// read straight from the node records of mcts.cuh.  Only FOLLOWED edges can have visits, and a node keeps those as the prefix
// [0, n_touched) of its edge arrays, sorted by `orig` (the reference's iteration order): "most visits, first in iteration order
// on ties" is "most visits, lowest position in the prefix".
//
// Read-only: the kernel stores to its output arrays and to nothing else.  Every loop is bounded by max_moves, max_pv or the
// touched-edge capacity of the record it reads (GameNodes::cap); a child id outside the pool or one that the pool holds as free
// ends a variation instead of being followed.
//
// One workgroup per game, one wave per candidate rank (ranks w, w + W, ... for wave w of W = min(max_moves, 16)): the walk down a
// variation is a chain of dependent loads, one coalesced round of 64 touched-edge entries per level for almost every node, and
// the arg-max of a round goes over the DPP network (wave_max_u32).  Every wave ranks the root's edges itself -- the visit counts
// of the prefix sit in at most NE / 64 registers per lane -- so the waves share nothing but the longest variation's length.
#pragma once
#include "mcts.cuh"

namespace elfgo {

constexpr int AN_MAX_MOVES = 64;   // candidates per game
constexpr int AN_MAX_PV = 32;      // coords per variation (one lane each)
constexpr int AN_WAVES = 16;       // waves of a workgroup
constexpr int AN_INFO_WORDS = 8;

struct AnalyzeOut {                // device arrays; every one but info may be null
  int32_t* info;                   // [G][8]
  int32_t *coord, *orig, *visits;  // [G][max_moves]
  float *reward, *prior;           // [G][max_moves]
  int32_t* pv_len;                 // [G][max_moves]
  int32_t* pv;                     // [G][max_moves][max_pv]
};

template <int N>
__global__ __launch_bounds__(64 * AN_WAVES) void k_mcts_analyze(TreePool<N> tp, int max_moves, int max_pv, AnalyzeOut out) {
  using NL = NodeL<N>;
  constexpr int R = (NL::NE + 63) / 64;      // rounds of 64 entries that cover the largest followed prefix
  __shared__ int s_len[AN_WAVES];
  const int g = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const GameNodes<N> nodes(tp, g);
  const int* po = tp.parent_of;
  const GameState& gs = tp.gs[g];
  const int root = rfl(gs.root);
  const bool root_ok = root >= 0 && root < tp.C;
  const NodeRef<N> r = nodes[root_ok ? root : 0];
  HdrU h;
  h.set(root_ok && lane < 16 ? reinterpret_cast<const int*>(r.p)[lane] : 0);
  int nt = root_ok ? h.n_touched : 0;
  nt = nt < 0 ? 0 : nt > nodes.cap(root) ? nodes.cap(root) : nt;
  // the visit counts of the root's followed prefix: entry k * 64 + lane in v[k]
  int v[R];
  int count = 0;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int pos = k * 64 + lane;
    v[k] = 0;
    if (pos < nt) v[k] = r.tst()[pos].visits;
    if (v[k] < 0) v[k] = 0;
    count += __popcll(ballot64(v[k] > 0));
  }
  // candidates in (visits descending, position ascending) order, compared as a pair: each round finds the successor of the
  // previous pick (pv, pp); a persistent tree's visit counts are not bounded by one move's rollouts, so nothing is packed
  int pvis = 0x7FFFFFFF, ppos = -1, longest = 0;
  for (int rank = 0; rank < max_moves; ++rank) {
    int bpos = -1;
    if (pvis > 0) {
      int lv = 0, lpos = 0;
#pragma unroll
      for (int k = 0; k < R; ++k) {          // ascending positions and a strict '>': the lane's lowest position among its maxima
        const int pos = k * 64 + lane;
        const bool after = v[k] < pvis || (v[k] == pvis && pos > ppos);
        if (after && v[k] > lv) { lv = v[k]; lpos = pos; }
      }
      const int vmax = (int)wave_max_u32((u32)lv);
      if (vmax > 0) bpos = 0xFFFF - (int)wave_max_u32(lv == vmax ? (u32)(0xFFFF - lpos) : 0u);
      pvis = vmax; ppos = bpos;              // vmax == 0: no visited edge is left, for this rank and all after it
    }
    if (rank % W != w) continue;
    int len = 0, mypv = -1;                  // lane d holds the d-th coord of the variation
    int c_coord = -1, c_orig = -1, c_vis = 0;
    float c_rew = 0.0f, c_pri = 0.0f;
    if (bpos >= 0) {
      const TStat t = r.tst()[bpos];
      c_coord = rfl((int)r.coord()[bpos]); c_orig = rfl((int)r.orig()[bpos]);
      c_pri = r.prior()[bpos]; c_vis = t.visits; c_rew = t.reward;
      if (lane == 0) mypv = c_coord;
      len = 1;
      int node = rfl(t.child);
      while (len < max_pv) {
        if (node < 0 || node >= tp.C) break;
        if (rfl(po[node]) == -2) break;      // the pool holds this id as free
        const NodeRef<N> nd = nodes[node];
        int cnt = rfl(nd.h().n_touched);
        cnt = cnt < 0 ? 0 : cnt > nodes.cap(node) ? nodes.cap(node) : cnt;
        int best_v = 0, best_pos = -1, best_child = -1;
        for (int base = 0; base < cnt; base += 64) {
          const int pos = base + lane;
          TStat s = tst_none();
          if (pos < cnt) s = nd.tst()[pos];
          const int sv = s.visits > 0 ? s.visits : 0;
          const int m = (int)wave_max_u32((u32)sv);
          if (m > best_v) {                  // strict: an earlier round's maximum keeps its place
            const int bl = (int)__builtin_ctzll(ballot64(sv == m));
            best_v = m; best_pos = base + bl; best_child = rl(s.child, bl);
          }
        }
        if (best_v == 0) break;              // no followed edge, or none with a visit
        const int c = rfl((int)nd.coord()[best_pos]);
        if (lane == len) mypv = c;
        ++len;
        node = best_child;
      }
    }
    const size_t o = (size_t)g * max_moves + rank;
    if (lane == 0) {
      if (out.coord) out.coord[o] = c_coord;
      if (out.orig) out.orig[o] = c_orig;
      if (out.visits) out.visits[o] = c_vis;
      if (out.reward) out.reward[o] = c_rew;
      if (out.prior) out.prior[o] = c_pri;
      if (out.pv_len) out.pv_len[o] = len;
    }
    if (out.pv && lane < max_pv) out.pv[o * max_pv + lane] = lane < len ? mypv : -1;
    longest = len > longest ? len : longest;
  }
  if (lane == 0) s_len[w] = longest;
  __syncthreads();
  if (threadIdx.x == 0) {
    int l = 0;
    for (int i = 0; i < W; ++i) l = s_len[i] > l ? s_len[i] : l;
    int32_t* inf = out.info + (size_t)g * AN_INFO_WORDS;
    inf[0] = count < max_moves ? count : max_moves;
    inf[1] = count;
    inf[2] = root_ok ? h.num_visits : 0;
    inf[3] = root_ok ? h.flip : 0;
    inf[4] = root_ok ? __float_as_int(h.V) : 0;
    inf[5] = gs.err | tp.tops->err;
    inf[6] = l;
    inf[7] = 0;
  }
}

}  // namespace elfgo
