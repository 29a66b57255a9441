// Host side of elfgo_setup / elfsp_setup / elfsp_undo (include/elf_amd.h): argument checks, the launch of k_setup (setup.cuh)
// and the self-play context's rebuild of a game from its set-up stones and move list.  Included by selfplay_host.hip, whose
// ElfSelfPlay / SpGame it works on.
#pragma once
#include "setup.cuh"

// slots ids[j] <- stones rows [k][N*N] with players [k], all host arrays; ok_host[j] = elfgo_setup's verdict.  Waits for the stream.
static int sp_setup_slots(ElfSelfPlay* sp, const std::vector<int32_t>& ids, const uint8_t* stones, const uint8_t* players, uint8_t* ok_host) {
  const int k = (int)ids.size();
  if (k == 0) return 0;
  const size_t np = (size_t)sp->opt.board_size * sp->opt.board_size;
  HIPCHK(sp->su_stones.up(k * np, sp->stream, stones));
  HIPCHK(sp->su_player.up(k, sp->stream, players));
  HIPCHK(sp->ids.up(k, sp->stream, ids.data()));
  SPCHK(elfgo_setup(sp->eng, sp->ids.d, sp->su_stones.d, sp->su_player.d, k, sp->ok.d, sp->stream));
  HIPCHK(sp->ok.down(k, sp->stream));
  HIPCHK(hipStreamSynchronize(sp->stream));
  memcpy(ok_host, sp->ok.h.data(), k);
  return 0;
}

// elfsp_undo failed after it had begun to rebuild boards (a device error; the moves and stones themselves were accepted
// before): the listed games are restarted from the empty board, so that boards, trees and host state agree again
static int sp_undo_failed(ElfSelfPlay* sp, const std::vector<int32_t>& ids, int rc) {
  if (sp_reset_boards_and_trees(sp, ids) == 0)
    for (int g : ids) sp_state_restart(sp->games[g]);
  return rc;
}
#define UNDOCHK(x)                                         \
  do {                                                     \
    int _rc = (int)(x);                                    \
    if (_rc != 0) return sp_undo_failed(sp, ids, _rc);     \
  } while (0)

// the trees of the listed games in both AIs are dropped (a tree holds the positions of the game it was grown in)
static int sp_clear_trees(ElfSelfPlay* sp, const std::vector<int32_t>& ids) {
  const int k = (int)ids.size();
  HIPCHK(sp->ids.up(k, sp->stream, ids.data()));
  for (int a = 0; a < 2; ++a)
    if (sp->pool[a].mcts) SPCHK(elfmcts_clear(sp->pool[a].mcts, sp->ids.d, k, sp->stream));
  HIPCHK(hipStreamSynchronize(sp->stream));
  return 0;
}

static bool sp_games_valid(const ElfSelfPlay* sp, const int32_t* games, int n) {
  if (n < 0 || n > sp->G || (n > 0 && !games)) return false;
  std::vector<uint8_t> seen(sp->G, 0);
  for (int j = 0; j < n; ++j) {
    if (games[j] < 0 || games[j] >= sp->G || seen[games[j]]) return false;
    seen[games[j]] = 1;
  }
  return true;
}

extern "C" {

int elfgo_setup(ElfGoEngine* e, const int32_t* ids, const uint8_t* stones, const uint8_t* next_player, int n, uint8_t* ok, void* stream) {
  if (!e || n < 0 || (!ids && n > e->capacity)) return ELFGO_E_BADARG;
  if (n == 0) return 0;
  if (!stones) return ELFGO_E_BADARG;
  DevGuard _dg(e->device);
  DISPATCH(e, hipLaunchKernelGGL(k_setup<N>, dim3(n), dim3(SETUP_WAVE), 0, (hipStream_t)stream, pool_of<N>(e), e->capacity, ids, stones,
                                 next_player, n, ok));
  HIPCHK(hipGetLastError());
  return 0;
}

int elfsp_setup(ElfSelfPlay* sp, const int32_t* games_host, int n, const uint8_t* stones_host, const uint8_t* next_player_host, void* stream) {
  if (!sp || !sp_games_valid(sp, games_host, n) || (n > 0 && !stones_host)) return ELFGO_E_BADARG;
  if (n == 0) return 0;
  if (sp_any_search_open(sp, games_host, n)) return ELFGO_E_BADARG;
  DevGuard _dg(sp->eng->device);
  sp->stream = (hipStream_t)stream;
  SPCHK(sp_poll_requests(sp));   // the games of a fresh context start (from the empty board) with their first request
  for (int j = 0; j < n; ++j)
    if (!sp->games[games_host[j]].played.empty() || sp->games[games_host[j]].ply != 1) return ELFGO_E_BADARG;   // PlaceHandicap's rule
  const size_t np = (size_t)sp->opt.board_size * sp->opt.board_size;
  const std::vector<int32_t> ids(games_host, games_host + n);
  std::vector<uint8_t> players(n, (uint8_t)S_BLACK), ok(n, 0);
  if (next_player_host) players.assign(next_player_host, next_player_host + n);
  SPCHK(sp_setup_slots(sp, ids, stones_host, players.data(), ok.data()));
  std::vector<int32_t> done;
  for (int j = 0; j < n; ++j) {
    if (ok[j] != 1) continue;
    SpGame& gm = sp->games[ids[j]];
    gm.set_up = true;
    gm.setup_player = players[j];
    gm.setup_stones.assign(stones_host + j * np, stones_host + (j + 1) * np);
    gm.ply = 1;
    done.push_back(ids[j]);
  }
  if (!done.empty()) SPCHK(sp_clear_trees(sp, done));
  return done.size() == (size_t)n ? 0 : ELFGO_E_MCTS_BASE - ELFMCTS_E_FORWARD;
}

int elfsp_undo(ElfSelfPlay* sp, const int32_t* games_host, int n, int count, void* stream) {
  if (!sp || !sp_games_valid(sp, games_host, n) || count <= 0 || !sp->sgf.empty()) return ELFGO_E_BADARG;
  if (n == 0) return 0;
  if (sp_any_search_open(sp, games_host, n)) return ELFGO_E_BADARG;
  for (int j = 0; j < n; ++j)
    if ((int)sp->games[games_host[j]].played.size() < count) return ELFGO_E_BADARG;
  DevGuard _dg(sp->eng->device);
  sp->stream = (hipStream_t)stream;
  const std::vector<int32_t> ids(games_host, games_host + n);
  // the start position of every listed game: its set-up stones, or the empty board
  std::vector<int32_t> plain, with_stones;
  std::vector<uint8_t> stones, players;
  for (int g : ids) {
    const SpGame& gm = sp->games[g];
    if (!gm.set_up) { plain.push_back(g); continue; }
    with_stones.push_back(g);
    stones.insert(stones.end(), gm.setup_stones.begin(), gm.setup_stones.end());
    players.push_back(gm.setup_player);
  }
  if (!plain.empty()) {
    UNDOCHK(sp->ids.up((int)plain.size(), sp->stream, plain.data()));
    UNDOCHK(elfgo_reset(sp->eng, sp->ids.d, (int)plain.size(), sp->stream));
    UNDOCHK(hipStreamSynchronize(sp->stream));
  }
  if (!with_stones.empty()) {
    std::vector<uint8_t> ok(with_stones.size(), 0);
    UNDOCHK(sp_setup_slots(sp, with_stones, stones.data(), players.data(), ok.data()));
    for (uint8_t v : ok) if (v != 1) return sp_undo_failed(sp, ids, ELFGO_E_MCTS_BASE - ELFMCTS_E_FORWARD);   // these stones were accepted before
  }
  // the moves that remain, one launch per ply over the games that still have one
  size_t longest = 0;
  for (int g : ids) longest = std::max(longest, sp->games[g].played.size() - (size_t)count);
  for (size_t t = 0; t < longest; ++t) {
    std::vector<int32_t> who, mv;
    for (int g : ids) {
      const SpGame& gm = sp->games[g];
      if (t + count < gm.played.size()) { who.push_back(g); mv.push_back(gm.played[t].move); }
    }
    const int k = (int)who.size();
    UNDOCHK(sp->ids.up(k, sp->stream, who.data()));
    UNDOCHK(sp->moves.up(k, sp->stream, mv.data()));
    UNDOCHK(elfgo_forward(sp->eng, sp->ids.d, sp->moves.d, k, sp->ok.d, sp->stream));
    UNDOCHK(sp->ok.down(k, sp->stream));
    UNDOCHK(hipStreamSynchronize(sp->stream));
    for (int j = 0; j < k; ++j)
      if (sp->ok.h[j] != 1) return sp_undo_failed(sp, ids, ELFGO_E_MCTS_BASE - ELFMCTS_E_FORWARD);   // these moves were played before
  }
  UNDOCHK(sp_clear_trees(sp, ids));
  // host state: the move list, the pending Record arrays, the ply
  const size_t pol_row = (size_t)(sp->opt.board_size + 2) * (sp->opt.board_size + 2);
  for (int g : ids) {
    SpGame& gm = sp->games[g];
    const size_t keep = gm.played.size() - (size_t)count;
    size_t nv = 0, npol = 0;
    for (size_t t = keep; t < gm.played.size(); ++t) { nv += gm.played[t].has_value; npol += gm.played[t].has_policy; }
    gm.played.resize(keep);
    if (gm.rec.moves.size() > keep) gm.rec.moves.resize(keep);
    gm.rec.values.resize(gm.rec.values.size() - std::min(nv, gm.rec.values.size()));
    gm.rec.policies.resize(gm.rec.policies.size() - std::min(npol * pol_row, gm.rec.policies.size()));
    gm.ply = 1 + (int)keep;
  }
  return 0;
}

}  // extern "C"
