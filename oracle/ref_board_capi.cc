// TEST INFRASTRUCTURE ONLY -- not part of the product path.
//
// extern "C" harness over the reference's board engine ALONE: base/board.cc + base/common.cc, compiled in place by oracle/Makefile
// into oracle/_ref/libelfboard{19,9}.so with nothing but the reference's own src_cpp on the include path -- no oracle/shim, no
// third-party include directory.  It shares no header with the stand-in builds (libelfref*, libelfsp*), so what it says about a
// position is evidence independent of them.  The recipe refuses the build if any dependency resolves under oracle/.
//
// A handle is a plain Board.  GoState-level rules (super-ko, the move limit, the hash history) do not exist here on purpose:
// GoState::checkMove is TryPlay2 and GoState::forward is TryPlay2 + Play (go_state.cc:74-94,123-128); rb_play is exactly that.
// Every rb_* entry point names the reference function it forwards to.
#include <cstdint>
#include <cstring>

#include "elfgames/go/base/board.h"

namespace {

constexpr int N = BOARD_SIZE;
constexpr int NP = BOARD_SIZE * BOARD_SIZE;

uint64_t hash_of(const Board* b) { return b->_hash; }

// same ten words as ref_info (oracle/ref_capi.cc)
void info_of(const Board* b, int32_t* info) {
  info[0] = b->_ply; info[1] = b->_next_player; info[2] = b->_last_move; info[3] = b->_last_move2;
  info[4] = b->_ko_age; info[5] = b->_simple_ko; info[6] = b->_simple_ko_color;
  info[7] = b->_b_cap; info[8] = b->_w_cap; info[9] = b->_num_groups - 1;
}

// per-point colour and liberties of the group at that point (0 for empty), action order a = x*N + y (board.h:189)
void board_of(const Board* b, uint8_t* colour, int16_t* libs) {
  for (int x = 0; x < N; ++x)
    for (int y = 0; y < N; ++y) {
      Coord c = OFFSETXY(x, y);
      int a = EXPORT_OFFSET_XY(x, y);
      colour[a] = b->_infos[c].color;
      libs[a] = b->_infos[c].id ? b->_groups[b->_infos[c].id].liberties : 0;
    }
}

// TryPlay2 (board.cc:784) of every point in action order, pass (M_PASS) last
void legal_of(const Board* b, uint8_t* mask) {
  GroupId4 ids;
  for (int x = 0; x < N; ++x)
    for (int y = 0; y < N; ++y) mask[EXPORT_OFFSET_XY(x, y)] = TryPlay2(b, OFFSETXY(x, y), &ids) ? 1 : 0;
  mask[NP] = TryPlay2(b, M_PASS, &ids) ? 1 : 0;
}

// isTrueEye (board.cc:1912-1914) of every point for `player`, action order
void eyes_of(const Board* b, int player, uint8_t* mask) {
  for (int x = 0; x < N; ++x)
    for (int y = 0; y < N; ++y) mask[EXPORT_OFFSET_XY(x, y)] = isTrueEye(b, OFFSETXY(x, y), (Stone)player) ? 1 : 0;
}

int play(Board* b, int c) {
  GroupId4 ids;
  if (!TryPlay2(b, (Coord)c, &ids)) return 0;
  Play(b, &ids);
  return 1;
}

}  // namespace

extern "C" {

int rb_board_size() { return BOARD_SIZE; }

void* rb_new() {
  Board* b = new Board;
  clearBoard(b);                                              // board.h:289
  return b;
}
void rb_free(void* h) { delete (Board*)h; }
void rb_reset(void* h) { clearBoard((Board*)h); }
void* rb_clone(void* h) {
  Board* b = new Board;
  copyBoard(b, (const Board*)h);                              // board.h:290
  return b;
}

// TryPlay2 then Play (what GoState::forward does to its Board); returns the TryPlay2 result
int rb_play(void* h, int c) { return play((Board*)h, c); }
int rb_try_play(void* h, int c) {
  GroupId4 ids;
  return TryPlay2((const Board*)h, (Coord)c, &ids) ? 1 : 0;
}
uint64_t rb_hash(void* h) { return hash_of((const Board*)h); }
void rb_info(void* h, int32_t* info) { info_of((const Board*)h, info); }
void rb_board(void* h, uint8_t* colour, int16_t* libs) { board_of((const Board*)h, colour, libs); }
void rb_legal_mask(void* h, uint8_t* mask) { legal_of((const Board*)h, mask); }
void rb_true_eye_mask(void* h, int player, uint8_t* mask) { eyes_of((const Board*)h, player, mask); }
int rb_is_true_eye(void* h, int c, int player) { return isTrueEye((const Board*)h, (Coord)c, (Stone)player) ? 1 : 0; }
int rb_is_game_end(void* h) { return isGameEnd((const Board*)h) ? 1 : 0; }                    // board.cc:2073-2077

// FindAllValidMoves (board.cc:949-968) for `player`, in that function's own order; returns the count
int rb_valid_moves(void* h, int player, int32_t* moves) {
  AllMoves am;
  FindAllValidMoves((const Board*)h, (Stone)player, &am);
  for (int i = 0; i < am.num_moves; ++i) moves[i] = am.moves[i];
  return am.num_moves;
}

// Replays moves[0..n) from the handle's current position and writes every array for each of the n + 1 positions (row 0 = before
// the first move, row t + 1 = after moves[t]): hash [n+1], info [n+1,10], colour / libs [n+1,NP], legal [n+1,NP+1],
// eyes [n+1,2,NP] (Black's, White's true eyes), game_end [n+1]; ok[t] = TryPlay2 result of moves[t].  A refused move leaves the
// board as it was (like GoState::forward) and the replay goes on.  Returns the number of moves that were played.
int rb_replay(void* h, const int32_t* moves, int n, uint8_t* ok, uint64_t* hash, int32_t* info, uint8_t* colour, int16_t* libs,
              uint8_t* legal, uint8_t* eyes, uint8_t* game_end) {
  Board* b = (Board*)h;
  int played = 0;
  for (int t = 0; t <= n; ++t) {
    hash[t] = hash_of(b);
    info_of(b, info + 10 * t);
    board_of(b, colour + (size_t)NP * t, libs + (size_t)NP * t);
    legal_of(b, legal + (size_t)(NP + 1) * t);
    eyes_of(b, S_BLACK, eyes + (size_t)2 * NP * t);
    eyes_of(b, S_WHITE, eyes + (size_t)2 * NP * t + NP);
    game_end[t] = isGameEnd(b) ? 1 : 0;
    if (t < n) {
      ok[t] = (uint8_t)play(b, moves[t]);
      played += ok[t];
    }
  }
  return played;
}

}  // extern "C"
