/* elf_amd.h -- C ABI of the MI355X-native ELF OpenGo self-play hot path (libelf_amd.so).
 *
 * Drop-in boundary for the board engine that the reference implements on the CPU in
 *   src_cpp/elfgames/go/base/{board,go_state,board_feature}.cc
 * and calls from src_cpp/elfgames/go/mcts/mcts.h and common/game_selfplay.cc.  Plain C: opaque
 * engine handle, raw pointers, sizes, int status.  No torch / C++ types cross this boundary.
 *
 * Conventions
 *  - status: 0 = ok, >0 = hipError_t from the runtime, <0 = ELFGO_E_* argument errors.
 *    No exceptions cross the ABI (the reference throws std::range_error for M_INVALID,
 *    go_state.cc:75-77; here the per-board `ok` byte is 0xFF for that move).
 *  - a board is addressed by its slot index in the engine-owned HBM pool.
 *  - every bulk pointer (ids, moves, masks, features, ...) is a DEVICE pointer unless the name ends
 *    in _host; `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls enqueue
 *    work and return; use elfgo_sync() or your own stream sync before reading results.
 *  - `ids` may be NULL, meaning slots [0, n).
 *  - devices: a handle belongs to the HIP device it was created on; every call switches to that device for its duration and
 *    restores the calling thread's current device on return, so handles on different GPUs can be driven from one process.
 *    `stream` must be a stream of the handle's device (NULL = that device's default stream).
 *  - threading: a handle (engine, search, self-play context, replay store) may be driven by one host thread at a time; different
 *    handles are independent.  Calls on one handle are ordered by the stream they are given; results written by a call on
 *    stream A may be consumed by a call on stream B only after the caller has ordered the streams (event / sync).
 *  - moves are reference Coords: c = (y+1)*(N+2) + (x+1), M_PASS=0, M_RESIGN=1 (base/board.h:183,
 *    base/common.h:43-47).  Actions are NN action ids a = x*N + y, pass = N*N (board.h:189).
 */
#ifndef ELF_AMD_H_
#define ELF_AMD_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ElfGoEngine ElfGoEngine;

#define ELFGO_E_BADARG (-1)
#define ELFGO_E_BADSIZE (-2)
#define ELFGO_E_NOMEM (-3)
#define ELFGO_E_NODATA (-4)   /* a draw found no eligible record (elfrq_draw); the draw state is left as it was before the call */

#define ELFGO_INFO_WORDS 16
/* per-board info record written by elfgo_info (int32 words):
 *  0 ply  1 next_player  2 last_move  3 last_move2  4 ko_age  5 simple_ko  6 simple_ko_color
 *  7 b_cap  8 w_cap  9 terminated  10 superko  11 hist_len  12 sk_len  13 hash_lo  14 hash_hi  15 0 */

/* Engine = HBM pool of `capacity` board slots for one board size (19 or 9) on HIP device `device`.
 * `zobrist` = the (N+2)^2 64-bit constants indexed by reference Coord (base/hash_num.h:12), host ptr. */
int elfgo_create(int board_size, int capacity, int device, const uint64_t* zobrist_host, ElfGoEngine** out);
int elfgo_destroy(ElfGoEngine* e);
int elfgo_board_size(const ElfGoEngine* e);
int elfgo_capacity(const ElfGoEngine* e);
size_t elfgo_slot_bytes(const ElfGoEngine* e);
int elfgo_sync(ElfGoEngine* e, void* stream);

/* GoState::reset (go_state.cc:134-141) / clearBoard (board.cc:79-107) */
int elfgo_reset(ElfGoEngine* e, const int32_t* ids, int n, void* stream);
/* GoState copy constructor (go_state.h:117-124): slot dst[i] <- slot src[i], superko records included */
int elfgo_copy(ElfGoEngine* e, const int32_t* dst_ids, const int32_t* src_ids, int n, void* stream);
/* GoState::forward (go_state.cc:74-94). moves[i] int32 Coord; ok[i] = 1 played, 0 refused, 0xFF M_INVALID */
int elfgo_forward(ElfGoEngine* e, const int32_t* ids, const int32_t* moves, int n, uint8_t* ok, void* stream);
/* legal-move mask: mask[i][a] = GoState::checkMove(action2Coord(a)) (go_state.cc:123-128 via
 * go/mcts/mcts.h:300-312), a in [0, N*N], D4 code 0; row stride = N*N+1 bytes */
int elfgo_legal_mask(ElfGoEngine* e, const int32_t* ids, int n, uint8_t* mask, void* stream);
/* BoardFeature::extractAGZ (board_feature.cc:247-290) under D4 code d4[i] (board_feature.h:88-113):
 * dst[i] = fp32 [18][N][N]; consecutive boards are `stride_floats` apart (>= 18*N*N).
 * This is the write into the batcher's "s" tensor (common/game_feature.h:38-40). d4 NULL = code 0. */
int elfgo_extract_agz(ElfGoEngine* e, const int32_t* ids, const int32_t* d4, int n, float* dst,
                      int64_t stride_floats, void* stream);
/* The same extraction with a selectable row format (emit what an fp16 channels_last net reads, so the
 * fp32->fp16 cast and the NCHW->NHWC permute of the reference's trainer.py/model path disappear):
 *   ELFGO_FEAT_F32_NCHW  fp32 [18][N][N]  (the reference's "s" row, what elfgo_extract_agz writes)
 *   ELFGO_FEAT_F16_NHWC  fp16 [N][N][18]  (= torch channels_last of a [18,N,N] half tensor)
 * stride_elems counts elements of the chosen type between consecutive rows (>= 18*N*N). */
#define ELFGO_FEAT_F32_NCHW 0
#define ELFGO_FEAT_F16_NHWC 1
int elfgo_extract_agz_fmt(ElfGoEngine* e, const int32_t* ids, const int32_t* d4, int n, void* dst, int64_t stride_elems,
                          int fmt, void* stream);
/* GoState::evaluate (go_state.h:194-203): Tromp-Taylor area(black) - area(white) - komi; superko -> +-1 */
int elfgo_evaluate(ElfGoEngine* e, const int32_t* ids, int n, float komi, float* out, void* stream);
/* per-board info records (ELFGO_INFO_WORDS int32 each) */
int elfgo_info(ElfGoEngine* e, const int32_t* ids, int n, int32_t* out, void* stream);
/* stone colour per point (uint8, 0/1/2) and liberties of the group on it (int16, 0 if empty), action order */
int elfgo_export_board(ElfGoEngine* e, const int32_t* ids, int n, uint8_t* colour, int16_t* libs, void* stream);
/* from each slot's current position play uniformly random legal, non-true-eye
 * moves until GoState::terminated(); pass when none.  The move is the (rand % count)-th candidate in x-major order with the
 * counter RNG   key = fmix32(lo32(seed)) ^ fmix32(hi32(seed) + 0x7F4A7C15);   rand = fmix32(key + ply * 0x9E3779B9)
 * (32-bit wrapping arithmetic; fmix32 = murmur3's 32-bit finaliser; oracle/go_oracle.c and oracle/ref_capi.cc state the same
 * function for the CPU checkers).
 * out[i] = {hash_lo, hash_hi, ply, steps}.  Whole games run inside one launch, position in LDS. */
int elfgo_playout(ElfGoEngine* e, const int32_t* ids, const uint64_t* seeds, int n, int max_steps,
                  uint32_t* out, void* stream);

/* Put stones on boards: slot ids[i] <- the position whose stones are stones[i][a] (0 empty, 1 black, 2 white; a = x*N + y,
 * the order of elfgo_export_board's colour rows, row stride N*N bytes) with next_player[i] (1 / 2; NULL = Black) to move.
 * ok[i] = 1 done, 0 refused (a byte > 2, a player other than 1 / 2, or a group without a liberty): a refused slot is left
 * exactly as it was.  ids NULL = slots [0, n); a slot named twice is the caller's error.  All pointers are device pointers.
 * The slot afterwards is what elfgo_reset leaves (clearBoard, board.cc:79-107: ply 1, last moves M_INVALID, no ko, no captures,
 * no super-ko records) plus the group tables and the Zobrist hash of the stones and the side to move -- for a legal arrangement
 * of black stones PlaceHandicap's board (board.cc:109-126), generalised to both colours -- and the position is the ONE entry of
 * the history ring (hist_len 1), so that elfgo_extract_agz shows the stones in planes 0 / 1 as it does for any position reached
 * by play.  (The reference's GoState::applyHandicap leaves _history empty, its net would see an empty board under the handicap
 * stones: a defect nobody exercises there -- nothing calls applyHandicap -- and not behaviour that is reproduced here.)
 * SGF carries no ko point, so none can be set up. */
int elfgo_setup(ElfGoEngine* e, const int32_t* ids, const uint8_t* stones, const uint8_t* next_player, int n, uint8_t* ok,
                void* stream);

/* Tromp-Taylor area of each point of a position (simple_flood_fill per colour + the black && !white / white && !black rule of
 * simple_tt_scoring, go_state.h:32-93): out[i][a] = 0 neutral, 1 black, 2 white, a = x*N + y (the action order of
 * elfgo_legal_mask under D4 code 0); row stride N*N bytes.  Always the flood fill of the stones: the super-ko +-1 rule of
 * GoState::evaluate plays no part. */
int elfgo_area_map(ElfGoEngine* e, const int32_t* ids, int n, uint8_t* out, void* stream);

/* Ladder reading for the side to move (checkLadder / checkLadderUseSearch, base/board.cc:299-439, :476-524):
 *     depth[i][a] = checkLadder(board, GroupId4 of a, next_player) where point a = x*N + y is legal by TryPlay2, else 0
 * A depth d > 0 means: the mover extends a group out of atari at a and is still captured in a ladder after d plies (the move at
 * a included).  calls (may be NULL) receives the reference's num_call after the search of each point: 0 where the point is
 * illegal or checkLadder's own test (two empty neighbours, one enemy group with >= 3 liberties, one own group in atari) rejects
 * it without a search, -1 where a bound of the device search cut it (a line of more than 1024 moves, or more than 32000 plays
 * for one point, backtracking replays included); such a point's depth is 0.  A row whose slot id lies outside the pool gets
 * depth 0 and calls -1.  int16 [n][N*N] each, device pointers; ids NULL = slots [0, n).  The slots are only read: the search
 * plays on a private copy with the reference's Board-level rules (no super-ko, termination or move-limit test). */
int elfgo_ladder_map(ElfGoEngine* e, const int32_t* ids, int n, int16_t* depth, int16_t* calls, void* stream);

/* Monte-Carlo ownership from device playouts.  The handle owns the scratch of the playout copies (one super-ko record area
 * per wave in flight) and the launch geometry; several handles may share an engine.  max_lanes = waves in flight
 * (<= 0: a default from the device's CU count); destroy the handle before its engine. */
typedef struct ElfGoOwnership ElfGoOwnership;
int elfgo_own_create(ElfGoEngine* e, int max_lanes, ElfGoOwnership** out);
int elfgo_own_destroy(ElfGoOwnership* o);
size_t elfgo_own_scratch_bytes(const ElfGoOwnership* o);
/* For source row i < n and playout k < playouts: a private copy of slot ids[i] is played with elfgo_playout's policy and RNG
 * to GoState::terminated() or max_steps, with
 *     seed(i, k) = seeds[i] + k * 0x9E3779B97F4A7C15   (mod 2^64)
 * (playout 0 of a row is what elfgo_playout would play from that slot with seeds[i]), and the area map of its end position
 * (elfgo_area_map's; a playout cut by max_steps is scored where it stands) is added into
 *     counts[i][0][a] black, counts[i][1][a] white                       int32 [n][2][N*N]
 *     stats[i] = { sum of (black area - white area), playouts with (float)diff - komi > 0,
 *                  playouts that ended with the super-ko flag set, sum of steps played }   int64 [n][4]
 * The call zeroes counts and stats on `stream` itself.  Integer sums only: the result does not depend on scheduling or on
 * max_lanes.  The source slots are only read (header, stones, Bloom words and super-ko records alike); a slot may be named
 * several times.  A row whose slot id lies outside the pool is not played and keeps zeros (elfgo_ld_run's rule).
 * ELFGO_E_BADARG for a null pointer (ids may be NULL), n <= 0 or playouts <= 0. */
int elfgo_own_run(ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts, int max_steps,
                  float komi, int32_t* counts, int64_t* stats, void* stream);

/* Self-atari reading and the reference's candidate moves for the side to move (isSelfAtari, base/board.cc:254-297;
 * FindAllCandidateMoves, board.cc:850-890):
 *     mask[i][a]   = 1 iff point a = x*N + y is in FindAllCandidateMoves(board, next_player, self_atari_thres): legal by
 *                    TryPlay, not the mover's own true eye, and not a self-atari of self_atari_thres stones or more
 *     stones[i][a] = the num_stones that isSelfAtari(board, NULL, a, next_player, &num_stones) writes where it returns true
 *                    (the group on a after the move has exactly one liberty; num_stones is its size), else 0
 * stones is 0 at illegal points; a mover's own true eye can carry a value although its mask byte is 0.  The threshold has the
 * reference's meaning (board.cc:883: the move is dropped when num_stones >= self_atari_thres), so a value <= 1 drops every
 * self-atari and one above N*N drops none; stones does not depend on it.  uint8 / int16 [n][N*N], device pointers, row stride
 * N*N; either may be NULL, not both.  ids NULL = slots [0, n).  A row whose slot id lies outside the pool gets mask 0 and
 * stones -1.  The slots are only read; a slot may be named several times.  ELFGO_E_BADARG for a null engine, n <= 0 or both
 * outputs NULL: nothing is launched. */
int elfgo_candidates(ElfGoEngine* e, const int32_t* ids, int n, int self_atari_thres, uint8_t* mask, int16_t* stones,
                     void* stream);
/* elfgo_playout with the move list of FindAllCandidateMoves(board, next_player, self_atari_thres) (board.cc:850-890) in place
 * of "legal and not the mover's own true eye": the same RNG, the same (rand % count)-th candidate in x-major order, pass when
 * there is none, the same termination and the same out words.  With a threshold above N*N it plays elfgo_playout's games. */
int elfgo_playout_cand(ElfGoEngine* e, const int32_t* ids, const uint64_t* seeds, int n, int max_steps, int self_atari_thres,
                       uint32_t* out, void* stream);
/* elfgo_own_run whose playouts are elfgo_playout_cand's (board.cc:850-890): the same seed rule, counts and stats. */
int elfgo_own_run_cand(ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts, int max_steps,
                       float komi, int self_atari_thres, int32_t* counts, int64_t* stats, void* stream);

/* The reference's static life reading of a position, for both colours at once: eye classes (isEye, isFakeEye, isSemiEye,
 * isTrueEye, getEyeColor, base/board.cc:1850-1922), groups that live by two eyes (GivenGroupLives / OneGroupLives,
 * board.cc:1108-1221), the eye-and-stone score (getFastScore, board.cc:1924-1952) and the framing of a life-and-death problem
 * (getBoardBBox, GuessLDAttacker, board.cc:1024-1106).  Per row i, a = x*N + y:
 *     eye[i][a]          uint8: Black's answers in bits 0-3, White's in bits 4-7: bit 0 isEye, 1 isFakeEye, 2 isTrueEye,
 *                        3 isSemiEye.  isFakeEye is answered at every point, stones included, as the reference function answers
 *                        there; the other three are 0 off empty points.  None depends on legality or on a pending ko.
 *     semi_move[i][c][a] int16, c = 0 Black / 1 White: the action of the *move isSemiEye writes where it returns true for that
 *                        colour (the one empty diagonal that is no eye of the colour), else -1
 *     alive[i][a]        uint8: 1 on every stone of a group for which GivenGroupLives holds (two true eyes of its colour next
 *                        to THIS group, each with enough territory on its diagonals, and more than one liberty), else 0
 *     summary[i]         int32 [12]: 0 getFastScore(RULE_CHINESE), 1 getFastScore(RULE_JAPANESE) (the slot's captures; the
 *                        reference never writes _rollout_passes, so it is 0), 2 / 3 OneGroupLives(Black / White, box),
 *                        4-7 the box left, top, right, bottom, 8 GuessLDAttacker(box) (1 Black, 2 White; White on a tie),
 *                        9 / 10 living Black / White groups with a stone in the box, 11 zero (reserved)
 * The box is the reference's half-open Region in x and y: regions int32 [n][4] (left, top, right, bottom), each value clamped
 * into [0, N]; NULL = getBoardBBox of the row ((N, N, 0, 0) on an empty board: attacker White, nothing lives).  The scores are
 * integers as the reference computes them; no komi.  Device pointers, row strides N*N, 2*N*N, N*N and 12; each output may be
 * NULL, not all four.  ids NULL = slots [0, n).  A row whose slot id lies outside the pool gets maps 0, semi_move -1 and summary
 * all -1.  The slots are only read; a slot may be named several times.  ELFGO_E_BADARG for a null engine, n <= 0, ids NULL with
 * n above the capacity, or all four outputs NULL: nothing is launched. */
int elfgo_life_map(ElfGoEngine* e, const int32_t* ids, int n, const int32_t* regions, uint8_t* eye, int16_t* semi_move,
                   uint8_t* alive, int32_t* summary, void* stream);

/* The reference's Region move lists of board slots (base/board.cc), per row i, a = x*N + y, all uint8:
 *     cand[i][a]   1 iff a is in FindAllCandidateMovesInRegion(board, &box, next_player, self_atari_thres) (:892-947): the
 *                  legal points of the side to move inside the box that are neither its own true eye nor a self-atari of
 *                  self_atari_thres stones or more -- elfgo_candidates' mask clipped to the box
 *     valid[i][a]  1 iff a is in FindAllValidMovesInRegion(board, &box) (:970-1005): the legal points of the side to move
 *                  inside the box
 *     groups[i][a] 1 on every stone whose group has GroupInRegion(board, id, &box) (:1183-1196) true -- some stone of the
 *                  group lies inside the box -- else 0
 * regions int32 [n][4] = left, top, right, bottom, half-open in x and y like the reference's Region, each value clamped into
 * [0, N].  regions NULL is the reference's nullptr, THE WHOLE BOARD -- unlike elfgo_life_map, where NULL means the bounding box
 * of the stones.  Device pointers, row stride N*N; any output may be NULL, not all three.  ids NULL = slots [0, n).  A row
 * whose slot id lies outside the pool gets zeros.  The slots are only read; a slot may be named several times.
 * ELFGO_E_BADARG for a null engine, n <= 0, ids NULL with n above the capacity, or all three outputs NULL: nothing is launched. */
int elfgo_region_moves(ElfGoEngine* e, const int32_t* ids, int n, const int32_t* regions, int self_atari_thres, uint8_t* cand,
                       uint8_t* valid, uint8_t* groups, void* stream);

/* Life-and-death reading by region playouts, on the scratch and launch geometry of an ElfGoOwnership handle.  Per row i:
 *   - the box is regions[i] (as above, clamped); regions NULL = getBoardBBox of the row, elfgo_life_map's rule (NOT the whole
 *     board);
 *   - the attacker is attackers[i] where that is 1 (Black) or 2 (White), else GuessLDAttacker(box) of the source position
 *     (attackers NULL = guess every row); the defender is the other colour;
 *   - playout k < playouts works on a private copy of the slot with seed seeds[i] + k * 0x9E3779B97F4A7C15 (mod 2^64), the
 *     counter RNG, x-major pick and GoState::terminated() of elfgo_playout_cand, and the move list
 *     FindAllCandidateMovesInRegion(board, &box, next_player, self_atari_thres); it passes when the list is empty, stops at
 *     termination or after max_steps moves, and is judged where it stands.
 * Outputs (device pointers; the call zeroes them on `stream` first):
 *     info[i]  int32 [8]: 0-3 the box used (left, top, right, bottom), 4 attacker, 5 defender, 6 side to move,
 *              7 OneGroupLives(defender, box) of the source position
 *     stats[i] int64 [8]: 0 playouts at whose end OneGroupLives(defender, box) holds ("lived"), 1 playouts at whose end the
 *              defender has a stone inside the box ("survived"), 2 / 3 sum of the defender's / the attacker's stones inside
 *              the box at the end, 4 super-ko endings, 5 steps played, 6 sum mod 2^64 of the end positions' hashes, 7 zero
 *     first[i] int32 [3][N*N + 1]: per first move of the playout (action a; index N*N = pass): playouts, lived, survived.  A
 *              playout that made no move is counted in stats only.
 * Integer sums: the result does not depend on scheduling or on the handle's max_lanes.  Source slots are only read and may be
 * named several times; a row whose slot id lies outside the pool is not played and keeps zeros.  ELFGO_E_BADARG for a null
 * handle, seeds or output, n <= 0, playouts <= 0, ids NULL with n above the capacity, or n * playouts above 2^31 - 16. */
int elfgo_ld_run(ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts, int max_steps,
                 int self_atari_thres, const int32_t* regions, const uint8_t* attackers, int32_t* info, int64_t* stats,
                 int32_t* first, void* stream);

/* The reference's 25 DarkForest planes (BoardFeature::extract, base/board_feature.cc:43-237; what GameOptions.use_df_feature
 * selects there) of board slots: fp32 [25][N][N] per row under D4 code d4[i], "ours" = the side to move:
 *    0-2 / 3-5  our / the opponent's stones of groups with 1, 2, >= 3 liberties (getLibertyMap3binary)
 *    6          the simple-ko point, whichever colour it binds (getSimpleKoLocation, board.cc:466-474)
 *    7 / 8 / 9  our stones, the opponent's, empty points
 *    10 / 11    on our / the opponent's stones (float)exp((last_placed - ply) / 10.0), last_placed = the ply at which the stone
 *               was placed (getHistoryExp); bit-equal to the reference: the values come from elfgo_df_exp_table's table
 *    14 / 15    Manhattan distance to our / the opponent's nearest stone, 0 on the stones, 10000 everywhere when the colour
 *               has none (getDistanceMap)
 *    16 / 17    all 1.0 when Black / White is to move
 *    12, 13, 18-24  zero
 * Planes 10 / 11 need Info::last_placed, which a board slot does not carry.  An ElfGoDf handle keeps it beside an engine: a
 * table uint16 [capacity][N*N] in action order (a = x*N + y), zeroed at creation, plus the device copy of the exponent table.
 * The elfgo_df_reset / _copy / _forward / _setup forms are the engine's calls of the same name (same arguments, same results,
 * same stream) followed by the table's part: rows to 0; rows copied; ply p under the stone of an accepted placement at ply p
 * (a pass, a resignation and a refused move change nothing; captured points keep their entry, which nothing reads: the
 * reference only reads entries under stones); after an accepted set-up 1 under every stone and 0 elsewhere (PlaceHandicap
 * plays at ply 1 and puts the ply back, board.cc:109-126), a refused row untouched.  ok may be NULL as in the engine's calls,
 * then n must not exceed the capacity.
 * THE TABLE FOLLOWS ONLY THESE FOUR CALLS.  Anything else that plays on the engine's slots leaves it stale: elfgo_reset /
 * _copy / _forward / _setup called without the handle, every elfgo_playout* call, and the self-play / MCTS contexts that
 * borrow an engine (elfsp_*, elfmcts_*).  Several handles may share an engine; destroy a handle before its engine. */
typedef struct ElfGoDf ElfGoDf;
int elfgo_df_create(ElfGoEngine* e, ElfGoDf** out);
int elfgo_df_destroy(ElfGoDf* df);
int elfgo_df_reset(ElfGoDf* df, const int32_t* ids, int n, void* stream);
int elfgo_df_copy(ElfGoDf* df, const int32_t* dst_ids, const int32_t* src_ids, int n, void* stream);
int elfgo_df_forward(ElfGoDf* df, const int32_t* ids, const int32_t* moves, int n, uint8_t* ok, void* stream);
int elfgo_df_setup(ElfGoDf* df, const int32_t* ids, const uint8_t* stones, const uint8_t* next_player, int n, uint8_t* ok,
                   void* stream);
/* dst[i] = the 25 planes of slot ids[i] with that slot's table row; consecutive rows are stride_floats apart (>= 25*N*N; dst
 * 4-byte aligned, rows need no further alignment).  d4 NULL = code 0, ids NULL = slots [0, n).  A row whose slot id lies
 * outside the pool is all zero.  The slots and the table are only read; a slot may be named several times. */
int elfgo_df_extract(ElfGoDf* df, const int32_t* ids, const int32_t* d4, int n, float* dst, int64_t stride_floats, void* stream);
/* out[i] = the table row of slot ids[i] (uint16 [n][N*N]; zero for an id outside the pool) */
int elfgo_df_placed(ElfGoDf* df, const int32_t* ids, int n, uint16_t* out, void* stream);
/* The same kernel for callers that keep last_placed themselves: row i of placed_rows (uint16 [n][N*N], device) serves
 * ids[i].  It takes the handle and not the engine because the exponent table on the device belongs to the handle (an engine
 * carries no DarkForest state at all); the handle's own table is not read. */
int elfgo_extract_df(ElfGoDf* df, const int32_t* ids, const int32_t* d4, int n, const uint16_t* placed_rows, float* dst,
                     int64_t stride_floats, void* stream);
/* Host only, no GPU needed: out_host[d] = (float)exp((0 - d) / 10.0) for d in [0, 2*N*N], 2*N*N + 1 floats -- the reference's own
 * expression through the C library's double exp, evaluated once per handle; the kernel looks planes 10 / 11 up at
 * d = ply - last_placed.  ELFGO_E_BADSIZE for a board size other than 19 or 9. */
int elfgo_df_exp_table(int board_size, float* out_host);

/* ------------------------------------------------------------------------------------------------
 * Device-resident MCTS (one tree per game) -- replaces, behind the same seams, the reference's
 *   elf/ai/tree_search/tree_search.h        TreeSearchT / TreeSearchSingleThreadT::batch_rollouts (:200-262)
 *   elf/ai/tree_search/tree_search_node.h   NodeT / SearchTreeT
 *   elfgames/go/mcts/mcts.h                 MCTSActor::evaluate / pi2response (:73-121, :256-332)
 * The net stays outside: elfmcts_select() writes the leaf features of every game into the caller's
 * "s" tensor (the write GoFeature::extractStateAGZ does into the batcher's tensor, common/game_feature.h:38-40)
 * and elfmcts_expand() consumes the caller's "pi"/"V" reply tensors (ReplyPolicy/ReplyValue, :42-71).
 * ------------------------------------------------------------------------------------------------ */
typedef struct ElfMcts ElfMcts;

/* TSOptions + SearchAlgoOptions (elf/ai/tree_search/tree_search_options.h:23-229), MCTSActorParams (go/mcts/mcts.h:17-37) */
typedef struct ElfMctsOptions {
  int32_t num_rollouts_per_batch;   /* TSOptions.num_rollouts_per_batch */
  int32_t virtual_loss;             /* TSOptions.virtual_loss */
  int32_t use_prior;                /* alg_opt.use_prior */
  int32_t unexplored_q_zero;        /* alg_opt.unexplored_q_zero */
  int32_t root_unexplored_q_zero;   /* alg_opt.root_unexplored_q_zero */
  float c_puct;                     /* alg_opt.c_puct */
  float komi;                       /* MCTSActorParams.komi */
  int32_t ply_pass_enabled;         /* MCTSActorParams.ply_pass_enabled */
  int32_t remove_pass_if_dangerous; /* MCTSActorParams.remove_pass_if_dangerous */
  int32_t rotation_flip;            /* MCTSActorParams.rotation_flip */
  int32_t num_threads;              /* TSOptions.num_threads: search threads per game (tree_search.h:345-368), >= 1; one step runs
                                     * their batch_rollouts in sequence on the shared tree, so a move costs
                                     * num_threads x num_rollouts_per_thread rollouts (tree_search.h:472-476).
                                     * num_threads x num_rollouts_per_batch must be <= elfmcts_max_rollouts_per_step() = 1024
                                     * (the leaf table of one step; ELFGO_E_BADARG otherwise) */
  int32_t reserved0;
  int64_t required_version;         /* MCTSActorParams.required_version: < 0 = replies of any model version are accepted */
} ElfMctsOptions;

#define ELFMCTS_E_POOL 1      /* the context's node pool is exhausted (raise nodes_per_game: the pool holds num_games x nodes_per_game ids) */
#define ELFMCTS_E_ROOT_HASH 2 /* TreeSearch::Root state is not the same as the input state (tree_search.h:488-492) */
#define ELFMCTS_E_FORWARD 4   /* a tree edge could not be played */
#define ELFMCTS_E_RNG 8       /* more D4 draws requested than uploaded with elfmcts_set_d4 */
#define ELFMCTS_E_VERSION 16  /* a reply row's model version ("rv") differs from required_version (go/mcts/mcts.h:209-217) */

#define ELFMCTS_ROOT_WORDS 8
/* per-game record of elfmcts_root (int32 words): 0 n_edges 1 num_visits 2 status 3 root id 4 V (float bits)
 * 5 d4 draws consumed this move 6 error bits 7 node ids the game's tree holds */

/* `num_games` trees over boards of engine `e` (game g searches from board slot board_ids[g]).
 * Node memory is ONE pool of num_games x nodes_per_game node ids (nodes_per_game a multiple of 64) shared by the context's games:
 * the reference takes its nodes from the heap (SearchTreeT::addNode, tree_search_node.h:439-443; recursiveFree :445-467), so a game
 * whose kept subtree is large simply holds more of them -- size nodes_per_game for the MEAN tree, not for the worst game.  A step's ids
 * are popped from the pool's free stack with one atomic per game, treeAdvance pushes the freed subtrees back.  d4_window = opt->num_threads x (max D4 draws ONE search thread makes per move):
 * every search thread's MCTSActor owns a generator (TreeSearchT's actor_gen, tree_search.h:339-343; all seeded alike,
 * game_selfplay.cc:45-47,77), so the draws are laid out as one window per thread. */
int elfmcts_create(ElfGoEngine* e, int num_games, int nodes_per_game, int d4_window, const ElfMctsOptions* opt, ElfMcts** out);
int elfmcts_destroy(ElfMcts* m);
/* new options for the following steps; num_threads must be the value the trees were created with (ELFGO_E_BADARG otherwise) */
int elfmcts_set_options(ElfMcts* m, const ElfMctsOptions* opt);
int elfmcts_num_threads(const ElfMcts* m);
/* D4 draws each search thread's actor has consumed this move: host int32 [num_games][num_threads], copied on `stream`
 * (synchronise before reading).  Thread 0's count is also RootInfo word 5. */
int elfmcts_thread_draws(ElfMcts* m, int32_t* out_host, void* stream);
/* row format elfmcts_select / elfsp_begin_step write into s_dst (ELFGO_FEAT_*; default fp32 NCHW). With
 * ELFGO_FEAT_F16_NHWC s_dst points to halfs and the stride argument counts halfs. */
int elfmcts_set_feature_format(ElfMcts* m, int fmt);
int elfmcts_get_feature_format(const ElfMcts* m, int* fmt);
/* largest num_threads x num_rollouts_per_batch a search step can hold (1024: the stride of the per-game leaf tables; the step's table in LDS is sized by the launch) */
int elfmcts_max_rollouts_per_step(void);
/* Which games the per-game launches that follow act on: mask = device bytes [num_games], 0 = the game is left alone (no root
 * check, no noise, no descents, no rows), 1 = it searches, 2 = TreeSearchT::runPolicyOnly (tree_search.h:385-407: the root is
 * evaluated if it has not been, nothing else).  NULL (the default) = every game searches.  Applies to elfmcts_set_root,
 * elfmcts_dirichlet, elfmcts_select (and through it to expand / backup).  The pointer is kept, not copied. */
int elfmcts_set_game_mask(ElfMcts* m, const uint8_t* mask);
/* MCTSActorParams.required_version per game (device int64 [num_games], < 0 = any version); NULL (the default) = the value of
 * ElfMctsOptions.required_version for every game.  The pointer is kept, not copied. */
int elfmcts_set_required_versions(ElfMcts* m, const int64_t* versions);
int elfmcts_num_games(const ElfMcts* m);
int elfmcts_edge_stride(const ElfMcts* m);   /* row length of the per-edge arrays (368 at 19x19, 96 at 9x9) */
/* HBM a game adds to a context at `nodes_per_game` node ids (its share of the pool's records of both classes and id arrays, plus
 * what is per game: stash, leaf / row tables, path rows, D4 windows): what a caller sizes num_games x nodes_per_game against
 * elfgo_mem_info.  A node lives in a 5 888-B record (19x19; 1 920 B at 9x9) until its 17th edge is followed, then in an 11 520-B one;
 * one big record per 16 small ones exists and that class cannot run out first (a big node has >= 17 children that are nodes).
 * The first form assumes 1 search thread, 16 rollouts per batch, a 1024-draw window; the second takes them (path rows are
 * 512 B per leaf of a step: 512 KB per game at the 1024-leaf maximum). */
size_t elfmcts_tree_bytes_per_game(int board_size, int nodes_per_game);
size_t elfmcts_tree_bytes_per_game2(int board_size, int nodes_per_game, int num_threads, int rollouts_per_batch, int d4_window);
size_t elfmcts_node_bytes(const ElfMcts* m);   /* elfmcts_tree_bytes_per_game2 / nodes_per_game, rounded up (6 6xx B at 19x19) */
/* Node ids of the context (synchronises the device).  out8_host: 0 small records in all, 1 of them free (on the pool's stack or in
 * a game's stash), 2 big records in all, 3 free, 4 ids held by all trees now, 5 by the largest tree now, 6 the most ONE tree has
 * held since the last reset, 7 the sum over games of those per-tree maxima (what G fixed per-game pools would have to provide:
 * compare with 4).  reset_peaks != 0 restarts the maxima.  No counterpart in the reference (its nodes live on the heap). */
int elfmcts_pool_info(ElfMcts* m, int64_t* out8_host, int reset_peaks);
/* test / debug service: node ids held per game (host int32 [num_games]), counted by a scan of the pool's owner array -- what RootInfo
 * word 7 tracks incrementally.  Synchronises the device. */
int elfmcts_count_live(ElfMcts* m, int32_t* out_host);
/* SearchTreeT::clear (tree_search_node.h:411-416) for games[0..n) (device int32, NULL = all games) */
int elfmcts_clear(ElfMcts* m, const int32_t* games, int n, void* stream);
/* TreeSearchT::setRootNodeState (tree_search.h:478-493) for every game; board_ids device int32 or NULL (slot g) */
int elfmcts_set_root(ElfMcts* m, const int32_t* board_ids, void* stream);
/* rng() % 8 draws of the search threads' actors (BoardFeature::RandomShuffle, board_feature.h:74-78), host uint8
 * [num_games][num_threads][d4_window / num_threads]: window t = the coming draws of thread t's mt19937 */
int elfmcts_set_d4(ElfMcts* m, const uint8_t* d4_host, void* stream);
/* NodeT::enhanceExploration (tree_search_node.h:132-155): etas device f32 [num_games][edge_stride] in edge
 * iteration order, Z device f32 [num_games] (= 1e-10 + sum of etas, accumulated in fp32 on the host) */
int elfmcts_dirichlet(ElfMcts* m, const float* etas, const float* Z, float epsilon, void* stream);
/* first half of batch_rollouts (:205-233): num_threads x num_rollouts_per_batch descents per game, then the features of
 * every leaf that needs the net into s_dst (row r at s_dst + r*stride_elems elements of the feature format, rows game-major);
 * counts (device int32[4], 8-byte aligned): [0] <- rows, [1] <- OR of error bits, [2..3] += rows (u64 running total). */
int elfmcts_select(ElfMcts* m, const int32_t* board_ids, void* s_dst, int64_t stride_elems, int32_t* counts, void* stream);
/* second half (:235-259): pi2response + setEvaluation for the n_rows leaves of the last select, then backup.
 * rv (device int64 [n_rows], may be NULL) = the "rv" reply column, checked against required_version.
 * n_rows < 0: use the row count the last select left in its `counts` buffer on the device (no host round trip). */
int elfmcts_expand(ElfMcts* m, const float* pi, int64_t pi_stride_floats, const float* value, const int64_t* rv, int n_rows,
                   void* stream);
/* root edges in the reference's iteration order (what MCTSResultT::addActions walks, tree_search_base.h:237-294);
 * info device int32 [num_games][ELFMCTS_ROOT_WORDS]; the per-edge outputs ([num_games][edge_stride]) may be NULL */
int elfmcts_root(ElfMcts* m, int32_t* info, int32_t* coord, int32_t* visits, float* prior, float* reward, int32_t* child, void* stream);
/* Search analysis: the candidate moves of every game's root and the principal variation the search expects below each (what
 * the reference shows with SearchTreeT::printTree, tree_search_node.h:479-528).  One read-only launch; nothing but the output
 * arrays is written.
 *   candidates  the root edges with visits > 0, ranked by visits descending, ties to the edge that comes first in the reference's
 *               iteration order (lower `orig`): rank 0 is MCTSResultT::best_action under MOST_VISITED (tree_search_base.h:248-292).
 *               The first max_moves of them are written.
 *   pv          pv[0] is the candidate's own Coord; then, from the candidate's child node on, the most-visited edge of each node
 *               (first in iteration order on ties) until a node has no followed edge, its most-visited edge has 0 visits, or
 *               max_pv Coords are written.
 * All outputs are device pointers.  info int32 [num_games][ELFMCTS_ANALYZE_WORDS]: 0 candidates written 1 root edges with
 * visits > 0 (before the cut at max_moves) 2 root num_visits 3 root flip (1 = White to move at the root) 4 root V (float bits)
 * 5 error bits, as word 6 of elfmcts_root 6 longest pv_len written 7 zero.  coord / orig / visits / reward / prior / pv_len are
 * [num_games][max_moves] and pv is int32 [num_games][max_moves][max_pv]; any of them may be NULL.  reward is the raw black-positive
 * sum and prior the stored prior: the bits elfmcts_root reports for that edge; orig is the edge's index in elfmcts_root's arrays.
 * Unused entries: coord -1, orig -1, visits 0, reward 0, prior 0, pv_len 0, pv -1.
 * 1 <= max_moves <= ELFMCTS_ANALYZE_MAX_MOVES, 1 <= max_pv <= ELFMCTS_ANALYZE_MAX_PV; anything else, or a NULL m / info, is
 * ELFGO_E_BADARG and nothing is launched.
 * Meaningful between an elfmcts_expand and the next elfmcts_select, when no virtual loss is outstanding.  At any other point of
 * the stream the call is still safe (every walk is bounded and checks the ids it follows) but reports the statistics of the
 * descents in flight. */
#define ELFMCTS_ANALYZE_WORDS 8
#define ELFMCTS_ANALYZE_MAX_MOVES 64
#define ELFMCTS_ANALYZE_MAX_PV 32
int elfmcts_analyze(ElfMcts* m, int max_moves, int max_pv, int32_t* info, int32_t* coord, int32_t* orig, int32_t* visits,
                    float* reward, float* prior, int32_t* pv_len, int32_t* pv, void* stream);
/* Test / debug service: checks the invariants of every live node record (scoring-order prefix sorted and linked to its child
   nodes, never-followed tail without statistics and by descending prior, visit counts add up).  Synchronises the device.
   out5_host: 0 number of violations, 1 code, 2 game, 3 node, 4 position of one of them.  No counterpart in the reference. */
int elfmcts_validate(ElfMcts* m, int32_t* out5_host);
/* statistics: total number of tree nodes descended through by all rollouts so far (mean depth = this / rollouts); synchronous */
int elfmcts_node_visits(ElfMcts* m, int64_t* out_host);
/* SearchTreeT::treeAdvance (tree_search_node.h:420-436), moves device int32 [num_games] (reference Coords) */
int elfmcts_advance(ElfMcts* m, const int32_t* moves, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Self-play driver: G games advanced in lock-step on one GPU -- the host half of
 *   elfgames/go/common/game_selfplay.cc  GoGameSelfPlay::act (:272-430) and
 *   elf/ai/tree_search/mcts.h            MCTSAI_T::act (:59-81)
 * One elfsp_begin_step / elfsp_end_step pair is one batch of the reference's batch interface
 * (GCWrapper._call, src_py/elf/utils_elf.py:368-414): begin fills "s" rows [0, n_rows), the caller runs the
 * net, end consumes "pi" and "V".  Moves, Dirichlet noise, move sampling, resignation and game restarts
 * happen inside end_step when a search completes.
 * ------------------------------------------------------------------------------------------------ */
#define ELFGO_E_MCTS_BASE (-100) /* status = ELFGO_E_MCTS_BASE - (OR of ELFMCTS_E_* bits) */
typedef struct ElfSelfPlay ElfSelfPlay;

typedef struct ElfSpOptions {
  int32_t board_size;               /* 19 or 9 */
  int32_t num_games;                /* ContextOptions.num_games (games per GPU) */
  int32_t nodes_per_game;           /* node records per tree (multiple of 64) */
  int32_t num_rollouts_per_thread;  /* TSOptions.num_rollouts_per_thread; one search thread per game */
  int32_t persistent_tree;          /* TSOptions.persistent_tree */
  float root_epsilon, root_alpha;   /* TSOptions.root_epsilon / root_alpha */
  uint32_t seed;                    /* GameOptions.seed; per-game rule below */
  int32_t policy_distri_cutoff;     /* GameOptions.policy_distri_cutoff */
  int32_t move_cutoff;              /* GameOptions.move_cutoff */
  float resign_thres;               /* ClientCtrl.{black,white}_resign_thres */
  float never_resign_prob;          /* ClientCtrl.never_resign_prob */
  int32_t log_searches;             /* keep the first N search results for elfsp_search_log (tests) */
  int32_t keep_records;             /* > 0: keep the Record JSON of the last N finished games for elfsp_pop_record */
  int32_t policy_distri_training_for_all; /* GameOptions.policy_distri_training_for_all: record the MCTS policy of every move */
  int32_t model_ver;                /* Record.request.vers.black_ver (the self-play model version; white_ver = -1) */
  int32_t game_idx_base;            /* global index of this context's game 0 in the whole job (rank x games + group offset) */
  uint64_t job_hash;                /* std::hash of ContextOptions.job_id, only used by the seed == 0 rule below */
  ElfMctsOptions mcts;
  /* the second AI of evaluation games (a request with white_ver >= 0): init_ai's overrides, game_selfplay.cc:171-181 */
  float white_puct;                         /* GameOptions.white_puct: > 0 replaces c_puct for the "actor_white" AI */
  int32_t white_mcts_rollout_per_batch;     /* GameOptions.white_mcts_rollout_per_batch: > 0 replaces num_rollouts_per_batch */
  int32_t white_mcts_rollout_per_thread;    /* GameOptions.white_mcts_rollout_per_thread: > 0 replaces num_rollouts_per_thread */
  int32_t black_use_policy_network_only;    /* GameOptions.*_use_policy_network_only: that colour's moves are MCTSAI_T::actPolicyOnly */
  int32_t white_use_policy_network_only;    /*   (elf/ai/tree_search/mcts.h:83-90, game_selfplay.cc:357-372) */
  int32_t pick_method;                      /* TSOptions.pick_method, ELFSP_PICK_* (tree_search.h:495-528) */
  int32_t cheat_eval_new_model_wins_half;   /* GameOptions.cheat_* (finish_game, game_selfplay.cc:122-129) */
  int32_t cheat_selfplay_random_result;
  int32_t following_pass;                   /* GameOptions.following_pass with a human opponent (mcts_update_info :104-111) */
  int32_t reserved1;
} ElfSpOptions;
#define ELFSP_PICK_MOST_VISITED 0
#define ELFSP_PICK_STRONGEST_PRIOR 1
#define ELFSP_PICK_UNIFORM_RANDOM 2   /* the reference draws from a process-wide mt19937 seeded with time(NULL) (tree_search_base.h:238);
                                         here one generator per context, seeded seed ^ 0x5EED, or time(NULL) for seed == 0;
                                         elfsp_set_pick_seed re-seeds it */
#define ELFSP_ACTOR_BLACK 0           /* the AI created as "actor_black" with the request's black_ver */
#define ELFSP_ACTOR_WHITE 1           /* the AI created as "actor_white" with the request's white_ver (evaluation games only) */
/* Per-game RNG seeds.  The reference seeds every GoGameBase with GameOptions.seed itself (common/game_base.h:32-38), so with a
 * non-zero seed and a deterministic net all its games are identical; its time-seeded default (seed == 0) is what production
 * runs use.  Here game g (global index i = game_idx_base + g) is seeded
 *   seed != 0:  seed + i            (the rule of this repository's reference harness, oracle/ref_selfplay.cc: distinct,
 *                                    reproducible games; i is unique over groups and ranks, so no two games of a job collide)
 *   seed == 0:  (unix_seconds*1000 + unix_milliseconds + int32(int32(i ^ job_hash) * 2341479)) % 100000000
 *                                   (elf_utils::get_seed(int), elf/utils/utils.h:50-57, as GoGameBase calls it: the game term is a
 *                                    32-bit int product that wraps; job_hash is any 64-bit hash of the job id -- the reference's
 *                                    std::hash<std::string> through the pybind boundary -- so the seeds are of the same form, and
 *                                    time-based like the reference's, never reproducible)
 * and the MCTS actor seed is the first draw of that generator (game_selfplay.cc:45-47). */

/* what GameNotifierBase::OnMCTSResult (common/notifier.h:13) sees after one search */
typedef struct ElfSpSearch {
  int32_t game, move_played, best_action, total_visits, n_edges;
  float root_value, max_score, predicted_value;
} ElfSpSearch;

int elfsp_create(const ElfSpOptions* opt, int device, const uint64_t* zobrist_host, ElfSelfPlay** out);
int elfsp_destroy(ElfSelfPlay* sp);
ElfGoEngine* elfsp_engine(ElfSelfPlay* sp);
ElfMcts* elfsp_mcts(ElfSelfPlay* sp);
/* requests that restarted SOME games with search options (TSOptions) other than the context's while other games were still playing
 * under the old ones: the tree pools belong to the whole context and are rebuilt only when no game is mid-play, so those restarted
 * games kept the context's options (the reference would build their AIs from the request's, game_selfplay.cc:166-180).  0 in every
 * flow where requests reach all games at a boundary (the reference's own server sends a request to all games of a client). */
int64_t elfsp_ts_requests_deferred(const ElfSelfPlay* sp);
/* games that play NOW under the context's search options although their request carried others (see above); their Records carry the
 * options that were used, not the request's */
int elfsp_ts_games_deferred(const ElfSelfPlay* sp);
int elfsp_max_rows(const ElfSelfPlay* sp);   /* num_games * num_threads * num_rollouts_per_batch */
/* the same bound for one of the two AIs (the "actor_white" AI may have its own batch override) */
int elfsp_max_rows_actor(const ElfSelfPlay* sp, int actor);
/* the tree pool of one AI; NULL until a request has created it (actor 1) */
ElfMcts* elfsp_mcts_actor(ElfSelfPlay* sp, int actor);
/* s_dst: device rows in the context's feature format (elfmcts_set_feature_format: fp32 [18][N][N] or fp16 [N][N][18]), rows
 * stride_elems elements apart.  n_rows != NULL: the call waits for the device and stores the number of rows that need the net.
 * n_rows == NULL: nothing is waited for inside a move -- the row count stays on the device, the net evaluates elfsp_max_rows()
 * rows (surplus rows hold stale features and are ignored) and elfsp_end_step expands exactly the counted ones; errors raised by
 * the kernels surface at the next move boundary.  Host work (Dirichlet draws, move choice, records) happens at move boundaries
 * either way. */
int elfsp_begin_step(ElfSelfPlay* sp, void* s_dst, int64_t stride_elems, int* n_rows, void* stream);
/* pi device f32 [rows][N*N+1] (rows pi_stride_floats apart), value device f32 [rows], rv device int64 [rows] or NULL (the reply's
 * model version, checked against the requested one: elfsp_set_request) */
int elfsp_end_step(ElfSelfPlay* sp, const float* pi, int64_t pi_stride_floats, const float* value, const int64_t* rv, void* stream);
/* rows of the last begin_step (synchronises the stream of that call) */
int elfsp_last_rows(ElfSelfPlay* sp, int* n_rows);
/* The same pair for games with two AIs (a request with white_ver >= 0): index ELFSP_ACTOR_BLACK / ELFSP_ACTOR_WHITE = the batch
 * group the rows belong to ("actor_black" / "actor_white", game_selfplay.cc:165-181), each evaluated by its own model.  s_dst[a]
 * may be NULL while AI a has no game searching (always true for actor 1 under a self-play request); n_rows (may be NULL) <- the
 * two row counts.  A game searches with the AI of the colour to move (player_swap exchanges the two); the AIs may need different
 * numbers of steps per move, so searches of different games are not in step.  elfsp_begin_step / elfsp_end_step are the
 * one-AI forms of these calls and refuse (ELFGO_E_BADARG) a step in which the second AI has rows. */
int elfsp_begin_step2(ElfSelfPlay* sp, void* const* s_dst, int64_t stride_elems, int* n_rows, void* stream);
int elfsp_end_step2(ElfSelfPlay* sp, const float* const* pi, int64_t pi_stride_floats, const float* const* value,
                    const int64_t* const* rv, void* stream);
int elfsp_last_rows2(ElfSelfPlay* sp, int* n_rows);
/* Client::setRequest / GameContext::setRequest (train/distri_client.h:318-331, inference/game_context.h:76-88): a MsgRequest
 * (common/record.h:119-149) for the games.  As in the reference a game looks at its mailbox at the top of every fifth act
 * (game_selfplay.cc:273-289) -- or at once while it is waiting -- and then (GoGameSelfPlay::OnReceive :222-270):
 *   black_ver < 0                      the game waits (ModelPair::wait) until a request gives it something to play;
 *   num_game_thread_used = k >= 0      games k, k+1, ... receive the request as a wait request (DispatcherCallback::OnFirstSend);
 *   new versions / new player_swap / the game was waiting:  restart from the empty board without a record, new AIs seeded with
 *                                      the next draws of the game's generator; white_ver >= 0 creates the second AI for White
 *                                      (own tree pool, ElfSpOptions.white_* overrides); player_swap exchanges the two;
 *   same versions or async             only thresholds (and with async: no version check on replies) change.
 * Restarted games stay idle until every game has received the request; then one "game_start" is due
 * (elfsp_take_game_starts) and they play.  Replies must carry the AI's version in "rv" unless async.
 * Requests queue: each is delivered to all games before the next one goes out (elf/base/dispatcher.h:104-152). */
typedef struct ElfTsOptions {         /* TSOptions + SearchAlgoOptions as they travel in a request (tree_search_options.h:23-75,77-213) */
  int32_t max_num_moves, num_threads, num_rollouts_per_thread, num_rollouts_per_batch;
  int32_t verbose, verbose_time, persistent_tree, pick_method /* ELFSP_PICK_*, -1 = a name the search does not know */;
  int64_t seed;
  float root_epsilon, root_alpha;
  int32_t virtual_loss;
  int32_t use_prior, unexplored_q_zero, root_unexplored_q_zero;
  float c_puct;
  char log_prefix[60];
} ElfTsOptions;
typedef struct ElfSpRequest {
  int64_t black_ver, white_ver;       /* ModelPair */
  float black_resign_thres, white_resign_thres, never_resign_prob;   /* ClientCtrl; the resign check uses the mean of the two */
  int32_t num_game_thread_used;       /* ClientCtrl.num_game_thread_used, -1 = all games */
  int32_t player_swap;                /* ClientCtrl.player_swap */
  int32_t async;                      /* ClientCtrl.async */
  int32_t client_type;                /* ClientCtrl.client_type as the server sent it (record.h:24-29); it only travels into the
                                         Records the games dump.  0 = unset: CLIENT_SELFPLAY_ONLY (1) */
} ElfSpRequest;
int elfsp_set_request2(ElfSelfPlay* sp, const ElfSpRequest* request);
/* The same with the TSOptions the request carries (MsgRequest.vers.mcts_opt).  In the reference the SERVER dictates the search
 * options: GoGameSelfPlay::restart builds its AIs from request.vers.mcts_opt (game_selfplay.cc:166-180), self-play requests carry the
 * server's options (train/ctrl_selfplay.h:426), evaluation requests the same with the Dirichlet noise and both *_q_zero flags
 * switched off (EvalSubCtrl, train/ctrl_eval.h:227-237), and ModelPair::operator== compares them, so a request that differs only
 * in mcts_opt restarts the games as a new model does.  Here: the games restart, wait at the barrier, and when every game has
 * received the request the tree pools are rebuilt for the new options (threads, rollouts per thread / per batch, virtual loss,
 * persistent tree, pick method, root epsilon / alpha, c_puct, use_prior, both q_zero flags); ElfSpOptions.white_* overrides still
 * apply on top for the second AI; an async request changes nothing until the next restart, as in the reference.
 * elfsp_max_rows_actor may change with it: size the row destinations for the largest request you send BEFORE the step that
 * delivers it.  mcts_opt == NULL: the context's options at creation (GameContext::setRequest, inference/game_context.h:83).
 * ELFGO_E_BADARG for options the engine cannot run (threads x rollouts per batch above elfmcts_max_rollouts_per_step, an unknown
 * pick method). */
int elfsp_set_request3(ElfSelfPlay* sp, const ElfSpRequest* request, const ElfTsOptions* mcts_opt);
/* the same with both thresholds equal, every game used, no swap */
int elfsp_set_request(ElfSelfPlay* sp, int64_t black_ver, int64_t white_ver, float resign_thres, float never_resign_prob, int async);
/* Seed of the uniform_random pick generator: MCTSResultT::addActions' `static std::mt19937 rng(time(NULL))`
 * (tree_search_base.h:238) draws random_idx = rng() % edges once per search of that method.  A context that is given the value
 * time(NULL) had in a reference process picks the edges that process picked (one game per context: the reference's game threads
 * race for the generator). */
int elfsp_set_pick_seed(ElfSelfPlay* sp, uint32_t seed);
/* host-only progress counters, no device synchronisation: out6 = {searches finished, games finished, searches open, steps,
 * games waiting for a request, games waiting at a request barrier} */
int elfsp_progress(const ElfSelfPlay* sp, int64_t* out6);
/* which AI of `game` is searching now (ELFSP_ACTOR_*), -1 = between two searches; host-only */
int elfsp_game_actor(const ElfSelfPlay* sp, int game);
/* number of times the games were (re)started by a request since the last call (each is one "game_start" batch of the reference,
 * common/dispatcher_callback.h:86-88); *black_ver / *white_ver <- the versions of the current request */
int elfsp_take_game_starts(ElfSelfPlay* sp, int64_t* black_ver, int64_t* white_ver);
/* out[12]: 0 moves played, 1 games finished, 2 rollouts, 3 net rows, 4 steps, 5 searches logged, 6 steps per move, 7 step in
 * move, 8 tree nodes descended through, 9 wall nanoseconds of move-boundary work (move choice, forward + treeAdvance, game
 * ends, Dirichlet / D4 draws up, root of the next search), 10 move boundaries, 11 wall nanoseconds the boundaries first waited
 * for the stream to drain what the host had queued ahead (pipeline depth, not boundary work).
 * Synchronises the device. */
int elfsp_stats(ElfSelfPlay* sp, int64_t* out);
/* Interactive play (the human_actor half of GoGameSelfPlay::act, game_selfplay.cc:290-330, that the GTP console
 * drives): between two searches, forward externally chosen moves (moves_host[g] = reference Coord, < 0 = none) on the game boards;
 * the trees follow.  Refused moves leave their game untouched and make the call return ELFGO_E_MCTS_BASE - ELFMCTS_E_FORWARD.
 * A move that completes two consecutive passes finishes that game (finish_game(FR_TWO_PASSES), :319-322). */
int elfsp_play(ElfSelfPlay* sp, const int32_t* moves_host, void* stream);
/* GameOptions.preload_sgf / preload_sgf_move_to (GoGameSelfPlay::restart, game_selfplay.cc:202-219): before the first search,
 * make every game follow the move list moves_host[0..n) (reference Coords): the first move_to moves are forwarded at once, then
 * each search's move is replaced by the next listed move (:392-405); the search that finds the list exhausted finishes the game
 * (FR_MAX_STEP).  An illegal listed move returns ELFGO_E_MCTS_BASE - ELFMCTS_E_FORWARD ("Preload sgf: move not valid!"). */
int elfsp_preload(ElfSelfPlay* sp, const uint16_t* moves_host, int n, int move_to, void* stream);
/* Between two searches: set the listed games up (stones_host [n][N*N], next_player_host [n] or NULL, as elfgo_setup; a game may
 * be listed once).  A game can be set up only before its first move (PlaceHandicap's rule, board.cc:110-112): ELFGO_E_BADARG
 * otherwise, or while a search is open; ELFGO_E_MCTS_BASE - ELFMCTS_E_FORWARD if a row is refused (that game is untouched, the
 * others are set up).  The trees of those games are cleared in both AIs.
 * A game that was set up finishes like any other (it is scored, elfsp_last_score / elfsp_take_finished report it, its seq
 * advances) but leaves NO Record for elfsp_pop_record: a Record has no field for set-up stones and the trainer replays it from
 * the empty board (GoStateExtOffline::fromRecord), so such a record could not be replayed. */
int elfsp_setup(ElfSelfPlay* sp, const int32_t* games_host, int n, const uint8_t* stones_host,
                const uint8_t* next_player_host, void* stream);
/* Between two searches: take back the last `count` moves of each listed game (moves of searches and of elfsp_play alike).
 * ELFGO_E_BADARG -- and nothing changes -- if count <= 0, if a game has played fewer than `count` moves since it
 * (re)started (a finished game is gone: it restarted), while a search is open, or in a context that follows a preloaded move
 * list (elfsp_preload).  The game is rebuilt on its slot from its set-up stones (or the empty board) and its first L - count
 * moves: board, history ring, super-ko records and Bloom words, ply and the pending Record arrays (moves, values, policies)
 * are those of the game after these moves; the trees of those games are cleared.  The game's random generators are NOT
 * rewound, and neither are what was drawn or derived from them and from the searches taken back: the never-resign draw of the
 * game and the last predicted value stay as they are.  Any other error (a device error while the boards are rebuilt) leaves
 * the listed games restarted from the empty board. */
int elfsp_undo(ElfSelfPlay* sp, const int32_t* games_host, int n, int count, void* stream);
/* finish_game(reason) + restart (game_selfplay.cc:121-149) for the listed games between two searches: the game is scored
 * (FR_RESIGN: the side to move loses; every other reason: GoState::evaluate(komi), go_state_ext.h:76-103), leaves its record and
 * starts over from the empty board.  reason = FinishReason of common/go_state_ext.h:24-32. */
#define ELFSP_FR_RESIGN 0
#define ELFSP_FR_TWO_PASSES 1
#define ELFSP_FR_MAX_STEP 2
#define ELFSP_FR_CLEAR 3
#define ELFSP_FR_ILLEGAL 4
int elfsp_finish(ElfSelfPlay* sp, const int32_t* games_host, int n, int reason, void* stream);
/* = elfsp_finish(..., ELFSP_FR_CLEAR, ...) (clear_board) */
int elfsp_restart(ElfSelfPlay* sp, const int32_t* games_host, int n, void* stream);
/* final values of the games finished since the last call, oldest first (what GameNotifier::OnGameEnd feeds to
 * GameStats::feedWinRate, train/distri_client.h:228-240); returns the number stored (<= cap) */
int elfsp_take_finished(ElfSelfPlay* sp, float* out_host, int cap);
/* GoGameSelfPlay::getLastScore: final value of the last finished game of every game slot, host f32 [num_games] */
int elfsp_last_score(const ElfSelfPlay* sp, float* out_host);
/* what the last finished search of every game did: out_host[g] = the Coord it forwarded on the game board (after move sampling /
 * preload substitution), 1 (M_RESIGN) if the engine resigned instead of moving, -1 if no search of that game has finished yet */
int elfsp_last_moves(const ElfSelfPlay* sp, int32_t* out_host);
/* elfmcts_analyze on the tree pool of AI `actor` (ELFSP_ACTOR_*), same outputs (device pointers); ELFGO_E_BADARG if that pool does
 * not exist (actor 1 before a request has created it).  Between two steps it shows the search in progress. */
int elfsp_analyze(ElfSelfPlay* sp, int actor, int max_moves, int max_pv, int32_t* info, int32_t* coord, int32_t* orig,
                  int32_t* visits, float* reward, float* prior, int32_t* pv_len, int32_t* pv, void* stream);
/* Analysis snapshots at the move boundary.  With max_moves, max_pv > 0 (limits as elfmcts_analyze) every search that finishes in
 * elfsp_end_step / elfsp_end_step2 leaves its analysis behind -- taken where the boundary fetches the root, before the tree is
 * re-rooted by the move -- and elfsp_last_analysis reports, per game, what the last finished search of that game saw: the
 * companion of elfsp_last_moves.  0, 0 = off (the default): the boundary launches and copies what it did without this call.
 * Every call forgets the snapshots taken so far.  ELFGO_E_BADARG for other values or while a step is open. */
int elfsp_set_analysis(ElfSelfPlay* sp, int max_moves, int max_pv);
/* host arrays, laid out as elfmcts_analyze's with the max_moves / max_pv of elfsp_set_analysis; any may be NULL.  A game whose
 * search has not finished since elfsp_set_analysis reports 0 candidates and the unused-entry values; with analysis off only info
 * is written (zeros). */
int elfsp_last_analysis(const ElfSelfPlay* sp, int32_t* info, int32_t* coord, int32_t* orig, int32_t* visits, float* reward,
                        float* prior, int32_t* pv_len, int32_t* pv);
/* Self-play records: with ElfSpOptions.keep_records > 0 every finished game leaves the Record the reference's
 * GameNotifier::OnGameEnd would send (GoStateExt::dumpRecord go_state_ext.h:131-148, Record::setJsonFields record.h:246-254),
 * as the JSON text nlohmann::json::dump() produces.  elfsp_pop_record copies the oldest pending record (NUL-terminated) into buf
 * and removes it; if cap is too small it returns ELFGO_E_BADSIZE, sets *len to the length needed (without NUL) and keeps the record.
 * *len = 0 when nothing is pending. */
int elfsp_records_pending(const ElfSelfPlay* sp);
int elfsp_pop_record(ElfSelfPlay* sp, char* buf, size_t cap, size_t* len);
/* games finished so far (host counter, no device synchronisation) */
int64_t elfsp_games_finished(const ElfSelfPlay* sp);
/* logged searches [first, first+n): records and root edges (host arrays, [n][edge_stride], may be NULL) */
int elfsp_search_log(const ElfSelfPlay* sp, int first, int n, ElfSpSearch* rec, int32_t* coord, int32_t* visits, float* prior,
                     float* reward);

/* ------------------------------------------------------------------------------------------------
 * Training-side replay loader: the trainer's input pipeline on the device.  Replaces, for a whole batch in
 * one launch, what the reference does on one std::thread per sample (2048 threads at batchsize 2048, start_server.sh:11-12):
 *   elfgames/go/train/game_train.cc        GoGameTrain::act :23-58
 *   elfgames/go/common/go_state_ext.h      GoStateExtOffline::fromRecord / switchRandomMove / switchBeforeMove :248-290
 *   elfgames/go/common/game_feature.h      the "train" extractors :73-145 (s, offline_a, winner, mcts_scores, predicted_value,
 *                                          move_idx, num_move, aug_code, selfplay_ver; schema :159-206)
 * Records live in HBM (`capacity` slots padded to `max_moves` plies; with_policies adds the 441-byte quantised MCTS policy
 * per ply, record.h:180-182).  Sample i of a batch replays in board slot i of engine `e` (capacity >= batch), so the
 * replayed GoState can be inspected with elfgo_info / elfgo_legal_mask afterwards.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ElfReplay ElfReplay;

/* A third row format, for ElfTrainBatch.s_format only: the 25 DarkForest planes (BoardFeature::extract, see elfgo_df_extract)
 * as fp32 [25][N][N] -- what the reference's "train" batch carries in "s" when GameOptions.use_df_feature is set
 * (common/game_feature.h:98-102, :159-170; the DarkForest policy nets of df_model.py train on it with offline_a
 * [num_future_actions]).  Rows need 4-byte alignment only and s_stride >= 25*N*N floats.  Info::last_placed of the replayed
 * position is rebuilt from the record's move list; the exponents of planes 10 / 11 come from elfgo_df_exp_table's values.
 * elfgo_extract_agz_fmt and elfmcts_set_feature_format refuse this value. */
#define ELFGO_FEAT_DF_F32_NCHW 2

typedef struct ElfTrainBatch {      /* device pointers, rows = samples; every pointer except s may be NULL */
  void* s;                          /* "s" in s_format, rows s_stride elements apart (>= the row's size): ELFGO_FEAT_F32_NCHW fp32
                                     * [n][18][N][N], ELFGO_FEAT_F16_NHWC fp16 [n][N][N][18] (extractStateExtAGZ), or
                                     * ELFGO_FEAT_DF_F32_NCHW fp32 [n][25][N][N] (GameOptions.use_df_feature) */
  int64_t s_stride;
  int32_t s_format;
  int32_t num_future_actions;       /* GameOptions.num_future_actions */
  int64_t* offline_a;               /* [n][num_future_actions]  coord2Action of moves[move_idx + j] */
  float* winner;                    /* [n]  +1 / -1 */
  float* mcts_scores;               /* [n][N*N+1]  normalised recorded policy, or one-hot of the played move */
  float* predicted_value;           /* [n]  Record.result.values[move_idx] */
  int32_t* move_idx;                /* [n]  GoState::getPly() - 1 after the replay */
  int32_t* num_move;                /* [n]  number of moves of the record */
  int32_t* aug_code;                /* [n]  D4 code */
  int64_t* selfplay_ver;            /* [n]  Record.request.vers.black_ver */
} ElfTrainBatch;

/* An ElfReplay is not synchronised: call put / draw / extract from one host thread at a time (the reference's reader thread and its
 * batch consumer are one pipeline here).  Device work is ordered by the streams the caller passes. */
int elftrain_create(ElfGoEngine* e, int capacity, int max_moves, int with_policies, uint32_t seed, ElfReplay** out);
int elftrain_destroy(ElfReplay* r);
int elftrain_capacity(const ElfReplay* r);
int elftrain_max_moves(const ElfReplay* r);
int elftrain_num_records(const ElfReplay* r);
/* GoStateExtOffline::fromRecord for record slot `slot`: moves_host = sgfstr2coords(Record.result.content) (see
 * elfrec_sgfstr_to_coords), reward = Record.result.reward, policies_host u8 [num_policies][(N+2)^2], values_host f32.
 * Host pointers; synchronous. */
int elftrain_put(ElfReplay* r, int slot, const uint16_t* moves_host, int num_moves, float reward, int64_t black_ver,
                 const uint8_t* policies_host, int num_policies, const float* values_host, int num_values);
/* the same, ordered on `stream` instead of the default stream: a put that reuses the slot of an evicted record cannot overtake an
 * extraction queued on that stream.  The host arrays may be reused on return. */
int elftrain_put_async(ElfReplay* r, int slot, const uint16_t* moves_host, int num_moves, float reward, int64_t black_ver,
                       const uint8_t* policies_host, int num_policies, const float* values_host, int num_values, void* stream);
/* on != 0 (the default): elftrain_extract does what switchBeforeMove does (go_state_ext.h:283-290: reset, forward x move_to) and
 * leaves the replayed GoState of sample i in board slot i of the engine (elfgo_info / elfgo_legal_mask / ... can look at it;
 * n <= elfgo_capacity).  on == 0 (the trainer's mode): a sample starts from the record's checkpoint below move_to -- the state
 * after every 16th move is written once per put, by the next extraction, together with the game's superko records -- and
 * forwards at most 15 moves; rows are identical, no board slot is written, n is not limited by the engine's capacity. */
int elftrain_set_keep_states(ElfReplay* r, int on);
/* GoGameTrain::act's draws for n samples with the store's std::mt19937 (seeded at create): record, move_to =
 * rng() % (num_moves - num_future_actions + 1), D4 code = rng() % 8; results into device int32 [n] arrays */
int elftrain_draw(ElfReplay* r, int n, int num_future_actions, int32_t* rec, int32_t* move_to, int32_t* d4, void* stream);
/* Sgf::load + its iterator (sgf/sgf.cc:28-240, sgf/sgf.h:21-46,125-245), host only: the entries of an SGF text as (player, Coord) --
 * player 1 = Black, 2 = White; Coord 0 = pass, 3 = M_INVALID (off the board, e.g. "tt" on 19x19: GoState::forward refuses it) -- with
 * the reference's reading of the format: the first node is the header (SZ, KM, HA, RE), setup stones (AB / AW) are not moves,
 * variations are not nested but follow each other, a backslash hides the next character.  Returns the number of entries (the first
 * `cap` are stored), 0 where Sgf::load returns false.  This is what GameOptions.preload_sgf and the ladder suite are read with. */
typedef struct ElfSgfHeader {
  int32_t size, handi, winner /* Stone: 1 Black, 2 White, 3 none */;
  float komi, win_margin;
} ElfSgfHeader;
int elfrec_sgf_parse(int board_size, const char* text, int32_t* players, uint16_t* coords, int cap, ElfSgfHeader* header);
/* The setup stones of an SGF text, which elfrec_sgf_parse leaves out: the AB[..][..] / AW[..][..] points of the header node as
 * a stones row for elfgo_setup (stones[a] = 0 / 1 / 2, a = x*N + y; a later property overwrites an earlier one on the same
 * point).  Same reading rules as elfrec_sgf_parse: a backslash hides the next character, points off the board are ignored.
 * A value that is not exactly one point -- a compressed list such as AB[aa:cc] (FF[4] rectangles) included -- is ignored:
 * rectangles are not expanded.
 * Returns the number of stones on the row (0: the text sets nothing up, or has no header node); `header` as elfrec_sgf_parse. */
int elfrec_sgf_setup(int board_size, const char* text, uint8_t* stones, ElfSgfHeader* header);
/* GoStateExt::dumpSgf (go_state_ext.cc:26-82): the SGF text the reference's finish_game writes for a finished game when
 * GameOptions.dump_record_prefix is set (file <prefix>_<game>_<seq>_<B|W>.sgf, go_state_ext.h:48-56): RE[] from the final value
 * ("B+R" / "W+R" for +-1, else the margin), PB / PW ("MCTS", "(policy only)" appended), KM, every move with "C[<n>: PredV: <v>]".
 * moves / values / final_value = Record.result.content (as Coords), .values, .reward.  git_hash / git_staged: the two lines of the
 * opening comment, NULL = this library's version and "0".  Returns the length; out == NULL queries it. */
int64_t elfrec_game_sgf(const ElfSpOptions* opt, const uint16_t* moves, int num_moves, const float* values, int num_values,
                        float final_value, const char* filename, const char* git_hash, const char* git_staged, char* out, size_t cap);
/* the same from the Record text of a finished game (elfsp_pop_record): *name_out <- <prefix>_<thread_id>_<seq>_<B|W>.sgf, the file
 * name GoStateExt::dumpSgf() uses (go_state_ext.h:48-56) */
int64_t elfrec_record_to_sgf(const ElfSpOptions* opt, const char* record_json, const char* prefix, char* name_out, size_t name_cap,
                             char* out, size_t cap);
/* ---- the client's wire formats (train/distri_client.h), host only --------------------------------------------------------------
 * What a self-play client sends to the reference's server: Records = {identity, states, records} (common/record.h:401-470) as
 * GuardedRecords keeps and dumps them (distri_client.h:111-170) -- and what it receives: MsgRequestSeq (record.h:152-171).  Texts
 * are byte-identical to nlohmann::json::dump() of the reference's objects, so its server parses them and its tests read them. */
typedef struct ElfThreadState {       /* ThreadState (record.h:354-380) = GoStateExt::getThreadState (go_state_ext.h:149-157) */
  int32_t thread_id, seq, move_idx, reserved;
  int64_t black, white;
} ElfThreadState;
typedef struct ElfClientRecords ElfClientRecords;
int elfrec_client_create(const char* identity, ElfClientRecords** out);
int elfrec_client_destroy(ElfClientRecords* c);
int elfrec_client_feed(ElfClientRecords* c, const char* record_json);              /* GuardedRecords::feed: one finished game */
int elfrec_client_update_state(ElfClientRecords* c, const ElfThreadState* state);  /* Records::updateState (GameNotifier::OnStateUpdate) */
int elfrec_client_size(const ElfClientRecords* c);                                  /* records waiting */
/* GuardedRecords::dumpAndClear: the message for the server.  Returns the text length; out == NULL only queries it (nothing is
 * cleared); ELFGO_E_BADSIZE when cap <= length. */
int64_t elfrec_client_dump_and_clear(ElfClientRecords* c, char* out, size_t cap);
/* the server's reply: MsgRequestSeq::createFromJson.  *mcts_opt <- the TSOptions the server dictates (GoGameSelfPlay::restart builds
 * its AIs from request.vers.mcts_opt, game_selfplay.cc:166-180: hand both to elfsp_set_request3).  ELFGO_E_BADARG
 * for malformed JSON or a missing mandatory field (the reference throws "... cannot not be found!"). */
int elfrec_parse_request_seq(const char* json_text, ElfSpRequest* request, int64_t* seq, ElfTsOptions* mcts_opt);
/* MsgRequestSeq::dumpJsonString: what the reference's server writes for this request */
int64_t elfrec_request_seq_to_json(const ElfSpRequest* request, const ElfTsOptions* mcts_opt, int64_t seq, char* out, size_t cap);
/* GoStateExt::getThreadState of every game of a self-play context (thread_id = the job-wide game index, seq, move_idx = ply - 1,
 * black / white = the versions of the game's current request): what GameNotifier::OnStateUpdate reports at every fifth act */
int elfsp_thread_states(const ElfSelfPlay* sp, ElfThreadState* out, int capacity);
/* The trainer's replay buffer and GoGameTrain::act's draws, host only: elf::shared::ReaderQueuesT<Record>
 * (elf/distributed/shared_reader.h:165-340) -- num_reader (even) queues, each a deque bounded by queue_max_size, filled as
 * TrainCtrl::OnReceive does with InsertWithParity(record, rng, reward > 0) (train/game_ctrl.h:306-311): games Black won go to the odd
 * queues, the others to the even ones -- and the draws of GoGameTrain::act (train/game_train.cc:23-58) over it.  A record is a
 * handle: the slot of an ElfReplay store the caller keeps the record in.  insert_seed seeds TrainCtrl's generator (0 = time(NULL),
 * the reference's rule). */
typedef struct ElfReaderQueues ElfReaderQueues;
int elfrq_create(int num_reader, int queue_min_size, int queue_max_size, uint32_t insert_seed, ElfReaderQueues** out);
int elfrq_destroy(ElfReaderQueues* q);
/* InsertWithParity: queue 2 * (rng() % (num_reader / 2)) + black_win, push_back, the queue's oldest record dropped when it holds
 * more than queue_max_size (*evicted <- its handle, -1 = none: the caller may reuse that slot).  Returns the queue index. */
int elfrq_insert(ElfReaderQueues* q, int32_t slot, int32_t num_moves, int black_win, int32_t* evicted);
int elfrq_sizes(const ElfReaderQueues* q, int32_t* per_queue);
/* one std::mt19937 per GoGameTrain game thread (GoGameBase, common/game_base.h:32-38): seed != 0 -> thread t gets seed + t (the
 * reference gives all of them `seed`: identical streams); seed == 0 -> elf_utils::get_seed(t ^ job_hash), time-based */
int elfrq_set_threads(ElfReaderQueues* q, int num_threads, int64_t seed, uint64_t job_hash);
/* num_acts acts of GoGameTrain::act, the threads taking turns, 64 states each (kNumState): getSamplerWithParity (queue pair
 * rng() % (nq / 2), the odd queue if uniform_real(0, 1) > even_ratio clamped to [0.45, 0.55]: Black's and White's wins are drawn
 * about equally often), Sampler::sample (rng() % queue size), switchRandomMove (a record shorter than num_future_actions is drawn
 * again; move_to = rng() % (num_moves - num_future_actions + 1)), generateD4Code (rng() % 8).  Host int32 arrays of num_acts * 64:
 * feed them to elftrain_extract.  ELFGO_E_BADARG while a queue holds fewer than queue_min_size records (the reference waits). */
int elfrq_draw(ElfReaderQueues* q, int num_acts, int num_future_actions, int32_t* slot, int32_t* move_to, int32_t* d4);
/* one launch: replay record rec[i] up to move_to[i] (switchBeforeMove), then every extractor of the "train" batch under
 * D4 code d4[i] (NULL = 0).  rec/move_to/d4 device int32 [n].  n <= elfgo_capacity(e) only while keep_states is on (sample i
 * replays in board slot i); with keep_states off n is not limited by the engine.  A move_to beyond the record is taken as its
 * number of moves: the row of the fully replayed game (offline_a 0, mcts_scores 0, predicted_value 0 when no move was refused). */
int elftrain_extract(ElfReplay* r, const int32_t* rec, const int32_t* move_to, const int32_t* d4, int n, const ElfTrainBatch* out,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Record format helpers (host only, no GPU needed): the SGF move string of Record.result.content and the quantised policy.
 * ------------------------------------------------------------------------------------------------ */
/* coords2sgfstr (sgf/sgf.h:87-95): "(;B[xy];W[xy]...)". Returns the length (without NUL); out may be NULL to query it;
 * ELFGO_E_BADSIZE if cap is too small. */
int elfrec_coords_to_sgfstr(int board_size, const uint16_t* coords, int n, char* out, size_t cap);
/* sgfstr2coords + str2coord (sgf/sgf.h:21-46,97-125): returns the number of moves in the string, stores the first `cap` */
int elfrec_sgfstr_to_coords(int board_size, const char* sgf, uint16_t* out, int cap);
/* Record (record.h:236-262) of one finished self-play game as JSON text, from plain host arrays -- the formatting half of
 * elfsp_pop_record on its own (policies u8 [num_policies][(N+2)^2]).  Returns the length (without NUL); out may be NULL. */
int elfrec_record_to_json(const ElfSpOptions* opt, const uint16_t* moves, int num_moves, const uint8_t* policies, int num_policies,
                          const float* values, int num_values, float reward, int never_resign, int seq, uint64_t thread_id,
                          uint64_t timestamp, char* out, size_t cap);
/* the same under an explicit MsgRequest (evaluation games: white_ver, player_swap, the request's thresholds and thread count);
 * request == NULL: the self-play request of the options, as above */
int elfrec_record_to_json2(const ElfSpOptions* opt, const ElfSpRequest* request, const uint16_t* moves, int num_moves,
                           const uint8_t* policies, int num_policies, const float* values, int num_values, float reward, int never_resign,
                           int seq, uint64_t thread_id, uint64_t timestamp, char* out, size_t cap);
/* GoStateExt::addMCTSPolicy (go_state_ext.h:158-181): out[(N+2)^2] = (unsigned char)(prob / max(prob) * 255) at each coord */
int elfrec_quantise_policy(int board_size, const int32_t* coord, const float* prob, int n, uint8_t* out);

/* ------------------------------------------------------------------------------------------------
 * Glue for the PyTorch-ROCm policy/value net (the net itself stays on PyTorch, BASELINE.json north_star): the
 * convolution's epilogue as ONE pass over the fp16 channels_last activation instead of PyTorch's separate
 * bias-add, residual-add and ReLU kernels (src_py/elfgames/go/df_model3.py:62-110 Block.forward:
 * relu(bn(conv(x))) and relu(bn(conv(h)) + x) with eval BatchNorm folded into the conv).
 *   x[r][c] <- act(x[r][c] + bias[c] + (res ? res[r][c] : 0)),  x/res fp16 [rows][channels] contiguous
 *   (channels % 8 == 0, 16-B aligned), bias fp16 [channels] or NULL, relu != 0 applies max(.,0).
 * fp32 arithmetic in the order (x + bias) + res, one rounding to fp16 (to nearest even); a sum beyond the largest finite value
 * saturates to Inf, subnormals are kept.  The max is fmaxf: a NaN before the ReLU comes out as +0 (torch.relu would keep it), and
 * -0 as a zero that compares equal to 0 (fmaxf does not promise its sign); without the ReLU NaN, Inf and -0 pass through. */
int elfnet_bias_act_f16(void* x, const void* bias, const void* res, int64_t rows, int channels, int relu, void* stream);
/* the same pass for a bfloat16 activation (round to nearest even) */
int elfnet_bias_act_bf16(void* x, const void* bias, const void* res, int64_t rows, int channels, int relu, void* stream);
/* The trunk convolution with that epilogue inside it (elf_amd/csrc/net_conv.hip, net_conv3x3.hip): one kernel, no second pass over y.
 * y = relu?(conv3x3_same(x, w) + bias (+ res)), fp16 NHWC in, fp16 NHWC out, fp32 accumulation.
 *   x [rows,H,W,C], w [K,3,3,C] (a channels_last torch weight as it lies in memory), bias [K], res/y [rows,H,W,K];
 *   res may be NULL; y must not alias x or res.  algo: 0 = Composable Kernel's implicit GEMM with the tile configuration
 *   MIOpen's tuned database picks for the 2048 x 19 x 19 x 256 trunk shape, 1 = the hand-written 256 x 256 x 64 LDS-DMA kernel, which
 *   takes c % 64 == 0, k % 256 == 0 and (2 W + 3) * c * 2 < 2^30 only (elfnet_conv3x3_f16_bufstage), keeps algo 0's accumulation order (the same output bits) and is the faster one from
 *   about 33 000 positions (rows * H * W) on.
 *   Algo 1 has two row orders with the same output bits for finite operands.  Linear: a work item is 256 consecutive positions
 *   (n, h, w) and runs all nine taps, an off-board tap as a multiplication by zeros.  Board: a work item is one board position
 *   (h, w) of 256 consecutive boards and runs only the taps that are on the board there (4 in a corner, 6 on an edge, 9 inside);
 *   its items are dealt longest first, the last round to the least loaded workgroups.  This entry takes board order iff
 *   rows >= 256 and board order's most loaded workgroup has strictly fewer K tiles (one tap x 64 input channels of one item) than
 *   the linear order's at the device's CU count (elfnet_conv3x3_f16_order says which); otherwise linear.
 *   The one difference: in linear order a non-finite weight at a tap that is off the board for a position still reaches that
 *   position (0 x Inf = NaN, as in algo 0); in board order it does not, that tap is never multiplied.
 * Rounding: the fp32 accumulator is rounded to fp16 (as a convolution that stores y does), then bias, res and the ReLU are applied
 * in fp32 in elfnet_bias_act_f16's order and the result is rounded once more: conv + elfnet_bias_act_f16, without the round trip.
 * Both roundings saturate to Inf (an accumulator beyond 65 504 is Inf before the bias is added), and the ReLU is that pass's fmaxf:
 * a NaN before it comes out as +0, and -0 as a zero of either sign; without the ReLU they pass through.
 * ELFGO_E_BADARG -- and nothing is launched -- for a null x / w / bias / y, pointers that are not 16-B aligned, c % 8 or k % 8 != 0,
 * y == x or y == res, an unknown algo, a tensor of 2^31 bytes or more, or a shape the chosen kernel does not take.
 * Runs on the device that owns x; allocates nothing and waits for nothing (it can be captured into a HIP graph). */
int elfnet_conv3x3_f16(const void* x, const void* w, const void* bias, const void* res, void* y,
                       int64_t rows, int h, int wd, int c, int k, int relu, int algo, void* stream);
/* elfnet_conv3x3_f16 with the round width of algo 1 named: how many of its work items (tiles of 256 positions x columns of 256
 * output channels) the device runs at a time.  Algo 1 runs the work items of a last round that is at most half full as two
 * work ids of 256 positions x 128 channels each, so that round takes a half tile's time: with total = tiles * (k / 256) and
 * r = total % round_width, iff total >= round_width and 0 < 2 r <= round_width.  The launch is min(round_width, work ids)
 * workgroups, each running every round_width-th id one after the other.  The output bits are the same whatever the width.
 * round_width 0 = the device's CU count (one workgroup per CU), which is what elfnet_conv3x3_f16 passes; a value above total never
 * splits and gives every work id a workgroup of its own; a negative one is ELFGO_E_BADARG.  Algo 0 ignores it.  For tests and
 * probes of the split and of the chains at sizes of a few tiles. */
int elfnet_conv3x3_f16_width(const void* x, const void* w, const void* bias, const void* res, void* y,
                             int64_t rows, int h, int wd, int c, int k, int relu, int algo, int round_width, void* stream);
/* Algo 1 in board order, at any rows and round width (elfnet_conv3x3_f16 chooses; a round_width above 0 through
 * elfnet_conv3x3_f16_width is always the linear order).  With B = ceil(rows / 256) the launch has H W * B * (k / 256) work ids and
 * min(round_width, ids) workgroups; round_width 0 = the device's CU count.  Refuses what algo 1 refuses, and a 1 x 1 board at
 * c == 64 (an item of a single K tile).  For tests and probes. */
int elfnet_conv3x3_f16_boards(const void* x, const void* w, const void* bias, const void* res, void* y,
                              int64_t rows, int h, int wd, int c, int k, int relu, int round_width, void* stream);
/* Host arithmetic: the work ids of that launch for round_width > 0, or ELFGO_E_BADARG.  With 0 <= id it also says what work id
 * `id` computes (any of the pointers may be NULL): its block of 256 boards, its board position h * W + w, its channel column and
 * its tap mask, bit 3 ky + kx set iff (h + ky - 1, w + kx - 1) is on the board.  id = (rank * columns + column) * B + block, where
 * rank lists the inner positions, then the edges, then the corners, each row-major (H or W below 3: rank = position). */
int64_t elfnet_conv3x3_f16_boards_plan(int64_t rows, int h, int wd, int k, int round_width, int64_t id,
                                       int* block, int* position, int* column, int* mask);
/* Host arithmetic: the deal of that launch.  g < 0: its workgroups G.  Otherwise the work id workgroup g runs as its j-th item
 * (j from 0), or -1 where it has fewer: g + j G in the full rounds, and the last, partial round is dealt from workgroup G - 1
 * downwards. */
int64_t elfnet_conv3x3_f16_boards_deal(int64_t rows, int h, int wd, int k, int round_width, int g, int j);
/* Host arithmetic: the K tiles workgroup g of that launch runs through at c input channels: popcount(mask) * c / 64, summed
 * over its items. */
int64_t elfnet_conv3x3_f16_boards_load(int64_t rows, int h, int wd, int c, int k, int round_width, int g);
/* The row order elfnet_conv3x3_f16(algo 1) takes for a shape: 0 linear, 1 board (the rule above; the linear order's most loaded
 * workgroup is its full rounds x 9 c / 64 K tiles plus 9 c / 64 for an unsplit last round or 3/4 of that for a split one).
 * round_width 0: at the current device's CU count; above 0: host arithmetic at that width. */
int elfnet_conv3x3_f16_order(int64_t rows, int h, int wd, int c, int k, int round_width);
/* Host arithmetic: the work ids of the launch elfnet_conv3x3_f16_width(algo 1) makes for tiles x columns work items and
 * round_width > 0.  Returns the number of work ids (tiles * columns when the last round is not split, one more per split item),
 * or ELFGO_E_BADARG.  With any of tile / column / half non-NULL it also says what work id `id` computes: its tile, its column,
 * and half = -1 for all 256 channels of the column or 0 / 1 for the lower / upper 128.  A work id is not a workgroup: see _grid. */
int64_t elfnet_conv3x3_f16_plan(int64_t tiles, int columns, int round_width, int64_t id, int* tile, int* column, int* half);
/* Host arithmetic: the workgroups G of that launch, min(round_width, work ids), or ELFGO_E_BADARG for what _plan refuses.
 * Workgroup g runs the work ids g, g + G, g + 2 G, ... in ascending order; a half id is the last one of its workgroup. */
int64_t elfnet_conv3x3_f16_grid(int64_t tiles, int columns, int round_width);
/* Host arithmetic: the multiplier and shift algo 1's kernel divides a position by `divisor` with (its launch's H * W and W):
 * for every 0 <= n < 2^31, n / divisor == (((n + 1) * mul) >> 32) >> shift, the product taken in 64 bits.  1 <= divisor <= 2^31,
 * otherwise (or with a NULL out pointer) ELFGO_E_BADARG; 0 on success. */
int elfnet_conv3x3_f16_recip(int64_t divisor, uint32_t* mul, uint32_t* shift);
/* Host arithmetic: what algo 1's kernel addresses x and w by when it stages a K tile.  It reads both through raw buffer descriptors
 * (stride 0): a lane's 32-bit byte offset in a vector register plus a wave-uniform scalar offset, both unsigned.  x's descriptor
 * starts *bias = (wd + 1) * c * 2 bytes in front of x, so that the scalar offset of a tap above or left of a position is not
 * negative.  *x_records and *w_records are the descriptors' sizes in bytes (x's: the tensor plus bias), *sentinel is the vector
 * offset of a lane that stages zeros (a row at or beyond its item's limit, an off-board tap in linear order): it is at or above
 * both sizes for every shape the launch takes, a multiple of 16 and the same for every shape.  With 0 <= tap < 9 (3 ky + kx) and
 * 0 <= kc < c / 64, *x_soff and *w_soff are the scalar offsets of that tap's channels 64 kc .. 64 kc + 63; tap < 0: the shape's
 * four values alone.  The vector offset of chunk q (16 bytes, 8 channels) of position p is p * c * 2 + 16 q, and
 * that + *x_soff - *bias is the byte offset in x of the same chunk of the tap's neighbour; a weight row n starts at n * 9 * c * 2.
 * No sum of a vector offset (the sentinel included) and a scalar offset reaches 2^32.  Any out pointer may be NULL.
 * ELFGO_E_BADARG for what the launch refuses: rows, h, wd, c, k not positive, c no multiple of 64, k none of 256, a tensor of 2^30
 * elements or more, and a board so wide that (2 wd + 3) * c * 2 >= 2^30 (which this kernel refuses too); tap >= 9 or kc out of
 * range. */
int elfnet_conv3x3_f16_bufstage(int64_t rows, int h, int wd, int c, int k, int tap, int kc, uint32_t* bias, uint32_t* x_records,
                                uint32_t* w_records, uint32_t* sentinel, uint32_t* x_soff, uint32_t* w_soff);
/* One staged piece of one wave of that kernel, for the test of what the hardware does with a lane that is out of range: 1 KiB of
 * LDS at byte lds_offset (a multiple of 1024, at most 159 KiB) is filled with 0xFF, lane l of 64 stages 16 bytes from
 * voffset[l] + soffset through a raw buffer descriptor of `records` bytes at src, and the KiB is copied to out.  src (16-byte
 * aligned), voffset (64 x uint32_t) and out (1 KiB) are device memory on the current device; every 16 bytes at
 * voffset[l] + soffset that end at or below `records` must lie inside src's allocation.  One launch on `stream`. */
int elfnet_conv3x3_f16_bufstage_probe(const void* src, uint32_t records, const void* voffset, uint32_t soffset, uint32_t lds_offset,
                                      void* out, void* stream);
/* The same function as elfnet_conv3x3_f16 -- same tensors, same roundings, algo 0's accumulation order and therefore its output
 * bits -- on a third main loop, for calls of a few thousand positions (a single game's 16-row net call is 5 776): tiles of
 * 64 positions x 64 output channels, one plain launch of ceil(rows * h * wd / 64) x (k / 64) workgroups, so that such a call
 * fills the chip where algo 0 and algo 1 give it 46 or 23 workgroups (elf_amd/csrc/net_conv3x3_small.hip).  An entry of its own:
 * elfnet_conv3x3_f16 has algos 0 and 1 and refuses any other.
 * ELFGO_E_BADARG -- and nothing is launched, y keeps its bytes -- for what elfnet_conv3x3_f16 refuses (a null x / w / bias / y,
 * pointers that are not 16-B aligned, y == x or y == res, a tensor of 2^31 bytes or more, a pointer that is no device pointer)
 * and for c % 64 != 0 or k % 64 != 0.  rows == 0 returns 0 and launches nothing.
 * Runs on the device that owns x; no workspace, allocates nothing and waits for nothing (it can be captured into a HIP graph). */
int elfnet_conv3x3_small_f16(const void* x, const void* w, const void* bias, const void* res, void* y,
                             int64_t rows, int h, int wd, int c, int k, int relu, void* stream);

/* The two ends of the fp16 net on this library's kernels (elf_amd/csrc/net_io.hip).  A C host evaluates a BN-folded net as
 *   elfnet_conv3x3_in_f16 (feature rows -> trunk activation), elfnet_conv3x3_f16 twice per residual block, elfnet_heads_f16
 * with no other library in between: no find step, no solver choice, the same bits on every call.
 *
 * The input convolution: y = relu?(conv3x3_same(x, w) + bias), fp32 accumulation over the flattened (tap, channel) axis.
 *   x fp16 [rows,H,W,C] -- for C = 18 exactly the rows ELFGO_FEAT_F16_NHWC writes (36 B per position; x needs 4-B alignment only),
 *   w fp16 [K,3,3,C] (a channels_last torch weight as it lies in memory), bias fp16 [K], y fp16 [rows,H,W,K].
 *   C even, 2 .. 32; K a multiple of 32.
 * Rounding as elfnet_conv3x3_f16: the accumulator is rounded to fp16, bias and the ReLU (fmaxf) are applied in fp32, and the result
 * is rounded once more.
 * ELFGO_E_BADARG -- and nothing is launched -- for a null pointer, another c or k, y == x, a tensor of 2^31 bytes or more, or w /
 * bias / y that are not 16-B aligned.  Runs on the device that owns x; allocates nothing and waits for nothing. */
int elfnet_conv3x3_in_f16(const void* x, const void* w, const void* bias, void* y,
                          int64_t rows, int h, int wd, int c, int k, int relu, void* stream);

/* Both heads from the trunk activation act fp16 [rows,H,W,C], with d = H * W:
 *   p[c][pos]  = relu(sum_i act[pos][i] * pconv_w[c][i] + pconv_b[c])         c = 0, 1
 *   logits[j]  = sum_f pi_w[j][f] * p_flat[f] + pi_b[j],  p_flat[c * d + pos] = p[c][pos]   (torch's flattening of [B,2,H,W])
 *   pi         = softmax(logits)                                               d + 1 entries
 *   v0[pos]    = relu(sum_i act[pos][i] * vconv_w[i] + vconv_b)
 *   v1         = relu(v1_w v0 + v1_b),   V = tanh(v2_w v1 + v2_b)
 * The weights are fp16 as the folded modules hold them; ALL arithmetic is fp32 and nothing in between is rounded to fp16 (the eager
 * net rounds after every op: this result differs from it by rounding only, and has fewer roundings).  pi, logits and value are fp32:
 * what elfmcts_expand / elfsp_end_step take.  pi (and logits, if not NULL) rows are pi_stride floats apart; value is [rows].
 * act is read once; the per-position head values go through `workspace` (elfnet_heads_workspace(rows, h, wd) bytes of device memory,
 * > 0 and monotone in rows), which the call leaves in an unspecified state.  Two launches on `stream`, no atomics: repeated
 * calls return the same bits, and a row's bits do not depend on the number of rows in the call.
 * Non-finite input: the three ReLUs of the head convolutions are fmaxf(sum + bias, 0), as the trunk's.  A NaN in act makes the three
 * sums of its position NaN and therefore p[0][pos] = p[1][pos] = v0[pos] = 0: the row's pi and V are FINITE, those of the same
 * weights with that position's head-convolution outputs at 0 -- a diverged trunk does not show as NaN here.  +Inf in act on a
 * channel with a positive pconv_w makes p[c][pos] +Inf, the row's logits +Inf, -Inf or NaN (0 x Inf) by pi_w's column and every
 * entry of the row's pi NaN, as torch.softmax of a row with an infinite logit is.  In both cases every other row is untouched.
 * ELFGO_E_BADARG -- and nothing is launched -- for a null act / hd / pi / value / workspace or a null weight pointer, channels % 8
 * != 0, value_hidden <= 0, workspace_bytes below rows * 3 * d * 4 (elfnet_heads_workspace's value, which is rounded up, always
 * suffices), pi_stride < d + 1, act or the head-convolution weights not 16-B aligned, pi_w / pi / value / logits / workspace not
 * 4-B aligned (the other weights need their 2 B only); and for a shape beyond the kernels' ranges: a row that does not fit the
 * 64 KiB of LDS of a workgroup, (4 d + 1 + value_hidden) * 4 > 65 536 (a 64 x 64 board with 256 value neurons; 63 x 63 fits),
 * rows * d >= 2^31, d > 2^20 or value_hidden > 2^20.  Allocates nothing and waits for nothing. */
typedef struct ElfNetHeads {            /* fp16 device pointers */
  const void *pconv_w, *pconv_b;        /* [2][C], [2]        pi_final_conv    */
  const void *vconv_w, *vconv_b;        /* [1][C], [1]        value_final_conv */
  const void *pi_w, *pi_b;              /* [d+1][2d], [d+1]   pi_linear        */
  const void *v1_w, *v1_b;              /* [vh][d], [vh]      value_linear1    */
  const void *v2_w, *v2_b;              /* [1][vh], [1]       value_linear2    */
  int32_t channels, value_hidden;       /* C, vh */
} ElfNetHeads;
size_t elfnet_heads_workspace(int64_t rows, int h, int wd);
int elfnet_heads_f16(const void* act, const ElfNetHeads* hd, int64_t rows, int h, int wd,
                     float* pi, int64_t pi_stride, float* value, float* logits,
                     void* workspace, size_t workspace_bytes, void* stream);

/* convenience for callers without a HIP runtime of their own (tests, the pybind11/cgo/ctypes side); these act on the calling
 * thread's current device unless a device is named */
int elfgo_set_device(int device);
int elfgo_get_device(int* device);
/* free / total HBM of a device in bytes (hipMemGetInfo): what a caller sizes num_games x nodes_per_game against --
 * elfmcts_tree_bytes_per_game() per game and AI */
int elfgo_mem_info(int device, size_t* free_bytes, size_t* total_bytes);
/* what kind of memory a caller-provided address is: 0 = pageable host (or unknown), 1 = page-locked (pinned) host, 2 = device;
 * *device (may be NULL) <- the owning device for kind 2 */
int elfgo_pointer_kind(const void* p, int* device);
/* 2-D copy between any two of {device, pinned host, pageable host} (hipMemcpyDefault), `rows` rows of width_bytes, row pitches
 * in bytes; asynchronous on `stream` when the host side is pinned */
int elfgo_memcpy2d_async(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width_bytes, size_t rows, void* stream);
int elfgo_stream_sync(void* stream);
int elfgo_malloc(void** dptr, size_t bytes);
int elfgo_free(void* dptr);
int elfgo_memcpy_h2d(void* dst, const void* src_host, size_t bytes);
int elfgo_memcpy_d2h(void* dst_host, const void* src, size_t bytes);
const char* elfgo_error_string(int status);
const char* elfgo_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ELF_AMD_H_ */
