// Host-side self-play record assembly shared by record_host.cpp (formatting) and selfplay_host.hip (capture).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/elf_amd.h"

// The host's one form of the reference's MsgRequest (common/record.h:119-149): ModelPair (versions + the TSOptions it carries) and
// ClientCtrl as the public structs hold them, plus the dispatcher's sequence number.  Built only by elfrec_request (a caller's
// request) and elfrec_request_of_options (the request of a context's options): flags are 0/1 and log_prefix is zero after its
// end, so the comparisons below are plain field comparisons.
struct SpRequest {
  ElfSpRequest q{-1, -1, 0.f, 0.f, 0.f, -1, 0, 0, 1};   // a game before its first request: waiting, CLIENT_SELFPLAY_ONLY
  ElfTsOptions ts{};                                     // ModelPair.mcts_opt: the search options the AIs of this request are built with
  int id = 0;                                            // 0: no request yet
  bool wait() const { return q.black_ver < 0; }                                   // ModelPair::wait
  bool is_selfplay() const { return q.black_ver >= 0 && q.white_ver == -1; }      // ModelPair::is_selfplay
  void set_wait() { q.black_ver = q.white_ver = -1; }
  bool same_model_pair(const SpRequest& o) const;        // ModelPair::operator== incl. TSOptions::operator== (tree_search_options.h:133-180)
};
bool operator==(const SpRequest& a, const SpRequest& b);   // MsgRequest: ModelPair and ClientCtrl, not the id

// The one way a caller's request comes in.  Always: every bool the reference carries becomes 0/1, log_prefix ends at its first NUL
// (or fills its 60 bytes) with zeros after it.  Per caller:
enum {
  SPREQ_AS_GIVEN = 0,
  SPREQ_DEFAULT_CLIENT_TYPE = 1,   // client_type 0 (unset) -> CLIENT_SELFPLAY_ONLY
  SPREQ_WAIT_VERSIONS = 2,         // black_ver < 0 -> both versions -1 (a wait request), white_ver < 0 -> -1
};
SpRequest elfrec_request(const ElfSpRequest& q, const ElfTsOptions& ts, int rules);
// the MsgRequest a self-play context with these options works under until it is sent one (Client::setRequest,
// train/distri_client.h:318-331): self-play with model_ver, every game used, the options' own TSOptions
SpRequest elfrec_request_of_options(const ElfSpOptions& o);

// The twelve fields of a request's TSOptions that the tree pools are built from, each next to the field of ElfSpOptions it lives in
// (`flag`: a bool of the reference, any non-zero value is true).  max_num_moves, seed, verbose*, log_prefix take part in
// ModelPair::operator== (SpRequest::same_model_pair) but never in the shape of a pool.
template <class T, class O, class F>   // ElfTsOptions, ElfSpOptions, either of them const or not
static void sp_ts_fields(T& t, O& o, F f) {
  f(t.num_threads, o.mcts.num_threads, false); f(t.num_rollouts_per_thread, o.num_rollouts_per_thread, false);
  f(t.num_rollouts_per_batch, o.mcts.num_rollouts_per_batch, false); f(t.persistent_tree, o.persistent_tree, true);
  f(t.pick_method, o.pick_method, false); f(t.root_epsilon, o.root_epsilon, false); f(t.root_alpha, o.root_alpha, false);
  f(t.virtual_loss, o.mcts.virtual_loss, false); f(t.use_prior, o.mcts.use_prior, true); f(t.c_puct, o.mcts.c_puct, false);
  f(t.unexplored_q_zero, o.mcts.unexplored_q_zero, true); f(t.root_unexplored_q_zero, o.mcts.root_unexplored_q_zero, true);
}
// TSOptions <- the fields of ElfSpOptions they live in
static inline void sp_ts_from(ElfTsOptions* t, const ElfSpOptions& o) {
  sp_ts_fields(*t, o, [](auto& tf, const auto& of, bool flag) { tf = flag ? of != 0 : of; });
}

struct SpRecord {              // the MsgResult half (record.h:184-234) + Record's own fields (:236-262)
  std::vector<uint16_t> moves;            // GoState::getAllMoves()
  std::vector<uint8_t> policies;          // [num_policies][(N+2)^2] CoordRecord.prob
  std::vector<float> values;              // predicted values, one per search
  float reward = 0.0f;
  bool never_resign = false;
  int num_move = 0;
  uint64_t timestamp = 0, thread_id = 0;
  int seq = 0;
  std::vector<int64_t> using_models;      // GoStateExt::using_models_ (a std::set: ascending, unique); empty = the request's versions
};

// Record::setJsonFields + nlohmann::json::dump() (compact, keys in std::map order); `req` = Record.request
std::string elfrec_record_json(int board_size, const SpRequest& req, const SpRecord& r);
// GoStateExt::addMCTSPolicy (go_state_ext.h:158-181): appends one (N+2)^2-byte row to `policies`
void elfrec_append_policy(int board_size, const int32_t* coord, const float* prob, int n, std::vector<uint8_t>* policies);
