// Search analysis of a self-play context (include/elf_amd.h: elfsp_analyze, elfsp_set_analysis, elfsp_last_analysis) over
// elfmcts_analyze.  Included by selfplay_host.hip, after its ElfSelfPlay, and by nothing else.
#pragma once

// the values elfmcts_analyze leaves in entries it does not use
static void sp_analysis_blank(ElfSelfPlay* sp) {
  const size_t G = sp->G, GM = G * sp->an_moves;
  sp->la_info.assign(G * ELFMCTS_ANALYZE_WORDS, 0);
  sp->la_coord.assign(GM, -1); sp->la_orig.assign(GM, -1); sp->la_visits.assign(GM, 0); sp->la_pvlen.assign(GM, 0);
  sp->la_reward.assign(GM, 0.0f); sp->la_prior.assign(GM, 0.0f);
  sp->la_pvs.assign(GM * sp->an_pv, -1);
}

static void sp_analysis_release(ElfSelfPlay* sp) {
  sp->an_info.release(); sp->an_coord.release(); sp->an_orig.release(); sp->an_visits.release(); sp->an_pvlen.release();
  sp->an_pvs.release(); sp->an_reward.release(); sp->an_prior.release();
}

// behind elfmcts_root on the boundary's stream: the analysis of every tree of pool a and its way back to the mirrors (the
// boundary's own wait follows)
static int sp_analysis_queue(ElfSelfPlay* sp, int a) {
  const size_t G = sp->G, GM = G * sp->an_moves;
  SPCHK(elfmcts_analyze(sp->pool[a].mcts, sp->an_moves, sp->an_pv, sp->an_info.d, sp->an_coord.d, sp->an_orig.d, sp->an_visits.d,
                        sp->an_reward.d, sp->an_prior.d, sp->an_pvlen.d, sp->an_pvs.d, sp->stream));
  HIPCHK(sp->an_info.down(G * ELFMCTS_ANALYZE_WORDS, sp->stream));
  HIPCHK(sp->an_coord.down(GM, sp->stream));
  HIPCHK(sp->an_orig.down(GM, sp->stream));
  HIPCHK(sp->an_visits.down(GM, sp->stream));
  HIPCHK(sp->an_reward.down(GM, sp->stream));
  HIPCHK(sp->an_prior.down(GM, sp->stream));
  HIPCHK(sp->an_pvlen.down(GM, sp->stream));
  HIPCHK(sp->an_pvs.down(GM * sp->an_pv, sp->stream));
  return 0;
}

// only the games whose search has just finished: the other trees of the pool are in the middle of theirs
static void sp_analysis_keep(ElfSelfPlay* sp, const std::vector<int32_t>& games) {
  const size_t M = sp->an_moves, P = sp->an_pv;
  for (int g : games) {
    std::copy_n(&sp->an_info.h[g * ELFMCTS_ANALYZE_WORDS], ELFMCTS_ANALYZE_WORDS, &sp->la_info[g * ELFMCTS_ANALYZE_WORDS]);
    std::copy_n(&sp->an_coord.h[g * M], M, &sp->la_coord[g * M]);
    std::copy_n(&sp->an_orig.h[g * M], M, &sp->la_orig[g * M]);
    std::copy_n(&sp->an_visits.h[g * M], M, &sp->la_visits[g * M]);
    std::copy_n(&sp->an_reward.h[g * M], M, &sp->la_reward[g * M]);
    std::copy_n(&sp->an_prior.h[g * M], M, &sp->la_prior[g * M]);
    std::copy_n(&sp->an_pvlen.h[g * M], M, &sp->la_pvlen[g * M]);
    std::copy_n(&sp->an_pvs.h[g * M * P], M * P, &sp->la_pvs[g * M * P]);
  }
}

extern "C" {

int elfsp_analyze(ElfSelfPlay* sp, int actor, int max_moves, int max_pv, int32_t* info, int32_t* coord, int32_t* orig,
                  int32_t* visits, float* reward, float* prior, int32_t* pv_len, int32_t* pv, void* stream) {
  if (!sp || actor < 0 || actor > 1 || !sp->pool[actor].mcts) return ELFGO_E_BADARG;
  return elfmcts_analyze(sp->pool[actor].mcts, max_moves, max_pv, info, coord, orig, visits, reward, prior, pv_len, pv, stream);
}

int elfsp_set_analysis(ElfSelfPlay* sp, int max_moves, int max_pv) {
  if (!sp || sp->step_open) return ELFGO_E_BADARG;
  const bool off = max_moves == 0 && max_pv == 0;
  if (!off && (max_moves < 1 || max_moves > ELFMCTS_ANALYZE_MAX_MOVES || max_pv < 1 || max_pv > ELFMCTS_ANALYZE_MAX_PV))
    return ELFGO_E_BADARG;
  DevGuard _dg(sp->eng->device);
  if (sp->an_moves > 0) HIPCHK(hipDeviceSynchronize());   // no copy into the mirrors is pending between two steps; the arrays go
  sp_analysis_release(sp);
  sp->an_moves = max_moves; sp->an_pv = max_pv;
  sp_analysis_blank(sp);
  if (off) return 0;
  const size_t G = sp->G, GM = G * max_moves;
  hipError_t e = sp->an_info.alloc(G * ELFMCTS_ANALYZE_WORDS);
  (e || (e = sp->an_coord.alloc(GM)) || (e = sp->an_orig.alloc(GM)) || (e = sp->an_visits.alloc(GM)) || (e = sp->an_pvlen.alloc(GM)) ||
   (e = sp->an_reward.alloc(GM)) || (e = sp->an_prior.alloc(GM)) || (e = sp->an_pvs.alloc(GM * max_pv)));
  if (e != hipSuccess) {
    sp_analysis_release(sp);
    sp->an_moves = sp->an_pv = 0;
    sp_analysis_blank(sp);
    return (int)e;
  }
  return 0;
}

int elfsp_last_analysis(const ElfSelfPlay* sp, int32_t* info, int32_t* coord, int32_t* orig, int32_t* visits, float* reward,
                        float* prior, int32_t* pv_len, int32_t* pv) {
  if (!sp) return ELFGO_E_BADARG;
  if (info) {
    if (sp->la_info.empty()) std::fill_n(info, (size_t)sp->G * ELFMCTS_ANALYZE_WORDS, 0);   // elfsp_set_analysis was never called
    else std::copy(sp->la_info.begin(), sp->la_info.end(), info);
  }
  if (coord) std::copy(sp->la_coord.begin(), sp->la_coord.end(), coord);
  if (orig) std::copy(sp->la_orig.begin(), sp->la_orig.end(), orig);
  if (visits) std::copy(sp->la_visits.begin(), sp->la_visits.end(), visits);
  if (reward) std::copy(sp->la_reward.begin(), sp->la_reward.end(), reward);
  if (prior) std::copy(sp->la_prior.begin(), sp->la_prior.end(), prior);
  if (pv_len) std::copy(sp->la_pvlen.begin(), sp->la_pvlen.end(), pv_len);
  if (pv) std::copy(sp->la_pvs.begin(), sp->la_pvs.end(), pv);
  return 0;
}

}  // extern "C"
