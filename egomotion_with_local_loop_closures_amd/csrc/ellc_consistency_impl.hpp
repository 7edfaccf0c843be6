// ellc_keyframe_depth_consistency (include/ellc_abi.h): the host side of the map-against-map check.
// Included at the end of ellc_hip.hip behind ellc_ring_common.hpp: its refusals, view and pair reduction are used here.
#pragma once
#include "ellc_ring_common.hpp"
#include "ellc_kernels_consistency.hpp"

using namespace ellc;

static_assert(sizeof(ConsistRec) == sizeof(ellc_depth_consistency) && sizeof(ellc_depth_consistency) == 72 &&
                  offsetof(ConsistRec, sum_w_st) == offsetof(ellc_depth_consistency, sum_w_st) &&
                  offsetof(ConsistRec, sum_abs_di) == offsetof(ellc_depth_consistency, sum_abs_di) &&
                  offsetof(ConsistRec, sum_di2) == offsetof(ellc_depth_consistency, sum_di2) &&
                  offsetof(ConsistRec, n_kept) == offsetof(ellc_depth_consistency, n_kept) &&
                  offsetof(ConsistRec, n_weighted) == offsetof(ellc_depth_consistency, n_weighted),
              "ConsistRec mirrors ellc_depth_consistency");

namespace {

const int CONSIST_MAX_B = 2048;
const size_t CONSIST_SCRATCH_BYTES = (size_t)32 << 20;   // partial records of one launch: a larger batch goes in several launches

// launches_ms (the diagnostic hook only): device time of the launches, HIP events around them
ellc_status depth_consistency_impl(ellc_ctx* c, int B, const int* src, const int* dst, const float* T12, int level, const ellc_map_filter* f,
                                   float agree_k2, ellc_depth_consistency* out, float* launches_ms) {
  const char* who = "ellc_keyframe_depth_consistency";
  if (!c) return ELLC_ERR_BAD_ARG;
  if (!src || !dst || !T12 || !f || !out) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: null pointer");
  if (B < 1 || B > CONSIST_MAX_B) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: B out of range");
  if (level < 0 || level >= c->L) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: level out of range");
  const LevelGeom& g = c->geom_h[level];
  if (g.n > (1 << 24)) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: more than 2^24 pixels on the level");
  ELLC_TRY(ring_check_filter(c, who, f));
  if (!(agree_k2 >= 0.0f) || !std::isfinite(agree_k2)) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: agree_k2 negative or not finite");
  ELLC_TRY(ring_check_slots(c, who, B, src, c->cfg.max_keyframes));
  ELLC_TRY(ring_check_slots(c, who, B, dst, c->cfg.max_keyframes));
  ELLC_TRY(ring_check_ready(c, who, B, src));
  ELLC_TRY(ring_check_ready(c, who, B, dst));
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  ConsistArgs a{};
  a.v = ring_view(c, level, f);
  const int per_launch = pair_per_launch(B, CONSIST_SCRATCH_BYTES, (size_t)a.v.tiles * sizeof(ConsistRec));
  ELLC_TRY(pair_reserve(c, c->consist, B, 14 * sizeof(int), sizeof(ConsistRec), (size_t)per_launch * a.v.tiles));
  ELLC_TRY(pair_stage_slots(c, c->consist, B, src, dst, T12));
  a.stage = (const int*)c->consist.stage_d;
  a.cap = c->consist.cap;
  a.agree_k2 = agree_k2;
  return pair_run(c, c->consist, B, per_launch, consist_pass, consist_finish, a, out, launches_ms);
}

}  // namespace

extern "C" {

ellc_status ellc_keyframe_depth_consistency(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, int level,
                                            const ellc_map_filter* filter, float agree_k2, ellc_depth_consistency* out) {
  return depth_consistency_impl(c, B, src_kf_slots, dst_kf_slots, T12, level, filter, agree_k2, out, nullptr);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_depth_consistency(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, int level,
                                           const ellc_map_filter* filter, float agree_k2, ellc_depth_consistency* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) { return depth_consistency_impl(c, B, src_kf_slots, dst_kf_slots, T12, level, filter, agree_k2, out, ms); });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
