// ellc_keyframe_trial_propagate, ellc_keyframe_trial_propagate_lit, ellc_trial_light_solve (include/ellc_abi.h): the host side of the
// per-pair trial records.
// Included at the end of ellc_hip.hip behind ellc_ring_common.hpp: its refusals, view and pair reduction are used here; the requests
// (TrialReq) and the bitmaps are this call's own.
#pragma once
#include "ellc_ring_common.hpp"
#include "ellc_kernels_trial.hpp"

using namespace ellc;

static_assert(sizeof(TrialRec) == sizeof(ellc_trial_propagation) && sizeof(ellc_trial_propagation) == 48 &&
                  offsetof(TrialRec, sum_abs_r) == offsetof(ellc_trial_propagation, sum_abs_r) &&
                  offsetof(TrialRec, n_kept) == offsetof(ellc_trial_propagation, n_kept) &&
                  offsetof(TrialRec, n_low_grad) == offsetof(ellc_trial_propagation, n_low_grad) &&
                  offsetof(TrialRec, n_targets) == offsetof(ellc_trial_propagation, n_targets) &&
                  offsetof(TrialRec, reserved) == offsetof(ellc_trial_propagation, reserved),
              "TrialRec mirrors ellc_trial_propagation");
static_assert(sizeof(TrialRecLit) == sizeof(ellc_trial_propagation_lit) && sizeof(ellc_trial_propagation_lit) == 96 && offsetof(TrialRecLit, t) == 0 &&
                  offsetof(ellc_trial_propagation_lit, reserved) == offsetof(ellc_trial_propagation, reserved) &&
                  offsetof(TrialRecLit, fit) == offsetof(ellc_trial_propagation_lit, sum_s) && offsetof(ellc_trial_propagation_lit, sum_s) == 48 &&
                  offsetof(ellc_trial_propagation_lit, sum_tt) == 48 + 4 * 8 && offsetof(TrialRecLit, n_fit) == offsetof(ellc_trial_propagation_lit, n_fit) &&
                  offsetof(ellc_trial_propagation_lit, n_fit) == 88 && offsetof(ellc_trial_propagation_lit, reserved2) == 92,
              "TrialRecLit mirrors ellc_trial_propagation_lit");

namespace {

const int TRIAL_MAX_B = 2048;
const size_t TRIAL_BITS_BYTES = (size_t)64 << 20;   // bitmaps of one launch: a larger batch goes in several launches

// max_group_requests (the diagnostic hook only, 0 = as the bitmaps fit): requests per launch; launches_ms: device time of the launches.
// Rec: TrialRec for ellc_keyframe_trial_propagate (light NULL: (1, 0) each), TrialRecLit for ellc_keyframe_trial_propagate_lit; each
// has a PairScratch of its own, their records differing in size.
template <class Rec>
ellc_status trial_propagate_impl(ellc_ctx* c, const char* who, PairScratch ellc_ctx::*scratch, void (*pass)(TrialArgs<Rec>), void (*finish)(TrialArgs<Rec>), int B, const int* src, int dst_is_kf, const int* dst,
                                 const float* T12, const float* light, const ellc_map_filter* f, int photo_gate, void* out, int max_group_requests,
                                 float* launches_ms) {
  if (!c) return ELLC_ERR_BAD_ARG;
  if (!src || !dst || !T12 || !f || !out) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  if (B < 1 || B > TRIAL_MAX_B) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": B out of range");
  if (dst_is_kf < 0 || dst_is_kf > 1 || photo_gate < 0 || photo_gate > 1) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": dst_is_keyframe / photo_gate not 0 or 1");
  if (max_group_requests < 0) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": max_group_requests negative");
  const LevelGeom& g = c->geom_h[0];
  if (g.n > (1 << 24)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": more than 2^24 pixels");
  ELLC_TRY(ring_check_filter(c, who, f));
  ELLC_TRY(ring_check_slots(c, who, B, src, c->cfg.max_keyframes));
  ELLC_TRY(ring_check_slots(c, who, B, dst, dst_is_kf ? c->cfg.max_keyframes : c->cfg.max_frames));
  ELLC_TRY(light_check(c, who, B, light));
  for (int b = 0; b < B; b++) {
    if (!c->kf_has_image[src[b]] || !c->kf_has_depth[src[b]]) return fail(c, ELLC_ERR_NOT_READY, std::string(who) + ": source slot lacks image or depth");
    if (!(dst_is_kf ? c->kf_has_image[dst[b]] : c->fr_has_image[dst[b]])) return fail(c, ELLC_ERR_NOT_READY, std::string(who) + ": destination slot lacks an image");
  }
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  PairScratch& ps = c->*scratch;
  TrialArgs<Rec> a{};
  a.v = ring_view(c, 0, f);
  const size_t words = ((size_t)g.n + 31) / 32;
  int per_launch = pair_per_launch(B, TRIAL_BITS_BYTES, words * sizeof(unsigned));
  if (max_group_requests > 0) per_launch = std::min(per_launch, max_group_requests);
  ELLC_TRY(pair_reserve(c, ps, B, sizeof(TrialReq), sizeof(Rec), (size_t)per_launch * a.v.tiles));
  ELLC_TRY(dev_grow(c, (void**)&c->trial_bits_d, &c->trial_bits_cap, (size_t)per_launch * words, sizeof(unsigned)));
  // the destinations' maxAbsGradient planes, built where they are not (as the absorb builds K's)
  std::vector<char>& grad_ok = dst_is_kf ? c->kf_maxgrad_valid : c->fr_maxgrad_valid;
  for (int b = 0; b < B; b++)
    if (!grad_ok[dst[b]]) ELLC_TRY(build_maxgrad(c, dst_is_kf != 0, dst[b]));
  TrialReq* rq = (TrialReq*)ps.stage_h;
  for (int b = 0; b < B; b++) {
    rq[b].dst_img = dst_is_kf ? c->kf_tab_h[dst[b]].img : c->fr_tab_h[dst[b]].img;   // (level 0: the first max_keyframes / max_frames entries)
    rq[b].dst_maxgrad = dst_is_kf ? c->kf_maxgrad[dst[b]] : c->fr_maxgrad[dst[b]];
    std::memcpy(rq[b].T, T12 + (size_t)12 * b, 12 * sizeof(float));
    rq[b].src = src[b];
    rq[b].gain = light ? light[2 * b] : 1.0f;
    rq[b].offset = light ? light[2 * b + 1] : 0.0f;
    rq[b].pad_ = 0;
  }
  ELLC_HIP(c, hipMemcpyAsync(ps.stage_d, ps.stage_h, (size_t)B * sizeof(TrialReq), hipMemcpyHostToDevice, c->stream));
  a.req = (const TrialReq*)ps.stage_d;
  a.bits = c->trial_bits_d;
  a.words = (unsigned)words;
  a.photo_gate = photo_gate;
  auto clear_bits = [&](int n) -> ellc_status {
    ELLC_HIP(c, hipMemsetAsync(c->trial_bits_d, 0, (size_t)n * words * sizeof(unsigned), c->stream));
    return ELLC_OK;
  };
  auto mark_readers = [&](int) -> ellc_status {   // a later upload into a frame slot waits for this reader
    std::vector<char> seen((size_t)c->cfg.max_frames, 0);
    for (int b = 0; b < B && !dst_is_kf; b++)
      if (!seen[dst[b]]) {
        seen[dst[b]] = 1;
        ELLC_TRY(mark_frame_use(c, dst[b]));
      }
    return ELLC_OK;
  };
  return pair_run(c, ps, B, per_launch, pass, finish, a, out, launches_ms, clear_bits, mark_readers);
}

}  // namespace

extern "C" {

ellc_status ellc_keyframe_trial_propagate(ellc_ctx* c, int B, const int* src_kf_slots, int dst_is_keyframe, const int* dst_slots, const float* T12,
                                          const ellc_map_filter* filter, int photo_gate, ellc_trial_propagation* out) {
  return trial_propagate_impl<TrialRec>(c, "ellc_keyframe_trial_propagate", &ellc_ctx::trial, trial_pass, trial_finish, B, src_kf_slots, dst_is_keyframe, dst_slots, T12, nullptr, filter,
                                        photo_gate, out, 0, nullptr);
}

ellc_status ellc_keyframe_trial_propagate_lit(ellc_ctx* c, int B, const int* src_kf_slots, int dst_is_keyframe, const int* dst_slots, const float* T12,
                                              const float* light, const ellc_map_filter* filter, int photo_gate, ellc_trial_propagation_lit* out) {
  return trial_propagate_impl<TrialRecLit>(c, "ellc_keyframe_trial_propagate_lit", &ellc_ctx::trial_lit, trial_lit_pass, trial_lit_finish, B, src_kf_slots, dst_is_keyframe, dst_slots, T12, light,
                                           filter, photo_gate, out, 0, nullptr);
}

// ellc_light_solve's rule with weight 1 over the interior pixels: the record's five sums as an ellc_light_normal
int ellc_trial_light_solve(const ellc_trial_propagation_lit* rec, const ellc_light_params* params, const float* light_in, float* light_out) {
  if (!rec || !params || !light_out) return 1;   // nothing to fit or nowhere to put it: refused, nothing written
  ellc_light_normal n;
  std::memset(&n, 0, sizeof(n));
  n.sum_w = (double)rec->n_fit;
  n.sum_w_s = rec->sum_s; n.sum_w_t = rec->sum_t; n.sum_w_ss = rec->sum_ss; n.sum_w_st = rec->sum_st; n.sum_w_tt = rec->sum_tt;
  n.n_photo = rec->n_fit;
  return ellc_light_solve(&n, params, light_in, light_out);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_trial_propagate(ellc_ctx* c, int B, const int* src_kf_slots, int dst_is_keyframe, const int* dst_slots, const float* T12,
                                         const ellc_map_filter* filter, int photo_gate, ellc_trial_propagation* out, int max_group_requests,
                                         float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) {
    return trial_propagate_impl<TrialRec>(c, "ellc_keyframe_trial_propagate", &ellc_ctx::trial, trial_pass, trial_finish, B, src_kf_slots, dst_is_keyframe, dst_slots, T12, nullptr,
                                          filter, photo_gate, out, max_group_requests, ms);
  });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
