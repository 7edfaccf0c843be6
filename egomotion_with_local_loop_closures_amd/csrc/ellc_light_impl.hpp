// ellc_keyframe_light_step, ellc_light_solve (include/ellc_abi.h): the affine brightness of a keyframe pair on its own. Included at the
// end of ellc_hip.hip behind ellc_sim3_impl.hpp, which holds light_evaluate beside sim3_evaluate, the refusals both share, and the loop
// that fits the light (ellc_keyframe_sim3_align_lit).
#pragma once
#include "ellc_sim3_impl.hpp"

using namespace ellc;

static_assert(sizeof(LightRec) == sizeof(ellc_light_normal) && sizeof(ellc_light_normal) == 72 && offsetof(LightRec, s) == offsetof(ellc_light_normal, sum_w) &&
                  offsetof(ellc_light_normal, sum_w_tt) == 5 * 8 && offsetof(ellc_light_normal, chi2_photo) == 6 * 8 &&
                  offsetof(LightRec, n) == offsetof(ellc_light_normal, n_kept) && offsetof(ellc_light_normal, n_photo_huber) == offsetof(LightRec, n) + 12,
              "LightRec mirrors ellc_light_normal");
static_assert(sizeof(ellc_light_params) == 12, "ellc_light_params is 12 bytes");

namespace {

ellc_status light_step_impl(ellc_ctx* c, int B, const int* src, const int* dst, const float* T12, const float* light, int level,
                            const ellc_map_filter* f, const ellc_sim3_params* p, ellc_light_normal* out, float* launches_ms) {
  if (!c) return ELLC_ERR_BAD_ARG;
  const char* who = "ellc_keyframe_light_step";
  if (!out) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  ELLC_TRY(sim3_validate(c, who, B, src, dst, T12, level, level, f, p));
  ELLC_TRY(light_check(c, who, B, light));
  ELLC_ENTER(c);
  return light_evaluate(c, B, src, dst, T12, light, level, f, p, out, launches_ms);
}

}  // namespace

extern "C" {

void ellc_light_default_params(ellc_light_params* p) {
  if (!p) return;
  p->gain_min = 0.25f; p->gain_max = 4.0f; p->min_pixels = 16;
}

int ellc_light_solve(const ellc_light_normal* n, const ellc_light_params* p, const float* light_in, float* light_out) {
  const float keep[2] = {light_in ? light_in[0] : 1.0f, light_in ? light_in[1] : 0.0f};
  const double det = n->sum_w * n->sum_w_ss - n->sum_w_s * n->sum_w_s;
  const double gain = (n->sum_w * n->sum_w_st - n->sum_w_s * n->sum_w_t) / det;
  const double offset = (n->sum_w_t - gain * n->sum_w_s) / n->sum_w;
  const bool ok = n->n_photo >= p->min_pixels && det > 1e-10 * n->sum_w * n->sum_w_ss && gain >= (double)p->gain_min && gain <= (double)p->gain_max &&
                  std::fabs(offset) <= 255.0;   // (NaN fails every test)
  light_out[0] = ok ? (float)gain : keep[0];
  light_out[1] = ok ? (float)offset : keep[1];
  return ok ? 0 : 1;
}

ellc_status ellc_keyframe_light_step(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, const float* light_in,
                                     int level, const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_light_normal* out) {
  return light_step_impl(c, B, src_kf_slots, dst_kf_slots, T12, light_in, level, filter, params, out, nullptr);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_light_step(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, const float* light_in,
                                    int level, const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_light_normal* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) { return light_step_impl(c, B, src_kf_slots, dst_kf_slots, T12, light_in, level, filter, params, out, ms); });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
