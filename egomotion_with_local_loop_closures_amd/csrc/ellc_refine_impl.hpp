// ellc_keyframe_refine_depth, ellc_refine_default_params, ellc_sim3_invert (include/ellc_abi.h): the host side of the per-pixel depth
// refinement of a keyframe slot against other views. Included at the end of ellc_hip.hip behind ellc_ring_common.hpp: its refusals,
// view, grow-only buffers and the run of a call of K against views (staging, plane carve, launches, fetches, destination store) are
// used here; the null-pointer and n_iter refusals, the Args and the copy of the record into the stats are this call's own.
#pragma once
#include "ellc_ring_common.hpp"
#include "ellc_sim3_impl.hpp"
#include "ellc_kernels_refine.hpp"

using namespace ellc;

static_assert(sizeof(ellc_refine_params) == 24 && sizeof(ellc_refine_stats) == 64 && offsetof(ellc_refine_stats, sum_views) == 32 &&
                  offsetof(ellc_refine_stats, sum_cost_before) == 40 && offsetof(ellc_refine_stats, reserved) == 56,
              "ellc_refine_params is 24 bytes, ellc_refine_stats 64");
static_assert(sizeof(RefineView) == 64, "a staged view is 64 bytes");

namespace {

// launches_ms (the diagnostic hook only): device time of refine_pixels and refine_finish, HIP events around them
ellc_status refine_depth_impl(ellc_ctx* c, int kf_slot, int level, int B, int views_are_kf, const int* view_slots, const float* T12, const float* light,
                              const ellc_map_filter* f, const ellc_refine_params* p, int dst, float* depth, float* var, uint8_t* views,
                              uint8_t* status, ellc_refine_stats* out, float* launches_ms) {
  const char* who = "ellc_keyframe_refine_depth";
  if (!c) return ELLC_ERR_BAD_ARG;
  const std::string w(who);
  // validated first: a refused call leaves the context and every slot as they were and writes nothing
  if (!view_slots || !T12 || !f || !p) return fail(c, ELLC_ERR_BAD_ARG, w + ": null pointer");
  ELLC_TRY(ring_views_check(c, who, B, ELLC_REFINE_MAX_VIEWS, views_are_kf, level, f, T12, light));
  ELLC_TRY(ring_views_check_params(c, who, p, B));
  if (p->n_iter < 1 || p->n_iter > 8) return fail(c, ELLC_ERR_BAD_ARG, w + ": parameters out of range");
  ELLC_TRY(ring_views_check_slots(c, who, dst, level, kf_slot, B, view_slots, views_are_kf));
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  const size_t n = (size_t)c->geom_h[level].n;
  RefineArgs a{};
  a.v = ring_view(c, level, f);
  ELLC_TRY(ring_views_scratch(c, c->refine, ELLC_REFINE_MAX_VIEWS, n, kf_slot, B, a));
  ELLC_TRY(dev_grow(c, &c->refine_planes_d, &c->refine_planes_cap, n, 10));   // two f32 planes and two u8 planes
  ELLC_TRY(ring_views_stage<RefineView>(c, c->refine, level, B, views_are_kf, view_slots, T12, light));
  const PlaneCarve planes{c->refine_planes_d, c->refine_planes_cap};
  a.depth = planes.at<float>(0);
  a.var = planes.at<float>(4);
  a.nviews = planes.at<uint8_t>(8);
  a.status = planes.at<uint8_t>(9);
  a.w0 = 1.0f / p->sigma_i2;
  a.sp = sqrtf(a.w0);
  a.huber_k = p->huber_k;
  a.prior_weight = p->prior_weight;
  a.max_step_rel = p->max_step_rel;
  a.n_iter = p->n_iter;
  a.min_views = p->min_views;
  const RefineRec* rec = (const RefineRec*)c->refine.out_h;
  const RingFetch fetch[4] = {{depth, a.depth, n * 4}, {var, a.var, n * 4}, {views, a.nviews, n}, {status, a.status, n}};
  ELLC_TRY(ring_views_run(c, a, refine_pixels, refine_finish, view_slots, views_are_kf, fetch, dst, n, &rec->n[8], launches_ms));
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->n_kept = rec->n[0]; out->n_taking_part = rec->n[1];
    out->n_refined = rec->n[2]; out->n_too_few_views = rec->n[3]; out->n_no_information = rec->n[4];
    out->n_bad_step = rec->n[5]; out->n_views_changed = rec->n[6]; out->n_cost_rose = rec->n[7];
    out->sum_views = rec->sum_views;
    out->sum_cost_before = rec->s[0];
    out->sum_cost_after = rec->s[1];
  }
  return ELLC_OK;
}

}  // namespace

extern "C" {

void ellc_refine_default_params(ellc_refine_params* p) {
  if (!p) return;
  p->sigma_i2 = 16.0f; p->huber_k = 1.345f; p->prior_weight = 1.0f; p->max_step_rel = 0.5f; p->n_iter = 3; p->min_views = 2;
}

void ellc_sim3_invert(const float* T12_in, const float* light_in, float* T12_out, float* light_out) {
  double M[9], t[3];
  for (int r = 0; r < 3; r++) {
    for (int q = 0; q < 3; q++) M[3 * r + q] = (double)T12_in[4 * r + q];
    t[r] = (double)T12_in[4 * r + 3];
  }
  // the adjugate over the determinant
  const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
  const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
  const double I[9] = {c00 / det, (M[2] * M[7] - M[1] * M[8]) / det, (M[1] * M[5] - M[2] * M[4]) / det,
                       c01 / det, (M[0] * M[8] - M[2] * M[6]) / det, (M[2] * M[3] - M[0] * M[5]) / det,
                       c02 / det, (M[1] * M[6] - M[0] * M[7]) / det, (M[0] * M[4] - M[1] * M[3]) / det};
  float o[12];
  for (int r = 0; r < 3; r++) {
    for (int q = 0; q < 3; q++) o[4 * r + q] = (float)I[3 * r + q];
    o[4 * r + 3] = (float)(-((I[3 * r] * t[0] + I[3 * r + 1] * t[1]) + I[3 * r + 2] * t[2]));
  }
  const double gain = light_in ? (double)light_in[0] : 1.0, offset = light_in ? (double)light_in[1] : 0.0;
  std::memcpy(T12_out, o, sizeof(o));
  if (light_out) {
    light_out[0] = (float)(1.0 / gain);
    light_out[1] = (float)(-offset / gain);
  }
}

ellc_status ellc_keyframe_refine_depth(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12,
                                       const float* light, const ellc_map_filter* filter, const ellc_refine_params* params, int dst_kf_slot,
                                       float* depth, float* var, uint8_t* views, uint8_t* status, ellc_refine_stats* out) {
  return refine_depth_impl(c, kf_slot, level, B, views_are_keyframes, view_slots, T12, light, filter, params, dst_kf_slot, depth, var, views, status,
                           out, nullptr);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_refine_depth(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12,
                                      const float* light, const ellc_map_filter* filter, const ellc_refine_params* params, int dst_kf_slot,
                                      float* depth, float* var, uint8_t* views, uint8_t* status, ellc_refine_stats* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) {
    return refine_depth_impl(c, kf_slot, level, B, views_are_keyframes, view_slots, T12, light, filter, params, dst_kf_slot, depth, var, views,
                             status, out, ms);
  });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
