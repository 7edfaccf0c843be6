// ellc_keyframe_refine_depth, ellc_refine_default_params, ellc_sim3_invert (include/ellc_abi.h): the host side of the per-pixel depth
// refinement of a keyframe slot against other views. Included at the end of ellc_hip.hip behind ellc_ring_common.hpp: its refusals,
// view, grow-only buffers and timing window are used here; the views' staging (RefineView) and the four planes are this call's own.
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
  const LevelGeom& g = c->geom_h[level];
  if (!std::isfinite(p->sigma_i2) || !std::isfinite(p->huber_k) || !std::isfinite(p->prior_weight) || !std::isfinite(p->max_step_rel) ||
      !(p->sigma_i2 > 0.0f) || !(p->huber_k > 0.0f) || !(p->prior_weight >= 0.0f) || !(p->max_step_rel > 0.0f) || p->n_iter < 1 || p->n_iter > 8 ||
      p->min_views < 1 || p->min_views > B)
    return fail(c, ELLC_ERR_BAD_ARG, w + ": parameters out of range");
  ELLC_TRY(ring_views_check_slots(c, who, dst, level, kf_slot, B, view_slots, views_are_kf));
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  const size_t n = (size_t)g.n;
  const int blocks = (int)((n + 255) / 256);
  ELLC_TRY(pair_reserve(c, c->refine, ELLC_REFINE_MAX_VIEWS, sizeof(RefineView), sizeof(RefineRec), (size_t)blocks));
  ELLC_TRY(dev_grow(c, &c->refine_planes_d, &c->refine_planes_cap, n, 10));   // two f32 planes and two u8 planes
  RefineView* vw = (RefineView*)c->refine.stage_h;
  for (int b = 0; b < B; b++) {
    vw[b].img = ring_view_image(c, level, views_are_kf, view_slots[b]);
    std::memcpy(vw[b].T, T12 + (size_t)12 * b, 12 * sizeof(float));
    vw[b].gain = light ? light[2 * b] : 1.0f;
    vw[b].offset = light ? light[2 * b + 1] : 0.0f;
  }
  ELLC_HIP(c, hipMemcpyAsync(c->refine.stage_d, c->refine.stage_h, (size_t)B * sizeof(RefineView), hipMemcpyHostToDevice, c->stream));
  RefineArgs a{};
  a.v = ring_view(c, level, f);
  a.views = (const RefineView*)c->refine.stage_d;
  a.partials = (RefineRec*)c->refine.partials_d;
  a.out = (RefineRec*)c->refine.out_dev_alias;
  char* planes = (char*)c->refine_planes_d;
  const size_t cap = c->refine_planes_cap;
  a.depth = (float*)planes;
  a.var = (float*)(planes + 4 * cap);
  a.nviews = (uint8_t*)(planes + 8 * cap);
  a.status = (uint8_t*)(planes + 9 * cap);
  a.kf_slot = kf_slot;
  a.B = B;
  a.blocks = blocks;
  a.first = 0;
  a.w0 = 1.0f / p->sigma_i2;
  a.sp = sqrtf(a.w0);
  a.huber_k = p->huber_k;
  a.prior_weight = p->prior_weight;
  a.max_step_rel = p->max_step_rel;
  a.n_iter = p->n_iter;
  a.min_views = p->min_views;
  LaunchTimer t(c, launches_ms);
  ELLC_TRY(t.begin());
  hipLaunchKernelGGL(refine_pixels, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(refine_finish, dim3(1), dim3(64), 0, c->stream, a);
  ELLC_HIP(c, hipGetLastError());
  ELLC_TRY(t.end());
  ELLC_TRY(ring_views_mark_use(c, B, view_slots, views_are_kf));
  if (depth) ELLC_HIP(c, hipMemcpyAsync(depth, a.depth, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (var) ELLC_HIP(c, hipMemcpyAsync(var, a.var, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (views) ELLC_HIP(c, hipMemcpyAsync(views, a.nviews, n, hipMemcpyDeviceToHost, c->stream));
  if (status) ELLC_HIP(c, hipMemcpyAsync(status, a.status, n, hipMemcpyDeviceToHost, c->stream));
  const RefineRec* rec = (const RefineRec*)c->refine.out_h;
  if (dst >= 0) ELLC_TRY(ring_views_store_dst(c, dst, a.depth, a.var, n, &rec->n[8]));
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->n_kept = rec->n[0]; out->n_taking_part = rec->n[1];
    out->n_refined = rec->n[2]; out->n_too_few_views = rec->n[3]; out->n_no_information = rec->n[4];
    out->n_bad_step = rec->n[5]; out->n_views_changed = rec->n[6]; out->n_cost_rose = rec->n[7];
    out->sum_views = rec->sum_views;
    out->sum_cost_before = rec->s[0];
    out->sum_cost_after = rec->s[1];
  }
  return t.read();
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
