// ellc_keyframe_sweep_depth, ellc_sweep_default_params (include/ellc_abi.h): the host side of the depth sweep that creates hypotheses in
// a keyframe slot from other views. Included at the end of ellc_hip.hip behind ellc_refine_impl.hpp: the refusals and the run of a call
// of K against views (ellc_ring_common.hpp), the staged view (RefineView) and the four planes of ellc_keyframe_refine_depth are used
// here as they stand; the parameter refusals, the Args, the record and the scratch are this call's own.
#pragma once
#include "ellc_refine_impl.hpp"
#include "ellc_kernels_sweep.hpp"

using namespace ellc;

static_assert(sizeof(ellc_sweep_params) == 40 && sizeof(ellc_sweep_stats) == 64 && offsetof(ellc_sweep_stats, sum_views) == 32 &&
                  offsetof(ellc_sweep_stats, sum_cost) == 40 && offsetof(ellc_sweep_stats, reserved) == 48,
              "ellc_sweep_params is 40 bytes, ellc_sweep_stats 64");

namespace {

// launches_ms (the diagnostic hook only): device time of sweep_pixels and sweep_finish, HIP events around them
ellc_status sweep_depth_impl(ellc_ctx* c, int kf_slot, int level, int B, int views_are_kf, const int* view_slots, const float* T12, const float* light,
                             const ellc_sweep_params* p, int dst, float* depth, float* var, uint8_t* views, uint8_t* status, ellc_sweep_stats* out,
                             float* launches_ms) {
  const char* who = "ellc_keyframe_sweep_depth";
  if (!c) return ELLC_ERR_BAD_ARG;
  const std::string w(who);
  // validated first: a refused call leaves the context and every slot as they were and writes nothing
  if (!view_slots || !T12 || !p) return fail(c, ELLC_ERR_BAD_ARG, w + ": null pointer");
  ELLC_TRY(ring_views_check(c, who, B, ELLC_REFINE_MAX_VIEWS, views_are_kf, level, nullptr, T12, light));
  if (!std::isfinite(p->sigma_i2) || !std::isfinite(p->huber_k) || !std::isfinite(p->d_min) || !std::isfinite(p->d_max) || !std::isfinite(p->min_grad2) ||
      !std::isfinite(p->max_cost) || !std::isfinite(p->distinct_ratio) || !std::isfinite(p->var_scale))
    return fail(c, ELLC_ERR_BAD_ARG, w + ": parameter not finite");
  if (!(p->sigma_i2 > 0.0f) || !(p->huber_k > 0.0f) || !(p->d_min > 0.0f) || !(p->d_min < p->d_max) || !std::isfinite(1.0f / p->d_min) ||
      !(p->min_grad2 >= 0.0f) || !(p->distinct_ratio > 0.0f) || !(p->distinct_ratio <= 1.0f) || !(p->var_scale > 0.0f) || p->n_samples < 3 ||
      p->n_samples > ELLC_SWEEP_MAX_SAMPLES || p->min_views < 1 || p->min_views > B)
    return fail(c, ELLC_ERR_BAD_ARG, w + ": parameters out of range");
  ELLC_TRY(ring_views_check_slots(c, who, dst, level, kf_slot, B, view_slots, views_are_kf));
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  const size_t n = (size_t)c->geom_h[level].n;
  const ellc_map_filter every = {0.0f, 0, 1.0f, 1};   // (ring_view wants one; no kernel of this call reads it)
  SweepArgs a{};
  a.v = ring_view(c, level, &every);
  ELLC_TRY(ring_views_scratch(c, c->sweep, ELLC_REFINE_MAX_VIEWS, n, kf_slot, B, a));
  ELLC_TRY(dev_grow(c, &c->refine_planes_d, &c->refine_planes_cap, n, 10));   // two f32 planes and two u8 planes, shared with the refinement
  ELLC_TRY(ring_views_stage<RefineView>(c, c->sweep, level, B, views_are_kf, view_slots, T12, light));
  const PlaneCarve planes{c->refine_planes_d, c->refine_planes_cap};
  a.depth = planes.at<float>(0);
  a.var = planes.at<float>(4);
  a.nviews = planes.at<uint8_t>(8);
  a.status = planes.at<uint8_t>(9);
  a.w0 = 1.0f / p->sigma_i2;
  a.sp = sqrtf(a.w0);
  a.huber_k = p->huber_k;
  a.d_min = p->d_min;
  a.dstep = (p->d_max - p->d_min) / (float)(p->n_samples - 1);
  a.min_grad2 = p->min_grad2;
  a.max_cost = p->max_cost;
  a.distinct_ratio = p->distinct_ratio;
  a.var_scale = p->var_scale;
  a.n_samples = p->n_samples;
  a.min_views = p->min_views;
  const SweepRec* rec = (const SweepRec*)c->sweep.out_h;
  const RingFetch fetch[4] = {{depth, a.depth, n * 4}, {var, a.var, n * 4}, {views, a.nviews, n}, {status, a.status, n}};
  ELLC_TRY(ring_views_run(c, a, sweep_pixels, sweep_finish, view_slots, views_are_kf, fetch, dst, n, &rec->n[8], launches_ms));
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->n_ok = rec->n[0]; out->n_swept = rec->n[1];
    out->n_created = rec->n[2]; out->n_no_valid_sample = rec->n[3]; out->n_at_range_end = rec->n[4];
    out->n_cost_too_high = rec->n[5]; out->n_not_distinct = rec->n[6]; out->n_flat = rec->n[7];
    out->sum_views = rec->sum_views;
    out->sum_cost = rec->s[0];
  }
  return ELLC_OK;
}

}  // namespace

extern "C" {

void ellc_sweep_default_params(ellc_sweep_params* p) {
  if (!p) return;
  p->sigma_i2 = 16.0f; p->huber_k = 1.345f; p->d_min = 0.125f; p->d_max = 4.0f; p->min_grad2 = 100.0f; p->max_cost = 0.0f;
  p->distinct_ratio = 0.7f; p->var_scale = 1.0f; p->n_samples = 64; p->min_views = 2;
}

ellc_status ellc_keyframe_sweep_depth(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12,
                                      const float* light, const ellc_sweep_params* params, int dst_kf_slot, float* depth, float* var, uint8_t* views,
                                      uint8_t* status, ellc_sweep_stats* out) {
  return sweep_depth_impl(c, kf_slot, level, B, views_are_keyframes, view_slots, T12, light, params, dst_kf_slot, depth, var, views, status, out,
                          nullptr);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_sweep_depth(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12,
                                     const float* light, const ellc_sweep_params* params, int dst_kf_slot, float* depth, float* var, uint8_t* views,
                                     uint8_t* status, ellc_sweep_stats* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) {
    return sweep_depth_impl(c, kf_slot, level, B, views_are_keyframes, view_slots, T12, light, params, dst_kf_slot, depth, var, views, status, out, ms);
  });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
