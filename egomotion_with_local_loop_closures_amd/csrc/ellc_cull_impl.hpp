// ellc_keyframe_cull_depth, ellc_cull_default_params (include/ellc_abi.h): the host side of the vote that removes the hypotheses of a
// keyframe slot which other views contradict. Included at the end of ellc_hip.hip behind ellc_sweep_impl.hpp: the refusals and the run
// of a call of K against views (ellc_ring_common.hpp) are used here as they stand; the staged view's two further fields (CullView: a
// view also carries its depth and variance planes), the parameter refusals, the Args, the record, the scratch and the five planes
// are this call's own.
#pragma once
#include "ellc_ring_common.hpp"
#include "ellc_refine_impl.hpp"
#include "ellc_kernels_cull.hpp"

using namespace ellc;

static_assert(sizeof(ellc_cull_params) == 28 && sizeof(ellc_cull_stats) == 64 && offsetof(ellc_cull_stats, n_culled_photo) == 20 &&
                  offsetof(ellc_cull_stats, sum_agree) == 24 && offsetof(ellc_cull_stats, sum_photo_bad) == 56,
              "ellc_cull_params is 28 bytes, ellc_cull_stats 64");
static_assert(sizeof(CullView) == 80, "a staged view is 80 bytes");

namespace {

// launches_ms (the diagnostic hook only): device time of cull_pixels and cull_finish, HIP events around them
ellc_status cull_depth_impl(ellc_ctx* c, int kf_slot, int level, int B, int views_are_kf, const int* view_slots, const float* T12, const float* light,
                            const ellc_map_filter* f, const ellc_cull_params* p, int dst, float* depth, float* var, uint32_t* votes, uint8_t* photo,
                            uint8_t* status, ellc_cull_stats* out, float* launches_ms) {
  const char* who = "ellc_keyframe_cull_depth";
  if (!c) return ELLC_ERR_BAD_ARG;
  const std::string w(who);
  // validated first: a refused call leaves the context and every slot as they were and writes nothing
  if (!view_slots || !T12 || !f || !p) return fail(c, ELLC_ERR_BAD_ARG, w + ": null pointer");
  ELLC_TRY(ring_views_check(c, who, B, ELLC_REFINE_MAX_VIEWS, views_are_kf, level, f, T12, light));
  if (!std::isfinite(p->agree_k2) || !std::isfinite(p->sigma_i2) || !std::isfinite(p->photo_k) || !(p->agree_k2 >= 0.0f) || !(p->sigma_i2 > 0.0f))
    return fail(c, ELLC_ERR_BAD_ARG, w + ": parameters out of range");
  if (p->min_support < 1 || p->min_support > B || p->min_in_front < 1 || p->min_in_front > B || p->min_photo < 1 || p->min_photo > B ||
      p->min_judged < 1 || p->min_judged > B)
    return fail(c, ELLC_ERR_BAD_ARG, w + ": a count outside 1..B");
  ELLC_TRY(ring_views_check_slots(c, who, dst, level, kf_slot, B, view_slots, views_are_kf));
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  const size_t n = (size_t)c->geom_h[level].n;
  CullArgs a{};
  a.v = ring_view(c, level, f);
  ELLC_TRY(ring_views_scratch(c, c->cull, ELLC_REFINE_MAX_VIEWS, n, kf_slot, B, a));
  ELLC_TRY(dev_grow(c, &c->cull_planes_d, &c->cull_planes_cap, n, 14));   // two f32 planes, one u32 plane and two u8 planes
  // a view also carries its depth and variance planes, where it is a keyframe slot that holds them (null otherwise: the staging's zeros)
  ELLC_TRY(ring_views_stage<CullView>(c, c->cull, level, B, views_are_kf, view_slots, T12, light, [&](CullView& vw, int b) {
    if (!views_are_kf || !c->kf_has_depth[view_slots[b]]) return;
    const KfLevelDev& k = c->kf_tab_h[ring_view_entry(c, level, 1, view_slots[b])];
    vw.depth = k.depth;
    vw.var = k.var;
  }));
  const PlaneCarve planes{c->cull_planes_d, c->cull_planes_cap};
  a.depth = planes.at<float>(0);
  a.var = planes.at<float>(4);
  a.votes = planes.at<uint32_t>(8);
  a.photo = planes.at<uint8_t>(12);
  a.status = planes.at<uint8_t>(13);
  a.agree_k2 = p->agree_k2;
  a.sp = sqrtf(1.0f / p->sigma_i2);
  a.photo_k = p->photo_k;
  a.min_support = p->min_support;
  a.min_judged = p->min_judged;
  a.min_in_front = p->min_in_front;
  a.min_photo = p->min_photo;
  const CullRec* rec = (const CullRec*)c->cull.out_h;
  const RingFetch fetch[5] = {{depth, a.depth, n * 4}, {var, a.var, n * 4}, {votes, a.votes, n * 4}, {photo, a.photo, n}, {status, a.status, n}};
  ELLC_TRY(ring_views_run(c, a, cull_pixels, cull_finish, view_slots, views_are_kf, fetch, dst, n, &rec->n[6], launches_ms));
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->n_kept = rec->n[0]; out->n_retained = rec->n[1];
    out->n_culled_free_space = rec->n[2]; out->n_culled_unsupported = rec->n[3]; out->n_culled_photo = rec->n[4];
    out->n_unseen = rec->n[5];
    out->sum_agree = rec->s[0]; out->sum_in_front = rec->s[1]; out->sum_behind = rec->s[2];
    out->sum_photo = rec->s[3]; out->sum_photo_bad = rec->s[4];
  }
  return ELLC_OK;
}

}  // namespace

extern "C" {

void ellc_cull_default_params(ellc_cull_params* p) {
  if (!p) return;
  p->agree_k2 = 1.0f; p->sigma_i2 = 16.0f; p->photo_k = 3.0f; p->min_support = 1; p->min_judged = 2; p->min_in_front = 1; p->min_photo = 2;
}

ellc_status ellc_keyframe_cull_depth(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12,
                                     const float* light, const ellc_map_filter* filter, const ellc_cull_params* params, int dst_kf_slot,
                                     float* depth, float* var, uint32_t* votes, uint8_t* photo, uint8_t* status, ellc_cull_stats* out) {
  return cull_depth_impl(c, kf_slot, level, B, views_are_keyframes, view_slots, T12, light, filter, params, dst_kf_slot, depth, var, votes, photo,
                         status, out, nullptr);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_cull_depth(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12,
                                    const float* light, const ellc_map_filter* filter, const ellc_cull_params* params, int dst_kf_slot,
                                    float* depth, float* var, uint32_t* votes, uint8_t* photo, uint8_t* status, ellc_cull_stats* out,
                                    float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) {
    return cull_depth_impl(c, kf_slot, level, B, views_are_keyframes, view_slots, T12, light, filter, params, dst_kf_slot, depth, var, votes,
                           photo, status, out, ms);
  });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
