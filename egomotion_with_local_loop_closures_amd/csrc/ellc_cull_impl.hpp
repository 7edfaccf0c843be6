// ellc_keyframe_cull_depth, ellc_cull_default_params (include/ellc_abi.h): the host side of the vote that removes the hypotheses of a
// keyframe slot which other views contradict. Included at the end of ellc_hip.hip behind ellc_sweep_impl.hpp:
// ellc_keyframe_refine_depth's refusals and destination store are used here as they stand; the views' staging (CullView: a view also
// carries its depth and variance planes), the record, the scratch and the five planes are this call's own.
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
  const LevelGeom& g = c->geom_h[level];
  if (!std::isfinite(p->agree_k2) || !std::isfinite(p->sigma_i2) || !std::isfinite(p->photo_k) || !(p->agree_k2 >= 0.0f) || !(p->sigma_i2 > 0.0f))
    return fail(c, ELLC_ERR_BAD_ARG, w + ": parameters out of range");
  if (p->min_support < 1 || p->min_support > B || p->min_in_front < 1 || p->min_in_front > B || p->min_photo < 1 || p->min_photo > B ||
      p->min_judged < 1 || p->min_judged > B)
    return fail(c, ELLC_ERR_BAD_ARG, w + ": a count outside 1..B");
  ELLC_TRY(ring_views_check_slots(c, who, dst, level, kf_slot, B, view_slots, views_are_kf));
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  const size_t n = (size_t)g.n;
  const int blocks = (int)((n + 255) / 256);
  ELLC_TRY(pair_reserve(c, c->cull, ELLC_REFINE_MAX_VIEWS, sizeof(CullView), sizeof(CullRec), (size_t)blocks));
  ELLC_TRY(dev_grow(c, &c->cull_planes_d, &c->cull_planes_cap, n, 14));   // two f32 planes, one u32 plane and two u8 planes
  CullView* vw = (CullView*)c->cull.stage_h;
  for (int b = 0; b < B; b++) {
    const size_t e = ring_view_entry(c, level, views_are_kf, view_slots[b]);
    const bool has_depth = views_are_kf && c->kf_has_depth[view_slots[b]];
    vw[b].img = views_are_kf ? c->kf_tab_h[e].img : c->fr_tab_h[e].img;
    vw[b].depth = has_depth ? c->kf_tab_h[e].depth : nullptr;
    vw[b].var = has_depth ? c->kf_tab_h[e].var : nullptr;
    std::memcpy(vw[b].T, T12 + (size_t)12 * b, 12 * sizeof(float));
    vw[b].gain = light ? light[2 * b] : 1.0f;
    vw[b].offset = light ? light[2 * b + 1] : 0.0f;
  }
  ELLC_HIP(c, hipMemcpyAsync(c->cull.stage_d, c->cull.stage_h, (size_t)B * sizeof(CullView), hipMemcpyHostToDevice, c->stream));
  CullArgs a{};
  a.v = ring_view(c, level, f);
  a.views = (const CullView*)c->cull.stage_d;
  a.partials = (CullRec*)c->cull.partials_d;
  a.out = (CullRec*)c->cull.out_dev_alias;
  char* planes = (char*)c->cull_planes_d;
  const size_t cap = c->cull_planes_cap;
  a.depth = (float*)planes;
  a.var = (float*)(planes + 4 * cap);
  a.votes = (uint32_t*)(planes + 8 * cap);
  a.photo = (uint8_t*)(planes + 12 * cap);
  a.status = (uint8_t*)(planes + 13 * cap);
  a.kf_slot = kf_slot;
  a.B = B;
  a.blocks = blocks;
  a.first = 0;
  a.agree_k2 = p->agree_k2;
  a.sp = sqrtf(1.0f / p->sigma_i2);
  a.photo_k = p->photo_k;
  a.min_support = p->min_support;
  a.min_judged = p->min_judged;
  a.min_in_front = p->min_in_front;
  a.min_photo = p->min_photo;
  LaunchTimer t(c, launches_ms);
  ELLC_TRY(t.begin());
  hipLaunchKernelGGL(cull_pixels, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(cull_finish, dim3(1), dim3(64), 0, c->stream, a);
  ELLC_HIP(c, hipGetLastError());
  ELLC_TRY(t.end());
  ELLC_TRY(ring_views_mark_use(c, B, view_slots, views_are_kf));
  if (depth) ELLC_HIP(c, hipMemcpyAsync(depth, a.depth, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (var) ELLC_HIP(c, hipMemcpyAsync(var, a.var, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (votes) ELLC_HIP(c, hipMemcpyAsync(votes, a.votes, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (photo) ELLC_HIP(c, hipMemcpyAsync(photo, a.photo, n, hipMemcpyDeviceToHost, c->stream));
  if (status) ELLC_HIP(c, hipMemcpyAsync(status, a.status, n, hipMemcpyDeviceToHost, c->stream));
  const CullRec* rec = (const CullRec*)c->cull.out_h;
  if (dst >= 0) ELLC_TRY(ring_views_store_dst(c, dst, a.depth, a.var, n, &rec->n[6]));
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->n_kept = rec->n[0]; out->n_retained = rec->n[1];
    out->n_culled_free_space = rec->n[2]; out->n_culled_unsupported = rec->n[3]; out->n_culled_photo = rec->n[4];
    out->n_unseen = rec->n[5];
    out->sum_agree = rec->s[0]; out->sum_in_front = rec->s[1]; out->sum_behind = rec->s[2];
    out->sum_photo = rec->s[3]; out->sum_photo_bad = rec->s[4];
  }
  return t.read();
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
