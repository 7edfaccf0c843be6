// ellc_keyframe_depth_consistency (include/ellc_abi.h): the host side of the map-against-map check.
// Included at the end of ellc_hip.hip (the library is one translation unit).
#pragma once
#include "ellc_context.hpp"
#include "ellc_kernels_consistency.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

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
  if (!c) return ELLC_ERR_BAD_ARG;
  // validated first: a refused call leaves the context as it was and `out` unwritten
  if (!src || !dst || !T12 || !f || !out) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: null pointer");
  if (B < 1 || B > CONSIST_MAX_B) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: B out of range");
  if (level < 0 || level >= c->L) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: level out of range");
  const LevelGeom& g = c->geom_h[level];
  if (g.n > (1 << 24)) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: more than 2^24 pixels on the level");
  if (f->min_support < 0 || f->min_support > 8 || f->stride < 1 || !(f->support_k2 >= 0.0f) || !std::isfinite(f->support_k2) || std::isnan(f->max_var))
    return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: filter out of range");
  if (!(agree_k2 >= 0.0f) || !std::isfinite(agree_k2)) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: agree_k2 negative or not finite");
  for (int b = 0; b < B; b++)
    if (!slot_ok(src[b], c->cfg.max_keyframes) || !slot_ok(dst[b], c->cfg.max_keyframes))
      return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_depth_consistency: slot index out of range");
  for (int b = 0; b < B; b++)
    if (!c->kf_has_image[src[b]] || !c->kf_has_depth[src[b]] || !c->kf_has_image[dst[b]] || !c->kf_has_depth[dst[b]])
      return fail(c, ELLC_ERR_NOT_READY, "ellc_keyframe_depth_consistency: keyframe slot lacks image or depth");
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  const int tiles = c->tile_begin[level + 1] - c->tile_begin[level];
  const int per_launch = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, CONSIST_SCRATCH_BYTES / ((size_t)tiles * sizeof(ConsistRec))));
  // (nothing of this call is in flight when its buffers grow: the call is synchronous)
  if (B > c->consist_cap) {
    if (c->consist_stage_h) (void)hipHostFree(c->consist_stage_h);
    if (c->consist_out_h) (void)hipHostFree(c->consist_out_h);
    if (c->consist_stage_d) (void)hipFree(c->consist_stage_d);
    c->consist_stage_h = nullptr; c->consist_out_h = nullptr; c->consist_stage_d = nullptr; c->consist_out_dev_alias = nullptr;
    c->consist_cap = 0;
    void *sh = nullptr, *oh = nullptr, *sd = nullptr, *da = nullptr;
    ELLC_HIP(c, hipHostMalloc(&sh, (size_t)14 * B * sizeof(int), hipHostMallocDefault));
    c->consist_stage_h = (int*)sh;
    ELLC_HIP(c, hipHostMalloc(&oh, (size_t)B * sizeof(ConsistRec), hipHostMallocDefault));
    c->consist_out_h = oh;
    ELLC_HIP(c, hipMalloc(&sd, (size_t)14 * B * sizeof(int)));
    c->consist_stage_d = (int*)sd;
    ELLC_HIP(c, hipHostGetDevicePointer(&da, oh, 0));
    c->consist_out_dev_alias = da;
    c->consist_cap = B;
  }
  const size_t need = (size_t)per_launch * tiles;
  if (need > c->consist_partials_cap) {
    if (c->consist_partials_d) (void)hipFree(c->consist_partials_d);
    c->consist_partials_d = nullptr;
    c->consist_partials_cap = 0;
    ELLC_HIP(c, hipMalloc(&c->consist_partials_d, need * sizeof(ConsistRec)));
    c->consist_partials_cap = need;
  }
  const int cap = c->consist_cap;
  std::memcpy(c->consist_stage_h, src, (size_t)B * sizeof(int));
  std::memcpy(c->consist_stage_h + cap, dst, (size_t)B * sizeof(int));
  std::memcpy(c->consist_stage_h + 2 * (size_t)cap, T12, (size_t)B * 12 * sizeof(float));
  ELLC_HIP(c, hipMemcpyAsync(c->consist_stage_d, c->consist_stage_h, (size_t)14 * cap * sizeof(int), hipMemcpyHostToDevice, c->stream));
  ConsistArgs a;
  a.m.geom = c->geom_d;
  a.m.kf_tab = c->kf_tab_d;
  a.m.stage = nullptr;
  a.m.tile_counts = nullptr;
  a.m.tile_offsets = nullptr;
  a.m.totals = nullptr;
  a.m.out = nullptr;
  a.m.out_cap = 0u;
  a.m.level = level;
  a.m.max_kf = c->cfg.max_keyframes;
  a.m.tiles = tiles;
  a.m.B = B;
  a.m.max_var = f->max_var;
  a.m.min_support = f->min_support;
  a.m.support_k2 = f->support_k2;
  a.m.stride = f->stride;
  a.stage = c->consist_stage_d;
  a.partials = (ConsistRec*)c->consist_partials_d;
  a.out = (ConsistRec*)c->consist_out_dev_alias;
  a.cap = cap;
  a.agree_k2 = agree_k2;
  if (launches_ms) ELLC_HIP(c, hipEventRecord(c->ev0, c->stream));
  for (int first = 0; first < B; first += per_launch) {   // (a record depends on its own request only: the split does not enter it)
    const int n = std::min(per_launch, B - first);
    a.first = first;
    hipLaunchKernelGGL(consist_pass, dim3(tiles, n), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(consist_finish, dim3(n), dim3(64), 0, c->stream, a);
  }
  ELLC_HIP(c, hipGetLastError());
  if (launches_ms) ELLC_HIP(c, hipEventRecord(c->ev1, c->stream));
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  std::memcpy(out, c->consist_out_h, (size_t)B * sizeof(ConsistRec));
  if (launches_ms) ELLC_HIP(c, hipEventElapsedTime(launches_ms, c->ev0, c->ev1));
  return ELLC_OK;
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
  float ms = 0.0f;
  const ellc_status s = depth_consistency_impl(c, B, src_kf_slots, dst_kf_slots, T12, level, filter, agree_k2, out, &ms);
  if (launches_ms) *launches_ms = ms;
  return s;
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
