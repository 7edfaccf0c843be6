// ellc_keyframe_trial_propagate (include/ellc_abi.h): the host side of the per-pair trial records.
// Included at the end of ellc_hip.hip (the library is one translation unit).
#pragma once
#include "ellc_context.hpp"
#include "ellc_kernels_trial.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace ellc;

static_assert(sizeof(TrialRec) == sizeof(ellc_trial_propagation) && sizeof(ellc_trial_propagation) == 48 &&
                  offsetof(TrialRec, sum_abs_r) == offsetof(ellc_trial_propagation, sum_abs_r) &&
                  offsetof(TrialRec, n_kept) == offsetof(ellc_trial_propagation, n_kept) &&
                  offsetof(TrialRec, n_low_grad) == offsetof(ellc_trial_propagation, n_low_grad) &&
                  offsetof(TrialRec, n_targets) == offsetof(ellc_trial_propagation, n_targets) &&
                  offsetof(TrialRec, reserved) == offsetof(ellc_trial_propagation, reserved),
              "TrialRec mirrors ellc_trial_propagation");

namespace {

const int TRIAL_MAX_B = 2048;
const size_t TRIAL_BITS_BYTES = (size_t)64 << 20;   // bitmaps of one launch: a larger batch goes in several launches

// max_group_requests (the diagnostic hook only, 0 = as the bitmaps fit): requests per launch; launches_ms: device time of the launches
ellc_status trial_propagate_impl(ellc_ctx* c, int B, const int* src, int dst_is_kf, const int* dst, const float* T12, const ellc_map_filter* f,
                                 int photo_gate, ellc_trial_propagation* out, int max_group_requests, float* launches_ms) {
  const char* who = "ellc_keyframe_trial_propagate";
  if (!c) return ELLC_ERR_BAD_ARG;
  // validated first: a refused call leaves the context as it was and `out` unwritten
  if (!src || !dst || !T12 || !f || !out) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  if (B < 1 || B > TRIAL_MAX_B) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": B out of range");
  if (dst_is_kf < 0 || dst_is_kf > 1 || photo_gate < 0 || photo_gate > 1) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": dst_is_keyframe / photo_gate not 0 or 1");
  if (max_group_requests < 0) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": max_group_requests negative");
  const LevelGeom& g = c->geom_h[0];
  if (g.n > (1 << 24)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": more than 2^24 pixels");
  if (f->min_support < 0 || f->min_support > 8 || f->stride < 1 || !(f->support_k2 >= 0.0f) || !std::isfinite(f->support_k2) || std::isnan(f->max_var))
    return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": filter out of range");
  const int n_dst = dst_is_kf ? c->cfg.max_keyframes : c->cfg.max_frames;
  for (int b = 0; b < B; b++)
    if (!slot_ok(src[b], c->cfg.max_keyframes) || !slot_ok(dst[b], n_dst)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": slot index out of range");
  for (int b = 0; b < B; b++) {
    if (!c->kf_has_image[src[b]] || !c->kf_has_depth[src[b]]) return fail(c, ELLC_ERR_NOT_READY, std::string(who) + ": source slot lacks image or depth");
    if (!(dst_is_kf ? c->kf_has_image[dst[b]] : c->fr_has_image[dst[b]])) return fail(c, ELLC_ERR_NOT_READY, std::string(who) + ": destination slot lacks an image");
  }
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  const int tiles = c->tile_begin[1] - c->tile_begin[0];
  const size_t words = ((size_t)g.n + 31) / 32;
  int per_launch = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, TRIAL_BITS_BYTES / (words * sizeof(unsigned))));
  if (max_group_requests > 0) per_launch = std::min(per_launch, max_group_requests);
  // (nothing of this call is in flight when its buffers grow: the call is synchronous)
  if (B > c->trial_cap) {
    if (c->trial_req_h) (void)hipHostFree(c->trial_req_h);
    if (c->trial_out_h) (void)hipHostFree(c->trial_out_h);
    if (c->trial_req_d) (void)hipFree(c->trial_req_d);
    c->trial_req_h = nullptr; c->trial_out_h = nullptr; c->trial_req_d = nullptr; c->trial_out_dev_alias = nullptr;
    c->trial_cap = 0;
    void *rh = nullptr, *oh = nullptr, *rd = nullptr, *da = nullptr;
    ELLC_HIP(c, hipHostMalloc(&rh, (size_t)B * sizeof(TrialReq), hipHostMallocDefault));
    c->trial_req_h = rh;
    ELLC_HIP(c, hipHostMalloc(&oh, (size_t)B * sizeof(TrialRec), hipHostMallocDefault));
    c->trial_out_h = oh;
    ELLC_HIP(c, hipMalloc(&rd, (size_t)B * sizeof(TrialReq)));
    c->trial_req_d = rd;
    ELLC_HIP(c, hipHostGetDevicePointer(&da, oh, 0));
    c->trial_out_dev_alias = da;
    c->trial_cap = B;
  }
  const size_t need = (size_t)per_launch * tiles;
  if (need > c->trial_partials_cap) {
    if (c->trial_partials_d) (void)hipFree(c->trial_partials_d);
    c->trial_partials_d = nullptr;
    c->trial_partials_cap = 0;
    ELLC_HIP(c, hipMalloc(&c->trial_partials_d, need * sizeof(TrialRec)));
    c->trial_partials_cap = need;
  }
  const size_t need_words = (size_t)per_launch * words;
  if (need_words > c->trial_bits_cap) {
    if (c->trial_bits_d) (void)hipFree(c->trial_bits_d);
    c->trial_bits_d = nullptr;
    c->trial_bits_cap = 0;
    void* bd = nullptr;
    ELLC_HIP(c, hipMalloc(&bd, need_words * sizeof(unsigned)));
    c->trial_bits_d = (unsigned*)bd;
    c->trial_bits_cap = need_words;
  }
  // the destinations' maxAbsGradient planes, built where they are not (as the absorb builds K's)
  std::vector<char>& grad_ok = dst_is_kf ? c->kf_maxgrad_valid : c->fr_maxgrad_valid;
  for (int b = 0; b < B; b++)
    if (!grad_ok[dst[b]]) {
      const ellc_status s = build_maxgrad(c, dst_is_kf != 0, dst[b]);
      if (s != ELLC_OK) return s;
    }
  TrialReq* rq = (TrialReq*)c->trial_req_h;
  for (int b = 0; b < B; b++) {
    rq[b].dst_img = dst_is_kf ? c->kf_tab_h[dst[b]].img : c->fr_tab_h[dst[b]].img;   // (level 0: the first max_keyframes / max_frames entries)
    rq[b].dst_maxgrad = dst_is_kf ? c->kf_maxgrad[dst[b]] : c->fr_maxgrad[dst[b]];
    std::memcpy(rq[b].T, T12 + (size_t)12 * b, 12 * sizeof(float));
    rq[b].src = src[b];
    rq[b].pad_ = 0;
  }
  ELLC_HIP(c, hipMemcpyAsync(c->trial_req_d, c->trial_req_h, (size_t)B * sizeof(TrialReq), hipMemcpyHostToDevice, c->stream));
  TrialArgs a;
  a.m.geom = c->geom_d;
  a.m.kf_tab = c->kf_tab_d;
  a.m.stage = nullptr;
  a.m.tile_counts = nullptr;
  a.m.tile_offsets = nullptr;
  a.m.totals = nullptr;
  a.m.out = nullptr;
  a.m.out_cap = 0u;
  a.m.level = 0;
  a.m.max_kf = c->cfg.max_keyframes;
  a.m.tiles = tiles;
  a.m.B = B;
  a.m.max_var = f->max_var;
  a.m.min_support = f->min_support;
  a.m.support_k2 = f->support_k2;
  a.m.stride = f->stride;
  a.req = (const TrialReq*)c->trial_req_d;
  a.bits = c->trial_bits_d;
  a.partials = (TrialRec*)c->trial_partials_d;
  a.out = (TrialRec*)c->trial_out_dev_alias;
  a.words = (unsigned)words;
  a.photo_gate = photo_gate;
  if (launches_ms) ELLC_HIP(c, hipEventRecord(c->ev0, c->stream));
  for (int first = 0; first < B; first += per_launch) {   // (a record depends on its own request only: the split does not enter it)
    const int n = std::min(per_launch, B - first);
    a.first = first;
    ELLC_HIP(c, hipMemsetAsync(c->trial_bits_d, 0, (size_t)n * words * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(trial_pass, dim3(tiles, n), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(trial_finish, dim3(n), dim3(64), 0, c->stream, a);
  }
  ELLC_HIP(c, hipGetLastError());
  if (launches_ms) ELLC_HIP(c, hipEventRecord(c->ev1, c->stream));
  if (!dst_is_kf) {   // a later upload into a frame slot waits for this reader
    std::vector<char> seen((size_t)c->cfg.max_frames, 0);
    for (int b = 0; b < B; b++)
      if (!seen[dst[b]]) {
        seen[dst[b]] = 1;
        const ellc_status s = mark_frame_use(c, dst[b]);
        if (s != ELLC_OK) return s;
      }
  }
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  std::memcpy(out, c->trial_out_h, (size_t)B * sizeof(TrialRec));
  if (launches_ms) ELLC_HIP(c, hipEventElapsedTime(launches_ms, c->ev0, c->ev1));
  return ELLC_OK;
}

}  // namespace

extern "C" {

ellc_status ellc_keyframe_trial_propagate(ellc_ctx* c, int B, const int* src_kf_slots, int dst_is_keyframe, const int* dst_slots, const float* T12,
                                          const ellc_map_filter* filter, int photo_gate, ellc_trial_propagation* out) {
  return trial_propagate_impl(c, B, src_kf_slots, dst_is_keyframe, dst_slots, T12, filter, photo_gate, out, 0, nullptr);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_trial_propagate(ellc_ctx* c, int B, const int* src_kf_slots, int dst_is_keyframe, const int* dst_slots, const float* T12,
                                         const ellc_map_filter* filter, int photo_gate, ellc_trial_propagation* out, int max_group_requests,
                                         float* launches_ms) {
  float ms = 0.0f;
  const ellc_status s = trial_propagate_impl(c, B, src_kf_slots, dst_is_keyframe, dst_slots, T12, filter, photo_gate, out, max_group_requests, &ms);
  if (launches_ms) *launches_ms = ms;
  return s;
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
