// ellc_keyframe_render_depth (include/ellc_abi.h): the host side of the map render.
// Included at the end of ellc_hip.hip (the library is one translation unit).
#pragma once
#include "ellc_context.hpp"
#include "ellc_kernels_render.hpp"
#include <cmath>
#include <cstring>

using namespace ellc;

namespace {

// the render's scratch, allocated by the first call that needs it (ellc_keyframe_fuse_depth runs the render's kernels on it too: both
// calls are synchronous)
ellc_status render_scratch(ellc_ctx* c) {
  const int MK = c->cfg.max_keyframes;
  const size_t n0 = (size_t)c->geom_h[0].n;
  const size_t blocks0 = (n0 + 255) / 256;
  if (!c->render_nvalid_h) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_stage = 0, o_keys = o_stage + up((size_t)13 * MK * 4), o_depth = o_keys + up(n0 * 8), o_var = o_depth + up(n0 * 4),
                 o_source = o_var + up(n0 * 4), o_agree = o_source + up(n0 * 4), o_int = o_agree + up(n0 * 4), o_counts = o_int + up(n0),
                 bytes = o_counts + up(blocks0 * 4);
    ellc_status s = c->render_stage_h ? ELLC_OK : host_alloc(c, &c->render_stage_h, (size_t)13 * MK);
    if (s != ELLC_OK) return s;
    if (!c->render_block_d) {
      ELLC_HIP(c, hipMalloc(&c->render_block_d, bytes));
      char* p = (char*)c->render_block_d;
      c->render_stage_d = (int*)(p + o_stage);
      c->render_keys_d = (unsigned long long*)(p + o_keys);
      c->render_depth_d = (float*)(p + o_depth);
      c->render_var_d = (float*)(p + o_var);
      c->render_source_d = (int32_t*)(p + o_source);
      c->render_agree_d = (int32_t*)(p + o_agree);
      c->render_intensity_d = (uint8_t*)(p + o_int);
      c->render_block_counts_d = (int*)(p + o_counts);
    }
    int* nh = nullptr;
    s = host_alloc(c, &nh, 1);
    if (s != ELLC_OK) return s;
    void* da = nullptr;
    ELLC_HIP(c, hipHostGetDevicePointer(&da, nh, 0));
    c->render_nvalid_dev_alias = (int*)da;
    c->render_nvalid_h = nh;
  }
  return ELLC_OK;
}

// the requests' slots and transforms, staged and on their way to the device
ellc_status render_stage(ellc_ctx* c, int B, const int* kf_slots, const float* T12) {
  const int MK = c->cfg.max_keyframes;
  for (int b = 0; b < B; b++) c->render_stage_h[b] = kf_slots[b];
  std::memcpy(c->render_stage_h + MK, T12, (size_t)B * 12 * sizeof(float));
  ELLC_HIP(c, hipMemcpyAsync(c->render_stage_d, c->render_stage_h, (size_t)13 * MK * sizeof(int), hipMemcpyHostToDevice, c->stream));
  return ELLC_OK;
}

RenderArgs render_args(ellc_ctx* c, int B, int level, const ellc_map_filter* f, float agree_k2) {
  const int MK = c->cfg.max_keyframes;
  const LevelGeom& g = c->geom_h[level];
  const size_t n = (size_t)g.n;
  RenderArgs a;
  a.m.geom = c->geom_d;
  a.m.kf_tab = c->kf_tab_d;
  a.m.stage = c->render_stage_d;
  a.m.tile_counts = nullptr;
  a.m.tile_offsets = nullptr;
  a.m.totals = nullptr;
  a.m.out = nullptr;
  a.m.out_cap = 0u;
  a.m.level = level;
  a.m.max_kf = MK;
  a.m.tiles = c->tile_begin[level + 1] - c->tile_begin[level];
  a.m.B = B;
  a.m.max_var = f->max_var;
  a.m.min_support = f->min_support;
  a.m.support_k2 = f->support_k2;
  a.m.stride = f->stride;
  a.keys = c->render_keys_d;
  a.depth = c->render_depth_d;
  a.var = c->render_var_d;
  a.source = c->render_source_d;
  a.agree = c->render_agree_d;
  a.intensity = c->render_intensity_d;
  a.block_counts = c->render_block_counts_d;
  a.n_valid = c->render_nvalid_dev_alias;
  a.n = g.n;
  a.blocks = (int)((n + 255) / 256);
  a.agree_k2 = agree_k2;
  return a;
}

// What ellc_keyframe_render_depth and ellc_keyframe_fuse_depth refuse alike (the fusion accepts a destination among its sources).
// Validated first: a refused call leaves the context and every slot as they were (the message is composed only when a call is refused)
ellc_status render_validate(ellc_ctx* c, const char* who, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* f,
                            float agree_k2, int dst, bool dst_may_be_source) {
  if (!c) return ELLC_ERR_BAD_ARG;
  if (!kf_slots || !T12 || !f) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  if (B < 1 || B > c->cfg.max_keyframes || B > 256) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": B out of range");
  if (level < 0 || level >= c->L) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": level out of range");
  const LevelGeom& g = c->geom_h[level];
  if (g.n > (1 << 24)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": more than 2^24 pixels on the level");
  if (f->min_support < 0 || f->min_support > 8 || f->stride < 1 || !(f->support_k2 >= 0.0f) || !std::isfinite(f->support_k2) || std::isnan(f->max_var))
    return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": filter out of range");
  if (!(agree_k2 >= 0.0f) || !std::isfinite(agree_k2)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": agree_k2 negative or not finite");
  if (dst < -1 || dst >= c->cfg.max_keyframes) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": destination slot out of range");
  if (dst >= 0 && level != 0) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": a destination slot takes level 0 only");
  for (int b = 0; b < B; b++)
    if (!slot_ok(kf_slots[b], c->cfg.max_keyframes)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": slot index out of range");
  for (int b = 0; b < B && !dst_may_be_source; b++)
    if (kf_slots[b] == dst) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": the destination slot is also a source");
  for (int b = 0; b < B; b++)
    if (!c->kf_has_image[kf_slots[b]] || !c->kf_has_depth[kf_slots[b]])
      return fail(c, ELLC_ERR_NOT_READY, std::string(who) + ": keyframe slot lacks image or depth");
  return ELLC_OK;
}

// launches_ms (the diagnostic hook only): device time from the preset of the keys to the end of render_agree, HIP events around them
ellc_status render_depth_impl(ellc_ctx* c, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* f, float agree_k2,
                              int dst, float* depth, float* var, int32_t* source, int32_t* agree, uint8_t* intensity, int* n_valid,
                              float* launches_ms) {
  const ellc_status ok = render_validate(c, "ellc_keyframe_render_depth", B, kf_slots, T12, level, f, agree_k2, dst, false);
  if (ok != ELLC_OK) return ok;
  const LevelGeom& g = c->geom_h[level];
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  ellc_status st = render_scratch(c);
  if (st == ELLC_OK) st = render_stage(c, B, kf_slots, T12);
  if (st != ELLC_OK) return st;
  const size_t n0 = (size_t)c->geom_h[0].n, n = (size_t)g.n;
  const RenderArgs a = render_args(c, B, level, f, agree_k2);
  const dim3 grd(a.m.tiles, B), blk(256);
  if (launches_ms) ELLC_HIP(c, hipEventRecord(c->ev0, c->stream));
  ELLC_HIP(c, hipMemsetAsync(c->render_keys_d, 0xff, n * 8, c->stream));
  hipLaunchKernelGGL(render_min, grd, blk, 0, c->stream, a);
  hipLaunchKernelGGL(render_resolve, dim3(a.blocks), blk, 0, c->stream, a);
  hipLaunchKernelGGL(render_finish, dim3(1), blk, 0, c->stream, a);
  hipLaunchKernelGGL(render_agree, grd, blk, 0, c->stream, a);
  ELLC_HIP(c, hipGetLastError());
  if (launches_ms) ELLC_HIP(c, hipEventRecord(c->ev1, c->stream));
  if (depth) ELLC_HIP(c, hipMemcpyAsync(depth, c->render_depth_d, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (var) ELLC_HIP(c, hipMemcpyAsync(var, c->render_var_d, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (source) ELLC_HIP(c, hipMemcpyAsync(source, c->render_source_d, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (agree) ELLC_HIP(c, hipMemcpyAsync(agree, c->render_agree_d, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (intensity) ELLC_HIP(c, hipMemcpyAsync(intensity, c->render_intensity_d, n, hipMemcpyDeviceToHost, c->stream));
  if (dst >= 0) {   // the planes go from device to device; the rest is what ellc_keyframe_set_depth does behind its upload
    const KfLevelDev& k = c->kf_tab_h[dst];
    invalidate_records(c, dst);
    ELLC_HIP(c, hipMemcpyAsync(k.depth, c->render_depth_d, n0 * 4, hipMemcpyDeviceToDevice, c->stream));
    ELLC_HIP(c, hipMemcpyAsync(k.var, c->render_var_d, n0 * 4, hipMemcpyDeviceToDevice, c->stream));
    // a rendered depth is > 0 exactly where a target has a winner: the count render_finish left, read once the stream has got there
    const ellc_status s = finish_depth_planes(c, dst, [&]() {
      (void)hipStreamSynchronize(c->stream);
      return (size_t)*c->render_nvalid_h;
    });
    if (s != ELLC_OK) return s;
  }
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  if (n_valid) *n_valid = *c->render_nvalid_h;
  if (launches_ms) ELLC_HIP(c, hipEventElapsedTime(launches_ms, c->ev0, c->ev1));
  return ELLC_OK;
}

}  // namespace

extern "C" {

ellc_status ellc_keyframe_render_depth(ellc_ctx* c, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* filter,
                                       float agree_k2, int dst_kf_slot, float* depth, float* var, int32_t* source, int32_t* agree,
                                       uint8_t* intensity, int* n_valid) {
  return render_depth_impl(c, B, kf_slots, T12, level, filter, agree_k2, dst_kf_slot, depth, var, source, agree, intensity, n_valid, nullptr);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_render_depth(ellc_ctx* c, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* filter,
                                      float agree_k2, int dst_kf_slot, float* depth, float* var, int32_t* source, int32_t* agree,
                                      uint8_t* intensity, int* n_valid, float* launches_ms) {
  float ms = 0.0f;
  const ellc_status s =
      render_depth_impl(c, B, kf_slots, T12, level, filter, agree_k2, dst_kf_slot, depth, var, source, agree, intensity, n_valid, &ms);
  if (launches_ms) *launches_ms = ms;
  return s;
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
