// ellc_keyframe_render_depth (include/ellc_abi.h): the host side of the map render.
// Included at the end of ellc_hip.hip behind ellc_ring_common.hpp. ellc_keyframe_fuse_depth and ellc_depth_absorb_keyframes build on
// what is here: the validation, the scratch, the staging, the arguments, and the enqueue / download / write-back steps of a view.
#pragma once
#include "ellc_ring_common.hpp"
#include "ellc_kernels_render.hpp"

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
    const size_t o_stage = 0, o_keys = o_stage + up((size_t)15 * MK * 4), o_depth = o_keys + up(n0 * 8), o_var = o_depth + up(n0 * 4),
                 o_source = o_var + up(n0 * 4), o_agree = o_source + up(n0 * 4), o_int = o_agree + up(n0 * 4), o_counts = o_int + up(n0),
                 bytes = o_counts + up(blocks0 * 4);
    ellc_status s = c->render_stage_h ? ELLC_OK : host_alloc(c, &c->render_stage_h, (size_t)15 * MK);
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

// the requests' slots, transforms and lights (NULL: (1, 0) each; the absorb's gate alone reads them), staged and on their way to the device
ellc_status render_stage(ellc_ctx* c, int B, const int* kf_slots, const float* T12, const float* light = nullptr) {
  const int MK = c->cfg.max_keyframes;
  for (int b = 0; b < B; b++) c->render_stage_h[b] = kf_slots[b];
  std::memcpy(c->render_stage_h + MK, T12, (size_t)B * 12 * sizeof(float));
  float* l = (float*)(c->render_stage_h + (size_t)13 * MK);
  for (int b = 0; b < B; b++) {
    l[2 * b] = light ? light[2 * b] : 1.0f;
    l[2 * b + 1] = light ? light[2 * b + 1] : 0.0f;
  }
  ELLC_HIP(c, hipMemcpyAsync(c->render_stage_d, c->render_stage_h, (size_t)15 * MK * sizeof(int), hipMemcpyHostToDevice, c->stream));
  return ELLC_OK;
}

RenderArgs render_args(ellc_ctx* c, int B, int level, const ellc_map_filter* f, float agree_k2) {
  const LevelGeom& g = c->geom_h[level];
  const size_t n = (size_t)g.n;
  RenderArgs a;
  a.v = ring_view(c, level, f);
  a.stage = c->render_stage_d;
  a.B = B;
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
// the number of requests a call over the render's staging takes
bool render_B_ok(const ellc_ctx* c, int B) { return B >= 1 && B <= c->cfg.max_keyframes && B <= 256; }

ellc_status render_validate(ellc_ctx* c, const char* who, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* f,
                            float agree_k2, int dst, bool dst_may_be_source) {
  if (!c) return ELLC_ERR_BAD_ARG;
  if (!kf_slots || !T12 || !f) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  if (!render_B_ok(c, B)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": B out of range");
  if (level < 0 || level >= c->L) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": level out of range");
  const LevelGeom& g = c->geom_h[level];
  if (g.n > (1 << 24)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": more than 2^24 pixels on the level");
  ELLC_TRY(ring_check_filter(c, who, f));
  if (!(agree_k2 >= 0.0f) || !std::isfinite(agree_k2)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": agree_k2 negative or not finite");
  if (dst < -1 || dst >= c->cfg.max_keyframes) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": destination slot out of range");
  if (dst >= 0 && level != 0) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": a destination slot takes level 0 only");
  ELLC_TRY(ring_check_slots(c, who, B, kf_slots, c->cfg.max_keyframes));
  for (int b = 0; b < B && !dst_may_be_source; b++)
    if (kf_slots[b] == dst) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": the destination slot is also a source");
  return ring_check_ready(c, who, B, kf_slots);
}

// the preset of the keys and the three launches that leave the winners' planes and their count (grd: tiles of the level x B)
ellc_status render_enqueue_view(ellc_ctx* c, const RenderArgs& a, dim3 grd) {
  ELLC_HIP(c, hipMemsetAsync(c->render_keys_d, 0xff, (size_t)a.n * 8, c->stream));
  hipLaunchKernelGGL(render_min, grd, dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(render_resolve, dim3(a.blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(render_finish, dim3(1), dim3(256), 0, c->stream, a);
  return ELLC_OK;
}

// the view's planes of n pixels to the caller, those it asked for
ellc_status render_download(ellc_ctx* c, size_t n, float* depth, float* var, int32_t* source, int32_t* agree, uint8_t* intensity) {
  if (depth) ELLC_HIP(c, hipMemcpyAsync(depth, c->render_depth_d, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (var) ELLC_HIP(c, hipMemcpyAsync(var, c->render_var_d, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (source) ELLC_HIP(c, hipMemcpyAsync(source, c->render_source_d, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (agree) ELLC_HIP(c, hipMemcpyAsync(agree, c->render_agree_d, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (intensity) ELLC_HIP(c, hipMemcpyAsync(intensity, c->render_intensity_d, n, hipMemcpyDeviceToHost, c->stream));
  return ELLC_OK;
}

// The level-0 view into keyframe slot dst, behind every kernel that read the slot: the planes go from device to device; the rest is
// what ellc_keyframe_set_depth does behind its upload.
ellc_status render_store_dst(ellc_ctx* c, int dst) {
  const size_t n0 = (size_t)c->geom_h[0].n;
  const KfLevelDev& k = c->kf_tab_h[dst];
  invalidate_records(c, dst);
  ELLC_HIP(c, hipMemcpyAsync(k.depth, c->render_depth_d, n0 * 4, hipMemcpyDeviceToDevice, c->stream));
  ELLC_HIP(c, hipMemcpyAsync(k.var, c->render_var_d, n0 * 4, hipMemcpyDeviceToDevice, c->stream));
  // a depth of the view is > 0 exactly where a target has a winner: the count render_finish left, read once the stream has got there
  return finish_depth_planes(c, dst, [&]() {
    (void)hipStreamSynchronize(c->stream);
    return (size_t)*c->render_nvalid_h;
  });
}

// launches_ms (the diagnostic hook only): device time from the preset of the keys to the end of render_agree, HIP events around them
ellc_status render_depth_impl(ellc_ctx* c, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* f, float agree_k2,
                              int dst, float* depth, float* var, int32_t* source, int32_t* agree, uint8_t* intensity, int* n_valid,
                              float* launches_ms) {
  const ellc_status ok = render_validate(c, "ellc_keyframe_render_depth", B, kf_slots, T12, level, f, agree_k2, dst, false);
  if (ok != ELLC_OK) return ok;
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  ELLC_TRY(render_scratch(c));
  ELLC_TRY(render_stage(c, B, kf_slots, T12));
  const RenderArgs a = render_args(c, B, level, f, agree_k2);
  const dim3 grd(a.v.tiles, B);
  LaunchTimer t(c, launches_ms);
  ELLC_TRY(t.begin());
  ELLC_TRY(render_enqueue_view(c, a, grd));
  hipLaunchKernelGGL(render_agree, grd, dim3(256), 0, c->stream, a);
  ELLC_HIP(c, hipGetLastError());
  ELLC_TRY(t.end());
  ELLC_TRY(render_download(c, (size_t)a.n, depth, var, source, agree, intensity));
  if (dst >= 0) ELLC_TRY(render_store_dst(c, dst));
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  if (n_valid) *n_valid = *c->render_nvalid_h;
  return t.read();
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
  return ring_profiled(launches_ms, [&](float* ms) {
    return render_depth_impl(c, B, kf_slots, T12, level, filter, agree_k2, dst_kf_slot, depth, var, source, agree, intensity, n_valid, ms);
  });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
