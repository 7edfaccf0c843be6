// ellc_depth_absorb_keyframes, ellc_depth_restart_from_keyframes and their _lit forms (include/ellc_abi.h): the host side of the fold of keyframe slots into the live depth map.
// Included at the end of ellc_hip.hip, behind ellc_fuse_impl.hpp and ellc_depth_impl.hpp: the render's validation, scratch and staging,
// the fusion's scratch, scan kernels and list, and the depth map's regularisation and export are used as they are (the fold writes the
// live map, so the render's enqueue / download / write-back steps do not apply).
#pragma once
#include "ellc_fuse_impl.hpp"
#include "ellc_kernels_absorb.hpp"

using namespace ellc;

namespace {

// launches_ms (the diagnostic hook only): device time from the preset of the count plane to the end of absorb_finish (finalise's
// launches are not inside), HIP events around them. The host's read of the list's size lies inside that window, as in the fusion.
// restart_slot >= 0: ellc_depth_restart_from_keyframes. That slot takes K's place, the state is wiped in front of the fold (behind
// everything that can refuse the call) and `finalise` runs createKeyFrame's tail, whose factor goes to *rescale_factor.
// light: the _lit entry points' [B][2] (gain, offset) of absorb_photo's residual; NULL, the unlit entry points too: (1, 0) each.
ellc_status absorb_impl(ellc_ctx* c, int B, const int* kf_slots, const float* T12, const float* light, const ellc_map_filter* f, const ellc_absorb_params* p,
                        ellc_absorb_stats* out, float* launches_ms, int restart_slot = -1, float* rescale_factor = nullptr, bool lit = false) {
  const bool restart = restart_slot >= 0;
  const char* who = restart ? (lit ? "ellc_depth_restart_from_keyframes_lit" : "ellc_depth_restart_from_keyframes")
                            : (lit ? "ellc_depth_absorb_keyframes_lit" : "ellc_depth_absorb_keyframes");
  if (!c) return ELLC_ERR_BAD_ARG;
  if (!p) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  // (the parameters first: a bad argument is reported in front of a slot that is not ready)
  if (p->max_fold < 1 || p->max_fold > ELLC_FUSE_MAX_MERGE) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": max_fold out of range");
  if (p->src_validity < 0 || p->src_validity > 255) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": src_validity out of range");
  if (p->photo_gate < 0 || p->photo_gate > 1 || p->finalise < 0 || p->finalise > 1) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": photo_gate / finalise not 0 or 1");
  // (a light that is not finite is a bad argument too, in front of the slots; render_validate refuses a B out of range)
  if (render_B_ok(c, B)) ELLC_TRY(light_check(c, who, B, light));
  ELLC_TRY(render_validate(c, who, B, kf_slots, T12, 0, f, p->agree_k2, restart_slot, !restart));   // (the new keyframe is no source)
  if (restart) {
    if (!c->kf_has_image[restart_slot]) return fail(c, ELLC_ERR_NOT_READY, std::string(who) + ": the new keyframe slot has no image");
  } else if (!c->dm_ready || c->dm_kf_slot < 0)
    return fail(c, ELLC_ERR_NOT_READY, std::string(who) + ": call ellc_depth_set_state and ellc_depth_set_keyframe first");
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  const int K = restart ? restart_slot : c->dm_kf_slot;
  ELLC_TRY(render_scratch(c));
  ELLC_TRY(fuse_scratch(c));
  const size_t n0 = (size_t)c->geom_h[0].n, blocks0 = (n0 + 255) / 256;
  if (!c->absorb_stats_h) {
    if (!c->absorb_block_d) ELLC_HIP(c, hipMalloc(&c->absorb_block_d, (64 + blocks0 * ELLC_ABSORB_FOLD_COUNTS) * sizeof(int)));
    int32_t* sh = nullptr;
    ELLC_TRY(host_alloc(c, &sh, 16));
    void* da = nullptr;
    ELLC_HIP(c, hipHostGetDevicePointer(&da, sh, 0));
    c->absorb_stats_dev_alias = (int32_t*)da;
    c->absorb_stats_h = sh;
  }
  // K's maxAbsGradient: the gate reads it, and so does the regularisation behind the fold (as ellc_depth_do_regularization builds it)
  if ((p->photo_gate || p->finalise) && !c->kf_maxgrad_valid[K]) ELLC_TRY(build_maxgrad(c, true, K));
  AbsorbArgs a;
  a.f.r = render_args(c, B, 0, f, p->agree_k2);
  const size_t mask_words = (size_t)B * (size_t)a.f.r.v.tiles * 32;   // 8 steps x 4 waves per (request, tile)
  ELLC_TRY(fuse_mask_reserve(c, mask_words));
  ELLC_TRY(render_stage(c, B, kf_slots, T12, light));
  a.f.mask = c->fuse_mask_d;
  a.f.cursor = c->fuse_cursor_d;
  a.f.tile_sums = c->fuse_tile_sums_d;
  a.f.list = c->fuse_list_d;
  a.f.list_cap = 0u;
  a.f.merged = nullptr;
  a.f.block_counts = nullptr;
  a.f.totals = c->fuse_totals_dev_alias;
  a.f.max_merge = 0;
  a.s = c->dm_cur;
  a.k_img = c->kf_tab_h[K].img;
  a.k_maxgrad = c->kf_maxgrad[K];
  a.mark_counts = (int*)c->absorb_block_d;
  a.fold_counts = (int*)c->absorb_block_d + 64;
  a.stats = c->absorb_stats_dev_alias;
  a.max_fold = p->max_fold;
  a.photo_gate = p->photo_gate;
  a.src_validity = p->src_validity;
  const dim3 grd(a.f.r.v.tiles, B), blk(256);
  LaunchTimer t(c, launches_ms);
  ELLC_TRY(t.begin());
  ELLC_HIP(c, hipMemsetAsync(c->render_agree_d, 0, n0 * 4, c->stream));
  ELLC_HIP(c, hipMemsetAsync(a.mark_counts, 0, 4 * sizeof(int), c->stream));
  hipLaunchKernelGGL(absorb_mark, grd, blk, 0, c->stream, a);
  hipLaunchKernelGGL(fuse_tile_sums, dim3(a.f.r.v.tiles), blk, 0, c->stream, a.f);
  hipLaunchKernelGGL(fuse_offsets, dim3(a.f.r.v.tiles), blk, 0, c->stream, a.f);
  ELLC_HIP(c, hipGetLastError());
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  const long long total = c->fuse_totals_h[0];
  // nothing of the state has been touched yet
  if (total > (long long)INT_MAX) return fail(c, ELLC_ERR_CAPACITY, std::string(who) + ": more than 2^31 - 1 candidates");
  ELLC_TRY(fuse_list_reserve(c, (size_t)total));
  a.f.list = c->fuse_list_d;
  a.f.list_cap = (unsigned)total;
  const int old_slot = c->dm_kf_slot;
  if (restart) {   // from here on the call cannot be refused: the map is re-seated on the new keyframe, EMPTY
    hipLaunchKernelGGL(absorb_wipe, dim3(a.f.r.blocks), blk, 0, c->stream, a.s, a.f.r.n);
    c->dm_kf_slot = K;
    c->dm_ready = true;
  }
  // a device error part-way through a restart: the map no longer matches either keyframe (as in ellc_depth_create_keyframe)
  auto broken = [&](ellc_status s) {
    if (restart) {
      c->dm_kf_slot = old_slot;
      c->dm_ready = false;
    }
    return s;
  };
  if (total > 0) hipLaunchKernelGGL(absorb_scatter, grd, blk, 0, c->stream, a);
  hipLaunchKernelGGL(absorb_fold, dim3(a.f.r.blocks), blk, 0, c->stream, a);
  hipLaunchKernelGGL(absorb_finish, dim3(1), blk, 0, c->stream, a);
  if (hipGetLastError() != hipSuccess) return broken(fail(c, ELLC_ERR_HIP, std::string(who) + ": a launch failed"));
  ELLC_TRY(t.end());
  float factor = 1.0f;
  if (p->finalise && restart) {   // createKeyFrame's tail, as ellc_depth_create_keyframe enqueues it
    const ellc_status st = do_create_keyframe_tail(c, &factor);
    if (st != ELLC_OK) return broken(st);
  } else if (p->finalise) {   // ellc_depth_do_regularization(ctx, 0) and ellc_depth_update_depth_image(ctx), as they enqueue them
    ELLC_TRY(do_fill_regularize(c, 0));
    ELLC_TRY(do_update_depth_image(c));
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess) return broken(fail(c, ELLC_ERR_HIP, std::string(who) + ": the stream failed"));
  if (rescale_factor) *rescale_factor = factor;
  if (out) std::memcpy(out, c->absorb_stats_h, sizeof(ellc_absorb_stats));
  return t.read();
}

}  // namespace

extern "C" {

void ellc_absorb_default_params(ellc_absorb_params* p) {
  if (!p) return;
  p->agree_k2 = 1.0f;
  p->max_fold = ELLC_FUSE_MAX_MERGE;
  p->photo_gate = 1;
  p->src_validity = 20;   // initializeRandomly's counter
  p->finalise = 1;
}

ellc_status ellc_depth_absorb_keyframes(ellc_ctx* c, int B, const int* kf_slots, const float* T12, const ellc_map_filter* filter,
                                        const ellc_absorb_params* params, ellc_absorb_stats* out) {
  return absorb_impl(c, B, kf_slots, T12, nullptr, filter, params, out, nullptr);
}

ellc_status ellc_depth_absorb_keyframes_lit(ellc_ctx* c, int B, const int* kf_slots, const float* T12, const float* light, const ellc_map_filter* filter,
                                            const ellc_absorb_params* params, ellc_absorb_stats* out) {
  return absorb_impl(c, B, kf_slots, T12, light, filter, params, out, nullptr, -1, nullptr, true);
}

ellc_status ellc_depth_restart_from_keyframes(ellc_ctx* c, int new_kf_slot, int B, const int* kf_slots, const float* T12, const ellc_map_filter* filter,
                                              const ellc_absorb_params* params, float* rescale_factor, ellc_absorb_stats* out) {
  if (!c) return ELLC_ERR_BAD_ARG;
  if (!slot_ok(new_kf_slot, c->cfg.max_keyframes)) return fail(c, ELLC_ERR_BAD_ARG, "ellc_depth_restart_from_keyframes: new keyframe slot out of range");
  return absorb_impl(c, B, kf_slots, T12, nullptr, filter, params, out, nullptr, new_kf_slot, rescale_factor);
}

ellc_status ellc_depth_restart_from_keyframes_lit(ellc_ctx* c, int new_kf_slot, int B, const int* kf_slots, const float* T12, const float* light,
                                                  const ellc_map_filter* filter, const ellc_absorb_params* params, float* rescale_factor,
                                                  ellc_absorb_stats* out) {
  if (!c) return ELLC_ERR_BAD_ARG;
  if (!slot_ok(new_kf_slot, c->cfg.max_keyframes)) return fail(c, ELLC_ERR_BAD_ARG, "ellc_depth_restart_from_keyframes_lit: new keyframe slot out of range");
  return absorb_impl(c, B, kf_slots, T12, light, filter, params, out, nullptr, new_kf_slot, rescale_factor, true);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_depth_absorb(ellc_ctx* c, int B, const int* kf_slots, const float* T12, const ellc_map_filter* filter,
                                      const ellc_absorb_params* params, ellc_absorb_stats* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) { return absorb_impl(c, B, kf_slots, T12, nullptr, filter, params, out, ms); });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
