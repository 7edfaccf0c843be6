// ellc_keyframe_fuse_depth (include/ellc_abi.h): the host side of the fused view.
// Included at the end of ellc_hip.hip, behind ellc_render_impl.hpp: the render's validation, scratch, staging and its enqueue / download /
// write-back steps are used as they are.
#pragma once
#include "ellc_render_impl.hpp"
#include "ellc_kernels_fuse.hpp"
#include <climits>

using namespace ellc;

namespace {

// the fusion's scratch of its own, allocated by the first call that needs it (ellc_depth_absorb_keyframes uses it too: both calls are synchronous)
ellc_status fuse_scratch(ellc_ctx* c) {
  const size_t n0 = (size_t)c->geom_h[0].n;
  if (!c->fuse_totals_h) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t tiles0 = (size_t)(c->tile_begin[1] - c->tile_begin[0]), blocks0 = (n0 + 255) / 256;
    const size_t o_cursor = 0, o_merged = o_cursor + up(n0 * 4), o_sums = o_merged + up(n0 * 4), o_counts = o_sums + up(tiles0 * 8),
                 bytes = o_counts + up(blocks0 * 4);
    if (!c->fuse_block_d) {
      ELLC_HIP(c, hipMalloc(&c->fuse_block_d, bytes));
      char* p = (char*)c->fuse_block_d;
      c->fuse_cursor_d = (unsigned*)(p + o_cursor);
      c->fuse_merged_d = (int32_t*)(p + o_merged);
      c->fuse_tile_sums_d = (unsigned long long*)(p + o_sums);
      c->fuse_block_counts_d = (int*)(p + o_counts);
    }
    long long* th = nullptr;
    const ellc_status st = host_alloc(c, &th, 2);
    if (st != ELLC_OK) return st;
    void* da = nullptr;
    ELLC_HIP(c, hipHostGetDevicePointer(&da, th, 0));
    c->fuse_totals_dev_alias = (long long*)da;
    c->fuse_totals_h = th;
  }
  return ELLC_OK;
}

// the bit per source pixel of every request: grown in front of a call's first enqueue
ellc_status fuse_mask_reserve(ellc_ctx* c, size_t mask_words) {
  return dev_grow(c, (void**)&c->fuse_mask_d, &c->fuse_mask_cap, mask_words, sizeof(unsigned long long));
}

// the list of candidate ids: grown once the call's total is known (nothing of this context is running: the stream was synchronised).
// Headroom of a half: totals that creep up from call to call do not allocate every time.
ellc_status fuse_list_reserve(ellc_ctx* c, size_t total) {
  return dev_grow(c, (void**)&c->fuse_list_d, &c->fuse_list_cap, total, sizeof(uint32_t), total / 2);
}

// launches_ms (the diagnostic hook only): device time from the preset of the keys to the end of fuse_finish, HIP events around them. The
// host's read of the list's size (one synchronisation, and the list's growth when it has to grow) lies inside that window.
ellc_status fuse_depth_impl(ellc_ctx* c, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* f, float agree_k2,
                            int max_merge, int dst, float* depth, float* var, int32_t* source, int32_t* agree, int32_t* merged,
                            uint8_t* intensity, int* n_valid, int* n_fused, float* launches_ms) {
  // the destination may be one of the sources: every kernel has read the slots before the copies into the destination, in stream order
  const ellc_status ok = render_validate(c, "ellc_keyframe_fuse_depth", B, kf_slots, T12, level, f, agree_k2, dst, true);
  if (ok != ELLC_OK) return ok;
  if (max_merge < 0 || max_merge > ELLC_FUSE_MAX_MERGE) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_fuse_depth: max_merge out of range");
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  ELLC_TRY(render_scratch(c));
  ELLC_TRY(fuse_scratch(c));
  FuseArgs a;
  a.r = render_args(c, B, level, f, agree_k2);
  const size_t mask_words = (size_t)B * (size_t)a.r.v.tiles * 32;   // 8 steps x 4 waves per (request, tile)
  if (max_merge > 0) ELLC_TRY(fuse_mask_reserve(c, mask_words));
  ELLC_TRY(render_stage(c, B, kf_slots, T12));
  a.mask = c->fuse_mask_d;
  a.cursor = c->fuse_cursor_d;
  a.tile_sums = c->fuse_tile_sums_d;
  a.list = c->fuse_list_d;
  a.list_cap = 0u;
  a.merged = c->fuse_merged_d;
  a.block_counts = c->fuse_block_counts_d;
  a.totals = c->fuse_totals_dev_alias;
  a.max_merge = max_merge;
  const dim3 grd(a.r.v.tiles, B), blk(256);
  LaunchTimer t(c, launches_ms);
  ELLC_TRY(t.begin());
  ELLC_TRY(render_enqueue_view(c, a.r, grd));
  if (max_merge == 0) hipLaunchKernelGGL(render_agree, grd, blk, 0, c->stream, a.r);   // (without a merge nothing reads a list: the render's planes go out as they are)
  if (max_merge > 0) {
    hipLaunchKernelGGL(fuse_agree, grd, blk, 0, c->stream, a);
    hipLaunchKernelGGL(fuse_tile_sums, dim3(a.r.v.tiles), blk, 0, c->stream, a);
    hipLaunchKernelGGL(fuse_offsets, dim3(a.r.v.tiles), blk, 0, c->stream, a);
    ELLC_HIP(c, hipGetLastError());
    ELLC_HIP(c, hipStreamSynchronize(c->stream));
    const long long total = c->fuse_totals_h[0];
    // nothing of a slot has been touched yet
    if (total > (long long)INT_MAX) return fail(c, ELLC_ERR_CAPACITY, "ellc_keyframe_fuse_depth: more than 2^31 - 1 agreeing candidates");
    ELLC_TRY(fuse_list_reserve(c, (size_t)total));
    a.list = c->fuse_list_d;
    a.list_cap = (unsigned)total;
    if (total > 0) hipLaunchKernelGGL(fuse_scatter, grd, blk, 0, c->stream, a);
  }
  hipLaunchKernelGGL(fuse_merge, dim3(a.r.blocks), blk, 0, c->stream, a);
  hipLaunchKernelGGL(fuse_finish, dim3(1), blk, 0, c->stream, a);
  ELLC_HIP(c, hipGetLastError());
  ELLC_TRY(t.end());
  ELLC_TRY(render_download(c, (size_t)a.r.n, depth, var, source, agree, intensity));
  if (merged) ELLC_HIP(c, hipMemcpyAsync(merged, c->fuse_merged_d, (size_t)a.r.n * 4, hipMemcpyDeviceToHost, c->stream));
  // a fused depth is > 0 exactly where a target has a winner (1 / id_t of positive terms), as a rendered one
  if (dst >= 0) ELLC_TRY(render_store_dst(c, dst));
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  if (n_valid) *n_valid = *c->render_nvalid_h;
  if (n_fused) *n_fused = (int)c->fuse_totals_h[1];
  return t.read();
}

}  // namespace

extern "C" {

ellc_status ellc_keyframe_fuse_depth(ellc_ctx* c, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* filter,
                                     float agree_k2, int max_merge, int dst_kf_slot, float* depth, float* var, int32_t* source, int32_t* agree,
                                     int32_t* merged, uint8_t* intensity, int* n_valid, int* n_fused) {
  return fuse_depth_impl(c, B, kf_slots, T12, level, filter, agree_k2, max_merge, dst_kf_slot, depth, var, source, agree, merged, intensity, n_valid,
                         n_fused, nullptr);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_fuse_depth(ellc_ctx* c, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* filter,
                                    float agree_k2, int max_merge, int dst_kf_slot, float* depth, float* var, int32_t* source, int32_t* agree,
                                    int32_t* merged, uint8_t* intensity, int* n_valid, int* n_fused, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) {
    return fuse_depth_impl(c, B, kf_slots, T12, level, filter, agree_k2, max_merge, dst_kf_slot, depth, var, source, agree, merged, intensity, n_valid,
                           n_fused, ms);
  });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
