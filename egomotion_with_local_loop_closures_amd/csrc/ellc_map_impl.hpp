// ellc_keyframe_map_points (include/ellc_abi.h): the host side of the map export.
// Included at the end of ellc_hip.hip behind ellc_ring_common.hpp: its refusals, view, timer and grow-only buffer are used here.
#pragma once
#include "ellc_ring_common.hpp"
#include <climits>

using namespace ellc;

static_assert(sizeof(MapRec) == sizeof(ellc_map_point) && sizeof(ellc_map_point) == 24 && offsetof(MapRec, var) == offsetof(ellc_map_point, var) &&
                  offsetof(MapRec, px) == offsetof(ellc_map_point, px) && offsetof(MapRec, intensity) == offsetof(ellc_map_point, intensity) &&
                  offsetof(MapRec, support) == offsetof(ellc_map_point, support) && offsetof(MapRec, source) == offsetof(ellc_map_point, source),
              "MapRec mirrors ellc_map_point");

namespace {

// launches_ms (the diagnostic hook only): device time of the three launches, HIP events around count + scan and around the scatter
ellc_status map_points_impl(ellc_ctx* c, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* f, ellc_map_point* out,
                            int capacity, int* counts, int* total, float* launches_ms) {
  const char* who = "ellc_keyframe_map_points";
  if (!c) return ELLC_ERR_BAD_ARG;
  if (!kf_slots || !T12 || !f) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_map_points: null pointer");
  if (B < 1 || B > c->cfg.max_keyframes || B > 65535) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_map_points: B out of range");
  if (level < 0 || level >= c->L) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_map_points: level out of range");
  if (out && capacity < 0) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_map_points: negative capacity");
  ELLC_TRY(ring_check_filter(c, who, f));
  ELLC_TRY(ring_check_slots(c, who, B, kf_slots, c->cfg.max_keyframes));
  ELLC_TRY(ring_check_ready(c, who, B, kf_slots));
  const LevelGeom& g = c->geom_h[level];
  if ((long long)B * g.n > (long long)INT_MAX) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_map_points: B x pixels of the level does not fit the int total");
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  const int MK = c->cfg.max_keyframes;
  if (!c->map_totals_h) {
    const size_t tiles0 = (size_t)(c->tile_begin[1] - c->tile_begin[0]);   // level 0 has the most tiles
    ellc_status s = host_alloc(c, &c->map_stage_h, (size_t)13 * MK);
    if (s == ELLC_OK) s = dev_alloc(c, &c->map_stage_d, (size_t)13 * MK);
    if (s == ELLC_OK) s = dev_alloc(c, &c->map_tile_counts_d, (size_t)MK * tiles0);
    if (s == ELLC_OK) s = dev_alloc(c, &c->map_tile_offsets_d, (size_t)MK * tiles0);
    int* th = nullptr;
    if (s == ELLC_OK) s = host_alloc(c, &th, (size_t)MK + 1);
    if (s != ELLC_OK) return s;
    void* da = nullptr;
    ELLC_HIP(c, hipHostGetDevicePointer(&da, th, 0));
    c->map_totals_dev_alias = (int*)da;
    c->map_totals_h = th;
  }
  for (int b = 0; b < B; b++) c->map_stage_h[b] = kf_slots[b];
  std::memcpy(c->map_stage_h + MK, T12, (size_t)B * 12 * sizeof(float));
  ELLC_HIP(c, hipMemcpyAsync(c->map_stage_d, c->map_stage_h, (size_t)13 * MK * sizeof(int), hipMemcpyHostToDevice, c->stream));
  MapArgs a;
  a.v = ring_view(c, level, f);
  a.stage = c->map_stage_d;
  a.tile_counts = c->map_tile_counts_d;
  a.tile_offsets = c->map_tile_offsets_d;
  a.totals = c->map_totals_dev_alias;
  a.out = nullptr;
  a.out_cap = 0u;
  a.B = B;
  const dim3 grd(a.v.tiles, B), blk(256);
  LaunchTimer t(c, launches_ms);   // two windows: count + scan, and the scatter
  ELLC_TRY(t.begin());
  hipLaunchKernelGGL(map_count, grd, blk, 0, c->stream, a);
  hipLaunchKernelGGL(map_scan, dim3(1), blk, 0, c->stream, a);
  ELLC_HIP(c, hipGetLastError());
  ELLC_TRY(t.end());
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  ELLC_TRY(t.read());
  const int sum = c->map_totals_h[MK];
  if (counts) std::memcpy(counts, c->map_totals_h, (size_t)B * sizeof(int));
  if (total) *total = sum;
  if (!out) return ELLC_OK;   // the sizing call
  if (sum > capacity) return fail(c, ELLC_ERR_CAPACITY, "ellc_keyframe_map_points: more points than the buffer holds");
  if (sum == 0) return ELLC_OK;
  // (nothing of this context is running: the stream was synchronised above)
  ELLC_TRY(dev_grow(c, &c->map_out_d, &c->map_out_cap, (size_t)sum, sizeof(MapRec)));
  a.out = (MapRec*)c->map_out_d;
  a.out_cap = (unsigned)sum;
  ELLC_TRY(t.begin());
  hipLaunchKernelGGL(map_scatter, grd, blk, 0, c->stream, a);
  ELLC_HIP(c, hipGetLastError());
  ELLC_TRY(t.end());
  ELLC_HIP(c, hipMemcpyAsync(out, c->map_out_d, (size_t)sum * sizeof(MapRec), hipMemcpyDeviceToHost, c->stream));
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  return t.read();
}

}  // namespace

extern "C" {

ellc_status ellc_keyframe_map_points(ellc_ctx* c, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* filter,
                                     ellc_map_point* out, int capacity, int* counts, int* total) {
  return map_points_impl(c, B, kf_slots, T12, level, filter, out, capacity, counts, total, nullptr);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_map_points(ellc_ctx* c, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* filter,
                                    ellc_map_point* out, int capacity, int* counts, int* total, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) { return map_points_impl(c, B, kf_slots, T12, level, filter, out, capacity, counts, total, ms); });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
