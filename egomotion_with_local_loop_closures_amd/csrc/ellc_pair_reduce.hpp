// The reduction tail of the ring's pair calls (ellc_keyframe_depth_consistency, ellc_keyframe_sim3_step, ellc_keyframe_trial_propagate,
// ellc_keyframe_light_step, ellc_keyframe_sim3_step_lit, ellc_keyframe_joint_step's view pairs) and of the stats of ellc_keyframe_refine_depth and
// its kin (_sweep_depth, _cull_depth, _joint_step / _apply: one request, a partial per 256-pixel block; what their pixel kernels share
// in front of this tail is in ellc_kernels_views.hpp):
// a pass kernel leaves one partial record per (request, tile), a finish kernel sums a request's tiles. No waiting between blocks, no
// floating-point atomics. A record type takes part through three plain overloads in namespace ellc:
//   rec_zero(Rec&)             every field zero
//   rec_add(Rec&, const Rec&)  a += b, field by field (one rounding per double field)
//   rec_wave_sum(Rec&)         the sum over the wave's 64 lanes, in every lane: a butterfly, so the order of the additions is fixed by
//                              the lane numbers alone (lane l and lane l ^ m add the same two values: every lane ends with the same bits)
// The order of every addition: j = 0..7 within a thread (the pass kernel's loop), the butterfly, the block's four waves ascending;
// then per lane the tiles l, l + 64, ... ascending, and the butterfly again. It follows from the level's size alone.
#pragma once
#include <hip/hip_runtime.h>

namespace ellc {

// The end of a 256-thread pass kernel: the wave leaders leave their wave's sum in LDS, thread 0 adds the four waves in ascending order
// and stores the block's record.
template <class Rec>
__device__ __forceinline__ void pair_store_block(Rec& r, Rec* dst) {
  rec_wave_sum(r);
  __shared__ Rec ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    Rec t = ws[0];
    rec_add(t, ws[1]);
    rec_add(t, ws[2]);
    rec_add(t, ws[3]);
    *dst = t;
  }
}

// The body of a finish kernel, one wave per request of the launch (blockIdx.x; request `first` + blockIdx.x of the call): lane l adds
// the request's tiles l, l + 64, ... in ascending order, the butterfly adds the lanes (gn_quality_finish's discipline). `out` is the
// call's records in pinned host memory.
template <class Rec>
__device__ __forceinline__ void pair_finish(const Rec* partials, int tiles, Rec* out, int first) {
  const Rec* part = partials + blockIdx.x * (unsigned)tiles;
  Rec r;
  rec_zero(r);
  for (int k = (int)threadIdx.x; k < tiles; k += 64) rec_add(r, part[k]);
  rec_wave_sum(r);
  if (threadIdx.x == 0) out[(unsigned)first + blockIdx.x] = r;
}

}  // namespace ellc
