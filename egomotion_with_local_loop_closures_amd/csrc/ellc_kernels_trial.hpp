// ellc_keyframe_trial_propagate: "if THIS keyframe slot's map were propagated into THAT image at THIS transform, how much map would there
// be?", for B pairs in one call and without touching the live depth map. Steps 1-4 of ellc_depth_absorb_keyframes with the destination's
// level-0 image and maxAbsGradient plane in K's role, as a reduction: map_keep, render_candidate, absorb_interior and absorb_photo decide
// every source pixel (nothing of them is restated here). consist_pass's shape: trial_pass leaves one partial record per (request, tile),
// trial_finish sums a request's tiles (ellc_pair_reduce.hpp holds the tail of both). The DISTINCT targets among the candidates are counted through one bit per (request, target) in
// device scratch: whoever finds its bit clear counts the target (an integer atomic OR: the total does not depend on the arrival order).
// No waiting between blocks, integer atomics only, no floating-point atomics.
// ellc_keyframe_trial_propagate_lit is the same pass over the wider record TrialRecLit (trial_pass_body's template parameter, one kernel
// body): the residual against the request's light, and the five sums of the straight-line fit of Iw on Is over the interior pixels.
#pragma once
#include "ellc_kernels_absorb.hpp"
#include "ellc_pair_reduce.hpp"

namespace ellc {

// ellc_trial_propagation as the kernels write it; the partial record of a tile has the same layout
struct TrialRec {
  double sum_r2, sum_abs_r;
  int32_t n_kept, n_in_view, n_interior, n_low_grad, n_candidates, n_targets;
  int32_t reserved[2];
};

// ellc_trial_propagation_lit as the kernels write it: the narrow record, then the sums of Is, Iw, Is * Is, Is * Iw and Iw * Iw over the
// pixels counted in n_interior, and their number
struct TrialRecLit {
  TrialRec t;
  double fit[5];
  int32_t n_fit, reserved;
};

// one request as the host stages it (device copy of the pinned record)
struct TrialReq {
  const uint8_t* dst_img;    // the destination's level-0 image (pitch geom.sw), a frame slot's or a keyframe slot's
  const float* dst_maxgrad;  // and its maxAbsGradient plane
  float T[12];
  int src;                   // source keyframe slot
  float gain, offset;        // the request's light: (1, 0) from ellc_keyframe_trial_propagate
  int pad_;
};

template <class Rec>
struct TrialArgs {
  MapView v;                 // what map_keep reads (level 0)
  const TrialReq* req;       // [B]
  unsigned* bits;            // [requests of the launch][words]: one bit per target pixel, zero in front of trial_pass
  Rec* partials;             // [requests of the launch][tiles]
  Rec* out;                  // pinned, through its device-side address: [B] records (trial_finish)
  unsigned words;            // ceil(n / 32)
  int first;                 // first request of this launch: blockIdx.y counts from it
  int photo_gate;
};

__device__ __forceinline__ void rec_zero(TrialRec& r) {
  r.sum_r2 = r.sum_abs_r = 0.0;
  r.n_kept = r.n_in_view = r.n_interior = r.n_low_grad = r.n_candidates = r.n_targets = 0;
  r.reserved[0] = r.reserved[1] = 0;
}

__device__ __forceinline__ void rec_add(TrialRec& a, const TrialRec& b) {
  a.sum_r2 += b.sum_r2; a.sum_abs_r += b.sum_abs_r;
  a.n_kept += b.n_kept; a.n_in_view += b.n_in_view; a.n_interior += b.n_interior; a.n_low_grad += b.n_low_grad;
  a.n_candidates += b.n_candidates; a.n_targets += b.n_targets;
}

__device__ __forceinline__ void rec_wave_sum(TrialRec& r) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    TrialRec o;
    o.sum_r2 = __shfl_xor(r.sum_r2, m, 64); o.sum_abs_r = __shfl_xor(r.sum_abs_r, m, 64);
    o.n_kept = __shfl_xor(r.n_kept, m, 64); o.n_in_view = __shfl_xor(r.n_in_view, m, 64); o.n_interior = __shfl_xor(r.n_interior, m, 64);
    o.n_low_grad = __shfl_xor(r.n_low_grad, m, 64); o.n_candidates = __shfl_xor(r.n_candidates, m, 64); o.n_targets = __shfl_xor(r.n_targets, m, 64);
    rec_add(r, o);
  }
}

__device__ __forceinline__ void rec_zero(TrialRecLit& r) {
  rec_zero(r.t);
#pragma unroll
  for (int k = 0; k < 5; k++) r.fit[k] = 0.0;
  r.n_fit = r.reserved = 0;
}

__device__ __forceinline__ void rec_add(TrialRecLit& a, const TrialRecLit& b) {
  rec_add(a.t, b.t);
#pragma unroll
  for (int k = 0; k < 5; k++) a.fit[k] += b.fit[k];
  a.n_fit += b.n_fit;
}

__device__ __forceinline__ void rec_wave_sum(TrialRecLit& r) {
  rec_wave_sum(r.t);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
    for (int k = 0; k < 5; k++) r.fit[k] += __shfl_xor(r.fit[k], m, 64);
    r.n_fit += __shfl_xor(r.n_fit, m, 64);
  }
}

// the narrow record inside either, and the fit's terms of one interior pixel (nothing for the narrow record)
__device__ __forceinline__ TrialRec& trial_counts(TrialRec& r) { return r; }
__device__ __forceinline__ TrialRec& trial_counts(TrialRecLit& r) { return r.t; }
__device__ __forceinline__ void trial_fit(TrialRec&, float, float) {}
__device__ __forceinline__ void trial_fit(TrialRecLit& r, float Is, float Iw) {
  // the product of two f32 values is exact in double, so the fused multiply-add rounds once, as the addition would
  const double s = (double)Is, t = (double)Iw;
  r.fit[0] += s;
  r.fit[1] += t;
  r.fit[2] = __builtin_fma(s, s, r.fit[2]);
  r.fit[3] = __builtin_fma(s, t, r.fit[3]);
  r.fit[4] = __builtin_fma(t, t, r.fit[4]);
  r.n_fit++;
}

// grid (tiles of level 0) x (requests of the launch), map_count's pixel layout: thread t of tile `local` owns pixels
// local * ELLC_TILE + j * 256 + t and adds them in the order j = 0..7; pair_store_block adds the lanes and the waves.
template <class Rec>
__device__ __forceinline__ void trial_pass_body(const TrialArgs<Rec>& a) {
  const unsigned b = (unsigned)a.first + blockIdx.y;
  const TrialReq& q = a.req[b];
  const int src = __builtin_amdgcn_readfirstlane(q.src);
  const KfLevelDev& S = a.v.kf_tab[a.v.level * a.v.max_kf + src];
  const LevelGeom& g = a.v.geom[a.v.level];
  const ELLC_GLOBAL float* depth = gptr(S.depth);
  const ELLC_GLOBAL float* var = gptr(S.var);
  const ELLC_GLOBAL uint8_t* img = gptr(S.img);
  const uint8_t* dimg = q.dst_img;
  const float* dgrad = q.dst_maxgrad;
  const int cols = g.cols, rows = g.rows;
  const RenderT T = load_T12(q.T);   // block-uniform: scalar loads
  const float gain = q.gain, offset = q.offset;   // (block-uniform too)
  unsigned* bits = a.bits + (size_t)blockIdx.y * a.words;
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
  Rec rec;
  rec_zero(rec);
  TrialRec& r = trial_counts(rec);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    MapPixel p;
    RenderCand c;
    if (!map_keep(a.v, depth, var, cols, rows, i, p)) continue;
    r.n_kept++;
    if (!render_candidate(g, T, 0u, i, p.x, p.y, p.Z, p.V, c)) continue;   // (the request number only enters the key, which is not used here)
    r.n_in_view++;
    if (!absorb_interior(g, c)) continue;
    r.n_interior++;
    float res, gr, Iw, Is;
    const bool pass = absorb_photo(g, dimg, dgrad, img, p.x, p.y, c, gain, offset, res, gr, Iw, Is);   // (computed whether or not the gate is on: the taps exist)
    r.n_low_grad += gr < 5.0f ? 1 : 0;
    r.sum_r2 += (double)(res * res);
    r.sum_abs_r += (double)fabsf(res);
    trial_fit(rec, Is, Iw);
    if (a.photo_gate && !pass) continue;
    r.n_candidates++;
    // (target < cols * rows <= 32 * words: render_candidate's bounds test)
    const unsigned bit = 1u << ((unsigned)c.target & 31u);
    const unsigned old = __hip_atomic_fetch_or(bits + ((unsigned)c.target >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    r.n_targets += (old & bit) ? 0 : 1;   // exactly one candidate of a target finds the bit clear, whoever arrives first
  }
  pair_store_block(rec, a.partials + (blockIdx.y * (unsigned)a.v.tiles + blockIdx.x));
}

// the two instances of the one body: the narrow record keeps ellc_keyframe_trial_propagate's launches at their registers and traffic
__global__ __launch_bounds__(256) void trial_pass(TrialArgs<TrialRec> a) { trial_pass_body(a); }
__global__ __launch_bounds__(256) void trial_lit_pass(TrialArgs<TrialRecLit> a) { trial_pass_body(a); }

__global__ __launch_bounds__(64) void trial_finish(TrialArgs<TrialRec> a) {
  pair_finish(a.partials, a.v.tiles, a.out, a.first);
}
__global__ __launch_bounds__(64) void trial_lit_finish(TrialArgs<TrialRecLit> a) {
  pair_finish(a.partials, a.v.tiles, a.out, a.first);
}

}  // namespace ellc
