// ellc_keyframe_light_step: the normal equations of the weighted affine fit Iw ~ gain * Is + offset between two keyframe slots at a given
// transform and light, over exactly the photometric pixels of ellc_keyframe_sim3_step (no reference counterpart: the reference assumes
// that a surface keeps its grey value between two keyframes). consist_pass / consist_finish's shape: two launches, no waiting between
// blocks and no atomics. light_pass leaves one partial record per (request, tile), light_finish sums a request's tiles. map_keep decides
// which source pixels take part, render_candidate where they land, sim3_photo_taps (ellc_kernels_sim3.hpp) which of them have four taps and
// what Iw and Is are.
#pragma once
#include "ellc_kernels_sim3.hpp"

namespace ellc {

// ellc_light_normal as the kernels write it; the partial record of a tile has the same layout
struct LightRec {
  double s[7];               // sum_w, sum_w_s, sum_w_t, sum_w_ss, sum_w_st, sum_w_tt, chi2_photo
  int32_t n[4];              // n_kept, n_in_view, n_photo, n_photo_huber
};

struct LightArgs {
  MapView v;                 // what map_keep reads
  const int* stage;          // [cap] source slots, [cap] destination slots, [cap][12] f32 transforms, [cap][2] f32 lights (device copy of the pinned record)
  LightRec* partials;        // [requests of the launch][tiles]
  LightRec* out;             // pinned, through its device-side address: [B] records (light_finish)
  int cap;                   // requests the staging holds
  int first;                 // first request of this launch: blockIdx.y counts from it
  float w0, sp;              // 1 / sigma_i2 and its square root, both rounded to f32 on the host
  float huber_k;
};

__device__ __forceinline__ void rec_zero(LightRec& r) { r = LightRec(); }

__device__ __forceinline__ void rec_add(LightRec& a, const LightRec& b) {
#pragma unroll
  for (int k = 0; k < 7; k++) a.s[k] += b.s[k];
#pragma unroll
  for (int k = 0; k < 4; k++) a.n[k] += b.n[k];
}

__device__ __forceinline__ void rec_wave_sum(LightRec& r) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    LightRec o;
#pragma unroll
    for (int k = 0; k < 7; k++) o.s[k] = __shfl_xor(r.s[k], m, 64);
#pragma unroll
    for (int k = 0; k < 4; k++) o.n[k] = __shfl_xor(r.n[k], m, 64);
    rec_add(r, o);
  }
}

// grid (tiles of the level) x (requests of the launch), map_count's pixel layout: thread t of tile `local` owns pixels
// local * ELLC_TILE + j * 256 + t and adds them in the order j = 0..7; pair_store_block adds the lanes and the waves.
__global__ __launch_bounds__(256) void light_pass(LightArgs a) {
  const unsigned b = (unsigned)a.first + blockIdx.y;
  const int src = __builtin_amdgcn_readfirstlane(a.stage[b]), dst = __builtin_amdgcn_readfirstlane(a.stage[(unsigned)a.cap + b]);
  const KfLevelDev& S = a.v.kf_tab[a.v.level * a.v.max_kf + src];
  const KfLevelDev& D = a.v.kf_tab[a.v.level * a.v.max_kf + dst];
  const LevelGeom& g = a.v.geom[a.v.level];
  const ELLC_GLOBAL float* depth = gptr(S.depth);
  const ELLC_GLOBAL float* var = gptr(S.var);
  const ELLC_GLOBAL uint8_t* img = gptr(S.img);
  const ELLC_GLOBAL uint8_t* timg = gptr(D.img);
  const int cols = g.cols, rows = g.rows, sw = g.sw;
  const RenderT T = load_T12((const float*)(a.stage + 2u * (unsigned)a.cap) + 12u * b);   // block-uniform: scalar loads
  float gain, offset;
  load_light(a.stage, a.cap, b, gain, offset);
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
  LightRec r;
  rec_zero(r);
#pragma unroll 1
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    // A pixel without a term keeps these zeros and adds exact zeros below: the accumulators are updated in ONE place, outside the branches
    float Is = 0.0f, Iw = 0.0f, rp = 0.0f, wp = 0.0f;
    MapPixel p;
    RenderCand c;
    if (map_keep(a.v, depth, var, cols, rows, i, p)) {
      r.n[0]++;
      if (render_candidate(g, T, 0u, i, p.x, p.y, p.Z, p.V, c)) {   // (the request number only enters the key, which is not used here)
        r.n[1]++;
        float gx, gy, tIw, tIs;
        if (sim3_photo_taps(c, p, img, timg, cols, rows, sw, tIw, gx, gy, tIs)) {
          r.n[2]++;
          Is = tIs;
          Iw = tIw;
          rp = Iw - (gain * Is + offset);
          const float e = fabsf(rp) * a.sp;
          wp = a.w0;
          if (!(e <= a.huber_k)) {
            wp = a.w0 * (a.huber_k / e);
            r.n[3]++;
          }
        }
      }
    }
    // wIs and wIw are f32; their products with an f32 are exact in double, so the fused multiply-add rounds once, as the addition would
    const float wIs = wp * Is, wIw = wp * Iw;
    r.s[0] += (double)wp;
    r.s[1] += (double)wIs;
    r.s[2] += (double)wIw;
    r.s[3] = __builtin_fma((double)wIs, (double)Is, r.s[3]);
    r.s[4] = __builtin_fma((double)wIs, (double)Iw, r.s[4]);
    r.s[5] = __builtin_fma((double)wIw, (double)Iw, r.s[5]);
    r.s[6] += (double)((rp * rp) * wp);
  }
  pair_store_block(r, a.partials + (blockIdx.y * (unsigned)a.v.tiles + blockIdx.x));
}

__global__ __launch_bounds__(64) void light_finish(LightArgs a) {
  pair_finish(a.partials, a.v.tiles, a.out, a.first);
}

}  // namespace ellc
