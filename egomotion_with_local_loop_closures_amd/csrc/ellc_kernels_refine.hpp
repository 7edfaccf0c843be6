// ellc_keyframe_refine_depth: a per-pixel photometric Gauss-Newton on the inverse depth of one keyframe slot against the images of B
// other views at known transforms and lights (no reference counterpart: the reference refines depth by small-baseline line stereo
// only, DepthPropagation.cpp:140-420). One pixel per thread, a short loop over the views inside a short loop over the iterations; the
// per-pixel state is a handful of f32 values: no LDS and no atomics in the pixel loop. map_keep (ellc_kernels_map.hpp) decides which
// pixels take part, render_candidate (ellc_kernels_render.hpp) where they land in a view and what their point there is,
// sim3_photo_taps (ellc_kernels_sim3.hpp) whether the view has four taps and what Iw, its gradients and Is are. The stats leave one
// partial record per block (pair_store_block), refine_finish sums the blocks (pair_finish): the order of the two double sums follows
// from the level's size alone.
#pragma once
#include <float.h>
#include "ellc_kernels_views.hpp"

namespace ellc {

// the stats as the kernels write them; a block's partial record has the same layout
struct RefineRec {
  double s[2];               // sum_cost_before, sum_cost_after
  long long sum_views;
  int32_t n[9];              // n_kept, n_taking_part, one count per status 1..6, pixels whose returned depth is > 0 (the dense hint of a destination)
  int32_t pad_;
};

struct RefineArgs {
  MapView v;                 // what map_keep reads
  const RefineView* views;   // [B] (device copy of the pinned record)
  RefineRec* partials;       // [blocks]
  RefineRec* out;            // pinned, through its device-side address: one record (refine_finish)
  float* depth;              // the four planes, [n of the level] each
  float* var;
  uint8_t* nviews;
  uint8_t* status;
  int kf_slot, B, blocks;
  int first;                 // 0 (pair_finish's request offset)
  float w0, sp;              // 1 / sigma_i2 and its square root, both rounded to f32 on the host
  float huber_k, prior_weight, max_step_rel;
  int n_iter, min_views;
};

__device__ __forceinline__ void rec_zero(RefineRec& r) { r = RefineRec(); }

__device__ __forceinline__ void rec_add(RefineRec& a, const RefineRec& b) {
  a.s[0] += b.s[0];
  a.s[1] += b.s[1];
  a.sum_views += b.sum_views;
#pragma unroll
  for (int k = 0; k < 9; k++) a.n[k] += b.n[k];
}

__device__ __forceinline__ void rec_wave_sum(RefineRec& r) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    RefineRec o;
    o.s[0] = __shfl_xor(r.s[0], m, 64);
    o.s[1] = __shfl_xor(r.s[1], m, 64);
    o.sum_views = __shfl_xor(r.sum_views, m, 64);
#pragma unroll
    for (int k = 0; k < 9; k++) o.n[k] = __shfl_xor(r.n[k], m, 64);
    rec_add(r, o);
  }
}

// Rule 2: H, g, E and n of pixel k.i = (p.x, p.y) of K at the inverse depth d, the views in ascending b
__device__ __forceinline__ void refine_evaluate(const RefineArgs& a, const KfPixels& k, const MapPixel& p, float d, float& H, float& gs, float& E, int& n) {
  const float Z = 1.0f / d;
  H = 0.0f; gs = 0.0f; E = 0.0f; n = 0;
#pragma unroll 1
  for (int b = 0; b < a.B; b++) {
    ViewTerm t;
    t.rp = 0.0f; t.wp = 0.0f; t.Jd = 0.0f;   // (set before the call: refine_pixels keeps its 58 registers with it, NOTEBOOK.md)
    if (!view_term<false>(a, k, a.views[b], p, Z, t)) continue;   // (a.views[b] is wave-uniform: scalar loads)
    const float wJ = t.wp * t.Jd;
    H = H + wJ * t.Jd;
    gs = gs + wJ * t.rp;
    E = E + (t.rp * t.rp) * t.wp;
    n++;
  }
}

// grid (256-pixel blocks of the level): thread t of block k owns pixel 256 k + t
__global__ __launch_bounds__(256) void refine_pixels(RefineArgs a) {
  const KfPixels k = kf_pixels(a.v, a.kf_slot, block_pixel());
  const int i = k.i;
  RefineRec r;
  rec_zero(r);
  if (i < k.cols * k.rows) {
    float Zout = k.depth[(unsigned)i], Vout = k.var[(unsigned)i];   // every pixel that is not refined keeps K's own bits
    int status = 0, nv = 0;
    MapPixel p;
    if (map_keep(a.v, k.depth, k.var, k.cols, k.rows, i, p)) {
      r.n[0]++;
      if (a.prior_weight == 0.0f || p.V > 0.0f) {
        r.n[1]++;
        const float d0 = 1.0f / p.Z;
        const float hp = (a.prior_weight == 0.0f) ? 0.0f : a.prior_weight / p.V;
        float d = d0, E0 = 0.0f;
        int n0 = 0;
        // n_iter steps and the acceptance's evaluation: one loop, so that the evaluation's code exists once
#pragma unroll 1
        for (int it = 0; it <= a.n_iter; it++) {
          float H, gs, E;
          int n;
          refine_evaluate(a, k, p, d, H, gs, E, n);
          nv = n;
          if (it == 0) { E0 = E; n0 = n; }
          const float Ht = H + hp;
          const bool informed = Ht > 0.0f && Ht <= FLT_MAX;
          if (it == a.n_iter) {   // rule 4
            if (n != n0) { status = 5; break; }
            if (!informed) { status = 3; break; }
            const float c1 = E + (hp * (d - d0)) * (d - d0);
            if (!(c1 <= E0)) { status = 6; break; }
            status = 1;
            Zout = 1.0f / d;
            Vout = 1.0f / Ht;
            r.sum_views = n;
            r.s[0] = (double)E0;
            r.s[1] = (double)c1;
            break;
          }
          if (n < a.min_views) { status = 2; break; }
          const float gt = gs + hp * (d - d0);
          if (!informed) { status = 3; break; }
          const float step = gt / Ht;
          const float dn = d - step;
          if (!(dn > 0.0f && dn <= FLT_MAX && fabsf(step) <= a.max_step_rel * d)) { status = 4; break; }
          d = dn;
        }
        rec_count_status<1, 6>(r.n + 1, status);   // (status is 1..6 here: the loop always ends through a break)
      }
    }
    a.depth[(unsigned)i] = Zout;
    a.var[(unsigned)i] = Vout;
    a.nviews[(unsigned)i] = (uint8_t)nv;
    a.status[(unsigned)i] = (uint8_t)status;
    r.n[8] = Zout > 0.0f ? 1 : 0;
  }
  pair_store_block(r, a.partials + blockIdx.x);
}

__global__ __launch_bounds__(64) void refine_finish(RefineArgs a) {
  pair_finish(a.partials, a.blocks, a.out, a.first);
}

}  // namespace ellc
