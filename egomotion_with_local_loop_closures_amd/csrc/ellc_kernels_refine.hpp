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
#include "ellc_kernels_sim3.hpp"

namespace ellc {

// one view as the kernel reads it: 64 bytes, staged once per call, read with a wave-uniform index (scalar loads)
struct RefineView {
  const uint8_t* img;        // the view's image on the level (stored pitch sw)
  float T[12];               // K's camera -> the view's
  float gain, offset;
};

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

// Rule 2: H, g, E and n of pixel i = (p.x, p.y) of K at the inverse depth d, the views in ascending b. The photometric lines (A, Bv,
// Cq, e, wp) are those of sim3_pass, which stays as it is.
__device__ __forceinline__ void refine_evaluate(const RefineArgs& a, const LevelGeom& g, const ELLC_GLOBAL uint8_t* img, const MapPixel& p, int i,
                                                float d, int cols, int rows, int sw, float& H, float& gs, float& E, int& n) {
  const float Z = 1.0f / d;
  const float fx = g.fx, fy = g.fy;
  H = 0.0f; gs = 0.0f; E = 0.0f; n = 0;
#pragma unroll 1
  for (int b = 0; b < a.B; b++) {
    const RefineView& vw = a.views[b];   // wave-uniform: scalar loads
    const RenderT T = load_T12(vw.T);
    RenderCand c;
    if (!render_candidate(g, T, 0u, i, p.x, p.y, Z, p.V, c)) continue;   // (the request number only enters the key, which is not used here)
    float Iw, gx, gy, Is;
    if (!sim3_photo_taps(c, p, img, (const ELLC_GLOBAL uint8_t*)vw.img, cols, rows, sw, Iw, gx, gy, Is)) continue;
    const float rp = Iw - (vw.gain * Is + vw.offset);
    const float A = (gx * fx) * c.nid, Bv = (gy * fy) * c.nid;
    const float Cq = -(((A * c.x) + (Bv * c.y)) * c.nid);
    const float e = fabsf(rp) * a.sp;
    float wp = a.w0;
    if (!(e <= a.huber_k)) wp = a.w0 * (a.huber_k / e);
    // dP'/dd = -Z (P' - t): the derivative of Iw by the inverse depth
    const float qx = c.x - T.t[3], qy = c.y - T.t[7], qz = c.z - T.t[11];
    const float J = -(Z * (((A * qx) + (Bv * qy)) + (Cq * qz)));
    const float wJ = wp * J;
    H = H + wJ * J;
    gs = gs + wJ * rp;
    E = E + (rp * rp) * wp;
    n++;
  }
}

// grid (256-pixel blocks of the level): thread t of block k owns pixel 256 k + t
__global__ __launch_bounds__(256) void refine_pixels(RefineArgs a) {
  const KfLevelDev& K = a.v.kf_tab[a.v.level * a.v.max_kf + a.kf_slot];
  const LevelGeom& g = a.v.geom[a.v.level];
  const ELLC_GLOBAL float* depth = gptr(K.depth);
  const ELLC_GLOBAL float* var = gptr(K.var);
  const ELLC_GLOBAL uint8_t* img = gptr(K.img);
  const int cols = g.cols, rows = g.rows, sw = g.sw;
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  RefineRec r;
  rec_zero(r);
  if (i < cols * rows) {
    float Zout = depth[(unsigned)i], Vout = var[(unsigned)i];   // every pixel that is not refined keeps K's own bits
    int status = 0, nv = 0;
    MapPixel p;
    if (map_keep(a.v, depth, var, cols, rows, i, p)) {
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
          refine_evaluate(a, g, img, p, i, d, cols, rows, sw, H, gs, E, n);
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
        // (status is 1..6 here: the loop always ends through a break. Compared, not indexed: an index known at run time only sends
        // the record from registers into LDS)
#pragma unroll
        for (int k = 1; k <= 6; k++) r.n[1 + k] += (status == k) ? 1 : 0;
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
