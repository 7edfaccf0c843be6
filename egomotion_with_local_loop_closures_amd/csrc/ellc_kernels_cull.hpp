// ellc_keyframe_cull_depth: the hypotheses of one keyframe slot that B other views CONTRADICT are removed (no reference counterpart: the
// reference drops a hypothesis at the target of a propagation only, DepthPropagation.cpp:1090-1148; a wrong one in a stored keyframe
// stays). refine_pixels' shape: one pixel per thread, the staged views read wave-uniformly, map_keep (ellc_kernels_map.hpp) decides
// which pixels take part, render_candidate (ellc_kernels_render.hpp) where they land in a view, the agreement rule of consist_pass
// (ellc_kernels_consistency.hpp) how the view's own map votes, sim3_photo_taps (ellc_kernels_sim3.hpp) whether the view has four taps
// and what Iw and Is are. Every count is an integer: the order of the views does not enter the result. The stats leave one partial
// record per block (pair_store_block), cull_finish sums the blocks (pair_finish).
#pragma once
#include <float.h>
#include "ellc_kernels_views.hpp"

namespace ellc {

// one view as the kernel reads it: 80 bytes, staged once per call, read with a wave-uniform index (scalar loads)
struct CullView : RefineView {
  const float* depth;        // the view's depth and variance planes on the level (dense), both null where the view has none: a frame
  const float* var;          //   slot, or a keyframe slot that holds an image only
};

// the stats as the kernels write them; a block's partial record has the same layout
struct CullRec {
  long long s[5];            // sum_agree, sum_in_front, sum_behind, sum_photo, sum_photo_bad
  int32_t n[7];              // n_kept, one count per status 1..5, pixels whose returned depth is > 0 (the dense hint of a destination)
  int32_t pad_;
};

struct CullArgs {
  MapView v;                 // what map_keep reads
  const CullView* views;     // [B] (device copy of the pinned record)
  CullRec* partials;         // [blocks]
  CullRec* out;              // pinned, through its device-side address: one record (cull_finish)
  float* depth;              // the five planes, [n of the level] each
  float* var;
  uint32_t* votes;
  uint8_t* photo;
  uint8_t* status;
  int kf_slot, B, blocks;
  int first;                 // 0 (pair_finish's request offset)
  float agree_k2;
  float sp;                  // sqrtf(1 / sigma_i2), both roundings on the host
  float photo_k;             // <= 0: no photometric vote
  int min_support, min_judged, min_in_front, min_photo;
};

__device__ __forceinline__ void rec_zero(CullRec& r) { r = CullRec(); }

__device__ __forceinline__ void rec_add(CullRec& a, const CullRec& b) {
#pragma unroll
  for (int k = 0; k < 5; k++) a.s[k] += b.s[k];
#pragma unroll
  for (int k = 0; k < 7; k++) a.n[k] += b.n[k];
}

__device__ __forceinline__ void rec_wave_sum(CullRec& r) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    CullRec o;
#pragma unroll
    for (int k = 0; k < 5; k++) o.s[k] = __shfl_xor(r.s[k], m, 64);
#pragma unroll
    for (int k = 0; k < 7; k++) o.n[k] = __shfl_xor(r.n[k], m, 64);
    rec_add(r, o);
  }
}

// grid (256-pixel blocks of the level): thread t of block k owns pixel 256 k + t
__global__ __launch_bounds__(256) void cull_pixels(CullArgs a) {
  const KfPixels k = kf_pixels(a.v, a.kf_slot, block_pixel());
  const int i = k.i;
  CullRec r;
  rec_zero(r);
  if (i < k.cols * k.rows) {
    float Zout = k.depth[(unsigned)i], Vout = k.var[(unsigned)i];   // every pixel that is not culled keeps K's own bits
    int status = 0, na = 0, nf = 0, nh = 0, np = 0, nbad = 0;
    MapPixel p;
    if (map_keep(a.v, k.depth, k.var, k.cols, k.rows, i, p)) {
      r.n[0]++;
#pragma unroll 1
      for (int b = 0; b < a.B; b++) {
        const CullView& vw = a.views[b];   // wave-uniform: scalar loads
        const RenderT T = load_T12(vw.T);
        RenderCand c;
        if (!render_candidate(k.g, T, 0u, i, p.x, p.y, p.Z, p.V, c)) continue;   // (the request number only enters the key, which is not used here)
        bool behind = false;
        if (vw.depth) {   // wave-uniform
          const ELLC_GLOBAL float* tdepth = (const ELLC_GLOBAL float*)vw.depth;
          const ELLC_GLOBAL float* tvar = (const ELLC_GLOBAL float*)vw.var;
          const float Zt = tdepth[(unsigned)c.target], Vt = tvar[(unsigned)c.target];   // (target < cols * rows: render_candidate's bounds test)
          if (map_ok(Zt, Vt)) {
            const float idt = 1.0f / Zt;
            const float d = c.nid - idt;
            const float s = c.nvar + Vt;
            if (d * d <= a.agree_k2 * s) na++;
            else if (d > 0.0f) nf++;
            else { nh++; behind = true; }
          }
        }
        if (a.photo_k > 0.0f && !behind) {
          float Iw, gx, gy, Is;
          if (sim3_photo_taps(c, p, k.img, (const ELLC_GLOBAL uint8_t*)vw.img, k.cols, k.rows, k.sw, Iw, gx, gy, Is)) {
            const PhotoTerm ph = photo_term(Iw, Is, vw.gain, vw.offset, 1.0f, a.sp, FLT_MAX);   // (e alone is read: no weight is asked for)
            np++;
            if (!(ph.e <= a.photo_k)) nbad++;
          }
        }
      }
      // rule 3, in its order
      if (nf >= a.min_in_front && nf > na) status = 2;
      else if (na + nf + nh >= a.min_judged && na < a.min_support) status = 3;
      else if (a.photo_k > 0.0f && np >= a.min_photo && 2 * nbad > np) status = 4;
      else if (na + nf + nh == 0 && np == 0) status = 5;
      else status = 1;
      rec_count_status<1, 5>(r.n, status);
      r.s[0] = na; r.s[1] = nf; r.s[2] = nh; r.s[3] = np; r.s[4] = nbad;
      if (status >= 2 && status <= 4) { Zout = 0.0f; Vout = -1.0f; }
    }
    a.depth[(unsigned)i] = Zout;
    a.var[(unsigned)i] = Vout;
    a.votes[(unsigned)i] = (uint32_t)na | ((uint32_t)nf << 8) | ((uint32_t)nh << 16) | ((uint32_t)nbad << 24);
    a.photo[(unsigned)i] = (uint8_t)np;
    a.status[(unsigned)i] = (uint8_t)status;
    r.n[6] = Zout > 0.0f ? 1 : 0;
  }
  pair_store_block(r, a.partials + blockIdx.x);
}

__global__ __launch_bounds__(64) void cull_finish(CullArgs a) {
  pair_finish(a.partials, a.blocks, a.out, a.first);
}

}  // namespace ellc
