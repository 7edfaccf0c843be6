// ellc_keyframe_sweep_depth: hypotheses CREATED for the pixels of one keyframe slot that hold none, by a sweep over n_samples inverse
// depths against the images of B other views at known transforms and lights (no reference counterpart: the reference creates a
// hypothesis by small-baseline line stereo against the tracked frame only, DepthPropagation.cpp:140-420). refine_pixels' shape: one pixel
// per thread, the staged views (RefineView) read wave-uniformly, render_candidate and sim3_photo_taps used as they stand, the stats
// through pair_store_block and pair_finish. A sample's cost is the mean over the views of a five-pixel pattern's weighted squared
// residuals; the decision (rule 4) needs the best sample, its two neighbours and the best sample at least two steps away. All of that
// is carried in eight registers while the samples go by ONCE (sweep_track): no per-thread array, no LDS, no second pass.
#pragma once
#include <float.h>
#include "ellc_kernels_views.hpp"

namespace ellc {

// the stats as the kernels write them; a block's partial record has the same layout
struct SweepRec {
  double s[1];               // sum_cost
  long long sum_views;
  int32_t n[9];              // n_ok, n_swept, one count per status 1..6, pixels whose returned depth is > 0 (the dense hint of a destination)
  int32_t pad_;
};

struct SweepArgs {
  MapView v;                 // the ring's tables and the level (no filter takes part)
  const RefineView* views;   // [B] (device copy of the pinned record)
  SweepRec* partials;        // [blocks]
  SweepRec* out;             // pinned, through its device-side address: one record (sweep_finish)
  float* depth;              // the four planes, [n of the level] each
  float* var;
  uint8_t* nviews;
  uint8_t* status;
  int kf_slot, B, blocks;
  int first;                 // 0 (pair_finish's request offset)
  float w0, sp;              // 1 / sigma_i2 and its square root, both rounded to f32 on the host
  float huber_k;
  float d_min, dstep;        // dstep = (d_max - d_min) / (n_samples - 1), rounded to f32 on the host
  float min_grad2, max_cost, distinct_ratio, var_scale;
  int n_samples, min_views;
};

__device__ __forceinline__ void rec_zero(SweepRec& r) { r = SweepRec(); }

__device__ __forceinline__ void rec_add(SweepRec& a, const SweepRec& b) {
  a.s[0] += b.s[0];
  a.sum_views += b.sum_views;
#pragma unroll
  for (int k = 0; k < 9; k++) a.n[k] += b.n[k];
}

__device__ __forceinline__ void rec_wave_sum(SweepRec& r) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    SweepRec o;
    o.s[0] = __shfl_xor(r.s[0], m, 64);
    o.sum_views = __shfl_xor(r.sum_views, m, 64);
#pragma unroll
    for (int k = 0; k < 9; k++) o.n[k] = __shfl_xor(r.n[k], m, 64);
    rec_add(r, o);
  }
}

// Rule 3, one pattern pixel (x, y) of K at the depth Z in the view (T, vw): its term c = (rp * rp) * wp, or false where the pattern
// pixel has no candidate or no four taps there.
__device__ __forceinline__ bool sweep_term(const SweepArgs& a, const KfPixels& k, const RenderT& T, const RefineView& vw, int x, int y, float Z, float& c) {
  MapPixel p;
  p.Z = Z; p.V = 0.0f; p.x = x; p.y = y; p.support = 0;
  RenderCand rc;
  if (!render_candidate(k.g, T, 0u, 0, x, y, Z, 0.0f, rc)) return false;   // (request and raster index only enter the key, which is not used here)
  float Iw, gx, gy, Is;
  if (!sim3_photo_taps(rc, p, k.img, (const ELLC_GLOBAL uint8_t*)vw.img, k.cols, k.rows, k.sw, Iw, gx, gy, Is)) return false;
  const PhotoTerm ph = photo_term(Iw, Is, vw.gain, vw.offset, a.w0, a.sp, a.huber_k);
  c = (ph.rp * ph.rp) * ph.wp;
  return true;
}

// Rule 3: cost and n of pixel (px, py) of K at the depth Z, the views in ascending b, the pattern in the header's order
__device__ __forceinline__ void sweep_cost(const SweepArgs& a, const KfPixels& k, int px, int py, float Z, float& cost, int& n) {
  float E = 0.0f;
  n = 0;
#pragma unroll 1
  for (int b = 0; b < a.B; b++) {
    const RefineView& vw = a.views[b];   // wave-uniform: scalar loads
    const RenderT T = load_T12(vw.T);
    float c0, c1, c2, c3, c4;
    if (!sweep_term(a, k, T, vw, px, py, Z, c0)) continue;
    if (!sweep_term(a, k, T, vw, px + 1, py, Z, c1)) continue;
    if (!sweep_term(a, k, T, vw, px - 1, py, Z, c2)) continue;
    if (!sweep_term(a, k, T, vw, px, py + 1, Z, c3)) continue;
    if (!sweep_term(a, k, T, vw, px, py - 1, Z, c4)) continue;
    E = E + ((((c0 + c1) + c2) + c3) + c4);
    n++;
  }
  cost = E / (float)n;   // (n == 0: NaN, and never valid)
}

// What rule 4 needs of the samples, kept while they go by in ascending k. A sample that is not valid enters as +inf, which no valid cost
// is (valid: cost <= FLT_MAX). k1 is the lowest k of smallest cost: a later sample replaces it only where it is strictly smaller.
//   cm, cp   the costs of k1 - 1 and k1 + 1 (+inf: not valid, or not there)
//   c2       the smallest valid cost with |k - k1| >= 2 (+inf: none). To the left of a NEW k1 = k that is the smallest valid cost of
//            the samples 0 .. k - 2, whatever k1 was before: `lag`, which runs two samples behind.
struct SweepTrack {
  int k1, n1;
  float c1, cm, cp, c2, prev, lag;
};

__device__ __forceinline__ void sweep_track(SweepTrack& t, int k, float cost, int n, bool valid) {
  const float cv = valid ? cost : INFINITY;
  if (t.k1 >= 0) {
    if (k == t.k1 + 1) t.cp = cv;
    else t.c2 = fminf(t.c2, cv);   // (k >= k1 + 2)
  }
  if (valid && (t.k1 < 0 || cost < t.c1)) {
    t.k1 = k; t.c1 = cost; t.n1 = n;
    t.cm = t.prev; t.cp = INFINITY; t.c2 = t.lag;
  }
  t.lag = fminf(t.lag, t.prev);
  t.prev = cv;
}

// grid (256-pixel blocks of the level): thread t of block k owns pixel 256 k + t
__global__ __launch_bounds__(256) void sweep_pixels(SweepArgs a) {
  const KfPixels kp = kf_pixels(a.v, a.kf_slot, block_pixel());
  const ELLC_GLOBAL uint8_t* img = kp.img;
  const int cols = kp.cols, rows = kp.rows, sw = kp.sw, i = kp.i;
  SweepRec r;
  rec_zero(r);
  if (i < cols * rows) {
    float Zout = kp.depth[(unsigned)i], Vout = kp.var[(unsigned)i];   // every pixel that gets no hypothesis keeps K's own bits
    int status = 0, nv = 0;
    const int py = i / cols, px = i - py * cols;
    bool swept = false;
    if (map_ok(Zout, Vout)) r.n[0]++;
    else if (px >= 1 && px <= cols - 2 && py >= 1 && py <= rows - 2) {   // rule 1
      const unsigned q = (unsigned)(py * sw + px);
      const float gxc = (float)img[q + 1u] - (float)img[q - 1u], gyc = (float)img[q + (unsigned)sw] - (float)img[q - (unsigned)sw];
      swept = (gxc * gxc) + (gyc * gyc) >= a.min_grad2;
    }
    if (swept) {
      r.n[1]++;
      SweepTrack t;
      t.k1 = -1; t.n1 = 0;
      t.c1 = t.cm = t.cp = t.c2 = t.prev = t.lag = INFINITY;
#pragma unroll 1
      for (int k = 0; k < a.n_samples; k++) {
        const float d = a.d_min + (float)k * a.dstep;   // rule 2
        float cost;
        int n;
        sweep_cost(a, kp, px, py, 1.0f / d, cost, n);
        sweep_track(t, k, cost, n, n >= a.min_views && cost <= FLT_MAX);
      }
      // rule 4
      nv = t.n1;
      if (t.k1 < 0) status = 2;
      else if (t.k1 == 0 || t.k1 == a.n_samples - 1 || !(t.cm <= FLT_MAX) || !(t.cp <= FLT_MAX)) status = 3;
      else if (a.max_cost > 0.0f && !(t.c1 <= a.max_cost)) status = 4;
      else if (!(t.c1 <= a.distinct_ratio * t.c2)) status = 5;
      else {
        const float curv = (t.cm - (2.0f * t.c1)) + t.cp;
        status = 6;
        if (curv > 0.0f && curv <= FLT_MAX) {
          const float off = (0.5f * (t.cm - t.cp)) / curv;
          const float d = (a.d_min + (float)t.k1 * a.dstep) + off * a.dstep;
          const float v = a.var_scale * ((2.0f * (a.dstep * a.dstep)) / ((float)t.n1 * curv));
          if (d > 0.0f && d <= FLT_MAX && v >= 0.0f && v <= FLT_MAX) {
            status = 1;
            Zout = 1.0f / d;
            Vout = v;
            r.sum_views = t.n1;
            r.s[0] = (double)t.c1;
          }
        }
      }
      rec_count_status<1, 6>(r.n + 1, status);
    }
    a.depth[(unsigned)i] = Zout;
    a.var[(unsigned)i] = Vout;
    a.nviews[(unsigned)i] = (uint8_t)nv;
    a.status[(unsigned)i] = (uint8_t)status;
    r.n[8] = Zout > 0.0f ? 1 : 0;
  }
  pair_store_block(r, a.partials + blockIdx.x);
}

__global__ __launch_bounds__(64) void sweep_finish(SweepArgs a) {
  pair_finish(a.partials, a.blocks, a.out, a.first);
}

}  // namespace ellc
