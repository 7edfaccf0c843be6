// ellc_keyframe_joint_step / _apply: one photometric Gauss-Newton step over the SE(3) of B <= 8 views and the inverse depths of keyframe
// slot K's kept pixels together, the depths eliminated per pixel (no reference counterpart: the reference optimises poses only,
// GlobalOptimize.cpp). Three kernels over view_term (ellc_kernels_views.hpp), the term refine_evaluate sums too:
//   joint_pixels  one pixel per thread (refine_pixels' shape): every view's term at the pixel's d, the pixel's status, ih = 1 / Ht and gd
//                 into planes, the counts and the two chi2 sums through pair_store_block / pair_finish;
//   joint_pairs   grid (tiles of the level) x (view pairs b <= c, then the B views), sim3_pass's pixel layout: a block recomputes the
//                 terms of its one or two views at the used pixels and adds ONE 6 x 6 outer product u v^T and u r per pixel:
//                   pair b < c    u = m_b, v = c_c          (the block S[b][c])
//                   pair b == b   u = m_b, v = c_b, r = gd  (S[b][b], of which the host reads k <= l, and s_b)
//                   view b        u = wp Jp, v = Jp, r = rp (A_b, k <= l, and a_b)
//                 no floating-point atomics, the order of sim3_pass's sums, the same bytes on every call;
//   joint_apply_pixels  one pixel per thread: the evaluation again, the back-substituted step and the five planes.
#pragma once
#include <float.h>
#include "ellc_kernels_views.hpp"

namespace ellc {

#define ELLC_JOINT_VIEWS 8
#define ELLC_JOINT_PAIR_SUMS 42   // 36 of u v^T (row-major), 6 of u r

// one view as the kernels read it: 96 bytes, staged once per call, read with a wave-uniform index (scalar loads)
struct JointView : RefineView {
  float xf[6];               // the view's pose step rounded to f32 (joint_apply_pixels only)
  float pad_[2];
};

// the counts and chi2 sums of joint_pixels and joint_apply_pixels; a block's partial record has the same layout
struct JointCountRec {
  double s[2];               // chi2_photo, chi2_prior (joint_pixels)
  long long n_terms;
  int32_t n[6];              // n_kept, n_taking_part, one count per status 1..4 (4, BAD_STEP: the apply only)
  int32_t nv[ELLC_JOINT_VIEWS];   // terms per view over the used pixels
  int32_t n_dense, pad_;     // pixels whose returned depth is > 0 (the dense hint of a destination; the apply only)
};

struct JointPairRec {
  double s[ELLC_JOINT_PAIR_SUMS];
};

struct JointArgs {
  MapView v;                 // what map_keep reads
  const JointView* views;    // [B] (device copy of the pinned record)
  JointCountRec* cpartials;  // [256-pixel blocks]
  JointCountRec* cout;       // pinned, through its device-side address: one record
  JointPairRec* partials;    // [B (B + 1) / 2 + B][tiles]
  JointPairRec* out;         // pinned, through its device-side address: [B (B + 1) / 2 + B] records
  const float* d_in;         // [n] the inverse depths given, or NULL
  float* d;                  // [n] the inverse depth every pixel is evaluated at, 0 where it does not take part (joint_pixels)
  float* ih;                 // [n] 1 / Ht of the used pixels
  float* gd;                 // [n] gd of the used pixels
  uint8_t* pstatus;          // [n] joint_pixels' status
  float* inv_depth_out;      // the apply's five planes, [n] each
  float* depth;
  float* var;
  uint8_t* nviews;
  uint8_t* status;
  int kf_slot, B, blocks;
  int first;                 // 0 (pair_finish's request offset)
  float w0, sp;              // 1 / sigma_i2 and its square root, both rounded to f32 on the host
  float huber_k, prior_weight, max_step_rel;
  int min_views;
};

__device__ __forceinline__ void rec_zero(JointCountRec& r) { r = JointCountRec(); }

__device__ __forceinline__ void rec_add(JointCountRec& a, const JointCountRec& b) {
  a.s[0] += b.s[0];
  a.s[1] += b.s[1];
  a.n_terms += b.n_terms;
#pragma unroll
  for (int k = 0; k < 6; k++) a.n[k] += b.n[k];
#pragma unroll
  for (int k = 0; k < ELLC_JOINT_VIEWS; k++) a.nv[k] += b.nv[k];
  a.n_dense += b.n_dense;
}

__device__ __forceinline__ void rec_wave_sum(JointCountRec& r) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    JointCountRec o;
    o.s[0] = __shfl_xor(r.s[0], m, 64);
    o.s[1] = __shfl_xor(r.s[1], m, 64);
    o.n_terms = __shfl_xor(r.n_terms, m, 64);
#pragma unroll
    for (int k = 0; k < 6; k++) o.n[k] = __shfl_xor(r.n[k], m, 64);
#pragma unroll
    for (int k = 0; k < ELLC_JOINT_VIEWS; k++) o.nv[k] = __shfl_xor(r.nv[k], m, 64);
    o.n_dense = __shfl_xor(r.n_dense, m, 64);
    rec_add(r, o);
  }
}

__device__ __forceinline__ void rec_zero(JointPairRec& r) { r = JointPairRec(); }

__device__ __forceinline__ void rec_add(JointPairRec& a, const JointPairRec& b) {
#pragma unroll
  for (int k = 0; k < ELLC_JOINT_PAIR_SUMS; k++) a.s[k] += b.s[k];
}

// (the exchanges go eight at a time, as in Sim3Rec's butterfly)
__device__ __forceinline__ void rec_wave_sum(JointPairRec& r) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
    for (int k = 0; k < ELLC_JOINT_PAIR_SUMS; k++) {
      r.s[k] += __shfl_xor(r.s[k], m, 64);
      if (k % 8 == 7) __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// What a pixel that takes part is at its d: the evaluation over the views in ascending b, the status (1 USED, 2 TOO_FEW_VIEWS,
// 3 NO_INFORMATION), ih and gd; with STEP also q, the pose steps' pull on the pixel: q = 0, then q = q + c_b[k] * xf_b[k], b and k ascending.
struct JointPixel {
  float d, d0, hp, ih, gd, E, q;
  int n, status;
  unsigned mask;             // bit b: view b has a term
};

template <bool STEP>
__device__ __forceinline__ void joint_pixel(const JointArgs& a, const KfPixels& k, const MapPixel& p, JointPixel& o) {
  o.d0 = 1.0f / p.Z;
  o.hp = (a.prior_weight == 0.0f) ? 0.0f : a.prior_weight / p.V;
  o.d = o.d0;
  if (a.d_in) {
    const float di = a.d_in[(unsigned)k.i];
    if (di > 0.0f && di <= FLT_MAX) o.d = di;
  }
  const float Z = 1.0f / o.d;
  float H = 0.0f, gs = 0.0f;
  o.E = 0.0f; o.q = 0.0f; o.n = 0; o.mask = 0u;
#pragma unroll 1
  for (int b = 0; b < a.B; b++) {
    const JointView& vw = a.views[b];   // wave-uniform: scalar loads
    ViewTerm t;
    if (!view_term<true>(a, k, vw, p, Z, t)) continue;
    const float wJ = t.wp * t.Jd;
    H = H + wJ * t.Jd;
    gs = gs + wJ * t.rp;
    o.E = o.E + (t.rp * t.rp) * t.wp;
    if (STEP) {
#pragma unroll
      for (int l = 0; l < 6; l++) o.q = o.q + (wJ * t.Jp[l]) * vw.xf[l];
    }
    o.n++;
    o.mask |= 1u << b;
  }
  o.ih = 0.0f; o.gd = 0.0f;
  if (o.n < a.min_views) { o.status = 2; return; }
  const float Ht = H + o.hp;
  o.gd = gs + o.hp * (o.d - o.d0);
  if (!(Ht > 0.0f && Ht <= FLT_MAX)) { o.status = 3; o.gd = 0.0f; return; }
  o.status = 1;
  o.ih = 1.0f / Ht;
}

// grid (256-pixel blocks of the level): thread t of block k owns pixel 256 k + t
__global__ __launch_bounds__(256) void joint_pixels(JointArgs a) {
  const KfPixels k = kf_pixels(a.v, a.kf_slot, block_pixel());
  const int i = k.i;
  JointCountRec r;
  rec_zero(r);
  if (i < k.cols * k.rows) {
    float d = 0.0f, ih = 0.0f, gd = 0.0f;
    int status = 0;
    MapPixel p;
    if (map_keep(a.v, k.depth, k.var, k.cols, k.rows, i, p)) {
      r.n[0]++;
      if (a.prior_weight == 0.0f || p.V > 0.0f) {
        r.n[1]++;
        JointPixel o;
        joint_pixel<false>(a, k, p, o);
        d = o.d; ih = o.ih; gd = o.gd; status = o.status;
        rec_count_status<1, 3>(r.n + 1, status);
        if (status == 1) {
          r.n_terms = o.n;
#pragma unroll
          for (int b = 0; b < ELLC_JOINT_VIEWS; b++) r.nv[b] = (int)((o.mask >> b) & 1u);
          r.s[0] = (double)o.E;
          r.s[1] = (double)((o.hp * (o.d - o.d0)) * (o.d - o.d0));
        }
      }
    }
    a.d[(unsigned)i] = d;
    a.ih[(unsigned)i] = ih;
    a.gd[(unsigned)i] = gd;
    a.pstatus[(unsigned)i] = (uint8_t)status;
  }
  pair_store_block(r, a.cpartials + blockIdx.x);
}

__global__ __launch_bounds__(64) void joint_count_finish(JointArgs a) {
  pair_finish(a.cpartials, a.blocks, a.cout, a.first);
}

// grid (tiles of the level) x (B (B + 1) / 2 + B), map_count's pixel layout; blockIdx.y counts the pairs (b, c), b <= c, by rows, then
// the views. Only joint_pixels' planes and K's variance and image are read: a used pixel was kept.
__global__ __launch_bounds__(256) void joint_pairs(JointArgs a) {
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
  KfPixels kp = kf_pixels(a.v, a.kf_slot, base);   // (.i moves with j below)
  const int n_pairs = (a.B * (a.B + 1)) / 2;
  int b = 0, c = 0;
  const bool per_view = (int)blockIdx.y >= n_pairs;
  if (per_view) {
    b = c = (int)blockIdx.y - n_pairs;
  } else {
    int rem = (int)blockIdx.y;
    while (rem >= a.B - b) { rem -= a.B - b; b++; }
    c = b + rem;
  }
  b = __builtin_amdgcn_readfirstlane(b);
  c = __builtin_amdgcn_readfirstlane(c);
  const JointView& vb = a.views[b];   // block-uniform: scalar loads
  const JointView& vc = a.views[c];
  JointPairRec r;
  rec_zero(r);
#pragma unroll 1
  for (int j = 0; j < 8; j++) {
    const int i = kp.i = base + j * 256;
    // a pixel without a term keeps these zeros and adds exact zeros below: the accumulators are updated in one place (sim3_pass)
    float u[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, rr = 0.0f;
    if (i < kp.cols * kp.rows && a.pstatus[(unsigned)i] == 1) {
      MapPixel p;
      p.y = i / kp.cols; p.x = i - p.y * kp.cols; p.V = kp.var[(unsigned)i]; p.Z = 0.0f; p.support = 0;
      const float Z = 1.0f / a.d[(unsigned)i];
      ViewTerm tb;
      if (view_term<true>(a, kp, vb, p, Z, tb)) {
        if (per_view) {
#pragma unroll
          for (int k = 0; k < 6; k++) { u[k] = tb.wp * tb.Jp[k]; v[k] = tb.Jp[k]; }
          rr = tb.rp;
        } else {
          const float ih = a.ih[(unsigned)i], wJ = tb.wp * tb.Jd;
          float cb[6];
#pragma unroll
          for (int k = 0; k < 6; k++) { cb[k] = wJ * tb.Jp[k]; u[k] = cb[k] * ih; }
          if (b == c) {
#pragma unroll
            for (int k = 0; k < 6; k++) v[k] = cb[k];
            rr = a.gd[(unsigned)i];
          } else {
            ViewTerm tc;
            if (view_term<true>(a, kp, vc, p, Z, tc)) {
              const float wJc = tc.wp * tc.Jd;
#pragma unroll
              for (int k = 0; k < 6; k++) v[k] = wJc * tc.Jp[k];
            } else {
#pragma unroll
              for (int k = 0; k < 6; k++) u[k] = 0.0f;   // (no term of the pair: 0 * 0, never 0 * inf)
            }
          }
        }
      }
    }
    // the products of two f32 values are exact in double: the fused multiply-add rounds once (sim3_term)
#pragma unroll
    for (int k = 0; k < 6; k++) {
#pragma unroll
      for (int l = 0; l < 6; l++) r.s[6 * k + l] = __builtin_fma((double)u[k], (double)v[l], r.s[6 * k + l]);
      r.s[36 + k] = __builtin_fma((double)u[k], (double)rr, r.s[36 + k]);
    }
  }
  rec_wave_sum(r);
  __shared__ JointPairRec ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = r;
  __syncthreads();
  // sim3_pass's block tail: thread k adds field k of the four waves in ascending order
  JointPairRec& out = a.partials[blockIdx.y * (unsigned)a.v.tiles + blockIdx.x];
  const unsigned k = threadIdx.x;
  if (k < ELLC_JOINT_PAIR_SUMS) out.s[k] = ((ws[0].s[k] + ws[1].s[k]) + ws[2].s[k]) + ws[3].s[k];
}

__global__ __launch_bounds__(64) void joint_pair_finish(JointArgs a) {
  pair_finish(a.partials, a.v.tiles, a.out, a.first);
}

// grid (256-pixel blocks of the level): the evaluation again, the pixel's step from the views' pose steps, the five planes
__global__ __launch_bounds__(256) void joint_apply_pixels(JointArgs a) {
  const KfPixels k = kf_pixels(a.v, a.kf_slot, block_pixel());
  const int i = k.i;
  JointCountRec r;
  rec_zero(r);
  if (i < k.cols * k.rows) {
    float Zout = k.depth[(unsigned)i], Vout = k.var[(unsigned)i], dout = 0.0f;   // every pixel that is not stepped keeps K's own bits
    int status = 0, nv = 0;
    MapPixel p;
    if (map_keep(a.v, k.depth, k.var, k.cols, k.rows, i, p)) {
      r.n[0]++;
      if (a.prior_weight == 0.0f || p.V > 0.0f) {
        r.n[1]++;
        JointPixel o;
        joint_pixel<true>(a, k, p, o);
        status = o.status; nv = o.n; dout = o.d;
        if (status == 1) {
          const float delta = -((o.gd + o.q) * o.ih);
          const float dn = o.d + delta;
          if (!(dn > 0.0f && dn <= FLT_MAX && fabsf(delta) <= a.max_step_rel * o.d)) {
            status = 4;
          } else {
            dout = dn;
            Zout = 1.0f / dn;
            Vout = o.ih;
          }
        }
        rec_count_status<1, 4>(r.n + 1, status);
      }
    }
    a.inv_depth_out[(unsigned)i] = dout;
    a.depth[(unsigned)i] = Zout;
    a.var[(unsigned)i] = Vout;
    a.nviews[(unsigned)i] = (uint8_t)nv;
    a.status[(unsigned)i] = (uint8_t)status;
    r.n_dense = Zout > 0.0f ? 1 : 0;
  }
  pair_store_block(r, a.cpartials + blockIdx.x);
}

}  // namespace ellc
