// What the pixel kernels of the calls of one keyframe slot K against B views share (ellc_keyframe_refine_depth, _sweep_depth, _cull_depth,
// _joint_step / _apply): the staged view, K's planes on the level, the photometric residual and its Huber weight, a view's term of a
// per-pixel Gauss-Newton on the inverse depth, the status counts. Every function is forced inline and the library is built with
// -ffp-contract=off: an f32 expression rounds here as it did written out in its kernel. sim3_pass and light_pass keep their own
// photometric lines: sim3_pass lies below this header, and light_pass's instruction stream does not stay identical with photo_term.
#pragma once
#include <float.h>
#include "ellc_kernels_sim3.hpp"

namespace ellc {

// one view as the kernels read it: 64 bytes, staged once per call, read with a wave-uniform index (scalar loads). A call whose views
// carry more derives its staged type from this one (CullView, JointView).
struct RefineView {
  const uint8_t* img;        // the view's image on the level (stored pitch sw)
  float T[12];               // K's camera -> the view's
  float gain, offset;
};

// K's planes on the level, the level's geometry and the pixel a thread owns
struct KfPixels {
  const ELLC_GLOBAL float* depth;
  const ELLC_GLOBAL float* var;
  const ELLC_GLOBAL uint8_t* img;
  const LevelGeom& g;
  int cols, rows, sw;
  int i;
};

__device__ __forceinline__ KfPixels kf_pixels(const MapView& v, int kf_slot, int i) {
  const KfLevelDev& K = v.kf_tab[v.level * v.max_kf + kf_slot];
  const LevelGeom& g = v.geom[v.level];
  return KfPixels{gptr(K.depth), gptr(K.var), gptr(K.img), g, g.cols, g.rows, g.sw, i};
}

// the pixel of thread t of 256-pixel block k: 256 k + t
__device__ __forceinline__ int block_pixel() { return (int)(blockIdx.x * 256u + threadIdx.x); }

// The photometric residual against a view's light, its size in sigmas and its Huber weight
struct PhotoTerm {
  float rp, e, wp;
};

__device__ __forceinline__ PhotoTerm photo_term(float Iw, float Is, float gain, float offset, float w0, float sp, float huber_k) {
  PhotoTerm t;
  t.rp = Iw - (gain * Is + offset);
  t.e = fabsf(t.rp) * sp;
  t.wp = w0;
  if (!(t.e <= huber_k)) t.wp = w0 * (huber_k / t.e);
  return t;
}

// One view's term at pixel k.i = (p.x, p.y) of K at the depth Z = 1 / d: rp, wp, Jd = dIw/dd and, with POSE, the six entries of
// dIw/d(the view's pose) as sim3_pass has them. Args gives w0, sp and huber_k. False: the view has no candidate or no four taps there.
struct ViewTerm {
  float rp, wp, Jd, Jp[6];
};

template <bool POSE, class Args>
__device__ __forceinline__ bool view_term(const Args& a, const KfPixels& k, const RefineView& vw, const MapPixel& p, float Z, ViewTerm& t) {
  const RenderT T = load_T12(vw.T);
  RenderCand c;
  if (!render_candidate(k.g, T, 0u, k.i, p.x, p.y, Z, p.V, c)) return false;   // (the request number only enters the key, which is not used here)
  float Iw, gx, gy, Is;
  if (!sim3_photo_taps(c, p, k.img, (const ELLC_GLOBAL uint8_t*)vw.img, k.cols, k.rows, k.sw, Iw, gx, gy, Is)) return false;
  const float A = (gx * k.g.fx) * c.nid, Bv = (gy * k.g.fy) * c.nid;
  const float Cq = -(((A * c.x) + (Bv * c.y)) * c.nid);
  if (POSE) {
    t.Jp[0] = Cq * c.y - Bv * c.z; t.Jp[1] = A * c.z - Cq * c.x; t.Jp[2] = Bv * c.x - A * c.y; t.Jp[3] = A; t.Jp[4] = Bv; t.Jp[5] = Cq;
  }
  const PhotoTerm ph = photo_term(Iw, Is, vw.gain, vw.offset, a.w0, a.sp, a.huber_k);
  t.rp = ph.rp;
  t.wp = ph.wp;
  // dP'/dd = -Z (P' - t): the derivative of Iw by the inverse depth
  const float qx = c.x - T.t[3], qy = c.y - T.t[7], qz = c.z - T.t[11];
  t.Jd = -(Z * (((A * qx) + (Bv * qy)) + (Cq * qz)));
  return true;
}

// n[k] counts the pixels of status k, FIRST <= k <= LAST. Compared, not indexed: an index known at run time only sends the record from
// registers into LDS.
template <int FIRST, int LAST>
__device__ __forceinline__ void rec_count_status(int32_t* n, int status) {
#pragma unroll
  for (int k = FIRST; k <= LAST; k++) n[k] += (status == k) ? 1 : 0;
}

}  // namespace ellc
