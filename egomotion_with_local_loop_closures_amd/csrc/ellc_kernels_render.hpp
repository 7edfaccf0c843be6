// ellc_keyframe_render_depth: the semi-dense maps of keyframe slots splatted forward into ONE camera view (no reference counterpart as
// a whole: the per-pixel arithmetic is propagateDepth's, DepthPropagation.cpp:1047-1086, without its photometric gate and its merge).
// Three passes over the same pixels, no waiting between blocks, integer atomics only: render_min leaves the smallest 64-bit key per
// target, render_resolve decodes it and computes the winner's values AGAIN with the same function, render_agree lets every candidate
// compare itself with its target's winner. map_keep (ellc_kernels_map.hpp) decides which pixels take part.
#pragma once
#include <float.h>
#include "ellc_kernels_map.hpp"

namespace ellc {

#define ELLC_RENDER_EMPTY 0xffffffffffffffffull   // what the key buffer is preset to: no candidate

struct RenderArgs {
  MapView v;                     // what map_keep reads
  const int* stage;              // [max_kf] keyframe slot of every request, then [max_kf][12] f32 transforms (map_slot, map_T12), then [max_kf][2] f32 lights (absorb_light)
  unsigned long long* keys;      // [n of the level]: (bits(z') << 32) | (b << 24) | i of the best candidate so far (render_min)
  float* depth;                  // the five planes of the view, [n] each (render_resolve; agree counted up by render_agree)
  float* var;
  int32_t* source;
  int32_t* agree;
  uint8_t* intensity;
  int* block_counts;             // [blocks of render_resolve] targets with a winner
  int* n_valid;                  // pinned, through its device-side address: their sum (render_finish)
  int n, blocks, B;              // pixels of the level, blocks of render_resolve, requests
  float agree_k2;
};

struct RenderT {
  float t[12];
};

// the twelve floats of a request's transform (block-uniform where the request is: scalar loads)
__device__ __forceinline__ RenderT load_T12(const float* T) {
  RenderT r;
#pragma unroll
  for (int k = 0; k < 12; k++) r.t[k] = T[k];
  return r;
}
__device__ __forceinline__ RenderT render_T12(const RenderArgs& a, unsigned b) { return load_T12(map_T12(a.stage, a.v.max_kf, b)); }

struct RenderCand {
  int target;                // raster index in the view
  unsigned long long key;
  float z, nid, nvar;        // depth in the view, its reciprocal, the propagated variance
  float x, y, u, v;          // the rest of the point in the view's camera and its projection, before the rounding (ellc_keyframe_sim3_step)
};

// THE rule, for all three passes: what source pixel i = (x, y) of request b with depth Z and variance V becomes in the view, or nothing.
// IEEE f32 in the order of PixelWisePyramid.cpp:236-244 (the point) and DepthPropagation.cpp:1050-1054, :1065, :1082-1086 (projection,
// target, variance); the library is compiled without contraction and with correctly rounded divisions.
__device__ __forceinline__ bool render_candidate(const LevelGeom& g, const RenderT& T, unsigned b, int i, int x, int y, float Z, float V, RenderCand& c) {
  const float fx = g.fx, fy = g.fy, cx = g.cx, cy = g.cy;
  const float X = (((float)x - cx) * Z) / fx;
  const float Y = (((float)y - cy) * Z) / fy;
  const float wx = ((T.t[0] * X + T.t[1] * Y) + T.t[2] * Z) + T.t[3];
  const float wy = ((T.t[4] * X + T.t[5] * Y) + T.t[6] * Z) + T.t[7];
  const float wz = ((T.t[8] * X + T.t[9] * Y) + T.t[10] * Z) + T.t[11];
  if (!(wz > 0.0f && wz <= FLT_MAX)) return false;   // behind the camera, overflowed or NaN
  const float nid = 1.0f / wz;
  const float u = (wx * nid) * fx + cx;
  const float v = (wy * nid) * fy + cy;
  const float ux = u + 0.5f, vy = v + 0.5f;
  if (!(ux >= 0.0f && ux < (float)g.cols && vy >= 0.0f && vy < (float)g.rows)) return false;   // outside the image (NaN too)
  float r = nid / (1.0f / Z);
  r *= r;
  r *= r;
  const float nvar = r * V;
  if (!(nvar >= 0.0f && nvar <= FLT_MAX)) return false;
  c.target = (int)vy * g.cols + (int)ux;
  c.key = ((unsigned long long)__builtin_bit_cast(uint32_t, wz) << 32) | ((unsigned long long)b << 24) | (unsigned long long)(unsigned)i;
  c.z = wz; c.nid = nid; c.nvar = nvar;
  c.x = wx; c.y = wy; c.u = u; c.v = v;
  return true;
}

// grid (tiles of the level) x B, map_count's pixel layout: one 64-bit unsigned minimum per candidate. z' > 0, so the order of its bits
// is the order of its values: the nearest surface wins, ties go to the lower request, then to the lower raster index.
__global__ __launch_bounds__(256) void render_min(RenderArgs a) {
  const unsigned b = blockIdx.y;
  const KfLevelDev& K = a.v.kf_tab[a.v.level * a.v.max_kf + map_slot(a.stage, b)];
  const LevelGeom& g = a.v.geom[a.v.level];
  const ELLC_GLOBAL float* depth = gptr(K.depth);
  const ELLC_GLOBAL float* var = gptr(K.var);
  const int cols = g.cols, rows = g.rows;
  const RenderT T = render_T12(a, b);   // block-uniform: scalar loads
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    MapPixel p;
    RenderCand c;
    if (!map_keep(a.v, depth, var, cols, rows, i, p)) continue;
    if (!render_candidate(g, T, b, i, p.x, p.y, p.Z, p.V, c)) continue;
    unsigned long long* k = a.keys + (unsigned)c.target;   // (target < cols * rows: render_candidate's bounds test)
    // the keys only ever fall: a stored key that is already smaller (however stale the load) makes the atomic pointless
    if (__hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= c.key) continue;
    (void)__hip_atomic_fetch_min(k, c.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// one thread per target: the winner's planes, and how many targets of the block have one
__global__ __launch_bounds__(256) void render_resolve(RenderArgs a) {
  const int t = (int)(blockIdx.x * 256u + threadIdx.x);
  const LevelGeom& g = a.v.geom[a.v.level];
  bool won = false;
  if (t < a.n) {
    const unsigned long long key = a.keys[(unsigned)t];
    float z = 0.0f, nvar = -1.0f;
    int32_t src = -1;
    uint32_t I = 0;
    if (key != ELLC_RENDER_EMPTY) {
      const unsigned b = (unsigned)(key >> 24) & 0xffu;
      const int i = (int)(key & 0xffffffull);
      const KfLevelDev& K = a.v.kf_tab[a.v.level * a.v.max_kf + a.stage[b]];
      const int y = i / g.cols, x = i - y * g.cols;
      RenderCand c;
      // (a key is only ever written for a pixel that gave a candidate: the same inputs give it again)
      if (render_candidate(g, render_T12(a, b), b, i, x, y, K.depth[(unsigned)i], K.var[(unsigned)i], c)) {
        won = true;
        z = c.z; nvar = c.nvar;
        src = (int32_t)(key & 0xffffffffull);
        I = K.img[(unsigned)(y * g.sw + x)];
      }
    }
    a.depth[(unsigned)t] = z;
    a.var[(unsigned)t] = nvar;
    a.source[(unsigned)t] = src;
    a.agree[(unsigned)t] = 0;
    a.intensity[(unsigned)t] = (uint8_t)I;
  }
  __shared__ int ws[4];
  const int n = __popcll(__ballot(won));
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) a.block_counts[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// One block: the sum of render_resolve's counts, for the host (integers: the order does not matter).
__global__ __launch_bounds__(256) void render_finish(RenderArgs a) {
  __shared__ int ws[4];
  int part = 0;
  for (int i = (int)threadIdx.x; i < a.blocks; i += 256) part += a.block_counts[i];
  int tot;
  wave_inclusive_scan(part, tot);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = tot;
  __syncthreads();
  if (threadIdx.x == 0) *a.n_valid = ws[0] + ws[1] + ws[2] + ws[3];
}

// render_min's grid: every candidate looks at its target's winner planes and counts itself in when its inverse depth agrees with the
// winner's within agree_k2 standard deviations^2 (the winner agrees with itself: d = 0).
__global__ __launch_bounds__(256) void render_agree(RenderArgs a) {
  const unsigned b = blockIdx.y;
  const KfLevelDev& K = a.v.kf_tab[a.v.level * a.v.max_kf + map_slot(a.stage, b)];
  const LevelGeom& g = a.v.geom[a.v.level];
  const ELLC_GLOBAL float* depth = gptr(K.depth);
  const ELLC_GLOBAL float* var = gptr(K.var);
  const int cols = g.cols, rows = g.rows;
  const RenderT T = render_T12(a, b);
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    MapPixel p;
    RenderCand c;
    if (!map_keep(a.v, depth, var, cols, rows, i, p)) continue;
    if (!render_candidate(g, T, b, i, p.x, p.y, p.Z, p.V, c)) continue;
    const float zw = a.depth[(unsigned)c.target], vw = a.var[(unsigned)c.target];
    const float d = c.nid - 1.0f / zw;   // (1 / z' of the winner: the same division render_candidate made for it)
    if (d * d <= a.agree_k2 * (c.nvar + vw)) (void)__hip_atomic_fetch_add(a.agree + (unsigned)c.target, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace ellc
