// ellc_keyframe_map_points: the semi-dense map of keyframe slots as filtered 3-D points (no reference counterpart: the reference
// only draws its depth map, DepthPropagation.cpp:1160-1250). Three launches, no waiting between blocks: map_count leaves one
// count per (request, tile), map_scan turns them into offsets in request-major order and hands the host the totals, map_scatter
// decides every pixel AGAIN with the same function and writes the kept ones at offset + raster rank inside the tile.
#pragma once
#include <float.h>
#include "ellc_kernels_prep.hpp"

namespace ellc {

// ellc_map_point as the kernels write it: three 8-byte words
struct MapRec {
  float x, y, z, var;
  uint16_t px, py;
  uint8_t intensity, support;
  uint16_t source;
};

// what map_keep reads: the ring's tables, the level and the filter. Every ring kernel's arguments begin with one. (The kernels take
// their arguments as one struct, which the kernel-argument preload leaves alone: the fields are scalar loads wherever they sit.)
struct MapView {
  const LevelGeom* geom;
  const KfLevelDev* kf_tab;
  int level, max_kf, tiles;
  float max_var;
  int min_support;
  float support_k2;
  int stride;
};

// ... and what the point export writes
struct MapArgs {
  MapView v;
  const int* stage;          // [max_kf] keyframe slot of every request, then [max_kf][12] f32 transforms (device copy of the pinned record)
  int* tile_counts;          // [B][tiles]: kept pixels per tile (map_count)
  unsigned* tile_offsets;    // [B][tiles]: records in front of the tile, request-major (map_scan)
  int* totals;               // pinned, through its device-side address: [max_kf] points per request, [max_kf] = their sum (map_scan)
  MapRec* out;               // device staging of the records (map_scatter)
  unsigned out_cap;          //   and how many it holds: the call's total
  int B;
};

// the keyframe slot of request b in a [max_kf] slots, [max_kf][12] transforms record, and its transform
// (block-uniform: through readfirstlane as prep_slot does, so that the slot's table entry stays in scalar registers)
__device__ __forceinline__ int map_slot(const int* stage, unsigned b) { return __builtin_amdgcn_readfirstlane(stage[b]); }
__device__ __forceinline__ const float* map_T12(const int* stage, int max_kf, unsigned b) { return (const float*)(stage + max_kf) + 12u * b; }

// a pixel that holds a hypothesis a point can be made of: NaN fails all three tests; updateDepthImage writes 1 / invDepthSmoothed
// for any invDepthSmoothed >= -0.05 (DepthPropagation.cpp:1285-1289), so +inf and negative depths do occur
__device__ __forceinline__ bool map_ok(float Z, float V) { return Z > 0.0f && Z <= FLT_MAX && V >= 0.0f; }

struct MapPixel {
  float Z, V;
  int x, y, support;
};

// THE rule, for map_count and map_scatter alike: is pixel i of the level kept, and what does its record need. The neighbours are read
// from global memory (adjacent threads read the same lines) and only for a centre that passed every test of its own.
__device__ __forceinline__ bool map_keep(const MapView& a, const ELLC_GLOBAL float* depth, const ELLC_GLOBAL float* var, int cols, int rows, int i, MapPixel& p) {
  if (i >= cols * rows) return false;
  const float Z = depth[(unsigned)i], V = var[(unsigned)i];
  if (!map_ok(Z, V)) return false;
  const int y = i / cols, x = i - y * cols;
  if (x % a.stride != 0 || y % a.stride != 0) return false;
  if (a.max_var > 0.0f && !(V <= a.max_var)) return false;
  const float iZ = 1.0f / Z;
  int support = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      if (dx == 0 && dy == 0) continue;
      const int xn = x + dx, yn = y + dy;
      if (xn < 0 || xn >= cols || yn < 0 || yn >= rows) continue;
      const unsigned in = (unsigned)(yn * cols + xn);
      const float Zn = depth[in], Vn = var[in];
      if (!map_ok(Zn, Vn)) continue;
      const float d = 1.0f / Zn - iZ;
      if (d * d <= a.support_k2 * (V + Vn)) support++;
    }
  if (support < a.min_support) return false;
  p.Z = Z; p.V = V; p.x = x; p.y = y; p.support = support;
  return true;
}

// Thread t of tile `local` owns pixels local * ELLC_TILE + j * 256 + t, j = 0..7 (prep_scatter's layout: a wave's loads are contiguous
// and (j, wave, lane) is raster order).
__global__ __launch_bounds__(256) void map_count(MapArgs a) {
  const int local = (int)blockIdx.x;
  const KfLevelDev& K = a.v.kf_tab[a.v.level * a.v.max_kf + map_slot(a.stage, blockIdx.y)];
  const LevelGeom& g = a.v.geom[a.v.level];
  const ELLC_GLOBAL float* depth = gptr(K.depth);
  const ELLC_GLOBAL float* var = gptr(K.var);
  const int cols = g.cols, rows = g.rows;
  const int base = local * ELLC_TILE + (int)threadIdx.x;
  int c = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    MapPixel p;
    c += map_keep(a.v, depth, var, cols, rows, base + j * 256, p) ? 1 : 0;
  }
  __shared__ int ws[4];
  int tot;
  wave_inclusive_scan(c, tot);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = tot;
  __syncthreads();
  if (threadIdx.x == 0) a.tile_counts[blockIdx.y * (unsigned)a.v.tiles + (unsigned)local] = ws[0] + ws[1] + ws[2] + ws[3];
}

// One block: exclusive scan of the B x tiles counts in request-major order; points per request and their sum for the host. Thread t
// owns a run of consecutive counts: it sums them (independent loads), the 256 sums are scanned, and it walks its run again to leave
// the offsets. (B x tiles is a few thousand at 640x480; the sum of a call is bounded by the host: it fits an int. The first form
// scanned request after request, 256 counts a step: 43 dependent steps of a load, two barriers and a store each made this launch
// most of the call's device time.)
__global__ __launch_bounds__(256) void map_scan(MapArgs a) {
  __shared__ int ws[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned N = (unsigned)a.B * (unsigned)a.v.tiles;
  const unsigned per = (N + 255u) / 256u;
  const unsigned i0 = min(N, threadIdx.x * per), i1 = min(N, i0 + per);
  int part = 0;
  for (unsigned i = i0; i < i1; i++) part += a.tile_counts[i];
  int tot;
  const int inc = wave_inclusive_scan(part, tot);
  if (lane == 0) ws[wave] = tot;
  __syncthreads();
  int run = inc - part;
#pragma unroll
  for (int w = 0; w < 4; w++) run += (w < wave) ? ws[w] : 0;
  const int total = ws[0] + ws[1] + ws[2] + ws[3];
  for (unsigned i = i0; i < i1; i++) {
    a.tile_offsets[i] = (unsigned)run;
    run += a.tile_counts[i];
  }
  __syncthreads();   // the offsets the block's other threads wrote are read below
  for (int b = (int)threadIdx.x; b < a.B; b += 256) {
    const unsigned s0 = a.tile_offsets[(unsigned)b * (unsigned)a.v.tiles];
    const unsigned s1 = (b + 1 < a.B) ? a.tile_offsets[(unsigned)(b + 1) * (unsigned)a.v.tiles] : (unsigned)total;
    a.totals[b] = (int)(s1 - s0);
  }
  if (threadIdx.x == 0) a.totals[a.v.max_kf] = total;
}

__global__ __launch_bounds__(256) void map_scatter(MapArgs a) {
  const int local = (int)blockIdx.x;
  const unsigned b = blockIdx.y;
  const KfLevelDev K = a.v.kf_tab[a.v.level * a.v.max_kf + map_slot(a.stage, b)];
  const LevelGeom& g = a.v.geom[a.v.level];
  const ELLC_GLOBAL float* depth = gptr(K.depth);
  const ELLC_GLOBAL float* var = gptr(K.var);
  const ELLC_GLOBAL uint8_t* img = gptr(K.img);
  const int cols = g.cols, rows = g.rows, sw = g.sw;
  const int base = local * ELLC_TILE + (int)threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int cnt[32];   // [j][wave] exclusive offsets inside the tile
  MapPixel p[8];
  bool keep[8];
  unsigned long long m[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    keep[j] = map_keep(a.v, depth, var, cols, rows, base + j * 256, p[j]);
    m[j] = __ballot(keep[j]);
    if (lane == 0) cnt[j * 4 + wave] = __popcll(m[j]);
  }
  __syncthreads();
  if (threadIdx.x < 64) {   // exclusive scan of the 32 (j, wave) counts
    int v = (lane < 32) ? cnt[lane] : 0, tot;
    const int inc = wave_inclusive_scan(v, tot);
    if (lane < 32) cnt[lane] = inc - v;
  }
  __syncthreads();
  const unsigned tile_off = a.tile_offsets[b * (unsigned)a.v.tiles + (unsigned)local];
  const float fx = g.fx, fy = g.fy, cx = g.cx, cy = g.cy;
  const float* T = map_T12(a.stage, a.v.max_kf, b);   // block-uniform: scalar loads
  const float t0 = T[0], t1 = T[1], t2 = T[2], t3 = T[3], t4 = T[4], t5 = T[5], t6 = T[6], t7 = T[7], t8 = T[8], t9 = T[9], t10 = T[10], t11 = T[11];
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (!keep[j]) continue;
    const unsigned pos = tile_off + (unsigned)cnt[j * 4 + wave] + (unsigned)__popcll(m[j] & lt);
    if (pos >= a.out_cap) continue;   // (cannot happen: both passes decide a pixel with map_keep; the staging is never overrun)
    const int x = p[j].x, y = p[j].y;
    const float Z = p[j].Z;
    // the reference's back-projection and transform, in its order (PixelWisePyramid.cpp:236-238, :244)
    const float X = (((float)x - cx) * Z) / fx;
    const float Y = (((float)y - cy) * Z) / fy;
    const float wx = ((t0 * X + t1 * Y) + t2 * Z) + t3;
    const float wy = ((t4 * X + t5 * Y) + t6 * Z) + t7;
    const float wz = ((t8 * X + t9 * Y) + t10 * Z) + t11;
    const uint32_t I = img[(unsigned)(y * sw + x)];
    ELLC_GLOBAL u32x2* r = (ELLC_GLOBAL u32x2*)((ELLC_GLOBAL char*)a.out + (size_t)pos * sizeof(MapRec));
    r[0] = (u32x2){__builtin_bit_cast(uint32_t, wx), __builtin_bit_cast(uint32_t, wy)};
    r[1] = (u32x2){__builtin_bit_cast(uint32_t, wz), __builtin_bit_cast(uint32_t, p[j].V)};
    r[2] = (u32x2){(uint32_t)x | ((uint32_t)y << 16), I | ((uint32_t)p[j].support << 8) | (b << 16)};
  }
}

}  // namespace ellc
