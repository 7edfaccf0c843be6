// ellc_keyframe_fuse_depth: the render's view with the candidates that agree with a target's winner merged into it (the EKF-style
// merge of DepthPropagation.cpp:1124-1148) in a FIXED order, so that the result stays a function of the inputs alone. The render's own
// kernels run first, as they stand (ellc_kernels_render.hpp; fuse_agree is render_agree with a memory): afterwards agree[target] is the number of candidates that agree with
// the target's winner, the winner included — the size of the target's segment in a list of 32-bit candidate ids (b << 24) | i.
//   fuse_agree                      in place of render_agree (the same walk, test and count): it also keeps a bit per decision
//   fuse_tile_sums + fuse_offsets   exclusive scan of the agree plane: cursor[target] = where the target's segment begins
//   fuse_scatter                    the walk again over the kept bits; every agreeing candidate takes the next entry of its target's segment
//                                   (an integer atomic on the cursor: arrival order is arbitrary, and afterwards cursor[target] is
//                                   where the segment ENDS — one plane serves as offset and as cursor)
//   fuse_merge + fuse_finish        one thread per target: members in ascending id order, selected from the segment eight at a walk
// No waiting between blocks, integer atomics only, no floating-point atomics. render_candidate and map_keep decide every pass.
#pragma once
#include "ellc_kernels_render.hpp"

namespace ellc {

struct FuseArgs {
  RenderArgs r;                    // the render's arguments: its planes are the winner's, read here and overwritten where a target fuses
  unsigned* cursor;                // [n]: begin of the target's segment (fuse_offsets), its end once fuse_scatter has run
  unsigned long long* tile_sums;   // [tiles]: agreeing candidates per tile of ELLC_TILE targets (fuse_tile_sums)
  unsigned long long* mask;        // [B][tiles][8][4]: which source pixels agree with their target's winner, a wave's ballot per word (fuse_agree)
  uint32_t* list;                  // [list_cap]: the segments, target after target
  unsigned list_cap;               //   entries it holds: the call's total
  int32_t* merged;                 // [n]: hypotheses fused into the target, the winner included (0: no winner)
  int* block_counts;               // [blocks]: targets with merged >= 2 per block of fuse_merge
  long long* totals;               // pinned, through its device-side address: [0] the list's size (fuse_offsets), [1] n_fused (fuse_finish)
  int max_merge;
};

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// thread t of a tile owns targets tile * ELLC_TILE + 8 t .. + 7 (raster order across the threads); counts are >= 0
__device__ __forceinline__ void fuse_load8(const FuseArgs& a, int first, unsigned v[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = (first + j < a.r.n) ? (unsigned)a.r.agree[(unsigned)(first + j)] : 0u;
}

// grid (tiles of the level): the sum of a tile's counts, in 64 bits (256 requests on 2^24 pixels do not fit 32)
__global__ __launch_bounds__(256) void fuse_tile_sums(FuseArgs a) {
  unsigned v[8];
  fuse_load8(a, (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x * 8, v);
  unsigned long long part = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) part += v[j];
  part = wave_sum64(part);
  __shared__ unsigned long long ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) a.tile_sums[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// grid (tiles of the level): every block adds up the tiles in front of its own (a few hundred words at 640x480; integers: the order
// does not matter), scans its own tile and leaves cursor[target] = candidates in front of the target. The last block hands the host the
// total. Offsets are 32-bit: the host refuses a total beyond 2^31 - 1 before anything reads them.
__global__ __launch_bounds__(256) void fuse_offsets(FuseArgs a) {
  __shared__ unsigned long long wb[4];
  __shared__ int ws[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long before = 0;
  for (unsigned i = threadIdx.x; i < blockIdx.x; i += 256) before += a.tile_sums[i];
  before = wave_sum64(before);
  if (lane == 0) wb[wave] = before;
  const int first = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x * 8;
  unsigned v[8];
  fuse_load8(a, first, v);
  unsigned part = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) part += v[j];
  int tot;
  const int inc = wave_inclusive_scan((int)part, tot);
  if (lane == 0) ws[wave] = tot;
  __syncthreads();
  const unsigned long long base = (wb[0] + wb[1]) + (wb[2] + wb[3]);
  unsigned run = (unsigned)base + ((unsigned)inc - part);
#pragma unroll
  for (int w = 0; w < 4; w++) run += (w < wave) ? (unsigned)ws[w] : 0u;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (first + j < a.r.n) a.cursor[(unsigned)(first + j)] = run;
    run += v[j];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) a.totals[0] = (long long)(base + a.tile_sums[blockIdx.x]);
}

// (request, tile, step j, wave) -> the word of the mask that holds the wave's 64 decisions of that step
__device__ __forceinline__ unsigned fuse_mask_word(const FuseArgs& a, unsigned b, unsigned tile, int j) {
  return ((b * (unsigned)a.r.v.tiles + tile) * 8u + (unsigned)j) * 4u + (threadIdx.x >> 6);
}

// render_agree (its grid, walk, test and count, through the same device functions: the agree plane is the render's) that also KEEPS what it
// decided: one bit per source pixel of every request, a wave's ballot per step. fuse_scatter reads the bits instead of deciding every
// pixel a third time: map_keep's sixteen neighbour loads per centre are what the walks over the sources cost.
__global__ __launch_bounds__(256) void fuse_agree(FuseArgs a) {
  const unsigned b = blockIdx.y;
  const KfLevelDev& K = a.r.v.kf_tab[a.r.v.level * a.r.v.max_kf + map_slot(a.r.stage, b)];
  const LevelGeom& g = a.r.v.geom[a.r.v.level];
  const ELLC_GLOBAL float* depth = gptr(K.depth);
  const ELLC_GLOBAL float* var = gptr(K.var);
  const int cols = g.cols, rows = g.rows;
  const RenderT T = render_T12(a.r, b);
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    MapPixel p;
    RenderCand c;
    bool ok = false;
    if (map_keep(a.r.v, depth, var, cols, rows, i, p) && render_candidate(g, T, b, i, p.x, p.y, p.Z, p.V, c)) {
      const float zw = a.r.depth[(unsigned)c.target], vw = a.r.var[(unsigned)c.target];
      const float d = c.nid - 1.0f / zw;   // (1 / z' of the winner: the same division render_candidate made for it)
      ok = d * d <= a.r.agree_k2 * (c.nvar + vw);
      if (ok) (void)__hip_atomic_fetch_add(a.r.agree + (unsigned)c.target, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long decided = __ballot(ok);
    if ((threadIdx.x & 63) == 0) a.mask[fuse_mask_word(a, b, blockIdx.x, j)] = decided;
  }
}

// fuse_agree's grid and walk: every candidate it counted computes its target again and writes its id into the target's segment
__global__ __launch_bounds__(256) void fuse_scatter(FuseArgs a) {
  const unsigned b = blockIdx.y;
  const KfLevelDev& K = a.r.v.kf_tab[a.r.v.level * a.r.v.max_kf + map_slot(a.r.stage, b)];
  const LevelGeom& g = a.r.v.geom[a.r.v.level];
  const ELLC_GLOBAL float* depth = gptr(K.depth);
  const ELLC_GLOBAL float* var = gptr(K.var);
  const int cols = g.cols;
  const RenderT T = render_T12(a.r, b);
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    const unsigned long long decided = a.mask[fuse_mask_word(a, b, blockIdx.x, j)];
    if (!((decided >> (threadIdx.x & 63)) & 1ull) || i >= a.r.n) continue;   // (a set bit is a kept pixel: i < n)
    const int y = i / cols, x = i - y * cols;
    RenderCand c;
    if (!render_candidate(g, T, b, i, x, y, depth[(unsigned)i], var[(unsigned)i], c)) continue;   // (the same inputs gave it before)
    const unsigned pos = __hip_atomic_fetch_add(a.cursor + (unsigned)c.target, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pos >= a.list_cap) continue;   // (cannot happen: fuse_agree counted this candidate; the list is never overrun)
    a.list[pos] = (b << 24) | (unsigned)i;
  }
}

#define ELLC_FUSE_TAKE 8   // members one walk over a segment selects

// One thread per target. Its segment holds the ids of the winner and of the members in arbitrary order. One walk over it leaves the
// ELLC_FUSE_TAKE smallest ids greater than the last one taken, sorted, in registers (a min / max chain per entry: no per-thread array
// in memory, no sort) and counts how many qualify, so a target with at most that many members is done after ONE walk; the first form
// took one member per walk, (members + 1) x segment loads a thread, each a cache line of its own. segment x ceil(visited /
// ELLC_FUSE_TAKE) loads, bounded by max_merge <= 64 where a transform piles a map onto one pixel. A member's values are computed AGAIN
// from its slot's planes, as render_resolve does for the winner, and merged in IEEE f32, this order (DepthPropagation.cpp:1128, :1129,
// :1139; no contraction, correctly rounded divisions).
__global__ __launch_bounds__(256) void fuse_merge(FuseArgs a) {
  const int t = (int)(blockIdx.x * 256u + threadIdx.x);
  const LevelGeom& g = a.r.v.geom[a.r.v.level];
  bool fused = false;
  if (t < a.r.n) {
    // a target has a winner iff its depth is z' > 0 (render_resolve); its source is no sign to go by: request 128 and up set bit 31
    const float zw = a.r.depth[(unsigned)t];
    const uint32_t src = (uint32_t)a.r.source[(unsigned)t];
    int m = 0;
    if (zw > 0.0f) {
      m = 1;
      const unsigned end = a.cursor[(unsigned)t], size = (unsigned)a.r.agree[(unsigned)t];
      if (size >= 2u && size <= end && end <= a.list_cap) {
        const unsigned begin = end - size;
        float id_t = 1.0f / zw, var_t = a.r.var[(unsigned)t];   // (1 / z' of the winner: the division render_candidate made for it)
        long long last = -1;
        int visited = 0;
        while (visited < a.max_merge) {
          // (an id of 0xffffffff is the largest there is: it ends up where the preset stands, and `more` says that it is one)
          uint32_t c[ELLC_FUSE_TAKE];
#pragma unroll
          for (int j = 0; j < ELLC_FUSE_TAKE; j++) c[j] = 0xffffffffu;
          unsigned more = 0;
          for (unsigned k = begin; k < end; k++) {
            const uint32_t id = a.list[k];
            const bool ok = (long long)id > last && id != src;
            more += ok ? 1u : 0u;
            uint32_t x = ok ? id : 0xffffffffu;
#pragma unroll
            for (int j = 0; j < ELLC_FUSE_TAKE; j++) {
              const uint32_t lo = min(c[j], x);
              x = max(c[j], x);
              c[j] = lo;
            }
          }
#pragma unroll
          for (int j = 0; j < ELLC_FUSE_TAKE; j++) {
            if ((unsigned)j >= more || visited >= a.max_merge) break;
            visited++;
            last = (long long)c[j];
            const unsigned b = c[j] >> 24, i = c[j] & 0xffffffu;
            if (b >= (unsigned)a.r.B || i >= (unsigned)a.r.n) continue;   // (cannot happen: fuse_scatter wrote the id)
            const KfLevelDev& K = a.r.v.kf_tab[a.r.v.level * a.r.v.max_kf + a.r.stage[b]];
            const int y = (int)i / g.cols, x = (int)i - y * g.cols;
            RenderCand cand;
            if (!render_candidate(g, render_T12(a.r, b), b, (int)i, x, y, K.depth[i], K.var[i], cand)) continue;   // (the same inputs gave it before)
            const float s = var_t + cand.nvar;
            if (!(s > 0.0f && s <= FLT_MAX)) continue;   // both variances 0, or their sum overflowed: skipped, not counted
            const float w = cand.nvar / s;
            id_t = (w * id_t) + ((1.0f - w) * cand.nid);
            var_t = 1.0f / ((1.0f / var_t) + (1.0f / cand.nvar));
            m++;
          }
          if (more <= (unsigned)ELLC_FUSE_TAKE) break;   // every member there was has been visited
        }
        if (m >= 2) {
          fused = true;
          a.r.depth[(unsigned)t] = 1.0f / id_t;
          a.r.var[(unsigned)t] = var_t;
        }
      }
    }
    a.merged[(unsigned)t] = m;
  }
  __shared__ int ws[4];
  const int n = __popcll(__ballot(fused));
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) a.block_counts[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// One block: the sum of fuse_merge's counts, for the host (as render_finish)
__global__ __launch_bounds__(256) void fuse_finish(FuseArgs a) {
  __shared__ int ws[4];
  int part = 0;
  for (int i = (int)threadIdx.x; i < a.r.blocks; i += 256) part += a.block_counts[i];
  int tot;
  wave_inclusive_scan(part, tot);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = tot;
  __syncthreads();
  if (threadIdx.x == 0) a.totals[1] = (long long)(ws[0] + ws[1] + ws[2] + ws[3]);
}

}  // namespace ellc
