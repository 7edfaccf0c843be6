// ellc_depth_absorb_keyframes: the maps of keyframe slots folded into the LIVE hypothesis state of the depth map (the per-hypothesis rule
// of depthMap::propagateDepth, DepthPropagation.cpp:1003-1157, for several sources and without its wipe of the destination), in a FIXED
// order, so that the result stays a function of the inputs alone. ellc_keyframe_fuse_depth's shape (ellc_kernels_fuse.hpp) without
// the render's winner passes:
//   absorb_mark                     fuse_agree's grid and walk: map_keep, render_candidate, the interior bound of :1059 and the photometric
//                                   gate of :1066-1076 decide every source pixel; a survivor counts itself in at its target (an integer
//                                   atomic), and a bit per source pixel keeps the decision
//   fuse_tile_sums + fuse_offsets   the exclusive scan of the count plane, as they stand: cursor[target] = where the target's segment begins
//   absorb_scatter                  the walk again over the kept bits: every candidate takes the next entry of its target's segment
//   absorb_fold + absorb_finish     one thread per target: its candidates in ascending id order, eight at a walk (fuse_merge's selection),
//                                   folded in registers into the target's own hypothesis, which is written in place
//   (the _lit entry points hand absorb_mark a light per request, gain and offset beside its T in the staging; the unlit ones stage
//   (1, 0) and go through the same kernels)
//   absorb_wipe                     ellc_depth_restart_from_keyframes only, in front of the scatter: every hypothesis empty
// No waiting between blocks, integer atomics only, no floating-point atomics. render_candidate and map_keep decide every pass.
// absorb_interior and absorb_photo, the two halves of absorb_mark's gate, also decide ellc_keyframe_trial_propagate's pass (ellc_kernels_trial.hpp).
#pragma once
#include "ellc_context.hpp"
#include "ellc_kernels_fuse.hpp"
#include "ellc_kernels_sim3.hpp"

namespace ellc {

#define ELLC_ABSORB_FOLD_COUNTS 11   // what absorb_fold counts per block, in the order of ellc_absorb_stats from n_visited on

struct AbsorbArgs {
  FuseArgs f;                  // the fusion's arguments: r.agree is the count plane (candidates per target), cursor, tile_sums, mask, list, totals
  DepthSoA s;                  // the live state: every thread of absorb_fold reads and writes its own hypothesis only
  const uint8_t* k_img;        // K's level-0 image (pitch geom.sw) and maxAbsGradient plane (the photometric gate)
  const float* k_maxgrad;
  int* mark_counts;            // [4]: n_kept, n_in_view, n_interior, n_candidates (zero in front of absorb_mark)
  int* fold_counts;            // [blocks][ELLC_ABSORB_FOLD_COUNTS]
  int32_t* stats;              // pinned, through its device-side address: the sixteen words of ellc_absorb_stats (absorb_finish)
  int max_fold, photo_gate, src_validity;
};

// The interior bound of :1059 on a candidate's projection: inside it the four bilinear taps exist
__device__ __forceinline__ bool absorb_interior(const LevelGeom& g, const RenderCand& c) {
  return c.u > 2.1f && c.v > 2.1f && c.u < (float)g.cols - 3.1f && c.v < (float)g.rows - 3.1f;
}

// The light of request b in the absorb's staging: [max_kf][2] f32 (gain, offset) behind the slots and the transforms (block-uniform
// where the request is: scalar loads)
__device__ __forceinline__ void absorb_light(const int* stage, int max_kf, unsigned b, float& gain, float& offset) {
  const float* l = (const float*)(stage + 13u * (unsigned)max_kf) + 2u * b;
  gain = l[0];
  offset = l[1];
}

// The photometric gate of :1066-1076 (MAX_DIFF_CONSTANT 1600, MAX_DIFF_GRAD_MULT 0.25, MIN_ABS_GRAD_DECREASE 5) on an INTERIOR candidate of
// source pixel (x, y) of image `img`, against the destination's level-0 image k_img (pitch g.sw) and maxAbsGradient plane k_maxgrad: does
// the candidate pass. The source's grey value goes through the request's light first, Ip = gain * Is + offset (two roundings; (1, 0)
// gives Is bit for bit); gr and both constants stay in the destination's units. r = Iw - Ip and gr (the gradient at the TARGET) are
// handed back for ellc_keyframe_trial_propagate's sums, Iw and Is for the sums of its fit.
__device__ __forceinline__ bool absorb_photo(const LevelGeom& g, const uint8_t* k_img, const float* k_maxgrad, const ELLC_GLOBAL uint8_t* img, int x, int y,
                                             const RenderCand& c, float gain, float offset, float& r, float& gr, float& Iw, float& Is) {
  // 2 < u < cols - 3 and 2 < v < rows - 3: the four taps exist
  const int x0 = (int)c.u, y0 = (int)c.v;
  const unsigned t0 = (unsigned)(y0 * g.sw + x0);
  const float I00 = (float)k_img[t0], I01 = (float)k_img[t0 + 1u], I10 = (float)k_img[t0 + (unsigned)g.sw], I11 = (float)k_img[t0 + (unsigned)g.sw + 1u];
  const float ax = c.u - (float)x0, ay = c.v - (float)y0;
  float gx, gy;
  Iw = sim3_bilinear(I00, I01, I10, I11, ax, ay, gx, gy);
  Is = (float)img[(unsigned)(y * g.sw + x)];
  r = Iw - __fadd_rn(__fmul_rn(gain, Is), offset);
  gr = k_maxgrad[(unsigned)c.target];   // at the TARGET (the reference reads the source's coordinates: dm_prop_project's Q14)
  return !((r * r) / (1600.0f + (0.25f * gr) * gr) > 1.0f || gr < 5.0f);
}

// THE rule behind render_candidate, for absorb_mark: does the candidate of source pixel (x, y) of image `img` pass the interior bound
// and, when it is on, the photometric gate against k_img / k_maxgrad at the request's light
__device__ __forceinline__ bool absorb_gate(const LevelGeom& g, const uint8_t* k_img, const float* k_maxgrad, int photo_gate, const ELLC_GLOBAL uint8_t* img,
                                            int x, int y, const RenderCand& c, float gain, float offset, bool& interior) {
  interior = absorb_interior(g, c);
  if (!interior) return false;
  if (!photo_gate) return true;
  float r, gr, Iw, Is;
  return absorb_photo(g, k_img, k_maxgrad, img, x, y, c, gain, offset, r, gr, Iw, Is);
}

// fuse_agree's grid (tiles of level 0) x B and walk
__global__ __launch_bounds__(256) void absorb_mark(AbsorbArgs a) {
  const RenderArgs& ra = a.f.r;
  const unsigned b = blockIdx.y;
  const KfLevelDev& K = ra.v.kf_tab[ra.v.level * ra.v.max_kf + map_slot(ra.stage, b)];
  const LevelGeom& g = ra.v.geom[ra.v.level];
  const ELLC_GLOBAL float* depth = gptr(K.depth);
  const ELLC_GLOBAL float* var = gptr(K.var);
  const ELLC_GLOBAL uint8_t* img = gptr(K.img);
  const int cols = g.cols, rows = g.rows;
  const RenderT T = render_T12(ra, b);
  float gain, offset;
  absorb_light(ra.stage, ra.v.max_kf, b, gain, offset);
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
  int n_kept = 0, n_view = 0, n_int = 0, n_cand = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    MapPixel p;
    RenderCand c;
    bool ok = false;
    if (map_keep(ra.v, depth, var, cols, rows, i, p)) {
      n_kept++;
      if (render_candidate(g, T, b, i, p.x, p.y, p.Z, p.V, c)) {
        n_view++;
        bool interior;
        ok = absorb_gate(g, a.k_img, a.k_maxgrad, a.photo_gate, img, p.x, p.y, c, gain, offset, interior);
        n_int += interior ? 1 : 0;
        if (ok) {
          n_cand++;
          (void)__hip_atomic_fetch_add(ra.agree + (unsigned)c.target, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (target < cols * rows)
        }
      }
    }
    const unsigned long long decided = __ballot(ok);
    if ((threadIdx.x & 63) == 0) a.f.mask[fuse_mask_word(a.f, b, blockIdx.x, j)] = decided;
  }
  __shared__ int ws[4][4];
  int v[4] = {n_kept, n_view, n_int, n_cand};
#pragma unroll
  for (int k = 0; k < 4; k++) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = (int)threadIdx.x, sum = ws[0][k] + ws[1][k] + ws[2][k] + ws[3][k];
    if (sum) (void)__hip_atomic_fetch_add(a.mark_counts + k, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (integers: the order does not matter)
  }
}

// fuse_scatter over absorb_mark's bits
__global__ __launch_bounds__(256) void absorb_scatter(AbsorbArgs a) {
  const RenderArgs& ra = a.f.r;
  const unsigned b = blockIdx.y;
  const KfLevelDev& K = ra.v.kf_tab[ra.v.level * ra.v.max_kf + map_slot(ra.stage, b)];
  const LevelGeom& g = ra.v.geom[ra.v.level];
  const ELLC_GLOBAL float* depth = gptr(K.depth);
  const ELLC_GLOBAL float* var = gptr(K.var);
  const int cols = g.cols;
  const RenderT T = render_T12(ra, b);
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    const unsigned long long decided = a.f.mask[fuse_mask_word(a.f, b, blockIdx.x, j)];
    if (!((decided >> (threadIdx.x & 63)) & 1ull) || i >= ra.n) continue;   // (a set bit is a kept pixel: i < n)
    const int y = i / cols, x = i - y * cols;
    RenderCand c;
    if (!render_candidate(g, T, b, i, x, y, depth[(unsigned)i], var[(unsigned)i], c)) continue;   // (the same inputs gave it before)
    const unsigned pos = __hip_atomic_fetch_add(a.f.cursor + (unsigned)c.target, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pos >= a.f.list_cap) continue;   // (cannot happen: absorb_mark counted this candidate; the list is never overrun)
    a.f.list[pos] = (b << 24) | (unsigned)i;
  }
}

// One thread per target: fuse_merge's walk (the ELLC_FUSE_TAKE smallest ids greater than the last one taken per walk over the segment),
// every candidate computed AGAIN from its slot's planes, and the five outcomes of DepthPropagation.cpp:1090-1148 in IEEE f32, this order
// (no contraction, correctly rounded divisions). The hypothesis is read once, folded in registers and written once, where it changed.
__global__ __launch_bounds__(256) void absorb_fold(AbsorbArgs a) {
  const RenderArgs& ra = a.f.r;
  const int t = (int)(blockIdx.x * 256u + threadIdx.x);
  const LevelGeom& g = ra.v.geom[ra.v.level];
  int n[ELLC_ABSORB_FOLD_COUNTS];   // visited, created, merged, replaced, occluded, skipped, hit, touched, truncated, valid before, valid after
#pragma unroll
  for (int k = 0; k < ELLC_ABSORB_FOLD_COUNTS; k++) n[k] = 0;
  if (t < ra.n) {
    bool valid = a.s.isValid[(unsigned)t] != 0;
    n[9] = valid ? 1 : 0;
    const unsigned end = a.f.cursor[(unsigned)t], size = (unsigned)ra.agree[(unsigned)t];
    bool touched = false;
    if (size >= 1u && size <= end && end <= a.f.list_cap) {
      n[6] = 1;
      n[8] = size > (unsigned)a.max_fold ? 1 : 0;
      const unsigned begin = end - size;
      float id_t = a.s.invDepth[(unsigned)t], var_t = a.s.variance[(unsigned)t];
      int val = a.s.validity[(unsigned)t];
      long long last = -1;
      int visited = 0;
      while (visited < a.max_fold) {
        uint32_t c[ELLC_FUSE_TAKE];
#pragma unroll
        for (int j = 0; j < ELLC_FUSE_TAKE; j++) c[j] = 0xffffffffu;
        unsigned more = 0;
        for (unsigned k = begin; k < end; k++) {
          const uint32_t id = a.f.list[k];
          const bool ok = (long long)id > last;
          more += ok ? 1u : 0u;
          uint32_t x = ok ? id : 0xffffffffu;
#pragma unroll
          for (int j = 0; j < ELLC_FUSE_TAKE; j++) {
            const uint32_t lo = min(c[j], x);
            x = max(c[j], x);
            c[j] = lo;
          }
        }
        // the selected ids one after the other through c[0] (ONE copy of the fold's branches: unrolled eight times, their saved
        // execution masks alone spilled scalar registers)
#pragma unroll 1
        for (unsigned j = 0; j < (unsigned)ELLC_FUSE_TAKE && j < more && visited < a.max_fold; j++) {
          const uint32_t cid = c[0];
#pragma unroll
          for (int k = 0; k + 1 < ELLC_FUSE_TAKE; k++) c[k] = c[k + 1];
          visited++;
          last = (long long)cid;
          const unsigned b = cid >> 24, i = cid & 0xffffffu;
          RenderCand cand;
          bool have = b < (unsigned)ra.B && i < (unsigned)ra.n;   // (always: absorb_scatter wrote the id)
          if (have) {
            const KfLevelDev& K = ra.v.kf_tab[ra.v.level * ra.v.max_kf + ra.stage[b]];
            const int y = (int)i / g.cols, x = (int)i - y * g.cols;
            have = render_candidate(g, render_T12(ra, b), b, (int)i, x, y, K.depth[i], K.var[i], cand);   // (the same inputs gave it before)
          }
          if (!have) {   // (cannot happen; counted as skipped so that the identity of the stats holds whatever happens)
            n[5]++;
            continue;
          }
          if (!valid) {   // :1109-1121
            id_t = cand.nid; var_t = cand.nvar; val = a.src_validity;
            valid = true; touched = true;
            n[1]++;
            continue;
          }
          const float d = cand.nid - id_t;
          if (!(d * d <= a.f.r.agree_k2 * (cand.nvar + var_t))) {   // a conflict (NaN too)
            if (d < 0.0f) {   // :1096-1099: behind what is there
              n[4]++;
            } else {          // :1101-1121: in front of it
              id_t = cand.nid; var_t = cand.nvar; val = a.src_validity;
              touched = true;
              n[3]++;
            }
            continue;
          }
          const float s = var_t + cand.nvar;
          if (!(s > 0.0f && s <= FLT_MAX)) {   // both variances 0, or their sum overflowed
            n[5]++;
            continue;
          }
          const float w = cand.nvar / s;   // :1128-1140
          id_t = (w * id_t) + ((1.0f - w) * cand.nid);
          var_t = 1.0f / ((1.0f / var_t) + (1.0f / cand.nvar));
          val = min(val + a.src_validity, 255);
          touched = true;
          n[2]++;
        }
        if (more <= (unsigned)ELLC_FUSE_TAKE) break;   // every candidate there was has been visited
      }
      n[0] = visited;
      if (touched) {   // :1112-1118, :1138-1145
        n[7] = 1;
        a.s.invDepth[(unsigned)t] = id_t;
        a.s.variance[(unsigned)t] = var_t;
        a.s.validity[(unsigned)t] = val;
        a.s.isValid[(unsigned)t] = (uint8_t)1;
        a.s.blacklisted[(unsigned)t] = 0;
        a.s.invDepthSmoothed[(unsigned)t] = -1.0f;
        a.s.varianceSmoothed[(unsigned)t] = -1.0f;
      }
    }
    n[10] = valid ? 1 : 0;
  }
  __shared__ int ws[4][ELLC_ABSORB_FOLD_COUNTS];
#pragma unroll
  for (int k = 0; k < ELLC_ABSORB_FOLD_COUNTS; k++) {
    int v = n[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < ELLC_ABSORB_FOLD_COUNTS)
    a.fold_counts[blockIdx.x * (unsigned)ELLC_ABSORB_FOLD_COUNTS + threadIdx.x] = ws[0][threadIdx.x] + ws[1][threadIdx.x] + ws[2][threadIdx.x] + ws[3][threadIdx.x];
}

// ellc_depth_restart_from_keyframes: every hypothesis EMPTY in front of the fold (all seven fields, unlike propagateDepth's two), so that
// what absorb_fold leaves is a function of the call's inputs alone
__global__ __launch_bounds__(256) void absorb_wipe(DepthSoA s, int n) {
  const int t = (int)(blockIdx.x * 256u + threadIdx.x);
  if (t >= n) return;
  s.invDepth[(unsigned)t] = 0.0f;
  s.variance[(unsigned)t] = 0.0f;
  s.invDepthSmoothed[(unsigned)t] = -1.0f;
  s.varianceSmoothed[(unsigned)t] = -1.0f;
  s.validity[(unsigned)t] = 0;
  s.blacklisted[(unsigned)t] = 0;
  s.isValid[(unsigned)t] = (uint8_t)0;
}

// One block: the sums of absorb_fold's counts and absorb_mark's four, as ellc_absorb_stats, for the host (integers: the order does not matter)
__global__ __launch_bounds__(256) void absorb_finish(AbsorbArgs a) {
  __shared__ int ws[4][ELLC_ABSORB_FOLD_COUNTS];
  int part[ELLC_ABSORB_FOLD_COUNTS];
#pragma unroll
  for (int k = 0; k < ELLC_ABSORB_FOLD_COUNTS; k++) part[k] = 0;
  for (int i = (int)threadIdx.x; i < a.f.r.blocks; i += 256)
#pragma unroll
    for (int k = 0; k < ELLC_ABSORB_FOLD_COUNTS; k++) part[k] += a.fold_counts[(unsigned)i * (unsigned)ELLC_ABSORB_FOLD_COUNTS + (unsigned)k];
#pragma unroll
  for (int k = 0; k < ELLC_ABSORB_FOLD_COUNTS; k++) {
    int v = part[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) a.stats[threadIdx.x] = a.mark_counts[threadIdx.x];
  else if (threadIdx.x < 4 + ELLC_ABSORB_FOLD_COUNTS) {
    const unsigned k = threadIdx.x - 4u;
    a.stats[threadIdx.x] = ws[0][k] + ws[1][k] + ws[2][k] + ws[3][k];
  } else if (threadIdx.x == 4 + ELLC_ABSORB_FOLD_COUNTS) a.stats[threadIdx.x] = 0;   // reserved
}

}  // namespace ellc
