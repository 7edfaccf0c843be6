// ellc_keyframe_depth_consistency: one keyframe slot's semi-dense map against another's at a given transform (no reference counterpart:
// GlobalOptimize.cpp:566-582 accepts every candidate of a loop closure unseen). A reduction, two launches, no waiting between blocks
// and no atomics: consist_pass leaves one partial record per (request, tile), consist_finish sums a request's tiles
// (ellc_pair_reduce.hpp holds the tail of both). map_keep (ellc_kernels_map.hpp) decides which source pixels take part,
// render_candidate (ellc_kernels_render.hpp) where they land.
#pragma once
#include <float.h>
#include "ellc_kernels_render.hpp"
#include "ellc_pair_reduce.hpp"

namespace ellc {

// ellc_depth_consistency as the kernels write it; the partial record of a tile has the same layout
struct ConsistRec {
  double sum_chi2, sum_w_ss, sum_w_st;
  long long sum_abs_di, sum_di2;
  int32_t n_kept, n_in_view, n_overlap, n_agree, n_in_front, n_behind, n_weighted;
  int32_t pad_;
};

struct ConsistArgs {
  MapView v;                 // what map_keep reads
  const int* stage;          // [cap] source slot of every request, [cap] destination slot, [cap][12] f32 transforms (device copy of the pinned record)
  ConsistRec* partials;      // [requests of the launch][tiles]
  ConsistRec* out;           // pinned, through its device-side address: [B] records (consist_finish)
  int cap;                   // requests the staging holds
  int first;                 // first request of this launch: blockIdx.y counts from it
  float agree_k2;
};

__device__ __forceinline__ void rec_zero(ConsistRec& r) {
  r.sum_chi2 = r.sum_w_ss = r.sum_w_st = 0.0;
  r.sum_abs_di = r.sum_di2 = 0;
  r.n_kept = r.n_in_view = r.n_overlap = r.n_agree = r.n_in_front = r.n_behind = r.n_weighted = 0;
  r.pad_ = 0;
}

__device__ __forceinline__ void rec_add(ConsistRec& a, const ConsistRec& b) {
  a.sum_chi2 += b.sum_chi2; a.sum_w_ss += b.sum_w_ss; a.sum_w_st += b.sum_w_st;
  a.sum_abs_di += b.sum_abs_di; a.sum_di2 += b.sum_di2;
  a.n_kept += b.n_kept; a.n_in_view += b.n_in_view; a.n_overlap += b.n_overlap; a.n_agree += b.n_agree;
  a.n_in_front += b.n_in_front; a.n_behind += b.n_behind; a.n_weighted += b.n_weighted;
}

__device__ __forceinline__ void rec_wave_sum(ConsistRec& r) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    ConsistRec o;
    o.sum_chi2 = __shfl_xor(r.sum_chi2, m, 64); o.sum_w_ss = __shfl_xor(r.sum_w_ss, m, 64); o.sum_w_st = __shfl_xor(r.sum_w_st, m, 64);
    o.sum_abs_di = __shfl_xor(r.sum_abs_di, m, 64); o.sum_di2 = __shfl_xor(r.sum_di2, m, 64);
    o.n_kept = __shfl_xor(r.n_kept, m, 64); o.n_in_view = __shfl_xor(r.n_in_view, m, 64); o.n_overlap = __shfl_xor(r.n_overlap, m, 64);
    o.n_agree = __shfl_xor(r.n_agree, m, 64); o.n_in_front = __shfl_xor(r.n_in_front, m, 64); o.n_behind = __shfl_xor(r.n_behind, m, 64);
    o.n_weighted = __shfl_xor(r.n_weighted, m, 64);
    rec_add(r, o);
  }
}

// grid (tiles of the level) x (requests of the launch), map_count's pixel layout: thread t of tile `local` owns pixels
// local * ELLC_TILE + j * 256 + t and adds them in the order j = 0..7; pair_store_block adds the lanes and the waves.
__global__ __launch_bounds__(256) void consist_pass(ConsistArgs a) {
  const unsigned b = (unsigned)a.first + blockIdx.y;
  const int src = __builtin_amdgcn_readfirstlane(a.stage[b]), dst = __builtin_amdgcn_readfirstlane(a.stage[(unsigned)a.cap + b]);
  const KfLevelDev& S = a.v.kf_tab[a.v.level * a.v.max_kf + src];
  const KfLevelDev& D = a.v.kf_tab[a.v.level * a.v.max_kf + dst];
  const LevelGeom& g = a.v.geom[a.v.level];
  const ELLC_GLOBAL float* depth = gptr(S.depth);
  const ELLC_GLOBAL float* var = gptr(S.var);
  const ELLC_GLOBAL uint8_t* img = gptr(S.img);
  const ELLC_GLOBAL float* tdepth = gptr(D.depth);
  const ELLC_GLOBAL float* tvar = gptr(D.var);
  const ELLC_GLOBAL uint8_t* timg = gptr(D.img);
  const int cols = g.cols, rows = g.rows, sw = g.sw;
  const RenderT T = load_T12((const float*)(a.stage + 2u * (unsigned)a.cap) + 12u * b);   // block-uniform: scalar loads
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
  ConsistRec r;
  rec_zero(r);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    MapPixel p;
    RenderCand c;
    if (!map_keep(a.v, depth, var, cols, rows, i, p)) continue;
    r.n_kept++;
    if (!render_candidate(g, T, 0u, i, p.x, p.y, p.Z, p.V, c)) continue;   // (the request number only enters the key, which is not used here)
    r.n_in_view++;
    const float Zt = tdepth[(unsigned)c.target], Vt = tvar[(unsigned)c.target];   // (target < cols * rows: render_candidate's bounds test)
    if (!map_ok(Zt, Vt)) continue;
    r.n_overlap++;
    const int ty = c.target / cols, tx = c.target - ty * cols;
    const int Is = (int)img[(unsigned)(p.y * sw + p.x)], It = (int)timg[(unsigned)(ty * sw + tx)];
    const float idt = 1.0f / Zt;
    const float d = c.nid - idt;
    const float s = c.nvar + Vt;
    const float d2 = d * d;
    if (d2 <= a.agree_k2 * s) r.n_agree++;
    else if (d > 0.0f) r.n_in_front++;
    else r.n_behind++;
    const int di = Is > It ? Is - It : It - Is;
    r.sum_abs_di += di;
    r.sum_di2 += di * di;
    if (s > 0.0f && s <= FLT_MAX) {
      const float w = 1.0f / s;
      const float q = d2 * w;
      const float ss = (c.nid * c.nid) * w;
      const float st = (c.nid * idt) * w;
      r.n_weighted++;
      r.sum_chi2 += (double)q;
      r.sum_w_ss += (double)ss;
      r.sum_w_st += (double)st;
    }
  }
  pair_store_block(r, a.partials + (blockIdx.y * (unsigned)a.v.tiles + blockIdx.x));
}

__global__ __launch_bounds__(64) void consist_finish(ConsistArgs a) {
  pair_finish(a.partials, a.v.tiles, a.out, a.first);
}

}  // namespace ellc
