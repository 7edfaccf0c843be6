// ellc_keyframe_light_step: the normal equations of the weighted affine fit Iw ~ gain * Is + offset between two keyframe slots at a given
// transform and light, over exactly the photometric pixels of ellc_keyframe_sim3_step (no reference counterpart: the reference assumes
// that a surface keeps its grey value between two keyframes). consist_pass / consist_finish's shape: two launches, no waiting between
// blocks and no atomics. light_pass leaves one partial record per (request, tile), light_finish sums a request's tiles. map_keep decides
// which source pixels take part, render_candidate where they land, sim3_photo_taps (below) which of them have four taps and what Iw
// and Is are. sim3l_pass / sim3l_finish, ellc_keyframe_sim3_step_lit's pair, are at the end.
#pragma once
#include "ellc_kernels_sim3.hpp"

namespace ellc {

// Rule 3's tap test and taps for a candidate c of source pixel p: whether (u, v) has four taps in the destination's image, and then
// Iw, its two gradients and Is, the source's grey value, all f32 - sim3_pass's lines as a function, for light_pass and sim3l_pass.
__device__ __forceinline__ bool sim3_photo_taps(const RenderCand& c, const MapPixel& p, const ELLC_GLOBAL uint8_t* img, const ELLC_GLOBAL uint8_t* timg,
                                                int cols, int rows, int sw, float& Iw, float& gx, float& gy, float& Is) {
  if (!(c.u >= 0.0f && c.v >= 0.0f)) return false;   // (NaN fails; u < cols and v < rows by render_candidate's bounds test, so the casts are in range)
  const int x0 = (int)c.u, y0 = (int)c.v;
  if (!(x0 + 1 < cols && y0 + 1 < rows)) return false;
  const unsigned t0 = (unsigned)(y0 * sw + x0);
  const float I00 = (float)timg[t0], I01 = (float)timg[t0 + 1u], I10 = (float)timg[t0 + (unsigned)sw], I11 = (float)timg[t0 + (unsigned)sw + 1u];
  Is = (float)img[(unsigned)(p.y * sw + p.x)];
  const float ax = c.u - (float)x0, ay = c.v - (float)y0;
  Iw = sim3_bilinear(I00, I01, I10, I11, ax, ay, gx, gy);
  return true;
}

// The light of request b in a 16-word staging: [cap][2] f32 (gain, offset) behind the 14 words of pair_stage_slots
__device__ __forceinline__ void load_light(const int* stage, int cap, unsigned b, float& gain, float& offset) {
  const float* l = (const float*)(stage + 14u * (unsigned)cap) + 2u * b;   // block-uniform: scalar loads
  gain = l[0];
  offset = l[1];
}

// ellc_light_normal as the kernels write it; the partial record of a tile has the same layout
struct LightRec {
  double s[7];               // sum_w, sum_w_s, sum_w_t, sum_w_ss, sum_w_st, sum_w_tt, chi2_photo
  int32_t n[4];              // n_kept, n_in_view, n_photo, n_photo_huber
};

struct LightArgs {
  MapView v;                 // what map_keep reads
  const int* stage;          // [cap] source slots, [cap] destination slots, [cap][12] f32 transforms, [cap][2] f32 lights (device copy of the pinned record)
  LightRec* partials;        // [requests of the launch][tiles]
  LightRec* out;             // pinned, through its device-side address: [B] records (light_finish)
  int cap;                   // requests the staging holds
  int first;                 // first request of this launch: blockIdx.y counts from it
  float w0, sp;              // 1 / sigma_i2 and its square root, both rounded to f32 on the host
  float huber_k;
};

__device__ __forceinline__ void rec_zero(LightRec& r) { r = LightRec(); }

__device__ __forceinline__ void rec_add(LightRec& a, const LightRec& b) {
#pragma unroll
  for (int k = 0; k < 7; k++) a.s[k] += b.s[k];
#pragma unroll
  for (int k = 0; k < 4; k++) a.n[k] += b.n[k];
}

__device__ __forceinline__ void rec_wave_sum(LightRec& r) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    LightRec o;
#pragma unroll
    for (int k = 0; k < 7; k++) o.s[k] = __shfl_xor(r.s[k], m, 64);
#pragma unroll
    for (int k = 0; k < 4; k++) o.n[k] = __shfl_xor(r.n[k], m, 64);
    rec_add(r, o);
  }
}

// grid (tiles of the level) x (requests of the launch), map_count's pixel layout: thread t of tile `local` owns pixels
// local * ELLC_TILE + j * 256 + t and adds them in the order j = 0..7; pair_store_block adds the lanes and the waves.
__global__ __launch_bounds__(256) void light_pass(LightArgs a) {
  const unsigned b = (unsigned)a.first + blockIdx.y;
  const int src = __builtin_amdgcn_readfirstlane(a.stage[b]), dst = __builtin_amdgcn_readfirstlane(a.stage[(unsigned)a.cap + b]);
  const KfLevelDev& S = a.v.kf_tab[a.v.level * a.v.max_kf + src];
  const KfLevelDev& D = a.v.kf_tab[a.v.level * a.v.max_kf + dst];
  const LevelGeom& g = a.v.geom[a.v.level];
  const ELLC_GLOBAL float* depth = gptr(S.depth);
  const ELLC_GLOBAL float* var = gptr(S.var);
  const ELLC_GLOBAL uint8_t* img = gptr(S.img);
  const ELLC_GLOBAL uint8_t* timg = gptr(D.img);
  const int cols = g.cols, rows = g.rows, sw = g.sw;
  const RenderT T = load_T12((const float*)(a.stage + 2u * (unsigned)a.cap) + 12u * b);   // block-uniform: scalar loads
  float gain, offset;
  load_light(a.stage, a.cap, b, gain, offset);
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
  LightRec r;
  rec_zero(r);
#pragma unroll 1
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    // A pixel without a term keeps these zeros and adds exact zeros below: the accumulators are updated in ONE place, outside the branches
    float Is = 0.0f, Iw = 0.0f, rp = 0.0f, wp = 0.0f;
    MapPixel p;
    RenderCand c;
    if (map_keep(a.v, depth, var, cols, rows, i, p)) {
      r.n[0]++;
      if (render_candidate(g, T, 0u, i, p.x, p.y, p.Z, p.V, c)) {   // (the request number only enters the key, which is not used here)
        r.n[1]++;
        float gx, gy, tIw, tIs;
        if (sim3_photo_taps(c, p, img, timg, cols, rows, sw, tIw, gx, gy, tIs)) {
          r.n[2]++;
          Is = tIs;
          Iw = tIw;
          rp = Iw - (gain * Is + offset);
          const float e = fabsf(rp) * a.sp;
          wp = a.w0;
          if (!(e <= a.huber_k)) {
            wp = a.w0 * (a.huber_k / e);
            r.n[3]++;
          }
        }
      }
    }
    // wIs and wIw are f32; their products with an f32 are exact in double, so the fused multiply-add rounds once, as the addition would
    const float wIs = wp * Is, wIw = wp * Iw;
    r.s[0] += (double)wp;
    r.s[1] += (double)wIs;
    r.s[2] += (double)wIw;
    r.s[3] = __builtin_fma((double)wIs, (double)Is, r.s[3]);
    r.s[4] = __builtin_fma((double)wIs, (double)Iw, r.s[4]);
    r.s[5] = __builtin_fma((double)wIw, (double)Iw, r.s[5]);
    r.s[6] += (double)((rp * rp) * wp);
  }
  pair_store_block(r, a.partials + (blockIdx.y * (unsigned)a.v.tiles + blockIdx.x));
}

__global__ __launch_bounds__(64) void light_finish(LightArgs a) {
  pair_finish(a.partials, a.v.tiles, a.out, a.first);
}

// ellc_keyframe_sim3_step_lit: sim3_pass with the photometric residual taken against Ip = gain * Is + offset, the request's light
// from the staging (16 words a request); Sim3Args as they are. A copy of sim3_pass's loop, not a shared body: written once as a
// force-inlined template with a compile-time switch, sim3_pass came out with the same 150 VGPRs and occupancy 3 but another register
// allocation and instruction stream (2052 -> 2040 instructions), and no kernel of the parent may change.
__global__ __launch_bounds__(256) void sim3l_pass(Sim3Args a) {
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
  const float fx = g.fx, fy = g.fy;
  const RenderT T = load_T12((const float*)(a.stage + 2u * (unsigned)a.cap) + 12u * b);   // block-uniform: scalar loads
  float gain, offset;
  load_light(a.stage, a.cap, b, gain, offset);
  const int base = (int)blockIdx.x * ELLC_TILE + (int)threadIdx.x;
  Sim3Rec r;
  rec_zero(r);
  const int idx_photo[6] = {0, 1, 2, 3, 4, 5}, idx_depth[4] = {0, 1, 5, 6};
#pragma unroll 1
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256;
    // (sim3_pass: a pixel without a term adds exact zeros, the accumulators are updated in ONE place, outside the branches)
    float Jp[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, rp = 0.0f, wp = 0.0f;
    float Jd[4] = {0.0f, 0.0f, 0.0f, 0.0f}, rd = 0.0f, wd = 0.0f;
    MapPixel p;
    RenderCand c;
    if (map_keep(a.v, depth, var, cols, rows, i, p)) {
      r.n[0]++;
      if (render_candidate(g, T, 0u, i, p.x, p.y, p.Z, p.V, c)) {
        r.n[1]++;
        float Iw, gx, gy, Is;
        if (sim3_photo_taps(c, p, img, timg, cols, rows, sw, Iw, gx, gy, Is)) {
          r.n[2]++;
          rp = Iw - (gain * Is + offset);   // the one line that differs from sim3_pass: the Jacobian is that of Iw
          const float A = (gx * fx) * c.nid, Bv = (gy * fy) * c.nid;
          const float Cq = -(((A * c.x) + (Bv * c.y)) * c.nid);
          Jp[0] = Cq * c.y - Bv * c.z; Jp[1] = A * c.z - Cq * c.x; Jp[2] = Bv * c.x - A * c.y; Jp[3] = A; Jp[4] = Bv; Jp[5] = Cq;
          const float e = fabsf(rp) * a.sp;
          wp = a.w0;
          if (!(e <= a.huber_k)) {
            wp = a.w0 * (a.huber_k / e);
            r.n[3]++;
          }
        }
        const float Zt = tdepth[(unsigned)c.target], Vt = tvar[(unsigned)c.target];   // (target < cols * rows: render_candidate's bounds test)
        const float s = c.nvar + Vt;
        if (map_ok(Zt, Vt) && s > 0.0f && s <= FLT_MAX) {
          const float d = c.nid - 1.0f / Zt;
          if (d * d <= a.gate_k2 * s) {
            r.n[4]++;
            rd = d;
            wd = a.depth_weight * (1.0f / s);
            const float a2 = c.nid * c.nid;
            Jd[0] = -(a2 * c.y); Jd[1] = a2 * c.x; Jd[2] = -a2; Jd[3] = -c.nid;
          } else {
            r.n[5]++;
          }
        }
      }
    }
    sim3_term(r, idx_photo, Jp, wp, rp);
    r.s[35] += (double)((rp * rp) * wp);
    sim3_term(r, idx_depth, Jd, wd, rd);
    r.s[36] += (double)((rd * rd) * wd);
  }
  rec_wave_sum(r);
  __shared__ Sim3Rec ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = r;
  __syncthreads();
  // sim3_pass's block tail: thread k adds field k of the four waves in ascending order
  Sim3Rec& out = a.partials[blockIdx.y * (unsigned)a.v.tiles + blockIdx.x];
  const unsigned k = threadIdx.x;
  if (k < ELLC_SIM3_SUMS) out.s[k] = ((ws[0].s[k] + ws[1].s[k]) + ws[2].s[k]) + ws[3].s[k];
  else if (k < ELLC_SIM3_SUMS + 6) out.n[k - ELLC_SIM3_SUMS] = ws[0].n[k - ELLC_SIM3_SUMS] + ws[1].n[k - ELLC_SIM3_SUMS] + ws[2].n[k - ELLC_SIM3_SUMS] + ws[3].n[k - ELLC_SIM3_SUMS];
}

__global__ __launch_bounds__(64) void sim3l_finish(Sim3Args a) {
  pair_finish(a.partials, a.v.tiles, a.out, a.first);
}

}  // namespace ellc
