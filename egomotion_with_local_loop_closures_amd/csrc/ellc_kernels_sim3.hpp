// ellc_keyframe_sim3_step: the normal equations of a seven-parameter (rotation, translation, log-scale) Gauss-Newton step between two
// keyframe slots at a given transform (no reference counterpart: frame::calculateSim3poseOtherWrtThis, Frame.cpp:419-439, states the
// intent only). consist_pass / consist_finish's shape: two launches, no waiting between blocks and no atomics. sim3_pass leaves one
// partial record per (request, tile), sim3_finish sums a request's tiles. map_keep (ellc_kernels_map.hpp) decides which source pixels
// take part, render_candidate (ellc_kernels_render.hpp) where they land and what their point in the destination's camera is.
// ellc_keyframe_sim3_step_lit is the same pair of kernels: every request carries a light (gain, offset) in the staging, and the plain
// call stages (1, 0), for which gain * Is + offset is Is exactly.
#pragma once
#include <float.h>
#include "ellc_kernels_render.hpp"
#include "ellc_pair_reduce.hpp"

namespace ellc {

#define ELLC_SIM3_SUMS 37   // 28 of H's upper triangle (row-major), 7 of b, chi2_photo, chi2_depth

// ellc_sim3_normal as the kernels write it; the partial record of a tile has the same layout
struct Sim3Rec {
  double s[ELLC_SIM3_SUMS];
  int32_t n[6];              // n_kept, n_in_view, n_photo, n_photo_huber, n_depth, n_depth_gated
};

struct Sim3Args {
  MapView v;                 // what map_keep reads
  const int* stage;          // [cap] source slots, [cap] destination slots, [cap][12] f32 transforms, [cap][2] f32 lights (device copy of the pinned record)
  Sim3Rec* partials;         // [requests of the launch][tiles]
  Sim3Rec* out;              // pinned, through its device-side address: [B] records (sim3_finish)
  int cap;                   // requests the staging holds
  int first;                 // first request of this launch: blockIdx.y counts from it
  float w0, sp;              // 1 / sigma_i2 and its square root, both rounded to f32 on the host
  float huber_k, gate_k2, depth_weight;
};

// H[i][j], i <= j, in the row-major upper triangle of a 7 x 7
__device__ __forceinline__ constexpr int sim3_h(int i, int j) { return i * 7 - (i * (i - 1)) / 2 + (j - i); }

// The sums no term ever reaches: the photometric Jacobian has no entry for the log-scale (index 6), the depth Jacobian none for
// indices 2, 3 and 4, so H[2][6], H[3][6] and H[4][6] stay the zero they start as. They are kept out of the reductions.
__device__ __forceinline__ constexpr bool sim3_never(int k) { return k == sim3_h(2, 6) || k == sim3_h(3, 6) || k == sim3_h(4, 6); }

// (one value-initialisation, not a loop over the fields: with the loop behind a call sim3_pass reloaded and reconverted the level's
// size inside its pixel loop, 1 to 2 % of the step's device time)
__device__ __forceinline__ void rec_zero(Sim3Rec& r) { r = Sim3Rec(); }

__device__ __forceinline__ void rec_add(Sim3Rec& a, const Sim3Rec& b) {
#pragma unroll
  for (int k = 0; k < ELLC_SIM3_SUMS; k++)
    if (!sim3_never(k)) a.s[k] += b.s[k];
#pragma unroll
  for (int k = 0; k < 6; k++) a.n[k] += b.n[k];
}

// The butterfly of this record: the sums no term reaches stay out, and the exchanges go eight at a time.
__device__ __forceinline__ void rec_wave_sum(Sim3Rec& r) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
    for (int k = 0; k < ELLC_SIM3_SUMS; k++) {
      if (!sim3_never(k)) r.s[k] += __shfl_xor(r.s[k], m, 64);
      if (k % 8 == 7) __builtin_amdgcn_sched_barrier(0);   // eight exchanges in flight, not all 34: the received copies would double the registers
    }
#pragma unroll
    for (int k = 0; k < 6; k++) r.n[k] += __shfl_xor(r.n[k], m, 64);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// One term of the normal equations over the Jacobian entries idx[0..N): wJ_i = w * J_i in f32; the products of two f32 values are
// exact in double, so the fused multiply-add rounds once, as the separate addition would.
template <int N>
__device__ __forceinline__ void sim3_term(Sim3Rec& a, const int (&idx)[N], const float (&J)[N], float w, float r) {
#pragma unroll
  for (int p = 0; p < N; p++) {
    const float wJ = w * J[p];
#pragma unroll
    for (int q = p; q < N; q++) a.s[sim3_h(idx[p], idx[q])] = __builtin_fma((double)wJ, (double)J[q], a.s[sim3_h(idx[p], idx[q])]);
    a.s[28 + idx[p]] = __builtin_fma((double)wJ, (double)r, a.s[28 + idx[p]]);
  }
}

// The bilinear value of four taps at the fractions (ax, ay), and its two gradients, in THE order every caller's result is held to
// (sim3_pass, absorb_mark): rows first, then the blend of the rows.
__device__ __forceinline__ float sim3_bilinear(float I00, float I01, float I10, float I11, float ax, float ay, float& gx, float& gy) {
  const float dx0 = I01 - I00, dx1 = I11 - I10;
  const float top = I00 + ax * dx0, bot = I10 + ax * dx1;
  gy = bot - top;
  gx = dx0 + ay * (dx1 - dx0);
  return top + ay * gy;
}

// Rule 3's tap test and taps for a candidate c of source pixel p: whether (u, v) has four taps in the destination's image, and then
// Iw, its two gradients and Is, the source's grey value, all f32 - for sim3_pass and light_pass.
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

// grid (tiles of the level) x (requests of the launch), map_count's pixel layout: thread t of tile `local` owns pixels
// local * ELLC_TILE + j * 256 + t and adds them in the order j = 0..7; the wave's lanes are summed by the butterfly, the four waves in
// ascending order. The partition follows from the level's size alone.
__global__ __launch_bounds__(256) void sim3_pass(Sim3Args a) {
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
    // A pixel without a term keeps these zeros and adds exact zeros below: the sums are those of the pixels that take part, and the
    // accumulators are updated in ONE place, outside the branches (updated inside them, every branch edge held a copy of all of them).
    float Jp[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, rp = 0.0f, wp = 0.0f;
    float Jd[4] = {0.0f, 0.0f, 0.0f, 0.0f}, rd = 0.0f, wd = 0.0f;
    MapPixel p;
    RenderCand c;
    if (map_keep(a.v, depth, var, cols, rows, i, p)) {
      r.n[0]++;
      if (render_candidate(g, T, 0u, i, p.x, p.y, p.Z, p.V, c)) {   // (the request number only enters the key, which is not used here)
        r.n[1]++;
        // the photometric term, where the destination's image has four taps around (u, v): the residual is taken against the request's
        // light, gain * Is + offset; the Jacobian is that of Iw
        float Iw, gx, gy, Is;
        if (sim3_photo_taps(c, p, img, timg, cols, rows, sw, Iw, gx, gy, Is)) {
          r.n[2]++;
          rp = Iw - (gain * Is + offset);
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
        // the depth term: the target of the destination's map, where it holds a hypothesis
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
  // A block tail of its own, not pair_store_block: thread k adds field k of the four waves in ascending order (one thread adding whole
  // records would hold four of them, 4 x 34 live doubles, in registers)
  Sim3Rec& out = a.partials[blockIdx.y * (unsigned)a.v.tiles + blockIdx.x];
  const unsigned k = threadIdx.x;
  if (k < ELLC_SIM3_SUMS) out.s[k] = ((ws[0].s[k] + ws[1].s[k]) + ws[2].s[k]) + ws[3].s[k];
  else if (k < ELLC_SIM3_SUMS + 6) out.n[k - ELLC_SIM3_SUMS] = ws[0].n[k - ELLC_SIM3_SUMS] + ws[1].n[k - ELLC_SIM3_SUMS] + ws[2].n[k - ELLC_SIM3_SUMS] + ws[3].n[k - ELLC_SIM3_SUMS];
}

__global__ __launch_bounds__(64) void sim3_finish(Sim3Args a) {
  pair_finish(a.partials, a.v.tiles, a.out, a.first);
}

}  // namespace ellc
