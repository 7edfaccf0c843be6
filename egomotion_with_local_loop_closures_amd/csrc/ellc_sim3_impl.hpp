// ellc_keyframe_sim3_step / _step_lit, ellc_keyframe_sim3_align / _align_lit, ellc_sim3_solve, ellc_sim3_apply (include/ellc_abi.h): the
// host side of the Sim(3) refinement, without and with the affine brightness - one evaluation and one Gauss-Newton loop behind each
// pair of entry points. Included at the end of ellc_hip.hip behind ellc_ring_common.hpp: its refusals, view and pair reduction are used here.
#pragma once
#include "ellc_ring_common.hpp"
#include "ellc_kernels_light.hpp"
#include "ellc_joint_solve.hpp"
#include <vector>

using namespace ellc;

static_assert(sizeof(Sim3Rec) == sizeof(ellc_sim3_normal) && sizeof(ellc_sim3_normal) == 320 && offsetof(Sim3Rec, s) == offsetof(ellc_sim3_normal, H) &&
                  offsetof(ellc_sim3_normal, b) == 28 * 8 && offsetof(ellc_sim3_normal, chi2_photo) == 35 * 8 &&
                  offsetof(ellc_sim3_normal, chi2_depth) == 36 * 8 && offsetof(Sim3Rec, n) == offsetof(ellc_sim3_normal, n_kept) &&
                  offsetof(ellc_sim3_normal, n_depth_gated) == offsetof(Sim3Rec, n) + 20,
              "Sim3Rec mirrors ellc_sim3_normal");

namespace {

const int SIM3_MAX_B = 2048;
const size_t SIM3_SCRATCH_BYTES = (size_t)32 << 20;   // partial records of one launch: a larger batch goes in several launches

// what both entry points refuse, before anything is touched
ellc_status sim3_validate(ellc_ctx* c, const char* who, int B, const int* src, const int* dst, const float* T12, int level_lo, int level_hi,
                          const ellc_map_filter* f, const ellc_sim3_params* p) {
  const std::string w(who);
  if (!src || !dst || !T12 || !f || !p) return fail(c, ELLC_ERR_BAD_ARG, w + ": null pointer");
  if (B < 1 || B > SIM3_MAX_B) return fail(c, ELLC_ERR_BAD_ARG, w + ": B out of range");
  if (level_lo < 0 || level_hi >= c->L || level_lo > level_hi) return fail(c, ELLC_ERR_BAD_ARG, w + ": level out of range");
  if (c->geom_h[level_lo].n > (1 << 24)) return fail(c, ELLC_ERR_BAD_ARG, w + ": more than 2^24 pixels on the level");
  ELLC_TRY(ring_check_filter(c, who, f));
  if (!std::isfinite(p->sigma_i2) || !std::isfinite(p->huber_k) || !std::isfinite(p->gate_k2) || !std::isfinite(p->depth_weight) ||
      !(p->sigma_i2 > 0.0f) || !(p->huber_k > 0.0f) || !(p->gate_k2 >= 0.0f) || !(p->depth_weight >= 0.0f))
    return fail(c, ELLC_ERR_BAD_ARG, w + ": parameters out of range");
  ELLC_TRY(ring_check_slots(c, who, B, src, c->cfg.max_keyframes));
  ELLC_TRY(ring_check_slots(c, who, B, dst, c->cfg.max_keyframes));
  ELLC_TRY(ring_check_ready(c, who, B, src));
  return ring_check_ready(c, who, B, dst);
}

ellc_status light_check_params(ellc_ctx* c, const char* who, const ellc_light_params* p) {
  if (!std::isfinite(p->gain_min) || !std::isfinite(p->gain_max) || !(p->gain_min > 0.0f) || !(p->gain_min <= 1.0f) || !(p->gain_max >= 1.0f) ||
      p->min_pixels < 2 || p->min_pixels > (1 << 30))
    return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": light parameters out of range");
  return ELLC_OK;
}

// What sim3_pass and light_pass are given alike (a: Sim3Args or LightArgs): the view, room for B requests and their partial records,
// the 16-word staging on its way to the device (light NULL: (1, 0) for every pair) and the photometric weights. Returns the requests
// of one launch through per_launch.
template <class Args>
ellc_status photo_args(ellc_ctx* c, PairScratch& s, int B, const int* src, const int* dst, const float* T12, const float* light, int level,
                       const ellc_map_filter* f, const ellc_sim3_params* p, Args& a, int& per_launch) {
  const size_t rec_bytes = sizeof(*a.partials);
  a.v = ring_view(c, level, f);
  per_launch = pair_per_launch(B, SIM3_SCRATCH_BYTES, (size_t)a.v.tiles * rec_bytes);
  ELLC_TRY(pair_reserve(c, s, B, 16 * sizeof(int), rec_bytes, (size_t)per_launch * a.v.tiles));
  if (!light) {
    float* unit = (float*)s.stage_h + 14 * (size_t)s.cap;
    for (int b = 0; b < B; b++) { unit[2 * b] = 1.0f; unit[2 * b + 1] = 0.0f; }
  }
  ELLC_TRY(pair_stage_slots(c, s, B, src, dst, T12, light, 2));
  a.stage = (const int*)s.stage_d;
  a.cap = s.cap;
  a.w0 = 1.0f / p->sigma_i2;
  a.sp = sqrtf(a.w0);
  a.huber_k = p->huber_k;
  return ELLC_OK;
}

// One evaluation of B validated requests on `level`, behind ELLC_ENTER; synchronous. launches_ms (the diagnostic hook only): device
// time of the launches, HIP events around them.
ellc_status sim3_evaluate(ellc_ctx* c, int B, const int* src, const int* dst, const float* T12, const float* light /* NULL: (1, 0) for every pair */,
                          int level, const ellc_map_filter* f, const ellc_sim3_params* p, ellc_sim3_normal* out, float* launches_ms) {
  Sim3Args a{};
  int per_launch;
  ELLC_TRY(photo_args(c, c->sim3, B, src, dst, T12, light, level, f, p, a, per_launch));
  a.gate_k2 = p->gate_k2;
  a.depth_weight = p->depth_weight;
  return pair_run(c, c->sim3, B, per_launch, sim3_pass, sim3_finish, a, out, launches_ms);
}

ellc_status light_evaluate(ellc_ctx* c, int B, const int* src, const int* dst, const float* T12, const float* light, int level,
                           const ellc_map_filter* f, const ellc_sim3_params* p, ellc_light_normal* out, float* launches_ms) {
  LightArgs a{};
  int per_launch;
  ELLC_TRY(photo_args(c, c->light, B, src, dst, T12, light, level, f, p, a, per_launch));
  return pair_run(c, c->light, B, per_launch, light_pass, light_finish, a, out, launches_ms);
}

// ellc_keyframe_sim3_step (light is NULL) and ellc_keyframe_sim3_step_lit, each under its own name
ellc_status sim3_step_impl(ellc_ctx* c, const char* who, int B, const int* src, const int* dst, const float* T12, const float* light, int level,
                           const ellc_map_filter* f, const ellc_sim3_params* p, ellc_sim3_normal* out, float* launches_ms) {
  if (!c) return ELLC_ERR_BAD_ARG;
  // validated first: a refused call leaves the context as it was and `out` unwritten
  if (!out) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  ELLC_TRY(sim3_validate(c, who, B, src, dst, T12, level, level, f, p));
  ELLC_TRY(light_check(c, who, B, light));
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  return sim3_evaluate(c, B, src, dst, T12, light, level, f, p, out, launches_ms);
}

// exp of the 4 x 4 generator [[w]x + sigma I, v; 0 0] in double: scaling by a power of two until the largest row sum is <= 1/4, the
// Taylor series to the 20th power (the remainder is below 1e-30), then the squarings. The zero generator gives the identity exactly.
void sim3_exp(const double xi[7], double M[16]) {
  double G[16] = {xi[6], -xi[2], xi[1], xi[3], xi[2], xi[6], -xi[0], xi[4], -xi[1], xi[0], xi[6], xi[5], 0, 0, 0, 0};
  double norm = 0.0;
  for (int r = 0; r < 3; r++) norm = std::max(norm, std::fabs(G[4 * r]) + std::fabs(G[4 * r + 1]) + std::fabs(G[4 * r + 2]) + std::fabs(G[4 * r + 3]));
  int squarings = 0;
  while (norm > 0.25 && squarings < 64) { norm *= 0.5; squarings++; }
  const double sc = std::ldexp(1.0, -squarings);
  for (int k = 0; k < 16; k++) G[k] *= sc;
  double term[16], next[16];
  for (int k = 0; k < 16; k++) M[k] = term[k] = (k % 5 == 0) ? 1.0 : 0.0;
  for (int n = 1; n <= 20; n++) {
    for (int r = 0; r < 4; r++)
      for (int q = 0; q < 4; q++) {
        double s = 0.0;
        for (int k = 0; k < 4; k++) s += term[4 * r + k] * G[4 * k + q];
        next[4 * r + q] = s / (double)n;
      }
    for (int k = 0; k < 16; k++) { term[k] = next[k]; M[k] += term[k]; }
  }
  for (int i = 0; i < squarings; i++) {
    for (int r = 0; r < 4; r++)
      for (int q = 0; q < 4; q++) {
        double s = 0.0;
        for (int k = 0; k < 4; k++) s += M[4 * r + k] * M[4 * k + q];
        next[4 * r + q] = s;
      }
    for (int k = 0; k < 16; k++) M[k] = next[k];
  }
}

// a trace of n entries, every one marked as not written (n_kept = -1)
template <class Rec>
void trace_unwritten(std::vector<Rec>& t, size_t n) {
  Rec unused;
  std::memset(&unused, 0, sizeof(unused));
  unused.n_kept = -1;
  t.assign(n, unused);
}

// The Gauss-Newton loop of ellc_keyframe_sim3_align and ellc_keyframe_sim3_align_lit, each under its own name. light_params NULL: no
// light is fitted, every evaluation is sim3_evaluate's alone at (1, 0), and the light's arrays (light_in, light_out, light_rec_out,
// trace_light, trace_light_rec) are all NULL.
ellc_status sim3_align_impl(ellc_ctx* c, const char* who, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12_in,
                            const float* light_in, int level_from, int level_to, const ellc_map_filter* filter, const ellc_sim3_params* params,
                            const ellc_light_params* light_params, int max_iter, float eps, float* T12_out, float* light_out, ellc_sim3_normal* out,
                            ellc_light_normal* light_rec_out, int* iters_out, float* trace_T12, ellc_sim3_normal* trace_rec, float* trace_light,
                            ellc_light_normal* trace_light_rec, int trace_capacity) {
  const bool lit = light_params != nullptr;
  if (!T12_out || !out || (lit && !light_out)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  if (level_from < level_to) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": level_from below level_to");
  if (max_iter < 1 || max_iter > 64) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": max_iter out of range");
  if (!(eps >= 0.0f) || !std::isfinite(eps)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": eps negative or not finite");
  ELLC_TRY(sim3_validate(c, who, B, src_kf_slots, dst_kf_slots, T12_in, level_to, level_from, filter, params));
  if (lit) {
    ELLC_TRY(light_check(c, who, B, light_in));
    ELLC_TRY(light_check_params(c, who, light_params));
  }
  const int n_levels = level_from - level_to + 1;
  const bool traced = trace_T12 || trace_rec || trace_light || trace_light_rec;
  if (traced && trace_capacity < n_levels * max_iter + 1) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": trace_capacity too small");
  ELLC_ENTER(c);
  // everything of the call is kept here until it has succeeded: a failure half-way leaves the caller's arrays as they were
  std::vector<float> T(T12_in, T12_in + (size_t)B * 12), l, tT, tL;
  std::vector<int> iters((size_t)B * n_levels, 0), n_trace((size_t)B, 0);
  std::vector<ellc_sim3_normal> tR, rec((size_t)B);
  std::vector<ellc_light_normal> tLR, lrec(lit ? (size_t)B : 0);
  if (lit) {
    l.resize((size_t)B * 2);
    for (int b = 0; b < B; b++) { l[2 * (size_t)b] = light_in ? light_in[2 * b] : 1.0f; l[2 * (size_t)b + 1] = light_in ? light_in[2 * b + 1] : 0.0f; }
  }
  if (trace_T12) tT.assign((size_t)B * trace_capacity * 12, 0.0f);
  if (trace_light) tL.assign((size_t)B * trace_capacity * 2, 0.0f);
  if (trace_rec) trace_unwritten(tR, (size_t)B * trace_capacity);
  if (trace_light_rec) trace_unwritten(tLR, (size_t)B * trace_capacity);
  std::vector<int> active, as, ad;
  std::vector<float> aT, aL;
  // one evaluation of the pairs in `active`: with a light the light records and the lights solved from them; the Sim(3) records at
  // those lights into rec[0..active.size()); and the traces
  auto evaluate = [&](int level) -> ellc_status {
    const int n = (int)active.size();
    as.resize(n); ad.resize(n); aT.resize((size_t)n * 12); aL.resize(lit ? (size_t)n * 2 : 0);
    for (int k = 0; k < n; k++) {
      as[k] = src_kf_slots[active[k]]; ad[k] = dst_kf_slots[active[k]];
      std::memcpy(&aT[(size_t)k * 12], &T[(size_t)active[k] * 12], 12 * sizeof(float));
      if (lit) std::memcpy(&aL[(size_t)k * 2], &l[(size_t)active[k] * 2], 2 * sizeof(float));
    }
    if (lit) {
      ELLC_TRY(light_evaluate(c, n, as.data(), ad.data(), aT.data(), aL.data(), level, filter, params, lrec.data(), nullptr));
      for (int k = 0; k < n; k++) (void)ellc_light_solve(&lrec[k], light_params, &aL[(size_t)k * 2], &aL[(size_t)k * 2]);
    }
    ELLC_TRY(sim3_evaluate(c, n, as.data(), ad.data(), aT.data(), lit ? aL.data() : nullptr, level, filter, params, rec.data(), nullptr));
    for (int k = 0; k < n; k++) {
      const int b = active[k];
      if (lit) std::memcpy(&l[(size_t)b * 2], &aL[(size_t)k * 2], 2 * sizeof(float));
      const size_t e = (size_t)b * trace_capacity + n_trace[b];
      if (trace_T12) std::memcpy(&tT[e * 12], &aT[(size_t)k * 12], 12 * sizeof(float));
      if (trace_light) std::memcpy(&tL[e * 2], &aL[(size_t)k * 2], 2 * sizeof(float));
      if (trace_rec) tR[e] = rec[k];
      if (trace_light_rec) tLR[e] = lrec[k];
      n_trace[b]++;
    }
    return ELLC_OK;
  };
  for (int li = 0; li < n_levels; li++) {
    const int level = level_from - li;
    active.resize(B);
    for (int b = 0; b < B; b++) active[b] = b;
    while (!active.empty()) {
      ELLC_TRY(evaluate(level));
      std::vector<int> still;
      for (size_t k = 0; k < active.size(); k++) {
        const int b = active[k];
        double xi[7];
        if (ellc_sim3_solve(&rec[k], xi)) continue;   // singular: no update, the pair leaves the level
        ellc_sim3_apply(xi, &T[(size_t)b * 12], &T[(size_t)b * 12]);
        const int made = ++iters[(size_t)b * n_levels + li];
        double m = 0.0;
        for (int i = 0; i < 7; i++) m = std::max(m, std::fabs(xi[i]));
        if (m <= (double)eps || made >= max_iter) continue;
        still.push_back(b);
      }
      active.swap(still);
    }
  }
  active.resize(B);
  for (int b = 0; b < B; b++) active[b] = b;
  ELLC_TRY(evaluate(level_to));
  std::memcpy(out, rec.data(), (size_t)B * sizeof(ellc_sim3_normal));
  std::memcpy(T12_out, T.data(), (size_t)B * 12 * sizeof(float));
  if (lit) std::memcpy(light_out, l.data(), (size_t)B * 2 * sizeof(float));
  if (light_rec_out) std::memcpy(light_rec_out, lrec.data(), (size_t)B * sizeof(ellc_light_normal));
  if (iters_out) std::memcpy(iters_out, iters.data(), iters.size() * sizeof(int));
  if (trace_T12) std::memcpy(trace_T12, tT.data(), tT.size() * sizeof(float));
  if (trace_rec) std::memcpy(trace_rec, tR.data(), tR.size() * sizeof(ellc_sim3_normal));
  if (trace_light) std::memcpy(trace_light, tL.data(), tL.size() * sizeof(float));
  if (trace_light_rec) std::memcpy(trace_light_rec, tLR.data(), tLR.size() * sizeof(ellc_light_normal));
  return ELLC_OK;
}

}  // namespace

extern "C" {

void ellc_sim3_default_params(ellc_sim3_params* p) {
  if (!p) return;
  p->sigma_i2 = 16.0f; p->huber_k = 1.345f; p->gate_k2 = 9.0f; p->depth_weight = 1.0f;
}

int ellc_sim3_solve(const ellc_sim3_normal* n, double* xi7) {
  for (int i = 0; i < 7; i++) xi7[i] = 0.0;
  double A[49];
  for (int i = 0, k = 0; i < 7; i++)
    for (int j = i; j < 7; j++, k++) A[7 * i + j] = A[7 * j + i] = n->H[k];
  return ldlt_solve_neg(7, A, n->b, xi7);   // (the routine ellc_joint_solve uses at 6 B unknowns)
}

void ellc_sim3_apply(const double* xi7, const float* T12_in, float* T12_out) {
  double M[16];
  sim3_exp(xi7, M);
  float o[12];
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 4; q++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += M[4 * r + k] * (double)T12_in[4 * k + q];
      if (q == 3) s += M[4 * r + 3];
      o[4 * r + q] = (float)s;
    }
  std::memcpy(T12_out, o, sizeof(o));
}

ellc_status ellc_keyframe_sim3_step(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, int level,
                                    const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_sim3_normal* out) {
  return sim3_step_impl(c, "ellc_keyframe_sim3_step", B, src_kf_slots, dst_kf_slots, T12, nullptr, level, filter, params, out, nullptr);
}

ellc_status ellc_keyframe_sim3_step_lit(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, const float* light,
                                        int level, const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_sim3_normal* out) {
  return sim3_step_impl(c, "ellc_keyframe_sim3_step_lit", B, src_kf_slots, dst_kf_slots, T12, light, level, filter, params, out, nullptr);
}

ellc_status ellc_keyframe_sim3_align(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12_in, int level_from,
                                     int level_to, const ellc_map_filter* filter, const ellc_sim3_params* params, int max_iter, float eps,
                                     float* T12_out, ellc_sim3_normal* out, int* iters_out, float* trace_T12, ellc_sim3_normal* trace_rec,
                                     int trace_capacity) {
  if (!c) return ELLC_ERR_BAD_ARG;
  return sim3_align_impl(c, "ellc_keyframe_sim3_align", B, src_kf_slots, dst_kf_slots, T12_in, nullptr, level_from, level_to, filter, params, nullptr,
                         max_iter, eps, T12_out, nullptr, out, nullptr, iters_out, trace_T12, trace_rec, nullptr, nullptr, trace_capacity);
}

ellc_status ellc_keyframe_sim3_align_lit(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12_in, const float* light_in,
                                         int level_from, int level_to, const ellc_map_filter* filter, const ellc_sim3_params* params,
                                         const ellc_light_params* light_params, int max_iter, float eps, float* T12_out, float* light_out,
                                         ellc_sim3_normal* out, ellc_light_normal* light_rec_out, int* iters_out, float* trace_T12,
                                         ellc_sim3_normal* trace_rec, float* trace_light, ellc_light_normal* trace_light_rec, int trace_capacity) {
  if (!c) return ELLC_ERR_BAD_ARG;
  if (!light_params) return fail(c, ELLC_ERR_BAD_ARG, "ellc_keyframe_sim3_align_lit: null pointer");   // (to the loop, NULL says "no light")
  return sim3_align_impl(c, "ellc_keyframe_sim3_align_lit", B, src_kf_slots, dst_kf_slots, T12_in, light_in, level_from, level_to, filter, params,
                         light_params, max_iter, eps, T12_out, light_out, out, light_rec_out, iters_out, trace_T12, trace_rec, trace_light,
                         trace_light_rec, trace_capacity);
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_sim3_step(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, int level,
                                   const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_sim3_normal* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) {
    return sim3_step_impl(c, "ellc_keyframe_sim3_step", B, src_kf_slots, dst_kf_slots, T12, nullptr, level, filter, params, out, ms);
  });
}

ellc_status ellc_profile_sim3_step_lit(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, const float* light,
                                       int level, const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_sim3_normal* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) {
    return sim3_step_impl(c, "ellc_keyframe_sim3_step_lit", B, src_kf_slots, dst_kf_slots, T12, light, level, filter, params, out, ms);
  });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"

