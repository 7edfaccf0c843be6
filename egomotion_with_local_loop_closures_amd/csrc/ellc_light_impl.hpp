// ellc_keyframe_light_step, ellc_keyframe_sim3_step_lit, ellc_keyframe_sim3_align_lit, ellc_light_solve (include/ellc_abi.h): the host
// side of the affine brightness in the Sim(3) refinement. Included at the end of ellc_hip.hip behind ellc_sim3_impl.hpp, whose
// refusals (sim3_validate) it shares.
#pragma once
#include "ellc_sim3_impl.hpp"
#include "ellc_kernels_light.hpp"

using namespace ellc;

static_assert(sizeof(LightRec) == sizeof(ellc_light_normal) && sizeof(ellc_light_normal) == 72 && offsetof(LightRec, s) == offsetof(ellc_light_normal, sum_w) &&
                  offsetof(ellc_light_normal, sum_w_tt) == 5 * 8 && offsetof(ellc_light_normal, chi2_photo) == 6 * 8 &&
                  offsetof(LightRec, n) == offsetof(ellc_light_normal, n_kept) && offsetof(ellc_light_normal, n_photo_huber) == offsetof(LightRec, n) + 12,
              "LightRec mirrors ellc_light_normal");
static_assert(sizeof(ellc_light_params) == 12, "ellc_light_params is 12 bytes");

namespace {

// a given light: every value finite (NULL means (1, 0) for every pair)
ellc_status light_check(ellc_ctx* c, const char* who, int B, const float* light) {
  if (!light) return ELLC_OK;
  for (int k = 0; k < 2 * B; k++)
    if (!std::isfinite(light[k])) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": light not finite");
  return ELLC_OK;
}

ellc_status light_check_params(ellc_ctx* c, const char* who, const ellc_light_params* p) {
  if (!std::isfinite(p->gain_min) || !std::isfinite(p->gain_max) || !(p->gain_min > 0.0f) || !(p->gain_min <= 1.0f) || !(p->gain_max >= 1.0f) ||
      p->min_pixels < 2 || p->min_pixels > (1 << 30))
    return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": light parameters out of range");
  return ELLC_OK;
}

// the lights of B requests as the staging takes them: the given ones, or (1, 0) each
const float* light_or_unit(const float* light, int B, std::vector<float>& unit) {
  if (light) return light;
  unit.resize((size_t)B * 2);
  for (int b = 0; b < B; b++) { unit[2 * (size_t)b] = 1.0f; unit[2 * (size_t)b + 1] = 0.0f; }
  return unit.data();
}

// One evaluation of B validated requests on `level`, behind ELLC_ENTER; synchronous (sim3_evaluate's twins; light: [B][2], not NULL)
ellc_status light_evaluate(ellc_ctx* c, int B, const int* src, const int* dst, const float* T12, const float* light, int level,
                           const ellc_map_filter* f, const ellc_sim3_params* p, ellc_light_normal* out, float* launches_ms) {
  LightArgs a{};
  a.v = ring_view(c, level, f);
  const int per_launch = pair_per_launch(B, SIM3_SCRATCH_BYTES, (size_t)a.v.tiles * sizeof(LightRec));
  ELLC_TRY(pair_reserve(c, c->light, B, 16 * sizeof(int), sizeof(LightRec), (size_t)per_launch * a.v.tiles));
  ELLC_TRY(pair_stage_slots(c, c->light, B, src, dst, T12, light, 2));
  a.stage = (const int*)c->light.stage_d;
  a.cap = c->light.cap;
  a.w0 = 1.0f / p->sigma_i2;
  a.sp = sqrtf(a.w0);
  a.huber_k = p->huber_k;
  return pair_run(c, c->light, B, per_launch, light_pass, light_finish, a, out, launches_ms);
}

ellc_status sim3l_evaluate(ellc_ctx* c, int B, const int* src, const int* dst, const float* T12, const float* light, int level,
                           const ellc_map_filter* f, const ellc_sim3_params* p, ellc_sim3_normal* out, float* launches_ms) {
  Sim3Args a{};
  a.v = ring_view(c, level, f);
  const int per_launch = pair_per_launch(B, SIM3_SCRATCH_BYTES, (size_t)a.v.tiles * sizeof(Sim3Rec));
  ELLC_TRY(pair_reserve(c, c->sim3l, B, 16 * sizeof(int), sizeof(Sim3Rec), (size_t)per_launch * a.v.tiles));
  ELLC_TRY(pair_stage_slots(c, c->sim3l, B, src, dst, T12, light, 2));
  a.stage = (const int*)c->sim3l.stage_d;
  a.cap = c->sim3l.cap;
  a.w0 = 1.0f / p->sigma_i2;
  a.sp = sqrtf(a.w0);
  a.huber_k = p->huber_k;
  a.gate_k2 = p->gate_k2;
  a.depth_weight = p->depth_weight;
  return pair_run(c, c->sim3l, B, per_launch, sim3l_pass, sim3l_finish, a, out, launches_ms);
}

ellc_status light_step_impl(ellc_ctx* c, int B, const int* src, const int* dst, const float* T12, const float* light, int level,
                            const ellc_map_filter* f, const ellc_sim3_params* p, ellc_light_normal* out, float* launches_ms) {
  if (!c) return ELLC_ERR_BAD_ARG;
  const char* who = "ellc_keyframe_light_step";
  if (!out) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  ELLC_TRY(sim3_validate(c, who, B, src, dst, T12, level, level, f, p));
  ELLC_TRY(light_check(c, who, B, light));
  ELLC_ENTER(c);
  std::vector<float> unit;
  return light_evaluate(c, B, src, dst, T12, light_or_unit(light, B, unit), level, f, p, out, launches_ms);
}

ellc_status sim3_step_lit_impl(ellc_ctx* c, int B, const int* src, const int* dst, const float* T12, const float* light, int level,
                               const ellc_map_filter* f, const ellc_sim3_params* p, ellc_sim3_normal* out, float* launches_ms) {
  if (!c) return ELLC_ERR_BAD_ARG;
  const char* who = "ellc_keyframe_sim3_step_lit";
  if (!out) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  ELLC_TRY(sim3_validate(c, who, B, src, dst, T12, level, level, f, p));
  ELLC_TRY(light_check(c, who, B, light));
  ELLC_ENTER(c);
  std::vector<float> unit;
  return sim3l_evaluate(c, B, src, dst, T12, light_or_unit(light, B, unit), level, f, p, out, launches_ms);
}

}  // namespace

extern "C" {

void ellc_light_default_params(ellc_light_params* p) {
  if (!p) return;
  p->gain_min = 0.25f; p->gain_max = 4.0f; p->min_pixels = 16;
}

int ellc_light_solve(const ellc_light_normal* n, const ellc_light_params* p, const float* light_in, float* light_out) {
  const float keep[2] = {light_in ? light_in[0] : 1.0f, light_in ? light_in[1] : 0.0f};
  const double det = n->sum_w * n->sum_w_ss - n->sum_w_s * n->sum_w_s;
  const double gain = (n->sum_w * n->sum_w_st - n->sum_w_s * n->sum_w_t) / det;
  const double offset = (n->sum_w_t - gain * n->sum_w_s) / n->sum_w;
  const bool ok = n->n_photo >= p->min_pixels && det > 1e-10 * n->sum_w * n->sum_w_ss && gain >= (double)p->gain_min && gain <= (double)p->gain_max &&
                  std::fabs(offset) <= 255.0;   // (NaN fails every test)
  light_out[0] = ok ? (float)gain : keep[0];
  light_out[1] = ok ? (float)offset : keep[1];
  return ok ? 0 : 1;
}

ellc_status ellc_keyframe_light_step(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, const float* light_in,
                                     int level, const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_light_normal* out) {
  return light_step_impl(c, B, src_kf_slots, dst_kf_slots, T12, light_in, level, filter, params, out, nullptr);
}

ellc_status ellc_keyframe_sim3_step_lit(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, const float* light,
                                        int level, const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_sim3_normal* out) {
  return sim3_step_lit_impl(c, B, src_kf_slots, dst_kf_slots, T12, light, level, filter, params, out, nullptr);
}

ellc_status ellc_keyframe_sim3_align_lit(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12_in, const float* light_in,
                                         int level_from, int level_to, const ellc_map_filter* filter, const ellc_sim3_params* params,
                                         const ellc_light_params* light_params, int max_iter, float eps, float* T12_out, float* light_out,
                                         ellc_sim3_normal* out, ellc_light_normal* light_rec_out, int* iters_out, float* trace_T12,
                                         ellc_sim3_normal* trace_rec, float* trace_light, ellc_light_normal* trace_light_rec, int trace_capacity) {
  if (!c) return ELLC_ERR_BAD_ARG;
  const char* who = "ellc_keyframe_sim3_align_lit";
  if (!T12_out || !out || !light_out || !light_params) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  if (level_from < level_to) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": level_from below level_to");
  if (max_iter < 1 || max_iter > 64) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": max_iter out of range");
  if (!(eps >= 0.0f) || !std::isfinite(eps)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": eps negative or not finite");
  ELLC_TRY(sim3_validate(c, who, B, src_kf_slots, dst_kf_slots, T12_in, level_to, level_from, filter, params));
  ELLC_TRY(light_check(c, who, B, light_in));
  ELLC_TRY(light_check_params(c, who, light_params));
  const int n_levels = level_from - level_to + 1;
  const bool traced = trace_T12 || trace_rec || trace_light || trace_light_rec;
  if (traced && trace_capacity < n_levels * max_iter + 1) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": trace_capacity too small");
  ELLC_ENTER(c);
  // everything of the call is kept here until it has succeeded: a failure half-way leaves the caller's arrays as they were
  std::vector<float> T(T12_in, T12_in + (size_t)B * 12), tT, tL, unit;
  const float* l0 = light_or_unit(light_in, B, unit);
  std::vector<float> l(l0, l0 + (size_t)B * 2);
  std::vector<int> iters((size_t)B * n_levels, 0), n_trace((size_t)B, 0);
  std::vector<ellc_sim3_normal> tR, rec((size_t)B);
  std::vector<ellc_light_normal> tLR, lrec((size_t)B);
  if (trace_T12) tT.assign((size_t)B * trace_capacity * 12, 0.0f);
  if (trace_light) tL.assign((size_t)B * trace_capacity * 2, 0.0f);
  if (trace_rec) {
    ellc_sim3_normal unused;
    std::memset(&unused, 0, sizeof(unused));
    unused.n_kept = -1;
    tR.assign((size_t)B * trace_capacity, unused);
  }
  if (trace_light_rec) {
    ellc_light_normal unused;
    std::memset(&unused, 0, sizeof(unused));
    unused.n_kept = -1;
    tLR.assign((size_t)B * trace_capacity, unused);
  }
  std::vector<int> active, as, ad;
  std::vector<float> aT, aL;
  // one evaluation of the pairs in `active`: the light records, the lights solved from them, the Sim(3) records at those lights into
  // rec[0..active.size()), and the traces
  auto evaluate = [&](int level) -> ellc_status {
    const int n = (int)active.size();
    as.resize(n); ad.resize(n); aT.resize((size_t)n * 12); aL.resize((size_t)n * 2);
    for (int k = 0; k < n; k++) {
      as[k] = src_kf_slots[active[k]]; ad[k] = dst_kf_slots[active[k]];
      std::memcpy(&aT[(size_t)k * 12], &T[(size_t)active[k] * 12], 12 * sizeof(float));
      std::memcpy(&aL[(size_t)k * 2], &l[(size_t)active[k] * 2], 2 * sizeof(float));
    }
    ELLC_TRY(light_evaluate(c, n, as.data(), ad.data(), aT.data(), aL.data(), level, filter, params, lrec.data(), nullptr));
    for (int k = 0; k < n; k++) (void)ellc_light_solve(&lrec[k], light_params, &aL[(size_t)k * 2], &aL[(size_t)k * 2]);
    ELLC_TRY(sim3l_evaluate(c, n, as.data(), ad.data(), aT.data(), aL.data(), level, filter, params, rec.data(), nullptr));
    for (int k = 0; k < n; k++) {
      const int b = active[k];
      std::memcpy(&l[(size_t)b * 2], &aL[(size_t)k * 2], 2 * sizeof(float));
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
  std::memcpy(light_out, l.data(), (size_t)B * 2 * sizeof(float));
  if (light_rec_out) std::memcpy(light_rec_out, lrec.data(), (size_t)B * sizeof(ellc_light_normal));
  if (iters_out) std::memcpy(iters_out, iters.data(), iters.size() * sizeof(int));
  if (trace_T12) std::memcpy(trace_T12, tT.data(), tT.size() * sizeof(float));
  if (trace_rec) std::memcpy(trace_rec, tR.data(), tR.size() * sizeof(ellc_sim3_normal));
  if (trace_light) std::memcpy(trace_light, tL.data(), tL.size() * sizeof(float));
  if (trace_light_rec) std::memcpy(trace_light_rec, tLR.data(), tLR.size() * sizeof(ellc_light_normal));
  return ELLC_OK;
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_light_step(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, const float* light_in,
                                    int level, const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_light_normal* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) { return light_step_impl(c, B, src_kf_slots, dst_kf_slots, T12, light_in, level, filter, params, out, ms); });
}

ellc_status ellc_profile_sim3_step_lit(ellc_ctx* c, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, const float* light,
                                       int level, const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_sim3_normal* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) { return sim3_step_lit_impl(c, B, src_kf_slots, dst_kf_slots, T12, light, level, filter, params, out, ms); });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
