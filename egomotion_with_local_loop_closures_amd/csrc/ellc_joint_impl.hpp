// ellc_keyframe_joint_step / _apply / _refine, ellc_joint_solve, ellc_joint_default_params (include/ellc_abi.h): the host side of the
// joint refinement of B views' poses and keyframe slot K's inverse depths. Included at the end of ellc_hip.hip behind
// ellc_ring_common.hpp: the refusals (the parameters' included), staging, plane carve, fetches, reader marks and destination store of
// the calls of K against views are used here; the staged view's pose step (JointView), the names of the planes, the launches of a
// step (four) and of an apply (two) with the wait the loop needs between them, and the assembly of the record are this family's own.
#pragma once
#include "ellc_ring_common.hpp"
#include "ellc_sim3_impl.hpp"
#include "ellc_joint_solve.hpp"
#include "ellc_kernels_joint.hpp"

using namespace ellc;

static_assert(sizeof(ellc_joint_params) == 20 && sizeof(ellc_joint_normal) == 11600 && offsetof(ellc_joint_normal, a) == 1344 &&
                  offsetof(ellc_joint_normal, S) == 1728 && offsetof(ellc_joint_normal, s) == 11136 && offsetof(ellc_joint_normal, chi2_photo) == 11520 &&
                  offsetof(ellc_joint_normal, n_terms) == 11536 && offsetof(ellc_joint_normal, n_kept) == 11544 && offsetof(ellc_joint_normal, B) == 11564 &&
                  offsetof(ellc_joint_normal, n_view_terms) == 11568 && sizeof(ellc_joint_apply_stats) == 32,
              "ellc_joint_params is 20 bytes, ellc_joint_normal 11600, ellc_joint_apply_stats 32");
static_assert(sizeof(JointView) == 96 && ELLC_JOINT_VIEWS == ELLC_JOINT_MAX_VIEWS, "a staged view is 96 bytes");

namespace {

const int JOINT_MAX_REQUESTS = (ELLC_JOINT_MAX_VIEWS * (ELLC_JOINT_MAX_VIEWS + 1)) / 2 + ELLC_JOINT_MAX_VIEWS;   // pairs b <= c, then views
// the planes of the family in one grow-only buffer, each named by the bytes a pixel in front of it (PlaneCarve): ten f32 planes (one
// spare), then five u8 planes
enum { JP_STATE = 0, JP_D = 4, JP_IH = 8, JP_GD = 12, JP_INV_OUT = 16, JP_DEPTH = 20, JP_VAR = 24, JP_KEPT_DEPTH = 28, JP_KEPT_VAR = 32,
       JP_PSTATUS = 40, JP_VIEWS, JP_STATUS, JP_KEPT_VIEWS, JP_KEPT_STATUS, JP_BYTES };

PlaneCarve joint_planes(ellc_ctx* c) { return PlaneCarve{c->joint_planes_d, c->joint_planes_cap}; }

// what all three calls refuse, in ellc_keyframe_refine_depth's order; dst is -1 for the step
ellc_status joint_validate(ellc_ctx* c, const char* who, int kf_slot, int level, int B, int views_are_kf, const int* view_slots, const float* T12,
                           const float* light, const ellc_map_filter* f, const ellc_joint_params* p, int dst) {
  const std::string w(who);
  if (!view_slots || !T12 || !f || !p) return fail(c, ELLC_ERR_BAD_ARG, w + ": null pointer");
  ELLC_TRY(ring_views_check(c, who, B, ELLC_JOINT_MAX_VIEWS, views_are_kf, level, f, T12, light));
  ELLC_TRY(ring_views_check_params(c, who, p, B));
  return ring_views_check_slots(c, who, dst, level, kf_slot, B, view_slots, views_are_kf);
}

// the buffers of a call on `level` and the arguments that do not change between its launches (behind ELLC_ENTER)
ellc_status joint_prepare(ellc_ctx* c, int kf_slot, int level, int B, const ellc_map_filter* f, const ellc_joint_params* p, JointArgs& a) {
  const size_t n = (size_t)c->geom_h[level].n;
  a = JointArgs{};
  a.v = ring_view(c, level, f);
  a.blocks = (int)((n + 255) / 256);
  ELLC_TRY(pair_reserve(c, c->joint, JOINT_MAX_REQUESTS, sizeof(JointView), sizeof(JointPairRec), (size_t)JOINT_MAX_REQUESTS * a.v.tiles));
  ELLC_TRY(pair_reserve(c, c->joint_count, 1, sizeof(int), sizeof(JointCountRec), (size_t)a.blocks));
  ELLC_TRY(dev_grow(c, &c->joint_planes_d, &c->joint_planes_cap, n, JP_BYTES));
  const PlaneCarve jp = joint_planes(c);
  a.views = (const JointView*)c->joint.stage_d;
  a.partials = (JointPairRec*)c->joint.partials_d;
  a.out = (JointPairRec*)c->joint.out_dev_alias;
  a.cpartials = (JointCountRec*)c->joint_count.partials_d;
  a.cout = (JointCountRec*)c->joint_count.out_dev_alias;
  a.d_in = jp.at<float>(JP_STATE);
  a.d = jp.at<float>(JP_D); a.ih = jp.at<float>(JP_IH); a.gd = jp.at<float>(JP_GD);
  a.pstatus = jp.at<uint8_t>(JP_PSTATUS);
  a.inv_depth_out = jp.at<float>(JP_INV_OUT); a.depth = jp.at<float>(JP_DEPTH); a.var = jp.at<float>(JP_VAR);
  a.nviews = jp.at<uint8_t>(JP_VIEWS); a.status = jp.at<uint8_t>(JP_STATUS);
  a.kf_slot = kf_slot;
  a.B = B;
  a.first = 0;
  a.w0 = 1.0f / p->sigma_i2;
  a.sp = sqrtf(a.w0);
  a.huber_k = p->huber_k;
  a.prior_weight = p->prior_weight;
  a.max_step_rel = p->max_step_rel;
  a.min_views = p->min_views;
  return ELLC_OK;
}

// the state plane: the caller's inverse depths, or zeros (a zero sends a pixel to its own d0)
ellc_status joint_set_state(ellc_ctx* c, size_t n, const float* inv_depth_in) {
  const PlaneCarve jp = joint_planes(c);
  if (inv_depth_in) ELLC_HIP(c, hipMemcpyAsync(jp.at<float>(JP_STATE), inv_depth_in, n * 4, hipMemcpyHostToDevice, c->stream));
  else ELLC_HIP(c, hipMemsetAsync(jp.at<float>(JP_STATE), 0, n * 4, c->stream));
  return ELLC_OK;
}

// the views on their way to the device; a view also carries its pose step rounded to f32. xi NULL: no pose steps (the staging's zeros)
ellc_status joint_stage(ellc_ctx* c, int level, int B, int views_are_kf, const int* view_slots, const float* T12, const float* light, const double* xi) {
  return ring_views_stage<JointView>(c, c->joint, level, B, views_are_kf, view_slots, T12, light, [&](JointView& vw, int b) {
    if (xi)
      for (int k = 0; k < 6; k++) vw.xf[k] = (float)xi[6 * b + k];
  });
}

// One step at the staged views and the state plane: the four launches, the wait, the record. launches_ms (the diagnostic hook only).
ellc_status joint_run_step(ellc_ctx* c, const JointArgs& a, ellc_joint_normal* out, float* launches_ms) {
  const int B = a.B, n_pairs = (B * (B + 1)) / 2, requests = n_pairs + B;
  LaunchTimer t(c, launches_ms);
  ELLC_TRY(t.begin());
  hipLaunchKernelGGL(joint_pixels, dim3(a.blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(joint_count_finish, dim3(1), dim3(64), 0, c->stream, a);
  hipLaunchKernelGGL(joint_pairs, dim3(a.v.tiles, requests), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(joint_pair_finish, dim3(requests), dim3(64), 0, c->stream, a);
  ELLC_HIP(c, hipGetLastError());
  ELLC_TRY(t.end());
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  const JointCountRec* cr = (const JointCountRec*)c->joint_count.out_h;
  const JointPairRec* pr = (const JointPairRec*)c->joint.out_h;
  std::memset(out, 0, sizeof(*out));
  const int N = 6 * B;
  for (int b = 0, y = 0; b < B; b++)
    for (int cc = b; cc < B; cc++, y++)
      for (int k = 0; k < 6; k++) {
        for (int l = (b == cc ? k : 0); l < 6; l++) out->S[tri_index(N, 6 * b + k, 6 * cc + l)] = pr[y].s[6 * k + l];
        if (b == cc) out->s[6 * b + k] = pr[y].s[36 + k];
      }
  for (int b = 0; b < B; b++)
    for (int k = 0; k < 6; k++) {
      for (int l = k; l < 6; l++) out->A[b][tri_index(6, k, l)] = pr[n_pairs + b].s[6 * k + l];
      out->a[b][k] = pr[n_pairs + b].s[36 + k];
    }
  out->chi2_photo = cr->s[0]; out->chi2_prior = cr->s[1];
  out->n_terms = cr->n_terms;
  out->n_kept = cr->n[0]; out->n_taking_part = cr->n[1]; out->n_used = cr->n[2]; out->n_too_few_views = cr->n[3]; out->n_no_information = cr->n[4];
  out->B = B;
  for (int b = 0; b < B; b++) out->n_view_terms[b] = cr->nv[b];
  return t.read();
}

// One apply at the staged views (with their pose steps) and the state plane: the five planes stay on the device; the wait, the stats.
ellc_status joint_run_apply(ellc_ctx* c, const JointArgs& a, ellc_joint_apply_stats* out, float* launches_ms) {
  LaunchTimer t(c, launches_ms);
  ELLC_TRY(t.begin());
  hipLaunchKernelGGL(joint_apply_pixels, dim3(a.blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(joint_count_finish, dim3(1), dim3(64), 0, c->stream, a);
  ELLC_HIP(c, hipGetLastError());
  ELLC_TRY(t.end());
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  const JointCountRec* cr = (const JointCountRec*)c->joint_count.out_h;
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->n_kept = cr->n[0]; out->n_taking_part = cr->n[1]; out->n_stepped = cr->n[2]; out->n_too_few_views = cr->n[3];
    out->n_no_information = cr->n[4]; out->n_bad_step = cr->n[5];
  }
  return t.read();
}

// T12_out[b] = ellc_sim3_apply((xi_b, log-scale 0), T12[b])
void joint_move_poses(int B, const double* xi, const float* T12, float* T12_out) {
  for (int b = 0; b < B; b++) {
    double xi7[7] = {xi[6 * b], xi[6 * b + 1], xi[6 * b + 2], xi[6 * b + 3], xi[6 * b + 4], xi[6 * b + 5], 0.0};
    ellc_sim3_apply(xi7, T12 + (size_t)12 * b, T12_out + (size_t)12 * b);
  }
}

ellc_status joint_step_impl(ellc_ctx* c, int kf_slot, int level, int B, int views_are_kf, const int* view_slots, const float* T12, const float* light,
                            const ellc_map_filter* f, const ellc_joint_params* p, const float* inv_depth_in, ellc_joint_normal* out, float* launches_ms) {
  const char* who = "ellc_keyframe_joint_step";
  if (!c) return ELLC_ERR_BAD_ARG;
  // validated first: a refused call leaves the context as it was and `out` unwritten
  if (!out) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  ELLC_TRY(joint_validate(c, who, kf_slot, level, B, views_are_kf, view_slots, T12, light, f, p, -1));
  ELLC_ENTER(c);   // behind the batches in flight, on the main stream
  JointArgs a;
  ELLC_TRY(joint_prepare(c, kf_slot, level, B, f, p, a));
  ELLC_TRY(joint_set_state(c, (size_t)c->geom_h[level].n, inv_depth_in));
  ELLC_TRY(joint_stage(c, level, B, views_are_kf, view_slots, T12, light, nullptr));
  ellc_joint_normal rec;
  ELLC_TRY(joint_run_step(c, a, &rec, launches_ms));
  ELLC_TRY(ring_views_mark_use(c, B, view_slots, views_are_kf));
  *out = rec;
  return ELLC_OK;
}

ellc_status joint_apply_impl(ellc_ctx* c, int kf_slot, int level, int B, int views_are_kf, const int* view_slots, const float* T12, const float* light,
                             const ellc_map_filter* f, const ellc_joint_params* p, const float* inv_depth_in, const double* xi, int dst, float* T12_out,
                             float* inv_depth_out, float* depth, float* var, uint8_t* views, uint8_t* status, ellc_joint_apply_stats* out,
                             float* launches_ms) {
  const char* who = "ellc_keyframe_joint_apply";
  if (!c) return ELLC_ERR_BAD_ARG;
  if (!xi || !T12_out) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": null pointer");
  ELLC_TRY(joint_validate(c, who, kf_slot, level, B, views_are_kf, view_slots, T12, light, f, p, dst));
  for (int k = 0; k < 6 * B; k++)
    if (!std::isfinite(xi[k])) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": xi not finite");
  ELLC_ENTER(c);
  const size_t n = (size_t)c->geom_h[level].n;
  JointArgs a;
  ELLC_TRY(joint_prepare(c, kf_slot, level, B, f, p, a));
  ELLC_TRY(joint_set_state(c, n, inv_depth_in));
  ELLC_TRY(joint_stage(c, level, B, views_are_kf, view_slots, T12, light, xi));
  ellc_joint_apply_stats st;
  ELLC_TRY(joint_run_apply(c, a, &st, launches_ms));
  ELLC_TRY(ring_views_mark_use(c, B, view_slots, views_are_kf));
  if (dst >= 0) ELLC_TRY(ring_views_store_dst(c, dst, a.depth, a.var, n, &((const JointCountRec*)c->joint_count.out_h)->n_dense));
  const RingFetch fetch[5] = {{inv_depth_out, a.inv_depth_out, n * 4}, {depth, a.depth, n * 4}, {var, a.var, n * 4}, {views, a.nviews, n}, {status, a.status, n}};
  ELLC_TRY(ring_fetch(c, fetch));
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  std::vector<float> T((size_t)B * 12);
  joint_move_poses(B, xi, T12, T.data());
  std::memcpy(T12_out, T.data(), T.size() * sizeof(float));
  if (out) *out = st;
  return ELLC_OK;
}

// c of the acceptance rule; false: the record cannot be judged
bool joint_cost(const ellc_joint_normal& r, double& cost) {
  if (r.n_used <= 0) return false;
  cost = (r.chi2_photo + r.chi2_prior) / (double)(r.n_terms + r.n_used);
  return cost == cost;
}

}  // namespace

extern "C" {

void ellc_joint_default_params(ellc_joint_params* p) {
  if (!p) return;
  p->sigma_i2 = 16.0f; p->huber_k = 1.345f; p->prior_weight = 1.0f; p->max_step_rel = 0.5f; p->min_views = 2;
}

int ellc_joint_solve(const ellc_joint_normal* rec, double lambda, double* xi) {
  if (!rec || !xi) return 1;
  return joint_solve_record(rec, lambda, xi);
}

ellc_status ellc_keyframe_joint_step(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12,
                                     const float* light, const ellc_map_filter* filter, const ellc_joint_params* params, const float* inv_depth_in,
                                     ellc_joint_normal* out) {
  return joint_step_impl(c, kf_slot, level, B, views_are_keyframes, view_slots, T12, light, filter, params, inv_depth_in, out, nullptr);
}

ellc_status ellc_keyframe_joint_apply(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12,
                                      const float* light, const ellc_map_filter* filter, const ellc_joint_params* params, const float* inv_depth_in,
                                      const double* xi, int dst_kf_slot, float* T12_out, float* inv_depth_out, float* depth, float* var, uint8_t* views,
                                      uint8_t* status, ellc_joint_apply_stats* out) {
  return joint_apply_impl(c, kf_slot, level, B, views_are_keyframes, view_slots, T12, light, filter, params, inv_depth_in, xi, dst_kf_slot, T12_out,
                          inv_depth_out, depth, var, views, status, out, nullptr);
}

ellc_status ellc_keyframe_joint_refine(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12_in,
                                       const float* light, const ellc_map_filter* filter, const ellc_joint_params* params, const float* inv_depth_in,
                                       int max_iter, float eps, double lambda, int dst_kf_slot, float* T12_out, ellc_joint_normal* out, int* iters_out,
                                       float* inv_depth_out, float* depth, float* var, uint8_t* views, uint8_t* status, float* trace_T12,
                                       ellc_joint_normal* trace_rec, double* trace_xi, int* trace_accepted, int trace_capacity) {
  const char* who = "ellc_keyframe_joint_refine";
  if (!c) return ELLC_ERR_BAD_ARG;
  const std::string w(who);
  if (!T12_out || !out) return fail(c, ELLC_ERR_BAD_ARG, w + ": null pointer");
  ELLC_TRY(joint_validate(c, who, kf_slot, level, B, views_are_keyframes, view_slots, T12_in, light, filter, params, dst_kf_slot));
  if (!(params->prior_weight > 0.0f)) return fail(c, ELLC_ERR_BAD_ARG, w + ": prior_weight must be > 0");
  if (max_iter < 1 || max_iter > 16) return fail(c, ELLC_ERR_BAD_ARG, w + ": max_iter out of range");
  if (!(eps >= 0.0f) || !std::isfinite(eps)) return fail(c, ELLC_ERR_BAD_ARG, w + ": eps negative or not finite");
  if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail(c, ELLC_ERR_BAD_ARG, w + ": lambda negative or not finite");
  const bool traced = trace_T12 || trace_rec || trace_xi || trace_accepted;
  if (traced && trace_capacity < max_iter + 1) return fail(c, ELLC_ERR_BAD_ARG, w + ": trace_capacity too small");
  ELLC_ENTER(c);
  const size_t n = (size_t)c->geom_h[level].n, T_len = (size_t)B * 12;
  JointArgs a;
  ELLC_TRY(joint_prepare(c, kf_slot, level, B, filter, params, a));
  const PlaneCarve jp = joint_planes(c);
  // everything of the call is kept here (and in planes of the call's own) until it has succeeded
  std::vector<float> T(T12_in, T12_in + T_len), Tt(T_len), tT;
  std::vector<ellc_joint_normal> tR;
  std::vector<double> tX, xi((size_t)6 * B);
  std::vector<int> tA;
  if (trace_T12) tT.assign(T_len * trace_capacity, 0.0f);
  if (trace_rec) trace_unwritten(tR, (size_t)trace_capacity);
  if (trace_xi) tX.assign((size_t)6 * B * trace_capacity, 0.0);
  if (trace_accepted) tA.assign((size_t)trace_capacity, 0);
  int n_trace = 0, iters = 0;
  auto traced_step = [&](const std::vector<float>& at, ellc_joint_normal* rec) -> ellc_status {
    ELLC_TRY(joint_stage(c, level, B, views_are_keyframes, view_slots, at.data(), light, nullptr));
    ELLC_TRY(joint_run_step(c, a, rec, nullptr));
    if (trace_T12) std::memcpy(&tT[T_len * n_trace], at.data(), T_len * sizeof(float));
    if (trace_rec) tR[n_trace] = *rec;
    n_trace++;
    return ELLC_OK;
  };
  // the accepted state: the state plane and, for the caller, the planes of the apply that made it. With no accepted trial K's own
  const KfLevelDev& K = c->kf_tab_h[(size_t)level * c->cfg.max_keyframes + kf_slot];
  ELLC_TRY(joint_set_state(c, n, inv_depth_in));
  ELLC_HIP(c, hipMemcpyAsync(jp.at<float>(JP_KEPT_DEPTH), K.depth, n * 4, hipMemcpyDeviceToDevice, c->stream));
  ELLC_HIP(c, hipMemcpyAsync(jp.at<float>(JP_KEPT_VAR), K.var, n * 4, hipMemcpyDeviceToDevice, c->stream));
  ELLC_HIP(c, hipMemsetAsync(jp.at<uint8_t>(JP_KEPT_VIEWS), 0, n, c->stream));
  ELLC_HIP(c, hipMemsetAsync(jp.at<uint8_t>(JP_KEPT_STATUS), 0, n, c->stream));
  ellc_joint_normal rec, trial;
  ELLC_TRY(traced_step(T, &rec));
  if (trace_accepted) tA[0] = 1;
  int dense = 0;   // pixels of the accepted planes with a depth > 0: counted by the apply that made them
  bool have_dense = false;
  while (iters < max_iter) {
    if (ellc_joint_solve(&rec, lambda, xi.data())) break;
    if (trace_xi) std::memcpy(&tX[(size_t)6 * B * (n_trace - 1)], xi.data(), xi.size() * sizeof(double));
    double m = 0.0;
    for (size_t k = 0; k < xi.size(); k++) m = std::max(m, std::fabs(xi[k]));
    if (m < (double)eps) break;
    // the trial: the depths stepped at the state's transforms, then the transforms moved
    ELLC_TRY(joint_stage(c, level, B, views_are_keyframes, view_slots, T.data(), light, xi.data()));
    a.d_in = jp.at<float>(JP_STATE);
    ELLC_TRY(joint_run_apply(c, a, nullptr, nullptr));
    const int trial_dense = ((const JointCountRec*)c->joint_count.out_h)->n_dense;
    joint_move_poses(B, xi.data(), T.data(), Tt.data());
    a.d_in = a.inv_depth_out;
    ELLC_TRY(traced_step(Tt, &trial));
    a.d_in = jp.at<float>(JP_STATE);
    double c0, c1;
    if (!joint_cost(rec, c0) || !joint_cost(trial, c1) || !(c1 <= c0)) break;
    const struct { void* to; const void* from; size_t bytes; } keep[5] = {{jp.at<float>(JP_STATE), a.inv_depth_out, n * 4}, {jp.at<float>(JP_KEPT_DEPTH), a.depth, n * 4},
                                                                         {jp.at<float>(JP_KEPT_VAR), a.var, n * 4}, {jp.at<uint8_t>(JP_KEPT_VIEWS), a.nviews, n},
                                                                         {jp.at<uint8_t>(JP_KEPT_STATUS), a.status, n}};
    for (int k = 0; k < 5; k++) ELLC_HIP(c, hipMemcpyAsync(keep[k].to, keep[k].from, keep[k].bytes, hipMemcpyDeviceToDevice, c->stream));
    T = Tt;
    rec = trial;
    dense = trial_dense;
    have_dense = true;
    if (trace_accepted) tA[n_trace - 1] = 1;
    iters++;
  }
  ELLC_TRY(ring_views_mark_use(c, B, view_slots, views_are_keyframes));
  if (dst_kf_slot >= 0) {
    int32_t hint = dense;
    if (!have_dense) {   // K's own planes: counted on a host copy, as ellc_keyframe_set_depth counts
      std::vector<float> z(n);
      ELLC_HIP(c, hipMemcpyAsync(z.data(), jp.at<float>(JP_KEPT_DEPTH), n * 4, hipMemcpyDeviceToHost, c->stream));
      ELLC_HIP(c, hipStreamSynchronize(c->stream));
      hint = 0;
      for (size_t i = 0; i < n; i++) hint += z[i] > 0.0f ? 1 : 0;
    }
    ELLC_TRY(ring_views_store_dst(c, dst_kf_slot, jp.at<float>(JP_KEPT_DEPTH), jp.at<float>(JP_KEPT_VAR), n, &hint));
  }
  const RingFetch fetch[5] = {{inv_depth_out, jp.at<float>(JP_STATE), n * 4}, {depth, jp.at<float>(JP_KEPT_DEPTH), n * 4}, {var, jp.at<float>(JP_KEPT_VAR), n * 4},
                              {views, jp.at<uint8_t>(JP_KEPT_VIEWS), n}, {status, jp.at<uint8_t>(JP_KEPT_STATUS), n}};
  ELLC_TRY(ring_fetch(c, fetch));
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  std::memcpy(T12_out, T.data(), T_len * sizeof(float));
  *out = rec;
  if (iters_out) *iters_out = iters;
  if (trace_T12) std::memcpy(trace_T12, tT.data(), tT.size() * sizeof(float));
  if (trace_rec) std::memcpy(trace_rec, tR.data(), tR.size() * sizeof(ellc_joint_normal));
  if (trace_xi) std::memcpy(trace_xi, tX.data(), tX.size() * sizeof(double));
  if (trace_accepted) std::memcpy(trace_accepted, tA.data(), tA.size() * sizeof(int));
  return ELLC_OK;
}

#ifdef ELLC_DIAG_ABI
ellc_status ellc_profile_joint_step(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12,
                                    const float* light, const ellc_map_filter* filter, const ellc_joint_params* params, const float* inv_depth_in,
                                    ellc_joint_normal* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) {
    return joint_step_impl(c, kf_slot, level, B, views_are_keyframes, view_slots, T12, light, filter, params, inv_depth_in, out, ms);
  });
}

ellc_status ellc_profile_joint_apply(ellc_ctx* c, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots, const float* T12,
                                     const float* light, const ellc_map_filter* filter, const ellc_joint_params* params, const float* inv_depth_in,
                                     const double* xi, int dst_kf_slot, float* T12_out, float* inv_depth_out, float* depth, float* var, uint8_t* views,
                                     uint8_t* status, ellc_joint_apply_stats* out, float* launches_ms) {
  return ring_profiled(launches_ms, [&](float* ms) {
    return joint_apply_impl(c, kf_slot, level, B, views_are_keyframes, view_slots, T12, light, filter, params, inv_depth_in, xi, dst_kf_slot, T12_out,
                            inv_depth_out, depth, var, views, status, out, ms);
  });
}
#endif   // ELLC_DIAG_ABI

}  // extern "C"
