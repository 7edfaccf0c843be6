// The host scaffold of the calls over the keyframe ring's semi-dense maps (ellc_keyframe_map_points, _render_depth, _fuse_depth,
// _depth_consistency, _sim3_step / _align, _light_step, _sim3_step_lit / _align_lit, _trial_propagate, _refine_depth, _sweep_depth, _cull_depth, _joint_step / _apply / _refine, ellc_depth_absorb_keyframes, ellc_depth_restart_from_keyframes): what they
// refuse alike, the view map_keep reads, the timing window of the diagnostic hooks, grow-only buffers, the launch loop of the pair
// reductions and the run of a call of one keyframe slot against views (ring_views_*: staging, plane carve, scratch, launches, fetches,
// destination store). Included at the end of ellc_hip.hip in front of the *_impl.hpp of those calls (the library is one translation
// unit). A new call of the family supplies a record type with rec_zero / rec_add / rec_wave_sum (ellc_pair_reduce.hpp), a pass kernel
// and a finish kernel over them, and its own list of refusals in its own order.
#pragma once
#include "ellc_context.hpp"
#include "ellc_kernels_map.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace ellc;

#define ELLC_TRY(expr)                   \
  do {                                   \
    const ellc_status s__ = (expr);      \
    if (s__ != ELLC_OK) return s__;      \
  } while (0)

namespace ellc {

void pair_free(PairScratch& s) {
  if (s.partials_d) (void)hipFree(s.partials_d);
  if (s.stage_d) (void)hipFree(s.stage_d);
  if (s.stage_h) (void)hipHostFree(s.stage_h);
  if (s.out_h) (void)hipHostFree(s.out_h);
  s = PairScratch();
}

}  // namespace ellc

namespace {

// ---- refusals: validated first, a refused call leaves the context as it was (the message is composed only when a call is refused)

ellc_status ring_check_filter(ellc_ctx* c, const char* who, const ellc_map_filter* f) {
  if (f->min_support < 0 || f->min_support > 8 || f->stride < 1 || !(f->support_k2 >= 0.0f) || !std::isfinite(f->support_k2) || std::isnan(f->max_var))
    return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": filter out of range");
  return ELLC_OK;
}

ellc_status ring_check_slots(ellc_ctx* c, const char* who, int B, const int* slots, int n_slots) {
  for (int b = 0; b < B; b++)
    if (!slot_ok(slots[b], n_slots)) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": slot index out of range");
  return ELLC_OK;
}

ellc_status ring_check_ready(ellc_ctx* c, const char* who, int B, const int* slots) {
  for (int b = 0; b < B; b++)
    if (!c->kf_has_image[slots[b]] || !c->kf_has_depth[slots[b]]) return fail(c, ELLC_ERR_NOT_READY, std::string(who) + ": keyframe slot lacks image or depth");
  return ELLC_OK;
}

// what map_keep reads on `level` under filter f
MapView ring_view(const ellc_ctx* c, int level, const ellc_map_filter* f) {
  MapView v;
  v.geom = c->geom_d;
  v.kf_tab = c->kf_tab_d;
  v.level = level;
  v.max_kf = c->cfg.max_keyframes;
  v.tiles = c->tile_begin[level + 1] - c->tile_begin[level];
  v.max_var = f->max_var;
  v.min_support = f->min_support;
  v.support_k2 = f->support_k2;
  v.stride = f->stride;
  return v;
}

// a given light: every value finite (NULL means (1, 0) for every pair)
ellc_status light_check(ellc_ctx* c, const char* who, int B, const float* light) {
  if (!light) return ELLC_OK;
  for (int k = 0; k < 2 * B; k++)
    if (!std::isfinite(light[k])) return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": light not finite");
  return ELLC_OK;
}

// ---- the calls of one keyframe slot K against B views (ellc_keyframe_refine_depth, _sweep_depth, _cull_depth, _joint_step / _apply /
// _refine): what they refuse alike, in two runs around the call's own parameter check, the views' images, the frame slots' reader
// marks and the store into a destination slot.

// B, views_are_keyframes, the level and its size, the filter (NULL: the call has none), the transforms and the lights
ellc_status ring_views_check(ellc_ctx* c, const char* who, int B, int max_B, int views_are_kf, int level, const ellc_map_filter* f, const float* T12,
                             const float* light) {
  const std::string w(who);
  if (B < 1 || B > max_B) return fail(c, ELLC_ERR_BAD_ARG, w + ": B out of range");
  if (views_are_kf < 0 || views_are_kf > 1) return fail(c, ELLC_ERR_BAD_ARG, w + ": views_are_keyframes not 0 or 1");
  if (level < 0 || level >= c->L) return fail(c, ELLC_ERR_BAD_ARG, w + ": level out of range");
  if (c->geom_h[level].n > (1 << 24)) return fail(c, ELLC_ERR_BAD_ARG, w + ": more than 2^24 pixels on the level");
  if (f) ELLC_TRY(ring_check_filter(c, who, f));
  for (int k = 0; k < 12 * B; k++)
    if (!std::isfinite(T12[k])) return fail(c, ELLC_ERR_BAD_ARG, w + ": transform not finite");
  return light_check(c, who, B, light);
}

// the destination, K's slot and the views' slots, and what they have to hold
ellc_status ring_views_check_slots(ellc_ctx* c, const char* who, int dst, int level, int kf_slot, int B, const int* view_slots, int views_are_kf) {
  const std::string w(who);
  if (dst < -1 || dst >= c->cfg.max_keyframes) return fail(c, ELLC_ERR_BAD_ARG, w + ": destination slot out of range");
  if (dst >= 0 && level != 0) return fail(c, ELLC_ERR_BAD_ARG, w + ": a destination slot takes level 0 only");
  ELLC_TRY(ring_check_slots(c, who, 1, &kf_slot, c->cfg.max_keyframes));
  ELLC_TRY(ring_check_slots(c, who, B, view_slots, views_are_kf ? c->cfg.max_keyframes : c->cfg.max_frames));
  ELLC_TRY(ring_check_ready(c, who, 1, &kf_slot));
  for (int b = 0; b < B; b++)
    if (!(views_are_kf ? c->kf_has_image[view_slots[b]] : c->fr_has_image[view_slots[b]]))
      return fail(c, ELLC_ERR_NOT_READY, w + ": view slot lacks an image");
  return ELLC_OK;
}

// the table entry of a view's slot on `level`, and its image there
size_t ring_view_entry(const ellc_ctx* c, int level, int views_are_kf, int slot) {
  return (size_t)level * (views_are_kf ? c->cfg.max_keyframes : c->cfg.max_frames) + slot;
}
const uint8_t* ring_view_image(const ellc_ctx* c, int level, int views_are_kf, int slot) {
  const size_t e = ring_view_entry(c, level, views_are_kf, slot);
  return views_are_kf ? c->kf_tab_h[e].img : c->fr_tab_h[e].img;
}

// behind the launches that read the views: a later upload into a frame slot waits for this reader
ellc_status ring_views_mark_use(ellc_ctx* c, int B, const int* view_slots, int views_are_kf) {
  if (views_are_kf) return ELLC_OK;
  std::vector<char> seen((size_t)c->cfg.max_frames, 0);
  for (int b = 0; b < B; b++)
    if (!seen[view_slots[b]]) {
      seen[view_slots[b]] = 1;
      ELLC_TRY(mark_frame_use(c, view_slots[b]));
    }
  return ELLC_OK;
}

// The level-0 planes (device) into keyframe slot dst, behind the kernel that read K and the views: device to device; the rest is what
// ellc_keyframe_set_depth does behind its upload (render_store_dst's shape). *dense is the pinned count of pixels whose depth is > 0,
// read once the stream has been waited for.
ellc_status ring_views_store_dst(ellc_ctx* c, int dst, const float* depth_d, const float* var_d, size_t n, const int32_t* dense) {
  const KfLevelDev& k = c->kf_tab_h[dst];
  invalidate_records(c, dst);
  ELLC_HIP(c, hipMemcpyAsync(k.depth, depth_d, n * 4, hipMemcpyDeviceToDevice, c->stream));
  ELLC_HIP(c, hipMemcpyAsync(k.var, var_d, n * 4, hipMemcpyDeviceToDevice, c->stream));
  return finish_depth_planes(c, dst, [&]() {
    (void)hipStreamSynchronize(c->stream);
    return (size_t)*dense;
  });
}

// what ellc_keyframe_refine_depth and the joint calls refuse of their parameters alike (P: ellc_refine_params, ellc_joint_params)
template <class P>
ellc_status ring_views_check_params(ellc_ctx* c, const char* who, const P* p, int B) {
  if (!std::isfinite(p->sigma_i2) || !std::isfinite(p->huber_k) || !std::isfinite(p->prior_weight) || !std::isfinite(p->max_step_rel) ||
      !(p->sigma_i2 > 0.0f) || !(p->huber_k > 0.0f) || !(p->prior_weight >= 0.0f) || !(p->max_step_rel > 0.0f) || p->min_views < 1 || p->min_views > B)
    return fail(c, ELLC_ERR_BAD_ARG, std::string(who) + ": parameters out of range");
  return ELLC_OK;
}

// ---- timing (the diagnostic hooks only): HIP events around a window of launches; read() adds the window's device time to *out, so a
// call with several windows reports their sum. out == nullptr: nothing is recorded.
struct LaunchTimer {
  ellc_ctx* c;
  float* out;
  LaunchTimer(ellc_ctx* c_, float* out_) : c(c_), out(out_) {
    if (out) *out = 0.0f;
  }
  ellc_status begin() {
    if (out) ELLC_HIP(c, hipEventRecord(c->ev0, c->stream));
    return ELLC_OK;
  }
  ellc_status end() {
    if (out) ELLC_HIP(c, hipEventRecord(c->ev1, c->stream));
    return ELLC_OK;
  }
  ellc_status read() {   // (behind a synchronisation of the stream)
    float ms = 0.0f;
    if (out) ELLC_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (out) *out += ms;
    return ELLC_OK;
  }
};

// the body of an ellc_profile_* twin: the call with its timing on, whether or not the caller wants the figure
template <class Call>
ellc_status ring_profiled(float* launches_ms, Call call) {
  float ms = 0.0f;
  const ellc_status s = call(&ms);
  if (launches_ms) *launches_ms = ms;
  return s;
}

// ---- a device buffer of its own that only grows: `need` elements of `elem` bytes, `extra` more when it has to be allocated anew.
// (hipFree waits for what still reads the old one)
ellc_status dev_grow(ellc_ctx* c, void** p, size_t* cap, size_t need, size_t elem, size_t extra = 0) {
  if (need <= *cap) return ELLC_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  ELLC_HIP(c, hipMalloc(p, (need + extra) * elem));
  *cap = need + extra;
  return ELLC_OK;
}

// ---- pair reductions: B requests, one record each, in launches of at most per_launch requests

// requests per launch when one request's scratch takes `bytes_each` of a budget
int pair_per_launch(int B, size_t budget, size_t bytes_each) { return (int)std::min<size_t>((size_t)B, std::max<size_t>(1, budget / bytes_each)); }

// room for B staged requests of stage_bytes each, B records of rec_bytes and `partials` partial records
// (nothing of the call is in flight when its buffers grow: the call is synchronous)
ellc_status pair_reserve(ellc_ctx* c, PairScratch& s, int B, size_t stage_bytes, size_t rec_bytes, size_t partials) {
  if (B > s.cap) {
    if (s.stage_h) (void)hipHostFree(s.stage_h);
    if (s.out_h) (void)hipHostFree(s.out_h);
    if (s.stage_d) (void)hipFree(s.stage_d);
    s.stage_h = s.out_h = s.stage_d = s.out_dev_alias = nullptr;
    s.cap = 0;
    ELLC_HIP(c, hipHostMalloc(&s.stage_h, (size_t)B * stage_bytes, hipHostMallocDefault));
    ELLC_HIP(c, hipHostMalloc(&s.out_h, (size_t)B * rec_bytes, hipHostMallocDefault));
    ELLC_HIP(c, hipMalloc(&s.stage_d, (size_t)B * stage_bytes));
    ELLC_HIP(c, hipHostGetDevicePointer(&s.out_dev_alias, s.out_h, 0));
    s.cap = B;
  }
  return dev_grow(c, &s.partials_d, &s.partials_cap, partials, rec_bytes);
}

// the [cap] source slots, [cap] destination slots, [cap][12] f32 transforms record, staged and on its way to the device
// (requests beyond B are never read: blockIdx.y < B). extra_words > 0: a further block of extra_words 4-byte words a request behind
// the 14, [cap][extra_words], for a call whose requests carry more than slots and a transform; the call has reserved 14 + extra_words
// words a request. It is copied from `extra`, or with extra NULL the caller has written it into stage_h itself.
ellc_status pair_stage_slots(ellc_ctx* c, PairScratch& s, int B, const int* src, const int* dst, const float* T12, const void* extra = nullptr,
                             int extra_words = 0) {
  int* h = (int*)s.stage_h;
  std::memcpy(h, src, (size_t)B * sizeof(int));
  std::memcpy(h + s.cap, dst, (size_t)B * sizeof(int));
  std::memcpy(h + 2 * (size_t)s.cap, T12, (size_t)B * 12 * sizeof(float));
  if (extra) std::memcpy(h + 14 * (size_t)s.cap, extra, (size_t)B * extra_words * sizeof(int));
  ELLC_HIP(c, hipMemcpyAsync(s.stage_d, s.stage_h, (size_t)(14 + extra_words) * s.cap * sizeof(int), hipMemcpyHostToDevice, c->stream));
  return ELLC_OK;
}

struct RingNoStep {
  ellc_status operator()(int) const { return ELLC_OK; }
};

// The launches of a pair call and its records: per chunk of per_launch requests pre(n), the pass kernel over (tiles, n) blocks and
// the finish kernel over n waves; then `enqueued(B)` (what has to follow the launches in stream order), the synchronisation and the B
// records into `out`. Args holds partials, out and first. (A record depends on its own request only: the split does not enter it.)
template <class Args, class Pre = RingNoStep, class Post = RingNoStep>
ellc_status pair_run(ellc_ctx* c, PairScratch& s, int B, int per_launch, void (*pass)(Args), void (*finish)(Args), Args a, void* out,
                     float* launches_ms, Pre pre = Pre(), Post enqueued = Post()) {
  a.partials = (decltype(a.partials))s.partials_d;
  a.out = (decltype(a.out))s.out_dev_alias;
  LaunchTimer t(c, launches_ms);
  ELLC_TRY(t.begin());
  for (int first = 0; first < B; first += per_launch) {
    const int n = std::min(per_launch, B - first);
    a.first = first;
    ELLC_TRY(pre(n));
    hipLaunchKernelGGL(pass, dim3(a.v.tiles, n), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(finish, dim3(n), dim3(64), 0, c->stream, a);
  }
  ELLC_HIP(c, hipGetLastError());
  ELLC_TRY(t.end());
  ELLC_TRY(enqueued(B));
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  std::memcpy(out, s.out_h, (size_t)B * sizeof(*a.out));
  return t.read();
}

// ---- the calls of one keyframe slot K against B views, continued: staging, planes, scratch and run of a call. A new call of K against
// views supplies a staged view type, an Args struct, a pixel kernel, a record and its own refusals.

// The views on their way to the device, View being the call's staged type (RefineView or derived from it): image, transform and light
// of every view, then what the call adds through more(view, b). (The stream has been waited for since the staging was last read.)
struct RingViewAsIs {
  template <class View>
  void operator()(View&, int) const {}
};

template <class View, class More = RingViewAsIs>
ellc_status ring_views_stage(ellc_ctx* c, PairScratch& s, int level, int B, int views_are_kf, const int* view_slots, const float* T12, const float* light,
                             More more = More()) {
  View* vw = (View*)s.stage_h;
  for (int b = 0; b < B; b++) {
    vw[b] = View{};
    vw[b].img = ring_view_image(c, level, views_are_kf, view_slots[b]);
    std::memcpy(vw[b].T, T12 + (size_t)12 * b, 12 * sizeof(float));
    vw[b].gain = light ? light[2 * b] : 1.0f;
    vw[b].offset = light ? light[2 * b + 1] : 0.0f;
    more(vw[b], b);
  }
  ELLC_HIP(c, hipMemcpyAsync(s.stage_d, s.stage_h, (size_t)B * sizeof(View), hipMemcpyHostToDevice, c->stream));
  return ELLC_OK;
}

// a grow-only buffer of `cap` pixels carved into planes: the plane that starts `bytes_before` bytes a pixel into it
struct PlaneCarve {
  void* base;
  size_t cap;
  template <class T>
  T* at(size_t bytes_before) const { return (T*)((char*)base + bytes_before * cap); }
};

// a device plane to the host; a NULL host pointer: not asked for
struct RingFetch {
  void* host;
  const void* dev;
  size_t bytes;
};

template <int N>
ellc_status ring_fetch(ellc_ctx* c, const RingFetch (&f)[N]) {
  for (int k = 0; k < N; k++)
    if (f[k].host) ELLC_HIP(c, hipMemcpyAsync(f[k].host, f[k].dev, f[k].bytes, hipMemcpyDeviceToHost, c->stream));
  return ELLC_OK;
}

// The scratch of a one-record call over the n pixels of a level, and what its Args hold of it: the staged views, a partial record
// per 256-pixel block, the pinned record.
template <class Args>
ellc_status ring_views_scratch(ellc_ctx* c, PairScratch& s, int max_B, size_t n, int kf_slot, int B, Args& a) {
  a.blocks = (int)((n + 255) / 256);
  ELLC_TRY(pair_reserve(c, s, max_B, sizeof(*a.views), sizeof(*a.out), (size_t)a.blocks));
  a.views = (decltype(a.views))s.stage_d;
  a.partials = (decltype(a.partials))s.partials_d;
  a.out = (decltype(a.out))s.out_dev_alias;
  a.kf_slot = kf_slot;
  a.B = B;
  a.first = 0;
  return ELLC_OK;
}

// The run of a one-record call: the pixel kernel over a.blocks blocks and the finish kernel inside the timing window (launches_ms: the
// diagnostic hook only), the frame slots' reader marks, the planes asked for, a.depth and a.var into slot dst (>= 0; *dense is the
// record's count of pixels with a depth > 0), the wait. The pinned record may be read when this returns.
template <class Args, int N>
ellc_status ring_views_run(ellc_ctx* c, const Args& a, void (*pixels)(Args), void (*finish)(Args), const int* view_slots, int views_are_kf,
                           const RingFetch (&fetch)[N], int dst, size_t n, const int32_t* dense, float* launches_ms) {
  LaunchTimer t(c, launches_ms);
  ELLC_TRY(t.begin());
  hipLaunchKernelGGL(pixels, dim3(a.blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(finish, dim3(1), dim3(64), 0, c->stream, a);
  ELLC_HIP(c, hipGetLastError());
  ELLC_TRY(t.end());
  ELLC_TRY(ring_views_mark_use(c, a.B, view_slots, views_are_kf));
  ELLC_TRY(ring_fetch(c, fetch));
  if (dst >= 0) ELLC_TRY(ring_views_store_dst(c, dst, a.depth, a.var, n, dense));
  ELLC_HIP(c, hipStreamSynchronize(c->stream));
  return t.read();
}

}  // namespace
