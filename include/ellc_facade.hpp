// ellc_facade.hpp — the reference's object API (frame / PixelWisePyramid / depthMap / GetImagePoseEstimate)
// re-expressed over the C ABI of libellc_hip.so, so a main.cpp-shaped driver keeps its structure.
// Header-only, host C++11; every numeric operation is a call into include/ellc_abi.h (no CPU fallback).
//
// Reference members mirrored (file:line under the reference's src/):
//   frame                     Frame.h:35-397, Frame.cpp:34-124 (constructor after decode/undistort/resize), :503-562, :678-695
//   PixelWisePyramid          PixelWisePyramid.h:89-101, PixelWisePyramid.cpp:14-51, :416-491, :500-552, :917-974
//   depthMap                  DepthPropagation.h:82-132, DepthPropagation.cpp:44-66, :83-184, :1254-1315, :1627-1635,
//                             :1749-1802, :1804-1830, :1932-1958
//   GetImagePoseEstimate      ImageFunc.h:31, ImageFunc.cpp:49-315
// Differences that are deliberate: image decode / undistort / VideoCapture stay with the caller (frame takes
// the grey W x H image); the process-wide globals of the reference (numberOfInstances, util::K*, GLOABL_DEPTH_SCALE)
// live in ellc::Runtime; failures throw std::runtime_error carrying ellc_last_error() instead of being ignored.
#ifndef ELLC_FACADE_HPP
#define ELLC_FACADE_HPP

#include "ellc_abi.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace ellc {

// Text checkpoint format of the reference (Frame.cpp:697-871): default ostream formatting of float (6 significant digits,
// %g style), one blank after every value; a Mat ends each row with '\n', an array is a single line. Host-only helpers.
namespace text {
inline void writeMat(const std::string& path, const float* data, int width, int height) {
  std::ofstream f(path.c_str());
  if (!f) throw std::runtime_error("saveMatAsText: cannot open " + path);
  for (int y = 0; y < height; y++) {
    for (int x = 0; x < width; x++) f << data[(size_t)y * width + x] << " ";
    f << "\n";
  }
}
inline void writeArray(const std::string& path, const float* data, size_t n) {
  std::ofstream f(path.c_str());
  if (!f) throw std::runtime_error("saveArrayAsText: cannot open " + path);
  for (size_t i = 0; i < n; i++) f << data[i] << " ";
}
// whitespace-separated values, rows and single lines alike (makeMatFromText / makeArrayFromText, Frame.cpp:738-810): the
// same `stream >> element` per entry, so entries a short file does not hold are left as they were
inline void readValues(const std::string& path, float* data, size_t n) {
  std::ifstream f(path.c_str());
  if (!f) throw std::runtime_error("makeMatFromText: cannot open " + path);
  for (size_t i = 0; i < n; i++) f >> data[i];
}
}  // namespace text

// Owner of the context and of the slot bookkeeping (keyframe slots: active + incoming; frame slots: ring).
class Runtime {
 public:
  ellc_config cfg;
  ellc_ctx* ctx = nullptr;
  int numberOfInstances = 0;      // Frame.cpp:24
  bool FLAG_DO_LOOP_CLOSURE = false;           // "LC" mode: save / average the tracking weights (ExternVariable.h:203,211)
  int BATCH_START_ID = 1;
  // text checkpoints of the active keyframe for the alternate Gauss-Newton <-> rotation-averaging loop (ToggleFlags.h:108-203)
  bool FLAG_ALTERNATE_GN_RA = false;           // file ids become frameId + BATCH_START_ID - 1 (Frame.cpp:700-704)
  bool FLAG_SAVE_MATS = false;                 // write <id>_{Depth,Depth_pyr0,DepthVarArr_pyr0}.txt at keyframe switches (ImageFunc.cpp:73-87)
  bool FLAG_REPLICATE_POSE_ESTIMATION = false; // read them back instead (ImageFunc.cpp:58-66)
  int KEYFRAME_PROPAGATE_INTERVAL = 8;         // ExternVariable.h:39
  std::string SAVED_MATS_PATH = ".";
  explicit Runtime(const ellc_config& c) : cfg(c) {
    if (cfg.max_frames < 3) cfg.max_frames = 3;
    if (cfg.max_keyframes < 2) cfg.max_keyframes = 2;
    if (cfg.max_batch < 1) cfg.max_batch = 1;
    check(ellc_ctx_create(&cfg, &ctx), "ellc_ctx_create");
  }
  ~Runtime() { if (ctx) ellc_ctx_destroy(ctx); }
  Runtime(const Runtime&) = delete;
  Runtime& operator=(const Runtime&) = delete;
  void check(int st, const char* what) const {
    if (st != ELLC_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(st) + "): " + (ctx ? ellc_last_error(ctx) : "no context"));
  }
  // Frame.cpp:45-75 after the decode: BGR -> grey -> undistort -> 1/4 resize as a device pre-pass. fx..cy are the full-size
  // intrinsics of cam_K (util::ORIG_FX*INTRINSIC_FACTOR ...), dist5 = util::distortion_parameters.
  bool ingest_configured = false;
  void configureIngest(int orig_w, int orig_h, float fx, float fy, float cx, float cy, const float* dist5, bool FLAG_DO_UNDISTORTION = true) {
    check(ellc_ingest_configure(ctx, orig_w, orig_h, fx, fy, cx, cy, dist5, FLAG_DO_UNDISTORTION ? 1 : 0, nullptr), "ellc_ingest_configure");
    ingest_configured = true;
  }
  // Multi-GPU (one process per GPU, every process tracks the whole sequence): the loop-closure batch is sharded over the
  // ranks and its results gathered once per batch (ellc_gather_results). comm == nullptr: single process.
  ellc_comm* comm = nullptr;
  int world = 1, rank = 0;
  // The loop-closure context's launch grids are fixed per batch — for the smallest of {4, 8, 16, 43} candidates that holds the WHOLE
  // batch (ellc_ctx_set_grid_batch before every batch, the same value on every rank) — so that the files a run writes do not depend
  // on how many ranks shared the batch, including one (ellc_main --world 2 equals the single process byte for byte), while the usual
  // batch of a handful of candidates no longer runs on grids sized for the ring's 43 (r03 advisor finding; r04 fixed them at 43).
  // A single process that does not need that may clear this before it constructs globalOptimize: grids then follow each call's B.
  bool lc_fixed_grids = true;
  int frame_ring = 3;             // tracking uses frame slots [0, frame_ring): current, t-1 and one spare
  int next_frame_slot() { int s = frame_cursor_; frame_cursor_ = (frame_cursor_ + 1) % frame_ring; return s; }
  int other_keyframe_slot(int current) const { return (current + 1) % 2; }   // keyframe slots 0 / 1: active and incoming
 private:
  int frame_cursor_ = 0;
};

class frame {
 public:
  Runtime* rt;
  int frameId;
  int parentKeyframeId = 0;
  bool isKeyframe = false;
  int width, height;
  int slot;                 // frame slot holding the u8 pyramid on the device
  int kf_slot = -1;         // keyframe slot once this frame has become a keyframe
  float poseWrtOrigin[6];   // w.r.t. the keyframe
  float poseWrtWorld[6];    // w.r.t. the first frame
  float rescaleFactor = 1.0f;
  int numWeightsAdded[ELLC_MAX_LEVELS];

  // Frame.cpp:34-124 from "width=image.cols" on: ids, zero poses, pyramids (constructImagePyramids on device)
  // `pixels` is the grey W x H image, or — with from_bgr — the decoded full-size BGR frame (Runtime::configureIngest first)
  frame(Runtime& r, const uint8_t* pixels, bool from_bgr = false) : rt(&r) {
    frameId = ++r.numberOfInstances;
    width = r.cfg.width;
    height = r.cfg.height;
    for (int i = 0; i < 6; i++) poseWrtOrigin[i] = poseWrtWorld[i] = 0.0f;
    for (int i = 0; i < ELLC_MAX_LEVELS; i++) numWeightsAdded[i] = 0;
    slot = r.next_frame_slot();
    if (from_bgr) r.check(ellc_frame_ingest_bgr(r.ctx, slot, pixels, nullptr, nullptr), "ellc_frame_ingest_bgr");
    else r.check(ellc_frame_upload(r.ctx, slot, pixels), "ellc_frame_upload");
  }
  void concatenateRelativePose(const float* src_1wrt2, const float* src_2wrt3, float* dest_1wrt3) const {
    ellc_concatenate_relative_pose(src_1wrt2, src_2wrt3, dest_1wrt3);
  }
  void concatenateOriginPose(const float* src_1wrt0, const float* src_2wrt0, float* dest_1wrt2) const {
    ellc_concatenate_origin_pose(src_1wrt0, src_2wrt0, dest_1wrt2);
  }
  void calculatePoseWrtOrigin(frame* prev_image, const float* poseChange) { concatenateRelativePose(poseChange, prev_image->poseWrtOrigin, poseWrtOrigin); }
  void calculatePoseWrtWorld(frame* prev_image, const float* poseChange) { concatenateRelativePose(poseChange, prev_image->poseWrtWorld, poseWrtWorld); }
  // ---- text checkpoints (Frame.cpp:697-871). `depth` and `depth_pyramid[0]` are one plane here (level 0 of the keyframe
  // slot); the variance array is depthMap::depthvararrpyr0 (DepthPropagation.cpp:1637-1746), the slot's level-0 variance.
  // Format: default ostream formatting of float (6 significant digits), one blank after every value; a Mat ends each
  // row with '\n', an array is a single line.
  std::string matFileName(const std::string& name, const std::string& dir) const {
    const int id = rt->FLAG_ALTERNATE_GN_RA ? (frameId + rt->BATCH_START_ID - 1) : frameId;
    std::stringstream ss;
    ss << dir << "/" << id << "_" << name << ".txt";
    return ss.str();
  }
  void level0(std::vector<float>& depth, std::vector<float>& var) const {
    if (kf_slot < 0) throw std::runtime_error("text checkpoint: frame is not a keyframe");
    depth.assign((size_t)width * height, 0.f);
    var.assign((size_t)width * height, 0.f);
    rt->check(ellc_keyframe_get_depth_level(rt->ctx, kf_slot, 0, depth.data(), var.data()), "ellc_keyframe_get_depth_level");
  }
  void saveMatAsText(const std::string& name, const std::string& save_mat_path) const {   // name: "Depth" | "Depth_pyr0"
    std::vector<float> d, v;
    level0(d, v);
    text::writeMat(matFileName(name, save_mat_path), d.data(), width, height);
  }
  void saveArrayAsText(const std::string& name, const std::string& save_arr_path, int pyr_level) const {   // "DepthVarArr_pyr0"
    if (pyr_level != 0) throw std::runtime_error("saveArrayAsText: only level 0 is checkpointed (ImageFunc.cpp:84)");
    std::vector<float> d, v;
    level0(d, v);
    text::writeArray(matFileName(name, save_arr_path), v.data(), v.size());
  }
  void makeMatFromText(const std::string& name, const std::string& read_txt_path) {
    std::vector<float> d, v;
    level0(d, v);
    text::readValues(matFileName(name, read_txt_path), d.data(), d.size());
    rt->check(ellc_keyframe_set_depth_level(rt->ctx, kf_slot, 0, d.data(), v.data()), "ellc_keyframe_set_depth_level");
  }
  void makeArrayFromText(const std::string& name, const std::string& read_txt_path, int pyr_level) {
    if (pyr_level != 0) throw std::runtime_error("makeArrayFromText: only level 0 is checkpointed (ImageFunc.cpp:65)");
    std::vector<float> d, v;
    level0(d, v);
    text::readValues(matFileName(name, read_txt_path), v.data(), v.size());
    rt->check(ellc_keyframe_set_depth_level(rt->ctx, kf_slot, 0, d.data(), v.data()), "ellc_keyframe_set_depth_level");
  }
  void finaliseWeights() {   // Frame.cpp:678-695
    if (kf_slot < 0) throw std::runtime_error("finaliseWeights: frame is not a keyframe");
    rt->check(ellc_keyframe_finalise_weights(rt->ctx, kf_slot), "ellc_keyframe_finalise_weights");
  }
};

class depthMap {
 public:
  Runtime* rt;
  frame* keyFrame = nullptr;
  frame* currentFrame = nullptr;
  float depthScale = 1.0f;
  explicit depthMap(Runtime& r) : rt(&r) {}

  // DepthPropagation.cpp:44-66
  void formDepthMap(frame* image_frame) {
    currentFrame = image_frame;
    currentFrame->isKeyframe = false;
    if (image_frame->frameId == 1) {
      keyFrame = image_frame;
      keyFrame->isKeyframe = true;
      keyFrame->rescaleFactor = 1.0f;
      keyFrame->kf_slot = 0;
      rt->check(ellc_keyframe_from_frame(rt->ctx, 0, image_frame->slot), "ellc_keyframe_from_frame");
      rt->check(ellc_depth_set_keyframe(rt->ctx, 0), "ellc_depth_set_keyframe");
      initializeRandomly();
    }
    currentFrame->parentKeyframeId = keyFrame->frameId;
    currentFrame->rescaleFactor = keyFrame->rescaleFactor;
  }
  // DepthPropagation.cpp:83-184 (random branch): glibc rand(), unseeded, raster order over the interior
  void initializeRandomly() {
    const int W = rt->cfg.width, H = rt->cfg.height;
    const size_t n = (size_t)W * H;
    std::vector<float> mg(n), id(n, 0.f), ids(n, 0.f), var(n, 0.f), vars(n, 0.f);
    std::vector<int32_t> val(n, 0), bl(n, 0);
    std::vector<uint8_t> ok(n, 0);
    rt->check(ellc_get_max_gradient(rt->ctx, 1, keyFrame->kf_slot, mg.data(), nullptr), "ellc_get_max_gradient");
    // The reference never seeds rand(), i.e. it consumes glibc's default sequence (seed 1) from its start. The GPU
    // runtime may draw from rand() while it initialises, so the default sequence is re-established explicitly.
    srand(1);
    for (int y = 1; y < H - 1; y++)
      for (int x = 1; x < W - 1; x++) {
        const size_t i = (size_t)x + (size_t)W * y;
        if (mg[i] > 1.0 * 1.0f) {   // MIN_ABS_GRAD_CREATE
          id[i] = 0.5f + 1.0f * ((rand() % 100001) / 100000.0f);
          var[i] = 0.125f;          // VAR_RANDOM_INIT_INITIAL
          vars[i] = 0.125f;
          ids[i] = id[i];
          val[i] = 20;
          ok[i] = 1;
        }
      }
    ellc_hypotheses h = {id.data(), ids.data(), var.data(), vars.data(), val.data(), bl.data(), ok.data()};
    rt->check(ellc_depth_set_state(rt->ctx, &h), "ellc_depth_set_state");
  }
  void updateDepthImage(bool = false) { rt->check(ellc_depth_update_depth_image(rt->ctx), "ellc_depth_update_depth_image"); }
  void doRegularization(bool removeOcclusions = false) {   // :1627-1635
    rt->check(ellc_depth_do_regularization(rt->ctx, removeOcclusions ? 1 : 0), "ellc_depth_do_regularization");   // fill + regularise: one launch
  }
  void finaliseKeyframe() { doRegularization(); updateDepthImage(); }   // :1749-1755
  void updateKeyFrame() {}   // :1796-1802: the Sim3-scaled pose it computes is overwritten before use (:1935)
  void observeDepthRowParallel() {   // :1932-1958
    rt->check(ellc_depth_observe(rt->ctx, currentFrame->slot, currentFrame->poseWrtOrigin), "ellc_depth_observe");
  }
  void createKeyFrame(frame* new_keyframe) {   // :1758-1794
    const int ns = rt->other_keyframe_slot(keyFrame->kf_slot);
    rt->check(ellc_keyframe_from_frame(rt->ctx, ns, new_keyframe->slot), "ellc_keyframe_from_frame");
    float f = 1.0f;
    rt->check(ellc_depth_create_keyframe(rt->ctx, ns, new_keyframe->poseWrtOrigin, &f), "ellc_depth_create_keyframe");
    new_keyframe->kf_slot = ns;
    keyFrame = new_keyframe;
    keyFrame->isKeyframe = true;
    keyFrame->rescaleFactor = f;
    depthScale = f;
    for (int i = 0; i < 6; i++) keyFrame->poseWrtOrigin[i] = 0.0f;
  }
  float calculate_no_of_Seeds(bool = true) {   // :1804-1830
    float p = 0;
    rt->check(ellc_depth_seeds(rt->ctx, &p), "ellc_depth_seeds");
    return p;
  }
};

// One pyramid level of the Gauss-Newton loop, one iteration per call (PixelWisePyramid.cpp:416-491, :917-974).
// The batched fast path is GetImagePoseEstimate below; this class exists for callers that drive single steps.
class PixelWisePyramid {
 public:
  Runtime* rt;
  frame* prev_frame;
  frame* current_frame;
  depthMap* currentDepthMap;
  float* pose;            // caller-owned 6-vector, updated in place (ImageFunc.cpp:183)
  int pyrlevel;
  float weightedPose = 0;
  float hessian[36], sd_param[6], deltapose[6];
  float prevPose[6];
  PixelWisePyramid(frame* prev, frame* cur, float* pose_, depthMap* dm, int level)
      : rt(prev->rt), prev_frame(prev), current_frame(cur), currentDepthMap(dm), pose(pose_), pyrlevel(level) {}
  void putPreviousPose(frame* tminus1) { tminus1->concatenateOriginPose(tminus1->poseWrtWorld, prev_frame->poseWrtWorld, prevPose); }
  void calculatePixelWiseParallel() { step(ELLC_MODE_FCA, 0); }
  void calculatePixelWiseParallelInvCompositional(int iter) { step(ELLC_MODE_ICA, iter); }
 private:
  void step(int mode, int iter) {
    float np[6];
    rt->check(ellc_gn_iterate(rt->ctx, prev_frame->kf_slot, current_frame->slot, pyrlevel, mode, iter, pose, hessian, sd_param, deltapose, np,
                              &weightedPose, nullptr), "ellc_gn_iterate");
    std::memcpy(pose, np, sizeof(np));
  }
};

// ImageFunc.cpp:49-315. The level / iteration loops run on the device (ellc_align); weights of the last executed
// iteration of every level are saved into the keyframe when the runtime is in LC mode and the call does not come
// from loop closure (ImageFunc.cpp:280-288).
namespace detail {
// ImageFunc.cpp:58-131: the text checkpoints at a keyframe switch and the initial relative pose of the alignment
inline void initial_pose_estimate(frame* prev_frame, frame* current_frame, frame* tminus1_prev_frame, float* initial_pose_estimate, bool fromLoopClosure, float* pose) {
  Runtime* rt = prev_frame->rt;
  if (prev_frame->kf_slot < 0) throw std::runtime_error("GetImagePoseEstimate: prev_frame is not a keyframe");
  const bool kf_switch = !fromLoopClosure && (current_frame->frameId % rt->KEYFRAME_PROPAGATE_INTERVAL == 0);
  if (rt->FLAG_REPLICATE_POSE_ESTIMATION && kf_switch) {   // :58-66 revive the keyframe's level-0 depth / variance
    prev_frame->makeMatFromText("Depth", rt->SAVED_MATS_PATH);
    prev_frame->makeMatFromText("Depth_pyr0", rt->SAVED_MATS_PATH);
    prev_frame->makeArrayFromText("DepthVarArr_pyr0", rt->SAVED_MATS_PATH, 0);
  }
  if (rt->FLAG_SAVE_MATS && kf_switch && (rt->FLAG_ALTERNATE_GN_RA || current_frame->frameId < 50)) {   // :73-87
    prev_frame->saveMatAsText("Depth", rt->SAVED_MATS_PATH);
    prev_frame->saveMatAsText("Depth_pyr0", rt->SAVED_MATS_PATH);
    prev_frame->saveArrayAsText("DepthVarArr_pyr0", rt->SAVED_MATS_PATH, 0);
  }
  prev_frame->concatenateOriginPose(tminus1_prev_frame->poseWrtWorld, prev_frame->poseWrtWorld, pose);   // :106
  if (initial_pose_estimate) {
    // FLAG_INITIALIZE_NONZERO_POSE (:109-131): the given world pose (so3poses7.txt) is converted to a pose w.r.t. the
    // keyframe and supplies the rotation; the translation stays the one predicted from frame t-1
    float from_file[6];
    prev_frame->concatenateOriginPose(initial_pose_estimate, prev_frame->poseWrtWorld, from_file);
    pose[0] = from_file[0];
    pose[1] = from_file[1];
    pose[2] = from_file[2];
  }
}
}  // namespace detail

inline std::vector<float> GetImagePoseEstimate(frame* prev_frame, frame* current_frame, int /*frame_num*/, depthMap* /*currDepthMap*/,
                                               frame* tminus1_prev_frame, float* initial_pose_estimate, bool fromLoopClosure = false,
                                               bool /*homo*/ = false) {
  Runtime* rt = prev_frame->rt;
  float pose[6];
  detail::initial_pose_estimate(prev_frame, current_frame, tminus1_prev_frame, initial_pose_estimate, fromLoopClosure, pose);
  const int save = (rt->FLAG_DO_LOOP_CLOSURE && !fromLoopClosure) ? 1 : 0;
  float out[6];
  rt->check(ellc_align(rt->ctx, 1, &prev_frame->kf_slot, &current_frame->slot, pose, fromLoopClosure ? ELLC_MODE_ICA : ELLC_MODE_FCA, save, out,
                       nullptr, nullptr), "ellc_align");
  if (save) for (int l = 0; l < rt->cfg.levels; l++) prev_frame->numWeightsAdded[l]++;
  current_frame->calculatePoseWrtOrigin(prev_frame, out);   // :305
  current_frame->calculatePoseWrtWorld(prev_frame, out);    // :306
  return std::vector<float>(out, out + 6);
}

// A tracked frame that does not switch the keyframe — main.cpp:330 (GetImagePoseEstimate), :368 (calculate_no_of_Seeds) and
// :499-502 (updateKeyFrame, observeDepthRowParallel, doRegularization, updateDepthImage) — as ONE device sequence
// (ellc_track_frame): the depth stages start behind the alignment's last kernel without waiting for the host. prev_frame must be
// the depth map's keyframe. *seeds_num: the seeds figure of the map before this frame's observation, as main.cpp writes it.
inline std::vector<float> TrackFrameAndObserve(frame* prev_frame, frame* current_frame, depthMap* currDepthMap, frame* tminus1_prev_frame,
                                               float* initial_pose_estimate, float* seeds_num) {
  Runtime* rt = prev_frame->rt;
  if (currDepthMap->keyFrame != prev_frame) throw std::runtime_error("TrackFrameAndObserve: prev_frame is not the depth map's keyframe");
  float pose[6];
  detail::initial_pose_estimate(prev_frame, current_frame, tminus1_prev_frame, initial_pose_estimate, false, pose);
  const int save = rt->FLAG_DO_LOOP_CLOSURE ? 1 : 0;
  float out[6], seeds = 0;
  rt->check(ellc_track_frame(rt->ctx, current_frame->slot, pose, save, out, nullptr, nullptr, &seeds), "ellc_track_frame");
  if (save) for (int l = 0; l < rt->cfg.levels; l++) prev_frame->numWeightsAdded[l]++;
  current_frame->calculatePoseWrtOrigin(prev_frame, out);   // :305
  current_frame->calculatePoseWrtWorld(prev_frame, out);    // :306
  if (seeds_num) *seeds_num = seeds;
  currDepthMap->formDepthMap(current_frame);   // main.cpp:391 (bookkeeping only beyond the first frame)
  return std::vector<float>(out, out + 6);
}

// Local loop-closure detection (GlobalOptimize.h:39-97, GlobalOptimize.cpp). Keeps a ring of finished keyframes
// (image, depth pyramid, averaged tracking weights) resident on the device, selects candidates for a test keyframe by
// intensity-histogram KL divergence, frame gap and view angle (findMatch :274-416), and aligns the test keyframe against
// ALL selected candidates with ONE batched constant-weight alignment (the reference runs them one by one, :566).
// The candidate sequence does not depend on the alignment results (the reference restores the test frame's poses after
// every match, :591-606), so collecting first and aligning once is equivalent.
//   As in the reference with FLAG_DO_PARALLEL_SHORT_LOOP_CLOSURE (on in LC mode, ToggleFlags.h:53-59), the matching of a pushed
// keyframe runs on a thread of its own beside tracking (t_group.create_thread, :241) and is joined at the next pushToArray
// (:161) — and when the object goes away. The ring lives in a Runtime of its own (`ring`: a second context with its own
// streams, so its batch overlaps the tracking context's work on the device); pushToArray deep-copies the finished keyframe
// into it (ellc_copy_slot_across = new frame(*currentframe) / new depthMap(*currentDepthMap), :185-186) and the thread only
// ever touches the ring context. The ring context fixes its launch grids per batch (ellc_ctx_set_grid_batch; Runtime::lc_fixed_grids):
// a rank's shard of a batch has the bits of the whole batch.
// What globalOptimize::renderLocalMap returns: the five planes of ellc_keyframe_render_depth (dense cols x rows of the level), the number
// of targets with a winner, and the requests they were rendered from.
struct RenderedView {
  int cols = 0, rows = 0, n_valid = 0;
  std::vector<int> ids, slots;    // ring array ids / ring keyframe slots of the requests, in request order (source >> 24 indexes them)
  std::vector<float> T;           // [requests][12]: keyframe camera -> view camera, as passed to the library
  std::vector<float> depth, var;
  std::vector<int32_t> source, agree;
  std::vector<uint8_t> intensity;
};
// What globalOptimize::fuseLocalMap returns: the view of ellc_keyframe_fuse_depth — a RenderedView whose depth and var hold the merged
// hypothesis where candidates agreed with the winner — with the merged plane, the number of targets that fused and the bound it was made with.
struct FusedView : RenderedView {
  int n_fused = 0, max_merge = 0;
  std::vector<int32_t> merged;    // hypotheses fused into the target, the winner included (0: no winner)
};

class globalOptimize {
 public:
  static const int MAX_LOOP_ARRAY_LENGTH = 20;                                   // ExternVariable.h:161
  static const int MAX_LOOP_ARRAY_LENGTH_SCALE_AVG = MAX_LOOP_ARRAY_LENGTH * 2 + 3;   // :162
  struct loopFrame {   // LoopFrame.h:24-39
    float image_histogram[256];
    int frameId = -1;
    float poseWrtWorld[6];
    float poseWrtOrigin[6];
    bool isValid = false;
    float rescaleFactor = 1.0f;   // this_frame->rescaleFactor
    float seeds = 0.0f;           // this_currentDepthMap->calculate_no_of_Seeds()
    int kf_slot = -1;             // ring-context slot holding this_frame / this_currentDepthMap
    bool isStray = false;         // pushed by findConnection: an image without a depth map (LoopFrame.h)
  };
  Runtime* rt;            // the tracking runtime (source of the finished keyframes; its comm / world / rank shard the batch)
  Runtime ring;           // the loop-closure context: keyframe slots [0, 43) = the ring, frame slot 0 = the test keyframe
  bool FLAG_DO_PARALLEL_SHORT_LOOP_CLOSURE = true;
  loopFrame loopFrameArray[MAX_LOOP_ARRAY_LENGTH_SCALE_AVG];
  loopFrame currentLoopFrame;
  std::ofstream match_file;
  bool isloopClosureDetected = false;
  bool connectionLost = false;
  int loopClosureArrayId = -1, lastTestedLoopClosureArrayId = -1, firstTestedLoopClosureArrayId = -1;
  int currentArrayId = 0, nextArrayId = 1;
  int match_window_beg = 0, match_window_end = MAX_LOOP_ARRAY_LENGTH - 1;
  float matchValue = 0, rms_error = 0, relative_view_angle = 0;
  // How well each candidate of a loop-closure batch fits at the pose the batch returned (ellc_align_quality_at, level 0): the match
  // file carries the histogram distance but no photometric figure (GlobalOptimize.cpp:566-582 accepts every candidate). Off by
  // default: nothing changes. On: lastMatchQuality holds one record per line the batch wrote to the match file, in that order, and
  // match_quality_file (when open) gets "frameId kfId n_depth n_used rms wrms" per line. What to do with the figures is the caller's.
  bool collectMatchQuality = false;
  std::vector<ellc_align_quality> lastMatchQuality;
  std::ofstream match_quality_file;
  // Whether each candidate's MAP agrees with the pushed keyframe's at that pose (ellc_keyframe_depth_consistency, level 0, candidate's
  // slot -> testFrame's slot, T = the top three rows of exp(pose)): every keyframe's map is rescaled to mean inverse depth one
  // (makeInvDepthOne), so the first call's sum_w_st / sum_w_ss is the relative scale of the two maps, and a second call with T divided
  // by it compares them at one scale. Off by default: nothing changes. On: lastMatchGeometry holds the second call's record and the
  // scale (1 where sum_w_ss is 0 or the ratio is not a positive finite number) per line the batch wrote to the match file, in that
  // order, and match_geometry_file (when open) gets "frameId kfId n_kept n_in_view n_overlap n_agree n_in_front n_behind scale
  // mean_chi2 mean_abs_di" per line (mean_chi2 = sum_chi2 / n_weighted, mean_abs_di = sum_abs_di / n_overlap; 0 for an empty
  // denominator). The ring is replicated, and a record does not depend on the batch it is computed in: every rank of a sharded run
  // computes the whole batch. What to do with the figures is the caller's.
  struct MatchGeometry {
    ellc_depth_consistency rec;
    double scale;
  };
  bool collectMatchGeometry = false;
  std::vector<MatchGeometry> lastMatchGeometry;
  std::ofstream match_geometry_file;
  // The similarity transform between each candidate and the pushed keyframe (ellc_keyframe_sim3_align): the batch's alignment has six
  // degrees of freedom and every keyframe's map a scale of its own, so each candidate is refined over seven - from the top three rows
  // of exp(pose) divided by ellc_keyframe_depth_consistency's scale (level 0, the filter of ellc_main --map, agree_k2 1; 1 where that
  // scale is not a positive finite number), coarse to fine from level 1 (where the pyramid has one) to level 0, at most 10 updates a
  // level, eps 1e-4, the default ellc_sim3_params and the same filter. Off by default: nothing changes. On: lastMatchSim3 holds one
  // entry per line the batch wrote to the match file, in that order - T takes the candidate's camera into the pushed keyframe's, scale
  // is the cube root of the determinant of its 3x3 block, rec the record at T, iters the updates over all levels - and match_sim3_file
  // (when open) gets "frameId kfId scale tx ty tz wx wy wz n_photo n_depth chi2_photo chi2_depth iters" per line, (wx, wy, wz) the
  // rotation vector of the 3x3 block over the scale. Every rank of a sharded run computes the whole batch, as for the geometry.
  // matchAffineLight (off by default: nothing changes; it needs refineMatchSim3): the refinement fits an affine brightness between the
  // pair before every step (ellc_keyframe_sim3_align_lit from the light (1, 0), the default ellc_light_params): the two ends of a loop
  // closure lie far apart in time and cameras adjust their exposure. gain and offset are the light the loop ended with (1 and 0
  // without matchAffineLight), and each line of match_sim3_file ends in " gain offset".
  struct MatchSim3 {
    ellc_sim3_normal rec;
    float T[12];
    double scale;
    int iters;
    float gain, offset;
  };
  bool refineMatchSim3 = false;
  bool matchAffineLight = false;
  std::vector<MatchSim3> lastMatchSim3;
  std::ofstream match_sim3_file;
  // The structure step behind the motion step (ellc_keyframe_refine_depth; off by default: nothing changes; it needs refineMatchSim3,
  // with or without matchAffineLight): the pushed keyframe's ring map is refined against the images of its candidates - level 0, K the
  // pushed keyframe's ring slot, the views the candidates' ring slots (the first ELLC_REFINE_MAX_VIEWS of them), each at the INVERSE of
  // its refined transform and light (ellc_sim3_invert: lastMatchSim3 holds candidate -> keyframe), the filter of ellc_main --map, the
  // default ellc_refine_params with min_views = min(2, views), and the keyframe's own ring slot as the destination. lastRefineStats
  // keeps the record and lastRefineViews the number of views of the push that ran last (0 and zeros: no candidates), and
  // refine_matches_file (when open) gets "frameId views n_kept n_taking_part n_refined n_too_few_views n_no_information n_bad_step
  // n_views_changed n_cost_rose sum_views sum_cost_before sum_cost_after" per push that had candidates. Every rank of a sharded run
  // computes the whole call, as for the Sim(3) refinement. The ring copy alone is refined: the tracking context's map is not touched.
  bool refineMatchDepth = false;
  ellc_refine_stats lastRefineStats = ellc_refine_stats();
  int lastRefineViews = 0;
  std::ofstream refine_matches_file;
  // The structure-CREATION step in front of that refinement (ellc_keyframe_sweep_depth; off by default: nothing changes; it needs
  // refineMatchSim3, with or without matchAffineLight and refineMatchDepth): the pixels of the pushed keyframe's ring map that hold no
  // hypothesis get one from a depth sweep against the same views at the same inverted transforms and lights - level 0, the default
  // ellc_sweep_params with min_views = min(2, views), the keyframe's own ring slot as the destination - BEFORE refineMatchDepth runs, so
  // that the refinement polishes what the sweep created. lastSweepStats / lastSweepViews keep the record (zeros: no candidates) and
  // sweep_matches_file (when open) gets "frameId views n_ok n_swept n_created n_no_valid_sample n_at_range_end n_cost_too_high
  // n_not_distinct n_flat sum_views sum_cost" per push that had candidates. The ring copy alone is touched.
  bool sweepMatchDepth = false;
  ellc_sweep_stats lastSweepStats = ellc_sweep_stats();
  int lastSweepViews = 0;
  std::ofstream sweep_matches_file;
  // The consistency filter behind that refinement (ellc_keyframe_cull_depth; off by default: nothing changes; it needs refineMatchSim3,
  // with or without matchAffineLight, sweepMatchDepth and refineMatchDepth): the hypotheses of the pushed keyframe's ring map that the
  // same views at the same inverted transforms and lights contradict are removed - level 0, the no-op filter {0, 0, 1, 1}, the default
  // ellc_cull_params with the four counts lowered to min(default, views), the keyframe's own ring slot as the destination - AFTER
  // refineMatchDepth ran, where both are asked for. lastCullStats / lastCullViews keep the record (zeros: no candidates) and
  // cull_matches_file (when open) gets "frameId views n_kept n_retained n_unseen n_culled_free_space n_culled_unsupported
  // n_culled_photo sum_agree sum_in_front sum_behind sum_photo sum_photo_bad" per push that had candidates. The ring copy alone is touched.
  bool cullMatchDepth = false;
  ellc_cull_stats lastCullStats = ellc_cull_stats();
  int lastCullViews = 0;
  std::ofstream cull_matches_file;
  // Poses and depths together (ellc_keyframe_joint_refine; off by default: nothing changes; it needs refineMatchSim3): the first
  // min(candidates, ELLC_JOINT_MAX_VIEWS) candidates' transforms and the pushed keyframe's ring map are refined in one Gauss-Newton loop -
  // level 0, the filter of ellc_main --map, the default ellc_joint_params with min_views = min(2, views), six iterations at most, eps
  // 1e-6, lambda 0, the keyframe's own ring slot as the destination - AFTER sweepMatchDepth, IN PLACE OF refineMatchDepth where both are
  // asked for, and BEFORE cullMatchDepth, which then votes at the refined transforms. The refined transforms go back into
  // lastMatchSim3[b].T (inverted again: candidate -> keyframe), so that absorbMatches and match_sim3_file see them. lastJointRecord /
  // lastJointViews / lastJointIters keep the accepted state's record (zeros: no candidates) and joint_matches_file (when open) gets
  // "frameId views iters n_kept n_taking_part n_used n_too_few_views n_no_information n_terms chi2_photo chi2_prior" per push that had
  // candidates. The ring copy alone is touched.
  bool refineMatchJoint = false;
  ellc_joint_normal lastJointRecord = ellc_joint_normal();
  int lastJointViews = 0, lastJointIters = 0;
  std::ofstream joint_matches_file;
  // What a closed loop teaches, kept in the TRACKING context (ellc_depth_absorb_keyframes): every candidate of the push's batch is folded
  // into the live depth map of the pushed keyframe at its refined Sim(3). Off by default: nothing changes. On: pushToArray runs
  // findMatchParallel synchronously with the Sim(3) refinement, copies the ring slot of every entry of lastMatchSim3 into the tracking
  // context's keyframe slots 2, 3, ... (ellc_copy_slot_across), calls ellc_depth_absorb_keyframes there with each entry's T (candidate ->
  // pushed keyframe, which is the depth map's keyframe at that moment), the filter of ellc_main --map and the default parameters
  // (finalise on: the map is regularised and exported, so what createKeyFrame propagates next is the absorbed map), and absorb_file
  // (when open) gets "frameId B" and the fifteen stats per push (B 0 and zeros for a push without a match). The tracking runtime
  // needs max_keyframes >= 2 + MAX_LOOP_ARRAY_LENGTH_SCALE_AVG; otherwise pushToArray throws. lastAbsorbStats keeps the record.
  // With matchAffineLight the fold is ellc_depth_absorb_keyframes_lit at every entry's gain and offset (candidate -> keyframe, T's direction).
  struct AbsorbRecord {
    int frameId = 0, B = 0;
    ellc_absorb_stats stats;
  };
  bool absorbMatches = false;
  AbsorbRecord lastAbsorbStats;
  std::vector<int> lastMatchSlots;   // ring slots of the candidates of the batch findMatchParallel ran last, in lastMatchSim3's order (empty: no match)
  std::ofstream absorb_file;

  static ellc_config ring_config(const ellc_config& tracking, bool fixed_grids) {
    ellc_config c = tracking;
    c.max_keyframes = MAX_LOOP_ARRAY_LENGTH_SCALE_AVG;
    c.max_frames = 1;
    c.max_batch = MAX_LOOP_ARRAY_LENGTH_SCALE_AVG;
    c.grid_batch = fixed_grids ? c.max_batch : 0;   // world-size invariant bits (ellc_abi.h; set per batch: lc_grid_bucket)
    c.concurrent_batches = 1;
    c.coalesce = 1;
    c.cache_records = 1;          // the ring's keyframes stay from push to push: only the slot a push replaces has its pixel lists rebuilt (same results)
    return c;
  }
  globalOptimize(Runtime& r, const std::string& matchfilepath)
      : rt(&r), ring(ring_config(r.cfg, r.lc_fixed_grids || r.world > 1)), fixed_grids_(r.lc_fixed_grids || r.world > 1) {
    ring.BATCH_START_ID = r.BATCH_START_ID;
    match_file.open(matchfilepath.c_str());
  }
  // the grids of a loop-closure batch of B candidates: the smallest of {4, 8, 16, ring} that holds the whole batch
  static int lc_grid_bucket(int B) {
    const int buckets[4] = {4, 8, 16, MAX_LOOP_ARRAY_LENGTH_SCALE_AVG};
    for (int k = 0; k < 4; k++)
      if (B <= buckets[k]) return buckets[k];
    return MAX_LOOP_ARRAY_LENGTH_SCALE_AVG;
  }

  // ---- tracking-loss recovery (FLAG_RESTORE_CONNECTION, ExternVariable.h:176: off as shipped; main.cpp:252-324) -------------------
  // GlobalOptimize.cpp:934-943: the connection is lost when the depth map has no seeds left (MIN_SEEDS_FOR_CONNECTION_LOST = 0, ExternVariable.h:171)
  static constexpr float MIN_SEEDS_FOR_CONNECTION_LOST = 0.0f;
  depthMap* temp_depthMap = nullptr;   // the depth map a recovered connection hands to main (main.cpp:270); never set while restoreConnection is off
  void checkConnection(depthMap* currentDepthMap) {
    checkedDepthMap_ = currentDepthMap;
    connectionLost = currentDepthMap->calculate_no_of_Seeds() <= MIN_SEEDS_FOR_CONNECTION_LOST;
  }
  // FLAG_RESTORE_CONNECTION. Off (the default), findConnection is GlobalOptimize.cpp:717-760 AS SHIPPED (below). On, it goes on with the
  // search of :760-913 as ONE batch instead of one candidate after the other:
  //   (a) the candidates are every ring entry findMatch(..., strayFlag = true) hands out, collected by the loop of :780-913 - with the
  //       stray flag the source takes every valid, non-stray entry of the match window that is more than MIN_MATCH_DIFFERENCE frames
  //       older, whatever its histogram distance (:365) and without the view-angle test;
  //   (b) the test frame is aligned against all of them from the zero pose (:849-864) in the ring context, as findMatchParallel runs its batch;
  //   (c) ONE ellc_keyframe_trial_propagate of all candidates into the test frame (ring frame slot 0): T = the top three rows of
  //       exp(pose_b), the gate on, the filter of ellc_main --map;
  //   (d) they are tried in descending n_targets, ties to the lower ring index; a candidate with n_targets == 0 is skipped;
  //   (e) each in turn: its ring slot is copied into keyframe slot 2 of the tracking context (which therefore needs max_keyframes >= 3),
  //       the test frame is promoted to the tracking context's other keyframe slot, ellc_depth_restart_from_keyframes (B = 1, the default
  //       parameters) re-seats the live map on it, and checkConnection decides; the first that leaves the connection not lost is kept.
  //       B = 1 on purpose: every ring map carries a scale of its own (makeInvDepthOne) and the lost frame has no depth to reconcile
  //       two of them against;
  //   (f) on success the test frame's poses are what GetImagePoseEstimate sets against the matched keyframe, then - as
  //       temp_depthMap->createKeyFrame(testFrame) leaves them (:890, DepthPropagation.cpp:1772-1789) - it is a keyframe with the
  //       restart's rescale factor and a zero poseWrtOrigin; connectionLost is false and temp_depthMap is the depth map main.cpp:262-314
  //       takes over. On failure connectionLost stays true, temp_depthMap stays null and the tracking context's depth map sits on the
  //       keyframe it sat on before, empty. Either way the stray entry is reset at the end (:919).
  // lastRestore keeps what the search saw.
  struct RestoreRecord {
    int frameId = 0;
    std::vector<int> ids, slots;                  // ring array ids / ring keyframe slots of the candidates, in the order findMatch handed them out
    std::vector<float> poses;                     // [candidates][6]: the test frame w.r.t. each candidate, as the batch returned them
    std::vector<float> T;                         // [candidates][12]: candidate camera -> test frame camera, as passed to the library
    std::vector<ellc_trial_propagation> records;  // per candidate (with restoreAffineLight: of the second trial, at the fitted lights)
    std::vector<float> lights;                    // [candidates][2]: gain and offset the candidates were scored at ((1, 0) without restoreAffineLight)
    std::vector<int> tried;                       // ring array ids in the order their restart was run
    int chosen = -1;                              // the ring array id the map was restarted from, -1: none
    int chosenFrameId = -1, newKeyframeSlot = -1;
    ellc_absorb_stats stats;                      // of the last restart that was run (zeros: none)
    float rescaleFactor = 0.0f, seedsAfter = 0.0f;
  };
  bool restoreConnection = false;
  // restoreAffineLight (off by default: nothing changes; it acts inside restoreConnection's search): the exposure has usually swung when
  // tracking is lost, so step (c) becomes one ellc_keyframe_trial_propagate_lit at (1, 0), ellc_trial_light_solve of every candidate's
  // record with the default ellc_light_params (a refused fit keeps (1, 0)), and a second trial at the fitted lights; (d) orders by the
  // second trial's n_targets, and (e) restarts with ellc_depth_restart_from_keyframes_lit at the winner's light. The alignment of (b)
  // stays blind to the light.
  bool restoreAffineLight = false;
  RestoreRecord lastRestore;
  // With restoreConnection off, GlobalOptimize.cpp:717-760 AS SHIPPED: waits for the match thread, pushes the stray test frame (no depth
  // map) into the ring at currentArrayId — histogram, ids, image — and returns: the search that follows in the source sits behind an
  // unconditional return (:759), so connectionLost stays as checkConnection left it and temp_depthMap stays null.
  void findConnection(frame* testFrame) {
    join_all();   // :725 t_group.join_all()
    loopFrame& slot = loopFrameArray[currentArrayId];
    if (slot.isValid) { slot.isValid = false; slot.isStray = false; slot.frameId = 0; }   // resetArrayElement (:124-147)
    slot.kf_slot = currentArrayId;
    ring.check(ellc_copy_slot_across(ring.ctx, 1, slot.kf_slot, rt->ctx, 0, testFrame->slot), "ellc_copy_slot_across");   // this_frame = new frame(*testFrame): the image
    TestFrame test;
    test.frameId = testFrame->frameId;
    test.ring_slot = slot.kf_slot;
    std::memcpy(test.poseWrtWorld, testFrame->poseWrtWorld, 24);
    std::memcpy(test.poseWrtOrigin, testFrame->poseWrtOrigin, 24);
    calculateImageHistogram(test);
    slot.isStray = true;   // :750 no depth map: findMatch never aligns against it (it needs one) until a keyframe replaces it
    slot.frameId = currentLoopFrame.frameId;
    slot.isValid = currentLoopFrame.isValid;
    std::memcpy(slot.image_histogram, currentLoopFrame.image_histogram, sizeof(slot.image_histogram));
    if (!restoreConnection) return;
    searchConnection(testFrame, test);
    slot.isValid = false; slot.isStray = false; slot.frameId = 0;   // :919 resetArrayElement(currentArrayId)
  }
  ~globalOptimize() {
    try { join_all(); } catch (...) {}
  }
  // t_group.join_all() (:161); rethrows what the matching thread failed with
  void join_all() {
    if (t_group.joinable()) t_group.join();
    if (!thread_error.empty()) {
      const std::string e = thread_error;
      thread_error.clear();
      throw std::runtime_error(e);
    }
  }

  // GlobalOptimize.cpp:151-272 (FLAG_USE_LOOP_CLOSURE_TRIGGER off: every finished keyframe is tested)
  void pushToArray(frame* currentframe, depthMap* currentDepthMap) {
    join_all();   // :161 wait for the match thread before pushing another frame
    loopFrame& slot = loopFrameArray[currentArrayId];
    slot.kf_slot = currentArrayId;
    slot.isStray = false;
    lastPushedArrayId = currentArrayId;
    // :185-186 deep copies of the keyframe and its depth map, into the ring context
    rt->check(ellc_copy_slot_across(ring.ctx, 1, slot.kf_slot, rt->ctx, 1, currentframe->kf_slot), "ellc_copy_slot_across");
    TestFrame test;
    test.frameId = currentframe->frameId;
    test.ring_slot = slot.kf_slot;
    std::memcpy(test.poseWrtWorld, currentframe->poseWrtWorld, 24);
    std::memcpy(test.poseWrtOrigin, currentframe->poseWrtOrigin, 24);
    calculateImageHistogram(test);
    slot.frameId = currentLoopFrame.frameId;
    slot.isValid = currentLoopFrame.isValid;
    std::memcpy(slot.image_histogram, currentLoopFrame.image_histogram, sizeof(slot.image_histogram));
    std::memcpy(slot.poseWrtWorld, currentframe->poseWrtWorld, 24);
    std::memcpy(slot.poseWrtOrigin, currentframe->poseWrtOrigin, 24);
    slot.rescaleFactor = currentframe->rescaleFactor;
    slot.seeds = currentDepthMap->calculate_no_of_Seeds();
    if (absorbMatches) {   // the batch, its Sim(3) refinement and the fold before the caller goes on to createKeyFrame
      if (rt->cfg.max_keyframes < 2 + MAX_LOOP_ARRAY_LENGTH_SCALE_AVG)
        throw std::runtime_error("absorbMatches: the tracking runtime needs max_keyframes >= 2 + MAX_LOOP_ARRAY_LENGTH_SCALE_AVG");
      const bool refine = refineMatchSim3;
      refineMatchSim3 = true;
      try { findMatchParallel(test); } catch (...) { refineMatchSim3 = refine; throw; }
      refineMatchSim3 = refine;
      absorbLastMatches(test.frameId);
    } else if (FLAG_DO_PARALLEL_SHORT_LOOP_CLOSURE) {   // :239-241
      t_group = std::thread([this, test]() {
        try { findMatchParallel(test); } catch (const std::exception& e) { thread_error = e.what(); }
      });
    } else {
      findMatchParallel(test);
    }
  }

  // absorbMatches: the candidates of the batch findMatchParallel just ran, folded into the tracking context's live depth map
  void absorbLastMatches(int frameId) {
    const int B = (int)lastMatchSlots.size();
    lastAbsorbStats = AbsorbRecord();
    lastAbsorbStats.frameId = frameId + rt->BATCH_START_ID - 1;
    lastAbsorbStats.B = B;
    std::memset(&lastAbsorbStats.stats, 0, sizeof(lastAbsorbStats.stats));
    if (B > 0) {
      if ((size_t)B != lastMatchSim3.size()) throw std::runtime_error("absorbMatches: the batch left no Sim(3) per candidate");
      std::vector<int> slots((size_t)B);
      std::vector<float> T((size_t)B * 12);
      for (int b = 0; b < B; b++) {
        slots[(size_t)b] = 2 + b;
        rt->check(ellc_copy_slot_across(rt->ctx, 1, 2 + b, ring.ctx, 1, lastMatchSlots[(size_t)b]), "ellc_copy_slot_across");
        for (int k = 0; k < 12; k++) T[(size_t)b * 12 + k] = lastMatchSim3[(size_t)b].T[k];
      }
      ellc_map_filter filter;   // the filter of ellc_main --map
      filter.max_var = 0.0f; filter.min_support = 3; filter.support_k2 = 1.0f; filter.stride = 1;
      ellc_absorb_params params;
      ellc_absorb_default_params(&params);
      if (matchAffineLight) {   // the refined light of every candidate, candidate -> keyframe (T's direction), in the fold's photometric gate
        std::vector<float> light((size_t)B * 2);
        for (int b = 0; b < B; b++) {
          light[(size_t)b * 2] = lastMatchSim3[(size_t)b].gain;
          light[(size_t)b * 2 + 1] = lastMatchSim3[(size_t)b].offset;
        }
        rt->check(ellc_depth_absorb_keyframes_lit(rt->ctx, B, slots.data(), T.data(), light.data(), &filter, &params, &lastAbsorbStats.stats),
                  "ellc_depth_absorb_keyframes_lit");
      } else
        rt->check(ellc_depth_absorb_keyframes(rt->ctx, B, slots.data(), T.data(), &filter, &params, &lastAbsorbStats.stats), "ellc_depth_absorb_keyframes");
    }
    if (absorb_file.is_open()) {
      const int32_t* v = &lastAbsorbStats.stats.n_kept;   // sixteen int32 in a row (ellc_abi.h); the reserved word is not written
      absorb_file << lastAbsorbStats.frameId << " " << B;
      for (int k = 0; k < 15; k++) absorb_file << " " << v[k];
      absorb_file << "\n";
      absorb_file.flush();
    }
  }

  // The ring's semi-dense map as 3-D points in world coordinates (ellc_keyframe_map_points; no reference counterpart — the reference
  // only draws its depth map, DepthPropagation.cpp:1160-1250). Waits for the match thread, then exports every valid, non-stray ring
  // entry in ring-array order, one request each: out[k].source is the request's number, and the entries' array ids are returned in
  // that order. exp(poseWrtWorld) takes world coordinates into the keyframe's (Frame.cpp:352-358), so entry i is exported through
  // T = exp(poseWrtWorld)^-1 (mapTransform); scale (optional, indexed by array id) multiplies its 3x3 block. Chaining the
  // per-keyframe rescaleFactor into such a scale stays with the caller, as it does for the pose files.
  static void mapTransform(const float* poseWrtWorld, float scale, float* T12) {
    float E[16];
    ellc_se3_exp(poseWrtWorld, E);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) T12[4 * r + c] = E[4 * c + r] * scale;                      // R^T (scaled)
      T12[4 * r + 3] = -((E[r] * E[3] + E[4 + r] * E[7]) + E[8 + r] * E[11]);                 // -R^T t
    }
  }
  std::vector<int> exportLocalMap(const ellc_map_filter& filter, int level, std::vector<ellc_map_point>& out, const float* scale = nullptr) {
    join_all();
    std::vector<int> ids, slots;
    std::vector<float> T;
    for (int i = 0; i < MAX_LOOP_ARRAY_LENGTH_SCALE_AVG; i++) {
      const loopFrame& e = loopFrameArray[i];
      if (!e.isValid || e.isStray || e.kf_slot < 0) continue;
      ids.push_back(i);
      slots.push_back(e.kf_slot);
      T.resize(T.size() + 12);
      mapTransform(e.poseWrtWorld, scale ? scale[i] : 1.0f, &T[T.size() - 12]);
    }
    out.clear();
    if (ids.empty()) return ids;
    int total = 0;
    ring.check(ellc_keyframe_map_points(ring.ctx, (int)ids.size(), slots.data(), T.data(), level, &filter, nullptr, 0, nullptr, &total),
               "ellc_keyframe_map_points");
    out.resize((size_t)total);
    ellc_map_point none;
    ring.check(ellc_keyframe_map_points(ring.ctx, (int)ids.size(), slots.data(), T.data(), level, &filter, total ? out.data() : &none, total, nullptr, &total),
               "ellc_keyframe_map_points");
    return ids;
  }

  // The ring's map seen from a camera pose (ellc_keyframe_render_depth; the reference's findConnection, GlobalOptimize.cpp:862-896, does
  // this with a copied depthMap and createKeyFrame behind its unconditional return). Waits for the match thread, then splats every
  // valid, non-stray ring entry, in ring-array order, into the view whose world-to-camera transform is exp(viewPoseWrtWorld) — the
  // poseWrtWorld convention of exportLocalMap: request b goes through T_b = exp(viewPoseWrtWorld) * exp(poseWrtWorld_b)^-1, composed in
  // f32 (viewTransform). into (may be null; level 0 only): a keyframe of the TRACKING runtime that receives the rendered depth and
  // variance as its level-0 planes (ellc_keyframe_set_depth: the ring lives in a context of its own, so the planes this call returns
  // anyway are handed across; inside one context ellc_keyframe_render_depth's dst_kf_slot does it without the host).
  static void viewTransform(const float* viewPoseWrtWorld, const float* poseWrtWorld, float* T12) {
    float V[16], M[12];
    ellc_se3_exp(viewPoseWrtWorld, V);
    mapTransform(poseWrtWorld, 1.0f, M);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++)
        T12[4 * r + c] = ((V[4 * r] * M[c] + V[4 * r + 1] * M[4 + c]) + V[4 * r + 2] * M[8 + c]) + (c == 3 ? V[4 * r + 3] : 0.0f);
  }
  // the requests of a view (every valid, non-stray ring entry in ring-array order) and its planes, empty: what renderLocalMap and
  // fuseLocalMap hand the library
  void viewRequests(const float* viewPoseWrtWorld, int level, RenderedView& out) {
    out.cols = ring.cfg.width >> level;
    out.rows = ring.cfg.height >> level;
    for (int i = 0; i < MAX_LOOP_ARRAY_LENGTH_SCALE_AVG; i++) {
      const loopFrame& e = loopFrameArray[i];
      if (!e.isValid || e.isStray || e.kf_slot < 0) continue;
      out.ids.push_back(i);
      out.slots.push_back(e.kf_slot);
      out.T.resize(out.T.size() + 12);
      viewTransform(viewPoseWrtWorld, e.poseWrtWorld, &out.T[out.T.size() - 12]);
    }
    const size_t n = (size_t)out.cols * out.rows;
    out.depth.assign(n, 0.0f);
    out.var.assign(n, -1.0f);
    out.source.assign(n, -1);
    out.agree.assign(n, 0);
    out.intensity.assign(n, 0);
  }
  void renderLocalMap(const float* viewPoseWrtWorld, int level, const ellc_map_filter& filter, float agree_k2, frame* into, RenderedView& out) {
    join_all();
    if (level < 0 || level >= ring.cfg.levels) throw std::runtime_error("renderLocalMap: level out of range");
    if (into && (level != 0 || into->kf_slot < 0)) throw std::runtime_error("renderLocalMap: the destination must be a keyframe and the level 0");
    out = RenderedView();
    viewRequests(viewPoseWrtWorld, level, out);
    if (!out.ids.empty())
      ring.check(ellc_keyframe_render_depth(ring.ctx, (int)out.ids.size(), out.slots.data(), out.T.data(), level, &filter, agree_k2, -1, out.depth.data(),
                                            out.var.data(), out.source.data(), out.agree.data(), out.intensity.data(), &out.n_valid),
                 "ellc_keyframe_render_depth");
    if (into) rt->check(ellc_keyframe_set_depth(rt->ctx, into->kf_slot, out.depth.data(), out.var.data()), "ellc_keyframe_set_depth");
  }
  // renderLocalMap with the candidates that agree with a target's winner merged into it (ellc_keyframe_fuse_depth): what the ring's
  // keyframes TOGETHER say about the surfaces the view sees, each target fused from at most max_merge agreeing candidates in ring-array
  // order. Requests, transforms, filter, agree_k2 and `into` as renderLocalMap.
  void fuseLocalMap(const float* viewPoseWrtWorld, int level, const ellc_map_filter& filter, float agree_k2, int max_merge, frame* into, FusedView& out) {
    join_all();
    if (level < 0 || level >= ring.cfg.levels) throw std::runtime_error("fuseLocalMap: level out of range");
    if (into && (level != 0 || into->kf_slot < 0)) throw std::runtime_error("fuseLocalMap: the destination must be a keyframe and the level 0");
    out = FusedView();
    viewRequests(viewPoseWrtWorld, level, out);
    out.max_merge = max_merge;
    out.merged.assign(out.depth.size(), 0);
    if (!out.ids.empty())
      ring.check(ellc_keyframe_fuse_depth(ring.ctx, (int)out.ids.size(), out.slots.data(), out.T.data(), level, &filter, agree_k2, max_merge, -1,
                                          out.depth.data(), out.var.data(), out.source.data(), out.agree.data(), out.merged.data(), out.intensity.data(),
                                          &out.n_valid, &out.n_fused),
                 "ellc_keyframe_fuse_depth");
    if (into) rt->check(ellc_keyframe_set_depth(rt->ctx, into->kf_slot, out.depth.data(), out.var.data()), "ellc_keyframe_set_depth");
  }
  int lastPushedArrayId = -1;   // the ring entry of the most recent pushToArray

 private:
  // what the matching thread keeps of the pushed keyframe (the reference hands it loopFrameArray[currentArrayId].this_frame, a
  // deep copy: the caller's frame object may be gone before the thread ends)
  struct TestFrame {
    int frameId, ring_slot;
    float poseWrtWorld[6], poseWrtOrigin[6];
  };
  std::thread t_group;
  std::string thread_error;
  bool fixed_grids_ = true;
  depthMap* checkedDepthMap_ = nullptr;   // what checkConnection looked at last: its keyframe's slot is the tracking context's active one

  // findConnection with restoreConnection on, behind the push of the stray frame: steps (a)-(f) above
  void searchConnection(frame* testFrame, const TestFrame& test) {
    lastRestore = RestoreRecord();
    lastRestore.frameId = testFrame->frameId;
    std::memset(&lastRestore.stats, 0, sizeof(lastRestore.stats));
    if (rt->cfg.max_keyframes < 3) throw std::runtime_error("restoreConnection: the tracking runtime needs max_keyframes >= 3");
    // (a) :776-913, the loop alone
    loopFrameArray[nextArrayId].frameId = testFrame->frameId;
    lastTestedLoopClosureArrayId = -1;
    firstTestedLoopClosureArrayId = -1;
    int num_matches = 0;
    do {
      const bool matchFound = findMatch(test, true);
      if (num_matches > 0 && lastTestedLoopClosureArrayId == firstTestedLoopClosureArrayId) break;
      if (matchFound) {
        if (num_matches == 0) firstTestedLoopClosureArrayId = lastTestedLoopClosureArrayId;
        num_matches++;
        lastRestore.ids.push_back(loopClosureArrayId);
        lastRestore.slots.push_back(loopFrameArray[loopClosureArrayId].kf_slot);
      }
    } while (lastTestedLoopClosureArrayId != -1);
    const int B = (int)lastRestore.ids.size();
    if (B == 0) return;
    // (b) one batched constant-weight alignment from the zero pose
    std::vector<int> fr((size_t)B, 0);
    std::vector<float> init((size_t)B * 6, 0.0f);
    lastRestore.poses.assign((size_t)B * 6, 0.0f);
    ring.check(ellc_copy_slot(ring.ctx, 0, 0, 1, test.ring_slot), "ellc_copy_slot");
    if (fixed_grids_) ring.check(ellc_ctx_set_grid_batch(ring.ctx, lc_grid_bucket(B)), "ellc_ctx_set_grid_batch");
    ring.check(ellc_align(ring.ctx, B, lastRestore.slots.data(), fr.data(), init.data(), ELLC_MODE_ICA, 0, lastRestore.poses.data(), nullptr, nullptr), "ellc_align");
    // (c) one trial propagation of all of them into the test frame
    ellc_map_filter filter;   // the filter of ellc_main --map
    filter.max_var = 0.0f; filter.min_support = 3; filter.support_k2 = 1.0f; filter.stride = 1;
    lastRestore.T.assign((size_t)B * 12, 0.0f);
    for (int b = 0; b < B; b++) {
      float M[16];
      ellc_se3_exp(&lastRestore.poses[(size_t)b * 6], M);
      for (int k = 0; k < 12; k++) lastRestore.T[(size_t)b * 12 + k] = M[k];
    }
    lastRestore.records.assign((size_t)B, ellc_trial_propagation());
    lastRestore.lights.assign((size_t)B * 2, 0.0f);
    for (int b = 0; b < B; b++) lastRestore.lights[(size_t)b * 2] = 1.0f;
    if (restoreAffineLight) {
      std::vector<ellc_trial_propagation_lit> lit((size_t)B);
      ring.check(ellc_keyframe_trial_propagate_lit(ring.ctx, B, lastRestore.slots.data(), 0, fr.data(), lastRestore.T.data(), nullptr, &filter, 1, lit.data()),
                 "ellc_keyframe_trial_propagate_lit");
      ellc_light_params lp;
      ellc_light_default_params(&lp);
      for (int b = 0; b < B; b++) (void)ellc_trial_light_solve(&lit[(size_t)b], &lp, nullptr, &lastRestore.lights[(size_t)b * 2]);
      ring.check(ellc_keyframe_trial_propagate_lit(ring.ctx, B, lastRestore.slots.data(), 0, fr.data(), lastRestore.T.data(), lastRestore.lights.data(), &filter,
                                                   1, lit.data()),
                 "ellc_keyframe_trial_propagate_lit");
      for (int b = 0; b < B; b++) std::memcpy(&lastRestore.records[(size_t)b], &lit[(size_t)b], sizeof(ellc_trial_propagation));   // its first 48 bytes
    } else
      ring.check(ellc_keyframe_trial_propagate(ring.ctx, B, lastRestore.slots.data(), 0, fr.data(), lastRestore.T.data(), &filter, 1, lastRestore.records.data()),
                 "ellc_keyframe_trial_propagate");
    // (d) descending n_targets, ties to the lower ring index
    std::vector<int> order;
    for (int b = 0; b < B; b++)
      if (lastRestore.records[(size_t)b].n_targets > 0) order.push_back(b);
    const RestoreRecord& lr = lastRestore;
    std::sort(order.begin(), order.end(), [&lr](int x, int y) {
      const int nx = lr.records[(size_t)x].n_targets, ny = lr.records[(size_t)y].n_targets;
      return nx != ny ? nx > ny : lr.ids[(size_t)x] < lr.ids[(size_t)y];
    });
    // (e) adopt the first that gives a map
    const int active = (checkedDepthMap_ && checkedDepthMap_->keyFrame && checkedDepthMap_->keyFrame->kf_slot >= 0) ? checkedDepthMap_->keyFrame->kf_slot : -1;
    const int ns = active >= 0 ? rt->other_keyframe_slot(active) : 0, copy_slot = 2;
    ellc_absorb_params params;
    ellc_absorb_default_params(&params);
    bool promoted = false;
    for (size_t q = 0; q < order.size(); q++) {
      const int b = order[q];
      const loopFrame& m = loopFrameArray[lastRestore.ids[(size_t)b]];
      rt->check(ellc_copy_slot_across(rt->ctx, 1, copy_slot, ring.ctx, 1, m.kf_slot), "ellc_copy_slot_across");
      if (!promoted) rt->check(ellc_keyframe_from_frame(rt->ctx, ns, testFrame->slot), "ellc_keyframe_from_frame");
      promoted = true;
      float factor = 1.0f;
      lastRestore.tried.push_back(lastRestore.ids[(size_t)b]);
      if (restoreAffineLight)
        rt->check(ellc_depth_restart_from_keyframes_lit(rt->ctx, ns, 1, &copy_slot, &lastRestore.T[(size_t)b * 12], &lastRestore.lights[(size_t)b * 2], &filter,
                                                        &params, &factor, &lastRestore.stats),
                  "ellc_depth_restart_from_keyframes_lit");
      else
        rt->check(ellc_depth_restart_from_keyframes(rt->ctx, ns, 1, &copy_slot, &lastRestore.T[(size_t)b * 12], &filter, &params, &factor, &lastRestore.stats),
                  "ellc_depth_restart_from_keyframes");
      depthMap* dm = new depthMap(*rt);
      dm->keyFrame = testFrame;
      dm->currentFrame = testFrame;
      dm->depthScale = factor;
      lastRestore.rescaleFactor = factor;
      lastRestore.seedsAfter = dm->calculate_no_of_Seeds();
      connectionLost = lastRestore.seedsAfter <= MIN_SEEDS_FOR_CONNECTION_LOST;   // checkConnection(temp_depthMap), :896
      if (connectionLost) { delete dm; continue; }
      // (f) GetImagePoseEstimate's poses (ImageFunc.cpp:305-306), then createKeyFrame's bookkeeping (:890)
      const float* pose = &lastRestore.poses[(size_t)b * 6];
      ellc_concatenate_relative_pose(pose, m.poseWrtOrigin, testFrame->poseWrtOrigin);
      ellc_concatenate_relative_pose(pose, m.poseWrtWorld, testFrame->poseWrtWorld);
      testFrame->parentKeyframeId = m.frameId;
      testFrame->kf_slot = ns;
      testFrame->isKeyframe = true;
      testFrame->rescaleFactor = factor;
      for (int i = 0; i < 6; i++) testFrame->poseWrtOrigin[i] = 0.0f;
      temp_depthMap = dm;
      lastRestore.chosen = lastRestore.ids[(size_t)b];
      lastRestore.chosenFrameId = m.frameId;
      lastRestore.newKeyframeSlot = ns;
      return;
    }
    // nobody gave a map: the (empty) depth map goes back to the keyframe the caller's depthMap names
    if (promoted && active >= 0) rt->check(ellc_depth_set_keyframe(rt->ctx, active), "ellc_depth_set_keyframe");
  }

  // :40-100 (the histogram of the copy in the ring context: the same image)
  void calculateImageHistogram(const TestFrame& f) {
    isloopClosureDetected = false;
    loopClosureArrayId = -1;
    currentLoopFrame.isValid = true;
    currentLoopFrame.frameId = f.frameId;
    std::memcpy(currentLoopFrame.poseWrtWorld, f.poseWrtWorld, 24);
    std::memcpy(currentLoopFrame.poseWrtOrigin, f.poseWrtOrigin, 24);
    ring.check(ellc_histogram(ring.ctx, 1, f.ring_slot, currentLoopFrame.image_histogram), "ellc_histogram");
  }
  // :436-452  third row of the rotation of exp(pose)
  static void calculateViewVec(const float* pose, float* view_vec) {
    float T[16];
    ellc_se3_exp(pose, T);
    view_vec[0] = T[8]; view_vec[1] = T[9]; view_vec[2] = T[10];
  }
  // :419-434
  void calculateRotationStats(const float* p1, const float* p2) {
    rms_error = (float)std::pow(std::pow(p1[0] - p2[0], 2) + std::pow(p1[1] - p2[1], 2) + std::pow(p1[2] - p2[2], 2), 0.5);
    float v1[3], v2[3];
    calculateViewVec(p1, v1);
    calculateViewVec(p2, v2);
    const float mag1 = (float)std::pow(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2], 0.5);
    const float mag2 = (float)std::pow(v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2], 0.5);
    relative_view_angle = std::acos((v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]) / (mag1 * mag2));
    relative_view_angle = (relative_view_angle * 180) / 3.14f;   // sic: 3.14
  }
  // :274-416. strayFlag (findConnection's test frame: it has no pose to compare): no rotation statistics, and every entry that is old
  // enough is handed out whatever its histogram distance (`matchValue <= MATCH_THRESHOLD || strayFlag`, :365)
  bool findMatch(const TestFrame& currentframe, bool strayFlag = false) {
    const int RING = MAX_LOOP_ARRAY_LENGTH_SCALE_AVG;
    calculateImageHistogram(currentframe);
    int i;
    if (lastTestedLoopClosureArrayId == -1) i = currentArrayId - 1;
    else if (lastTestedLoopClosureArrayId != 0) i = lastTestedLoopClosureArrayId - 1;
    else i = RING - 1;
    if (i < 0) i = RING - 1;
    int conditionToTerminateLoop = 0;
    while (1) {
      lastTestedLoopClosureArrayId = i;
      if (match_window_end > match_window_beg) {
        if (!((i >= match_window_beg) && (i <= match_window_end))) conditionToTerminateLoop = 1;
      } else if (match_window_end < match_window_beg) {
        if (!((i >= match_window_beg) || (i <= match_window_end))) conditionToTerminateLoop = 1;
      } else if (loopFrameArray[i].isValid == false) conditionToTerminateLoop = 1;
      if (conditionToTerminateLoop == 1) { lastTestedLoopClosureArrayId = -1; break; }
      if (loopFrameArray[i].isValid == 0) { lastTestedLoopClosureArrayId = -1; return false; }
      // (a stray entry — an image findConnection pushed, no depth map — is never a candidate: the reference would hand its null
      // depth map to GetImagePoseEstimate; unreachable as shipped, FLAG_RESTORE_CONNECTION is off)
      if (!loopFrameArray[i].isStray && currentframe.frameId - loopFrameArray[i].frameId > 8) {   // MIN_MATCH_DIFFERENCE = KEYFRAME_PROPAGATE_INTERVAL
        matchValue = (float)ellc_kl_divergence(loopFrameArray[i].image_histogram, currentLoopFrame.image_histogram, 256);
        if (!strayFlag) calculateRotationStats(loopFrameArray[i].poseWrtWorld, currentLoopFrame.poseWrtWorld);
        if (matchValue <= 0.1f || strayFlag) {          // MATCH_THRESHOLD
          if (strayFlag || relative_view_angle <= 10.0f) {   // MAX_REL_VIEW_ANGLE
            isloopClosureDetected = true;
            loopClosureArrayId = i;
            break;
          }
        }
      }
      i--;
      if (i < 0) i = RING - 1;
    }
    return isloopClosureDetected;
  }
  // :454-646
  void findMatchParallel(const TestFrame& testFrame) {
    const int RING = MAX_LOOP_ARRAY_LENGTH_SCALE_AVG;
    struct Match { int arrayId; float matchValue, rms, angle; };
    std::vector<Match> matches;
    lastMatchSlots.clear();
    lastRefineStats = ellc_refine_stats();
    lastRefineViews = 0;
    lastSweepStats = ellc_sweep_stats();
    lastSweepViews = 0;
    lastCullStats = ellc_cull_stats();
    lastCullViews = 0;
    lastJointRecord = ellc_joint_normal();
    lastJointViews = lastJointIters = 0;
    loopFrameArray[nextArrayId].frameId = testFrame.frameId;
    lastTestedLoopClosureArrayId = -1;
    firstTestedLoopClosureArrayId = -1;
    int num_matches = 0;
    do {
      const bool matchFound = findMatch(testFrame);
      if (num_matches > 0 && lastTestedLoopClosureArrayId == firstTestedLoopClosureArrayId) break;
      if (matchFound) {
        if (num_matches == 0) firstTestedLoopClosureArrayId = lastTestedLoopClosureArrayId;
        num_matches++;
        matches.push_back(Match{loopClosureArrayId, matchValue, rms_error, relative_view_angle});
      }
    } while (lastTestedLoopClosureArrayId != -1);
    if (!matches.empty()) {
      // one batched constant-weight alignment for all candidates (GetImagePoseEstimate(..., fromLoopClosure = true), :566)
      const int B = (int)matches.size();
      std::vector<int> kf(B), fr(B, 0);
      std::vector<float> init((size_t)B * 6), out((size_t)B * 6);
      ring.check(ellc_copy_slot(ring.ctx, 0, 0, 1, testFrame.ring_slot), "ellc_copy_slot");
      for (int b = 0; b < B; b++) {
        const loopFrame& m = loopFrameArray[matches[b].arrayId];
        kf[b] = m.kf_slot;
        ellc_concatenate_origin_pose(testFrame.poseWrtWorld, m.poseWrtWorld, &init[(size_t)b * 6]);   // ImageFunc.cpp:106
      }
      lastMatchSlots = kf;
      if (fixed_grids_) ring.check(ellc_ctx_set_grid_batch(ring.ctx, lc_grid_bucket(B)), "ellc_ctx_set_grid_batch");   // of the WHOLE batch, on every rank
      if (rt->comm && rt->world > 1) {
        // this rank's contiguous block of the candidates on its own GPU, then the one exchange of the batch: 8 floats per
        // alignment [pose6, weightedPose, iterations] from every rank, in global order on every rank
        int lo = 0, hi = B;
        ellc_shard_range(B, rt->world, rt->rank, &lo, &hi);
        const int n = hi - lo;
        std::vector<float> pose((size_t)std::max(n, 1) * 6), wgt((size_t)std::max(n, 1)), local((size_t)std::max(n, 1) * 8), table((size_t)B * 8);
        std::vector<int> iters((size_t)std::max(n, 1) * ring.cfg.levels);
        if (n > 0)
          ring.check(ellc_align(ring.ctx, n, kf.data() + lo, fr.data() + lo, init.data() + (size_t)lo * 6, ELLC_MODE_ICA, 0, pose.data(), iters.data(), wgt.data()),
                     "ellc_align");
        for (int b = 0; b < n; b++) {
          for (int k = 0; k < 6; k++) local[(size_t)b * 8 + k] = pose[(size_t)b * 6 + k];
          local[(size_t)b * 8 + 6] = wgt[b];
          int it = 0;
          for (int l = 0; l < ring.cfg.levels; l++) it += iters[(size_t)b * ring.cfg.levels + l];
          local[(size_t)b * 8 + 7] = (float)it;
        }
        if (ellc_gather_results(rt->comm, B, local.data(), n, table.data()) != ELLC_OK)
          throw std::runtime_error(std::string("ellc_gather_results failed: ") + ellc_comm_last_error(rt->comm));
        for (int b = 0; b < B; b++)
          for (int k = 0; k < 6; k++) out[(size_t)b * 6 + k] = table[(size_t)b * 8 + k];
      } else {
        ring.check(ellc_align(ring.ctx, B, kf.data(), fr.data(), init.data(), ELLC_MODE_ICA, 0, out.data(), nullptr, nullptr), "ellc_align");
      }
      if (collectMatchQuality) {   // the call site beside GlobalOptimize.cpp:566: one pixel pass per candidate at the pose it came back with
        lastMatchQuality.assign((size_t)B, ellc_align_quality());
        ring.check(ellc_align_quality_at(ring.ctx, B, kf.data(), fr.data(), out.data(), 0, lastMatchQuality.data()), "ellc_align_quality_at");
      }
      if (collectMatchGeometry) {
        std::vector<int> dst((size_t)B, testFrame.ring_slot);
        std::vector<float> T((size_t)B * 12);
        std::vector<ellc_depth_consistency> rec((size_t)B);
        ellc_map_filter filter;   // the filter of ellc_main --map; agree_k2 1
        filter.max_var = 0.0f; filter.min_support = 3; filter.support_k2 = 1.0f; filter.stride = 1;
        for (int b = 0; b < B; b++) {
          float M[16];
          ellc_se3_exp(&out[(size_t)b * 6], M);
          for (int k = 0; k < 12; k++) T[(size_t)b * 12 + k] = M[k];
        }
        ring.check(ellc_keyframe_depth_consistency(ring.ctx, B, kf.data(), dst.data(), T.data(), 0, &filter, 1.0f, rec.data()),
                   "ellc_keyframe_depth_consistency");
        lastMatchGeometry.assign((size_t)B, MatchGeometry());
        for (int b = 0; b < B; b++) {
          double scale = rec[(size_t)b].sum_w_ss > 0.0 ? rec[(size_t)b].sum_w_st / rec[(size_t)b].sum_w_ss : 1.0;
          if (!(scale > 0.0 && scale <= (double)FLT_MAX)) scale = 1.0;
          lastMatchGeometry[(size_t)b].scale = scale;
          for (int k = 0; k < 12; k++) T[(size_t)b * 12 + k] = (float)((double)T[(size_t)b * 12 + k] / scale);
        }
        ring.check(ellc_keyframe_depth_consistency(ring.ctx, B, kf.data(), dst.data(), T.data(), 0, &filter, 1.0f, rec.data()),
                   "ellc_keyframe_depth_consistency");
        for (int b = 0; b < B; b++) lastMatchGeometry[(size_t)b].rec = rec[(size_t)b];
      }
      if (refineMatchSim3) {
        std::vector<int> dst((size_t)B, testFrame.ring_slot);
        std::vector<float> T((size_t)B * 12), Tout((size_t)B * 12);
        std::vector<ellc_depth_consistency> rec((size_t)B);
        ellc_map_filter filter;   // the filter of ellc_main --map
        filter.max_var = 0.0f; filter.min_support = 3; filter.support_k2 = 1.0f; filter.stride = 1;
        for (int b = 0; b < B; b++) {
          float M[16];
          ellc_se3_exp(&out[(size_t)b * 6], M);
          for (int k = 0; k < 12; k++) T[(size_t)b * 12 + k] = M[k];
        }
        ring.check(ellc_keyframe_depth_consistency(ring.ctx, B, kf.data(), dst.data(), T.data(), 0, &filter, 1.0f, rec.data()),
                   "ellc_keyframe_depth_consistency");
        for (int b = 0; b < B; b++) {
          double scale = rec[(size_t)b].sum_w_ss > 0.0 ? rec[(size_t)b].sum_w_st / rec[(size_t)b].sum_w_ss : 1.0;
          if (!(scale > 0.0 && scale <= (double)FLT_MAX)) scale = 1.0;
          for (int k = 0; k < 12; k++) T[(size_t)b * 12 + k] = (float)((double)T[(size_t)b * 12 + k] / scale);
        }
        ellc_sim3_params params;
        ellc_sim3_default_params(&params);
        const int level_from = ring.cfg.levels > 1 ? 1 : 0, n_levels = level_from + 1;
        std::vector<ellc_sim3_normal> normal((size_t)B);
        std::vector<int> iters((size_t)B * n_levels);
        std::vector<float> light((size_t)B * 2);
        for (int b = 0; b < B; b++) { light[(size_t)b * 2] = 1.0f; light[(size_t)b * 2 + 1] = 0.0f; }
        if (matchAffineLight) {
          ellc_light_params light_params;
          ellc_light_default_params(&light_params);
          ring.check(ellc_keyframe_sim3_align_lit(ring.ctx, B, kf.data(), dst.data(), T.data(), nullptr, level_from, 0, &filter, &params, &light_params, 10,
                                                  1e-4f, Tout.data(), light.data(), normal.data(), nullptr, iters.data(), nullptr, nullptr, nullptr, nullptr, 0),
                     "ellc_keyframe_sim3_align_lit");
        } else {
          ring.check(ellc_keyframe_sim3_align(ring.ctx, B, kf.data(), dst.data(), T.data(), level_from, 0, &filter, &params, 10, 1e-4f, Tout.data(),
                                              normal.data(), iters.data(), nullptr, nullptr, 0),
                     "ellc_keyframe_sim3_align");
        }
        lastMatchSim3.assign((size_t)B, MatchSim3());
        for (int b = 0; b < B; b++) {
          MatchSim3& q = lastMatchSim3[(size_t)b];
          q.rec = normal[(size_t)b];
          const float* A = &Tout[(size_t)b * 12];
          for (int k = 0; k < 12; k++) q.T[k] = A[k];
          const double det = (double)A[0] * ((double)A[5] * A[10] - (double)A[6] * A[9]) - (double)A[1] * ((double)A[4] * A[10] - (double)A[6] * A[8]) +
                             (double)A[2] * ((double)A[4] * A[9] - (double)A[5] * A[8]);
          q.scale = std::cbrt(det);
          q.iters = 0;
          for (int l = 0; l < n_levels; l++) q.iters += iters[(size_t)b * n_levels + l];
          q.gain = light[(size_t)b * 2];
          q.offset = light[(size_t)b * 2 + 1];
        }
      }
      // the views of the three structure steps: the candidates' ring slots, each at the INVERSE of its refined transform and light
      const int V = std::min(B, (int)ELLC_REFINE_MAX_VIEWS);
      std::vector<float> T, light;
      if (refineMatchSim3 && (sweepMatchDepth || refineMatchDepth || refineMatchJoint || cullMatchDepth)) {
        T.resize((size_t)V * 12); light.resize((size_t)V * 2);
        for (int b = 0; b < V; b++) {
          const MatchSim3& q = lastMatchSim3[(size_t)b];
          const float l[2] = {q.gain, q.offset};
          ellc_sim3_invert(q.T, l, &T[(size_t)b * 12], &light[(size_t)b * 2]);
        }
      }
      if (refineMatchSim3 && sweepMatchDepth) {
        ellc_sweep_params params;
        ellc_sweep_default_params(&params);
        params.min_views = std::min(params.min_views, V);
        lastSweepStats = ellc_sweep_stats();
        lastSweepViews = V;
        ring.check(ellc_keyframe_sweep_depth(ring.ctx, testFrame.ring_slot, 0, V, 1, kf.data(), T.data(), light.data(), &params, testFrame.ring_slot,
                                             nullptr, nullptr, nullptr, nullptr, &lastSweepStats),
                   "ellc_keyframe_sweep_depth");
        if (sweep_matches_file.is_open()) {
          const ellc_sweep_stats& r = lastSweepStats;
          sweep_matches_file << (testFrame.frameId + rt->BATCH_START_ID - 1) << " " << V << " " << r.n_ok << " " << r.n_swept << " " << r.n_created << " "
                             << r.n_no_valid_sample << " " << r.n_at_range_end << " " << r.n_cost_too_high << " " << r.n_not_distinct << " " << r.n_flat
                             << " " << r.sum_views << " " << r.sum_cost << "\n";
          sweep_matches_file.flush();
        }
      }
      if (refineMatchSim3 && refineMatchJoint) {
        ellc_map_filter filter;   // the filter of ellc_main --map
        filter.max_var = 0.0f; filter.min_support = 3; filter.support_k2 = 1.0f; filter.stride = 1;
        ellc_joint_params params;
        ellc_joint_default_params(&params);
        const int VJ = std::min(V, (int)ELLC_JOINT_MAX_VIEWS);
        params.min_views = std::min(params.min_views, VJ);
        lastJointViews = VJ;
        std::vector<float> Tj((size_t)VJ * 12);
        ring.check(ellc_keyframe_joint_refine(ring.ctx, testFrame.ring_slot, 0, VJ, 1, kf.data(), T.data(), light.data(), &filter, &params, nullptr, 6, 1e-6f,
                                              0.0, testFrame.ring_slot, Tj.data(), &lastJointRecord, &lastJointIters, nullptr, nullptr, nullptr, nullptr,
                                              nullptr, nullptr, nullptr, nullptr, nullptr, 0),
                   "ellc_keyframe_joint_refine");
        for (int b = 0; b < VJ; b++) {   // for the cull below (keyframe -> candidate) and for the absorb (candidate -> keyframe)
          for (int k = 0; k < 12; k++) T[(size_t)b * 12 + k] = Tj[(size_t)b * 12 + k];
          ellc_sim3_invert(&Tj[(size_t)b * 12], nullptr, lastMatchSim3[(size_t)b].T, nullptr);
        }
        if (joint_matches_file.is_open()) {
          const ellc_joint_normal& r = lastJointRecord;
          joint_matches_file << (testFrame.frameId + rt->BATCH_START_ID - 1) << " " << VJ << " " << lastJointIters << " " << r.n_kept << " "
                             << r.n_taking_part << " " << r.n_used << " " << r.n_too_few_views << " " << r.n_no_information << " " << r.n_terms << " "
                             << r.chi2_photo << " " << r.chi2_prior << "\n";
          joint_matches_file.flush();
        }
      } else if (refineMatchSim3 && refineMatchDepth) {
        ellc_map_filter filter;   // the filter of ellc_main --map
        filter.max_var = 0.0f; filter.min_support = 3; filter.support_k2 = 1.0f; filter.stride = 1;
        ellc_refine_params params;
        ellc_refine_default_params(&params);
        params.min_views = std::min(params.min_views, V);
        lastRefineStats = ellc_refine_stats();
        lastRefineViews = V;
        ring.check(ellc_keyframe_refine_depth(ring.ctx, testFrame.ring_slot, 0, V, 1, kf.data(), T.data(), light.data(), &filter, &params,
                                              testFrame.ring_slot, nullptr, nullptr, nullptr, nullptr, &lastRefineStats),
                   "ellc_keyframe_refine_depth");
        if (refine_matches_file.is_open()) {
          const ellc_refine_stats& r = lastRefineStats;
          refine_matches_file << (testFrame.frameId + rt->BATCH_START_ID - 1) << " " << V << " " << r.n_kept << " " << r.n_taking_part << " " << r.n_refined
                              << " " << r.n_too_few_views << " " << r.n_no_information << " " << r.n_bad_step << " " << r.n_views_changed << " "
                              << r.n_cost_rose << " " << r.sum_views << " " << r.sum_cost_before << " " << r.sum_cost_after << "\n";
          refine_matches_file.flush();
        }
      }
      if (refineMatchSim3 && cullMatchDepth) {
        ellc_map_filter filter;   // every hypothesis takes part
        filter.max_var = 0.0f; filter.min_support = 0; filter.support_k2 = 1.0f; filter.stride = 1;
        ellc_cull_params params;
        ellc_cull_default_params(&params);
        params.min_support = std::min(params.min_support, V);
        params.min_judged = std::min(params.min_judged, V);
        params.min_in_front = std::min(params.min_in_front, V);
        params.min_photo = std::min(params.min_photo, V);
        lastCullStats = ellc_cull_stats();
        lastCullViews = V;
        ring.check(ellc_keyframe_cull_depth(ring.ctx, testFrame.ring_slot, 0, V, 1, kf.data(), T.data(), light.data(), &filter, &params,
                                            testFrame.ring_slot, nullptr, nullptr, nullptr, nullptr, nullptr, &lastCullStats),
                   "ellc_keyframe_cull_depth");
        if (cull_matches_file.is_open()) {
          const ellc_cull_stats& r = lastCullStats;
          cull_matches_file << (testFrame.frameId + rt->BATCH_START_ID - 1) << " " << V << " " << r.n_kept << " " << r.n_retained << " " << r.n_unseen << " "
                            << r.n_culled_free_space << " " << r.n_culled_unsupported << " " << r.n_culled_photo << " " << r.sum_agree << " "
                            << r.sum_in_front << " " << r.sum_behind << " " << r.sum_photo << " " << r.sum_photo_bad << "\n";
          cull_matches_file.flush();
        }
      }
      for (int b = 0; b < B; b++) {
        const loopFrame& m = loopFrameArray[matches[b].arrayId];
        float poseWrtOrigin[6];
        ellc_concatenate_relative_pose(&out[(size_t)b * 6], m.poseWrtOrigin, poseWrtOrigin);   // ImageFunc.cpp:305
        const int seeds_num = (int)m.seeds;   // `int seeds_num` in the reference (:466)
        if (match_file.is_open()) {           // :580
          match_file << (testFrame.frameId + rt->BATCH_START_ID - 1) << " " << (m.frameId + rt->BATCH_START_ID - 1) << " " << poseWrtOrigin[0] << " "
                     << poseWrtOrigin[1] << " " << poseWrtOrigin[2] << " " << poseWrtOrigin[3] << " " << poseWrtOrigin[4] << " " << poseWrtOrigin[5]
                     << " " << m.rescaleFactor << " " << seeds_num << " " << matches[b].matchValue << " " << matches[b].rms << " "
                     << matches[b].angle << "\n";
        }
        if (collectMatchQuality && match_quality_file.is_open()) {
          const ellc_align_quality& q = lastMatchQuality[(size_t)b];
          const double rms = q.n_used > 0 ? std::sqrt(q.sum_r2 / (double)q.n_used) : 0.0, wrms = q.sum_w != 0.0 ? std::sqrt(q.sum_wr2 / q.sum_w) : 0.0;
          match_quality_file << (testFrame.frameId + rt->BATCH_START_ID - 1) << " " << (m.frameId + rt->BATCH_START_ID - 1) << " " << q.n_depth << " "
                             << q.n_used << " " << rms << " " << wrms << "\n";
        }
        if (refineMatchSim3 && match_sim3_file.is_open()) {
          const MatchSim3& q = lastMatchSim3[(size_t)b];
          float R16[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, w6[6] = {0, 0, 0, 0, 0, 0};
          if (q.scale > 0.0 && q.scale <= (double)FLT_MAX) {   // the rotation vector of the 3x3 block over the scale
            for (int r = 0; r < 3; r++)
              for (int k = 0; k < 3; k++) R16[4 * r + k] = (float)((double)q.T[4 * r + k] / q.scale);
            ellc_se3_log(R16, w6);
          }
          match_sim3_file << (testFrame.frameId + rt->BATCH_START_ID - 1) << " " << (m.frameId + rt->BATCH_START_ID - 1) << " " << q.scale << " " << q.T[3]
                          << " " << q.T[7] << " " << q.T[11] << " " << w6[0] << " " << w6[1] << " " << w6[2] << " " << q.rec.n_photo << " "
                          << q.rec.n_depth << " " << q.rec.chi2_photo << " " << q.rec.chi2_depth << " " << q.iters;
          if (matchAffineLight) match_sim3_file << " " << q.gain << " " << q.offset;
          match_sim3_file << "\n";
        }
        if (collectMatchGeometry && match_geometry_file.is_open()) {
          const MatchGeometry& q = lastMatchGeometry[(size_t)b];
          const double mean_chi2 = q.rec.n_weighted > 0 ? q.rec.sum_chi2 / (double)q.rec.n_weighted : 0.0;
          const double mean_abs_di = q.rec.n_overlap > 0 ? (double)q.rec.sum_abs_di / (double)q.rec.n_overlap : 0.0;
          match_geometry_file << (testFrame.frameId + rt->BATCH_START_ID - 1) << " " << (m.frameId + rt->BATCH_START_ID - 1) << " " << q.rec.n_kept << " "
                              << q.rec.n_in_view << " " << q.rec.n_overlap << " " << q.rec.n_agree << " " << q.rec.n_in_front << " " << q.rec.n_behind
                              << " " << q.scale << " " << mean_chi2 << " " << mean_abs_di << "\n";
        }
      }
      match_file.flush();
      if (match_quality_file.is_open()) match_quality_file.flush();
      if (match_sim3_file.is_open()) match_sim3_file.flush();
      if (match_geometry_file.is_open()) match_geometry_file.flush();
    }
    // :614-641
    currentArrayId++;
    nextArrayId++;
    if (currentArrayId == match_window_end + 2) { match_window_beg++; match_window_end++; }
    if (currentArrayId == 1 && match_window_end == RING - 1) { match_window_beg++; match_window_end = 0; }
    if (currentArrayId == RING) currentArrayId = 0;
    if (nextArrayId == RING) nextArrayId = 0;
    if (match_window_end == RING) match_window_end = 0;
    if (match_window_beg == RING) match_window_beg = 0;
  }
};

// Points as a binary little-endian PLY: x y z float, intensity uchar, var float (17 bytes a vertex). Host-only.
inline void write_ply(const std::string& path, const std::vector<ellc_map_point>& points) {
  std::ofstream f(path.c_str(), std::ios::binary);
  if (!f) throw std::runtime_error("write_ply: cannot open " + path);
  f << "ply\nformat binary_little_endian 1.0\nelement vertex " << points.size()
    << "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar intensity\nproperty float var\nend_header\n";
  std::vector<char> buf(points.size() * 17);
  for (size_t i = 0; i < points.size(); i++) {   // (the hosts this library runs on are little-endian)
    char* r = &buf[i * 17];
    std::memcpy(r, &points[i].x, 12);
    r[12] = (char)points[i].intensity;
    std::memcpy(r + 13, &points[i].var, 4);
  }
  f.write(buf.data(), (std::streamsize)buf.size());
  if (!f) throw std::runtime_error("write_ply: cannot write " + path);
}

// A float plane as a little-endian greyscale PFM ("Pf", scale -1.0); PFM stores its scanlines bottom to top. Host-only.
inline void write_pfm(const std::string& path, const std::vector<float>& plane, int cols, int rows) {
  if (plane.size() != (size_t)cols * rows) throw std::runtime_error("write_pfm: plane size");
  std::ofstream f(path.c_str(), std::ios::binary);
  if (!f) throw std::runtime_error("write_pfm: cannot open " + path);
  f << "Pf\n" << cols << " " << rows << "\n-1.0\n";
  for (int y = rows - 1; y >= 0; y--) f.write((const char*)&plane[(size_t)y * cols], (std::streamsize)cols * 4);   // (little-endian hosts)
  if (!f) throw std::runtime_error("write_pfm: cannot write " + path);
}

}  // namespace ellc
#endif
