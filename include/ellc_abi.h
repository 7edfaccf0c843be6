/*
 * ellc_abi.h — C ABI of libellc_hip.so, the MI355X (gfx950) implementation of ELLC's per-keyframe
 * data-parallel hot path: pyramidal direct image alignment (Gauss-Newton on se(3)) and the semi-dense
 * inverse-depth map update.
 *
 * The reference has no plugin/FFI layer: the seam is the C++ object API that main.cpp and
 * GlobalOptimize.cpp call (frame, PixelWisePyramid, depthMap, GetImagePoseEstimate).  Each entry point
 * below names the reference member(s) it replaces (file:line under the reference's src/).  The C++
 * facade with the reference's own class/method names lives in ellc_facade.hpp and calls only this ABI.
 *
 * Conventions
 *   - every function returns an ellc_status (0 = ok, negative = error); numeric degeneracy is not an
 *     error (singular 6x6 H => zero update, as cv::Mat::inv returns zeros, PixelWisePyramid.cpp:451).
 *   - all pointers are HOST pointers unless the parameter name ends in _dev.
 *   - pose = 6 f32 [wx wy wz vx vy vz] (rotation first, PixelWisePyramid.cpp:153).
 *   - images are u8 row-major W x H; depth / variance / weights are f32 row-major.
 *   - a context owns its HIP streams (one, plus one per extra batch in flight: ellc_align_enqueue) and behaves as one
 *     in-order queue; calls on one context are serialised by the caller, calls on different contexts are independent
 *     and may come from different threads (the reference's loop-closure thread, GlobalOptimize.cpp:241).
 */
#ifndef ELLC_ABI_H
#define ELLC_ABI_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ELLC_MAX_LEVELS 8
#define ELLC_ABI_VERSION 24   /* ellc_depth_absorb_keyframes_lit, ellc_depth_restart_from_keyframes_lit, ellc_keyframe_trial_propagate_lit, ellc_trial_light_solve; 23: ellc_keyframe_joint_step, ellc_joint_solve, ellc_keyframe_joint_apply, ellc_keyframe_joint_refine, ellc_joint_default_params; 22: ellc_keyframe_cull_depth, ellc_cull_default_params; 21: ellc_keyframe_sweep_depth, ellc_sweep_default_params; 20: ellc_keyframe_refine_depth, ellc_refine_default_params, ellc_sim3_invert; 19: ellc_keyframe_light_step, ellc_keyframe_sim3_step_lit, ellc_keyframe_sim3_align_lit, ellc_light_solve; 18: ellc_keyframe_trial_propagate, ellc_depth_restart_from_keyframes; 17: ellc_depth_absorb_keyframes; 16: ellc_keyframe_fuse_depth; 15: ellc_keyframe_sim3_step, ellc_keyframe_sim3_align; 14: ellc_keyframe_depth_consistency; 13: ellc_keyframe_render_depth; 12: ellc_keyframe_map_points; 11: ellc_align_quality_at; 10 (r06): measurement hooks and self-tests moved out (ellc_abi_diag.h) */

typedef enum {
  ELLC_OK = 0,
  ELLC_ERR_BAD_ARG = -1,
  ELLC_ERR_HIP = -2,
  ELLC_ERR_NOT_READY = -3,   /* slot never uploaded, depth map not initialised, ... */
  ELLC_ERR_NO_DEVICE = -4,
  ELLC_ERR_CAPACITY = -5
} ellc_status;

typedef enum {
  ELLC_MODE_FCA = 0,  /* forward-compositional, per-iteration weights: calculatePixelWiseParallel, PixelWisePyramid.cpp:416-455 */
  ELLC_MODE_ICA = 1   /* constant saved weights, template gradient: calculatePixelWiseParallelInvCompositional, :917-974 */
} ellc_mode;

typedef enum {
  ELLC_ARITH_EXACT = 0, /* every per-pixel value is computed with the reference's expression order in IEEE f32 (f64 where its
                         * pow() promotes): bit-identical to the CPU path per pixel; only the order of the 27 sums differs */
  ELLC_ARITH_FAST = 1   /* tolerance mode: fused multiply-adds, hardware reciprocal / rsqrt (1 ulp) for the divisions and the
                         * sqrt, f32 for the double-promoted Jacobian terms, the 6x6 system solved by L D L^T in double, the
                         * pose carried as exp(pose) through the schedule. Per-pixel values agree with EXACT to a few 1e-7
                         * relative, the final pose to <= 1e-5 (tests/test_gpu_fast.py); about half the instructions per pixel.
                         * Requires width, height <= 4096. */
} ellc_arith;

/* Run-time form of the compile-time constants in ExternVariable.h:39-59 and main.cpp:34. */
typedef struct {
  int width, height;            /* ORIG_COLS, ORIG_ROWS */
  int levels;                   /* MAX_PYRAMID_LEVEL (reference: 4) */
  float fx, fy, cx, cy;         /* ORIG_FX, ORIG_FY, ORIG_CX, ORIG_CY */
  int max_iter[ELLC_MAX_LEVELS];/* util::MAX_ITER, index = pyramid level (0 = finest) */
  int early_exit;               /* 1: stop a level when weightedPose < 1 (ImageFunc.cpp:251-252) */
  int max_keyframes;            /* keyframe (reference-side) slots resident in HBM */
  int max_frames;               /* current-frame slots resident in HBM */
  int max_batch;                /* largest B accepted by ellc_align */
  int device;                   /* HIP device ordinal */
  int concurrent_batches;       /* 1..16: how many batches the caller keeps in flight (ellc_align_enqueue); > 1 sizes the
                                 * fine-level grids for sharing the device. Fixed per context, so a batch's result does
                                 * not depend on what else happens to be in flight (the grid fixes the summation order) */
  int arith;                    /* ELLC_ARITH_EXACT (default) or ELLC_ARITH_FAST: arithmetic of the Gauss-Newton pixel pass and solve */
  int coalesce;                 /* 1 (default) .. 4: full batches (B = max_batch) enqueued one after the other are launched side by
                                 * side, up to this many per launch sequence, and 4 x coalesce batches may be in flight. Fixed per
                                 * context: a full batch's grids are those of a full group whether it runs alone or not, so its
                                 * result does not depend on what it was launched with */
  int cache_records;            /* 0 (default): the compact pixel lists of a batch's keyframes are rebuilt by every call, as the
                                 * reference recomputes its masks per alignment (ImageFunc.cpp:158). 1: they are kept with the
                                 * keyframe slot and rebuilt only after the slot's image, depth or weights have changed (every
                                 * entry point that writes them marks the slot); batches that only READ a slot's lists then also
                                 * run concurrently instead of one after the other. Results are identical either way */
  int grid_batch;               /* 0 (default): the launch grids — which fix the order of the 27 sums, i.e. the last bits of a result —
                                 * are chosen for the size of each call's batch. N > 0: for a batch of N, whatever a call's B is.
                                 * A rank that aligns its block of a sharded loop-closure batch (ellc_shard_range) sets the same N on
                                 * every rank (e.g. max_batch): every alignment's result is then bit-identical to what ONE context
                                 * with the same N computes for the whole batch, for every world size (such a context always runs
                                 * the level-bound schedule, also for one or two alignments) */
} ellc_config;

typedef struct ellc_ctx ellc_ctx;

/* ---- lifetime ------------------------------------------------------------------------------------ */
int ellc_abi_version(void);
int ellc_device_count(void);                           /* HIP devices visible to the process (0: none); a launcher maps LOCAL_RANK to cfg.device with it */
void ellc_default_config(ellc_config* cfg, int width, int height, int levels);
ellc_status ellc_ctx_create(const ellc_config* cfg, ellc_ctx** out);
ellc_status ellc_ctx_destroy(ellc_ctx* ctx);
const char* ellc_last_error(const ellc_ctx* ctx);   /* human-readable text of the last failure */
ellc_status ellc_sync(ellc_ctx* ctx);               /* hipStreamSynchronize on the context stream */
/* Diagnostic counters since the context was created (v7; no reference counterpart: they make the library's two ways of waiting for a
 * batch observable to tests). out[i], i < n: ELLC_CTR_* below, 0 beyond ELLC_CTR_COUNT. */
enum {
  ELLC_CTR_POLLED = 0,        /* batches whose result records the host polled successfully (pinned memory, no event wait) */
  ELLC_CTR_POLL_TIMEOUT = 1,  /* polls that ran out (ellc_ctx_set_poll_timeout_us, default 2 ms) and fell back to the event */
  ELLC_CTR_EVENT_WAIT = 2,    /* batches waited for through their event (never polled, or after a timeout) */
  ELLC_CTR_CONTINUATION = 3,  /* continuation graphs of the state-driven early-exit schedule */
  ELLC_CTR_COUNT = 4
};
ellc_status ellc_ctx_counters(ellc_ctx* ctx, long long* out, int n);
ellc_status ellc_ctx_set_poll_timeout_us(ellc_ctx* ctx, int microseconds);
/* cfg.grid_batch for the calls that follow (v8; 0: grids follow each call's B again). The loop-closure batch of
 * globalOptimize::findMatchParallel (GlobalOptimize.cpp:454-646, call :566) has 1 .. 43 candidates, usually a handful: every rank
 * of a sharded run sets the same N — the smallest of {4, 8, 16, 43} that holds the WHOLE batch — before it aligns its block, so the
 * bits stay independent of the world size (ellc_shard_range) while a batch of three candidates no longer runs on grids sized for
 * 43. Batches in flight keep the grids they were launched with. */
ellc_status ellc_ctx_set_grid_batch(ellc_ctx* ctx, int n);
/* The list-free path for dense maps (v10). A keyframe whose level-0 depth plane was uploaded with at least nine tenths of its
 * pixels valid (ellc_keyframe_set_depth counts them) is aligned — FCA, no saved weights, every keyframe of the batch dense — by
 * kernels that read its planes directly instead of compact lists (gn_fca_dense / gn_fca_dense4 in the tolerance mode, gn_fca_dense_x
 * in the exact mode: there every per-pixel value is the list path's bit for bit). The two paths chunk the pixels differently (plane
 * index / list index), so their SUMS differ in the last bits: within the mode's tolerance (pose <= 1e-5 vs the CPU path either
 * way; measured <= 2e-6 between the paths), but NOT bit-identical — and a batch flips to the list path as soon as one of its
 * keyframes is not dense. A caller that compares runs bit for bit (world-size invariance, regression hashes) pins the choice:
 * mode 0 = automatic (default), 1 = always the lists. Batches in flight keep the path they were launched with. */
ellc_status ellc_ctx_set_dense_maps(ellc_ctx* ctx, int mode);
/* How the state-driven schedule (early exit on, one or two alignments per call: the tracking call, main.cpp:330) reaches the device
 * (r05, ABI v9). 1 (default): as ONE resident launch whenever the call finds the context's pipeline empty (with other batches of
 * the context in flight: as mode 0, so that their launches keep overlapping) — the level's blocks stay on the device for the whole
 * schedule and hand their partial sums to each other through tagged records in device memory (gn_fca_persist); a launch whose blocks do not all
 * become resident within ~50 ms (a device shared with more such launches than it holds) is abandoned and the schedule finished with
 * ordinary launches, with the same results as mode 0 from the iteration it had reached. 0: one launch per iteration (as up to
 * ABI v8). 2: test hook — every resident launch is abandoned at its first hand-over. Takes effect with the next call; ends the
 * context's adaptive hint. */
ellc_status ellc_ctx_set_persistent_schedule(ellc_ctx* ctx, int mode);
void* ellc_stream(ellc_ctx* ctx);                   /* the context's hipStream_t (for event timing by callers) */

/* ---- frame side: frame::frame / constructImagePyramids / calculateGradient / buildMaxGradients
 *      (Frame.cpp:78-124, 170-182, 185-285, 618-674) -------------------------------------------------- */
/* Upload a W x H u8 image into a current-frame slot; builds the u8 pyramid on device (cv::pyrDown). */
ellc_status ellc_frame_upload(ellc_ctx* ctx, int slot, const uint8_t* image);
/* Frame ingest as a device pre-pass (frame::frame(VideoCapture), Frame.cpp:45-75, after the decode): BGR 8-bit frame of
 * orig_w x orig_h (= 4 x the context size: DIM_FACTOR, ExternVariable.h:41-43) -> cvtColor BGR2GRAY -> undistort with the
 * 5-coefficient model {k1,k2,p1,p2,k3} and the alpha=0 getOptimalNewCameraMatrix (FLAG_DO_UNDISTORTION, :58-72) -> resize by
 * 1/4 (INTER_LINEAR) -> level 0 of frame slot `slot` + pyramid. fx..cy are the FULL-size intrinsics the reference builds
 * cam_K from (ORIG_FX*INTRINSIC_FACTOR ..., :61). configure builds the fixed-point map once; new_camera4 (optional)
 * receives {fx,fy,cx,cy} of the new camera matrix. The probes (optional, tests) receive the grey value of source pixel
 * (4x+1, 4y+1) [W*H] and the four undistorted source pixels of every output pixel [W*H*4]. */
ellc_status ellc_ingest_configure(ellc_ctx* ctx, int orig_w, int orig_h, float fx, float fy, float cx, float cy,
                                  const float* dist5, int do_undistort, float* new_camera4);
ellc_status ellc_frame_ingest_bgr(ellc_ctx* ctx, int slot, const uint8_t* bgr, uint8_t* gray_probe, uint8_t* undistorted_probe);
/* Same for a keyframe slot (the reference-side / template frame of an alignment). Also builds
 * maxAbsGradient (level 0). */
ellc_status ellc_keyframe_upload(ellc_ctx* ctx, int slot, const uint8_t* image);
/* Copy a frame slot's pyramid into a keyframe slot on device (depthMap::createKeyFrame makes the tracked
 * frame the next keyframe, DepthPropagation.cpp:1772). */
ellc_status ellc_keyframe_from_frame(ellc_ctx* ctx, int kf_slot, int frame_slot);
/* Read back pyramid level `level` of a slot (is_keyframe selects the slot table). out holds
 * stored_w*stored_h bytes; stored sizes follow pyrDown's ceil rule. Any size pointer may be NULL. */
ellc_status ellc_get_image_level(ellc_ctx* ctx, int is_keyframe, int slot, int level, uint8_t* out,
                                 int* stored_w, int* stored_h, int* cols, int* rows);
/* frame::calculateGradient at `level` (Frame.cpp:185-285): gx, gy each rows*cols f32. */
ellc_status ellc_get_gradient(ellc_ctx* ctx, int is_keyframe, int slot, int level, float* gx, float* gy);
/* frame::buildMaxGradients (Frame.cpp:618-674): W*H f32 and the count of pixels >= MIN_ABS_GRAD_DECREASE. */
ellc_status ellc_get_max_gradient(ellc_ctx* ctx, int is_keyframe, int slot, float* out, int* n_substantial);

/* ---- keyframe depth / variance / weights pyramids -------------------------------------------------- */
/* keyFrame->depth (0 = no hypothesis) and depthMap::depthvararrpyr0 (-1 = none), W*H f32 each; builds
 * levels 1.. on device as depthMap::buildInvVarDepth + mapDepthArr2Mat do (DepthPropagation.cpp:1637-1746). */
ellc_status ellc_keyframe_set_depth(ellc_ctx* ctx, int slot, const float* depth0, const float* var0);
/* Explicit per-level override: frame::depth_pyramid[level] and depthMap::depthvararrptr[level]. */
ellc_status ellc_keyframe_set_depth_level(ellc_ctx* ctx, int slot, int level, const float* depth, const float* var);
ellc_status ellc_keyframe_get_depth_level(ellc_ctx* ctx, int slot, int level, float* depth, float* var);
/* frame::weight_pyramid[level] / numWeightsAdded[level] (Frame.h:57,73). */
ellc_status ellc_keyframe_set_weights(ellc_ctx* ctx, int slot, int level, const float* weights, int num_added);
ellc_status ellc_keyframe_get_weights(ellc_ctx* ctx, int slot, int level, float* weights, int* num_added);
/* frame::finaliseWeights (Frame.cpp:678-695). */
ellc_status ellc_keyframe_finalise_weights(ellc_ctx* ctx, int slot);

/* ---- alignment: GetImagePoseEstimate (ImageFunc.cpp:49-315) ----------------------------------------
 * B independent alignments: alignment b aligns frame slot frame_slots[b] to keyframe slot kf_slots[b],
 * starting from init_pose[b] (the relative pose the reference derives at ImageFunc.cpp:106), visiting
 * levels (levels-1 .. 0) with up to max_iter[level] Gauss-Newton iterations each.
 *   mode            ELLC_MODE_FCA or ELLC_MODE_ICA (fromLoopClosure with FLAG_DO_CONST_WEIGHT_POSE_ESTIMATION)
 *   save_weights    1: add the last executed iteration's weights of every level into the keyframe's
 *                   weight_pyramid (PixelWisePyramid::saveWeights(true), :544-549; ImageFunc.cpp:280-288). The weights
 *                   are accumulated per keyframe slot, so with save_weights every alignment of the batch must use a
 *                   different keyframe slot (ELLC_ERR_BAD_ARG otherwise): the reference saves weights on the tracking
 *                   path only, one alignment at a time (ImageFunc.cpp:280)
 *   out_pose        B*6 f32 relative poses
 *   out_iters       B*levels ints: iterations executed per level (may be NULL)
 *   out_weighted    B f32: weightedPose of the last executed iteration (may be NULL)
 */
ellc_status ellc_align(ellc_ctx* ctx, int B, const int* kf_slots, const int* frame_slots, const float* init_pose,
                       int mode, int save_weights, float* out_pose, int* out_iters, float* out_weighted);
/* Asynchronous form: enqueue only. Up to THREE batches may be in flight; each runs on a stream of its own with its own
 * staging, state and result records, so batches in flight execute CONCURRENTLY on the device (the latency-bound coarse
 * iterations of one batch overlap the fine iterations of another) unless they share a keyframe slot, in which case the
 * later one is ordered after the earlier one. A fourth enqueue returns ELLC_ERR_NOT_READY.
 *   With cfg.coalesce = c > 1 the unit that runs is a GROUP: full batches (B = max_batch, same mode, no saved weights)
 * enqueued one after the other are staged side by side and launched as ONE sequence over all their alignments once c of
 * them have arrived — or as soon as the oldest of them is fetched, or any other entry point is called. A launch over 2 x 32
 * alignments costs little more than one over 32, so a caller that keeps the queue full gets more alignments per second
 * (r02: +20...35 %); up to 4 x c batches may be in flight (three groups run concurrently, a fourth is queued behind the
 * oldest). Results are per batch and do not depend on the grouping.
 *   ellc_align_fetch waits for
 * the OLDEST batch in flight only (an event) and returns its results (B must be that batch's size: ELLC_ERR_BAD_ARG
 * otherwise, the batch stays in flight); with nothing in flight it returns
 * ELLC_ERR_NOT_READY. Every other entry point is ordered after the batches in flight and before the batches enqueued
 * later, exactly as if the context had a single in-order queue: an upload into a slot a batch in flight reads takes
 * effect behind that batch.
 *   With cfg.early_exit on, an FCA call of one or two alignments (the tracking call) runs a schedule whose launch sequence is
 * as long as alignments usually need; when one needs more, ellc_align_fetch replays the remainder before it returns. Only
 * the host can start that remainder, so while such a batch is in flight a batch sharing one of its keyframe slots, and
 * every non-batch entry point, first WAITS for it on the host (results and ordering are unchanged). */
ellc_status ellc_align_enqueue(ellc_ctx* ctx, int B, const int* kf_slots, const int* frame_slots, const float* init_pose,
                               int mode, int save_weights);
ellc_status ellc_align_fetch(ellc_ctx* ctx, int B, float* out_pose, int* out_iters, float* out_weighted);

/* One Gauss-Newton iteration at one level, for parity tests (PixelWisePyramid::calculatePixelWiseParallel
 * or ...InvCompositional(iter)): returns H (6x6 row-major), b, delta = -Hinv*b, the updated pose
 * log(exp(delta)*exp(pose)) and weightedPose (:460-491). iter == 0 in ICA mode runs the precompute.
 * planes (optional, may be NULL): 10 f32 planes rows*cols each in this order: residual, weight,
 * warpedX, warpedY, J0..J5 (display_iterationres, display_weightimg, savedWarpedPointsX/Y, steepest descent). */
ellc_status ellc_gn_iterate(ellc_ctx* ctx, int kf_slot, int frame_slot, int level, int mode, int iter, const float* pose,
                            float* H36, float* b6, float* delta6, float* new_pose6, float* weighted, float* planes);

/* How well a frame fits a keyframe at a pose the caller names (v11): ONE forward-compositional pixel pass at `level`, no update. The
 * reference computes all of this in its pixel loop and keeps none of it: its own sum of the weighted squared residuals stands
 * commented out at PixelWisePyramid.cpp:357 (//sumRes += wh * w_p * rp*rp;). */
typedef struct {
  int32_t n_depth;    /* pixels of the level with depth > 0 (the mask, Frame.cpp:295-301) */
  int32_t n_used;     /* of those, pixels whose warped point gets an intensity (warpedintensity != -1, PixelWisePyramid.cpp:273) */
  double  sum_r2;     /* sum of residual^2 over the used pixels (residual: :330) */
  double  sum_abs_r;  /* sum of |residual| */
  double  sum_w;      /* sum of res_weight (:358) */
  double  sum_wr2;    /* sum of res_weight * residual^2: the reference's commented-out sumRes (:357) */
  float   H[36];      /* sum of w J^T J, row-major, exactly symmetric (:373) */
  float   b[6];       /* sum of w r J (:374) */
  float   Hinv[36];   /* cv::Mat::inv(DECOMP_LU) of H as the solve restates it; all zeros when singular (:451) */
} ellc_align_quality;
/* B evaluations: record b describes frame slot frame_slots[b] against keyframe slot kf_slots[b] at pose[b] (B*6 f32) on pyramid level
 * `level`. The quantities are always the forward-compositional ones (the per-iteration robust weight, :341-358), whatever mode the pose
 * came from, in the arithmetic of cfg.arith: per pixel the values of ellc_gn_iterate's planes. Hinv is the f32 LU in both modes. A
 * record is a function of the configuration, the level, the two slots and the pose ALONE: the grid per evaluation follows from the
 * level's size, the block sums are combined in double in a fixed order, so B, the position in the batch, cfg.grid_batch and whatever
 * else is in flight do not enter it, and a shard of a batch gives the bits of the whole batch. Evaluations of one call may share
 * slots. Synchronous, ordered like every other non-batch entry point (behind the batches in flight, before later ones); reads the
 * slots' planes only and writes nothing that belongs to a slot (no compact list, tile count, weight plane or validity mark).
 * ELLC_ERR_BAD_ARG: B < 1, B > max_batch, a slot or the level out of range, a NULL pointer; ELLC_ERR_NOT_READY: a slot never
 * uploaded, a keyframe without depth. */
ellc_status ellc_align_quality_at(ellc_ctx* ctx, int B, const int* kf_slots, const int* frame_slots, const float* pose, int level,
                                  ellc_align_quality* out);

/* The display planes PixelWisePyramid fills beside the residual and the weights in a pass at `level` with `pose`
 * (PixelWisePyramid.cpp:209-225, :275-284; the reference shows display_warpedimg, ImageFunc.cpp:277): where the keyframe has a
 * depth, display_templateimg = the current image (u8), display_2bewarpedimg = the keyframe image (u8), display_origres = their
 * difference before warping, display_warpedimg = the current image interpolated at the warped point (0 outside); 0 where
 * masked. rows*cols elements each; any pointer may be NULL. (display_iterationres, display_weightimg and the saved warped
 * points are planes 0-3 of ellc_gn_iterate.) */
ellc_status ellc_gn_display_planes(ellc_ctx* ctx, int kf_slot, int frame_slot, int level, const float* pose, uint8_t* templateimg,
                                   uint8_t* tobewarpedimg, float* warpedimg, float* origres);

/* se(3) helpers used by callers (frame::concatenateRelativePose Frame.cpp:503-530,
 * frame::concatenateOriginPose :534-562); host-side, no device work. */
void ellc_concatenate_relative_pose(const float* src_1wrt2, const float* src_2wrt3, float* dest_1wrt3);
void ellc_concatenate_origin_pose(const float* src_1wrt0, const float* src_2wrt0, float* dest_1wrt2);
void ellc_se3_exp(const float* pose6, float* T16);
void ellc_se3_log(const float* T16, float* pose6);

/* ---- loop-closure candidate selection support (globalOptimize, GlobalOptimize.cpp) -------------------------
 * calculateImageHistogram (:40-100): 256-bin histogram of the level-0 image, counts as f32 divided by their f32 sum. */
ellc_status ellc_histogram(ellc_ctx* ctx, int is_keyframe, int slot, float* hist256);
/* compareImageHistogram (:116-122) = cv::compareHist(H1, H2, CV_COMP_KL_DIV): sum p*log(p/q) over bins with |p| > DBL_EPSILON,
 * q replaced by 1e-10 when |q| <= DBL_EPSILON. Host-side. */
double ellc_kl_divergence(const float* p, const float* q, int n);
/* pushToArray deep-copies the finished keyframe and its depth map into a ring slot (:185-223): device-to-device copy of a
 * slot's pyramids (keyframe -> keyframe also copies depth / variance / weight pyramids, maxAbsGradient and weight counts). */
ellc_status ellc_copy_slot(ellc_ctx* ctx, int dst_is_keyframe, int dst_slot, int src_is_keyframe, int src_slot);
/* The same between two contexts on one device with the same width / height / levels. The reference hands its loop-closure
 * thread deep copies of the finished keyframe and depth map (new frame(*currentframe), new depthMap(*currentDepthMap),
 * GlobalOptimize.cpp:185-186) and lets it run beside tracking (:241, joined at :161): here the loop-closure ring lives in a
 * context of its own (own streams, own batches) and this call is the deep copy. Ordered on the device: the copy runs behind
 * everything enqueued on src_ctx so far, and src_ctx's later work behind the copy; the host does not wait. The caller
 * serialises it with every other call on either context. */
ellc_status ellc_copy_slot_across(ellc_ctx* dst_ctx, int dst_is_keyframe, int dst_slot, ellc_ctx* src_ctx, int src_is_keyframe, int src_slot);

/* ---- the semi-dense map as 3-D points (v12) ------------------------------------------------------------------
 * The map lives on the device: every keyframe slot holds depth and variance pyramids. The reference never hands it out — its only
 * consumer is the display code (displayColourDepthMap, DepthPropagation.cpp:1160-1250) — so this entry point has no reference
 * counterpart; the per-pixel arithmetic is the reference's back-projection. */
typedef struct {
  float    x, y, z;     /* the point in the caller's frame (T below) */
  float    var;         /* variance of the INVERSE depth at the pixel: depthMap::depthvararrptr[level] */
  uint16_t px, py;      /* the pixel on `level` (column, row) */
  uint8_t  intensity;   /* keyframe grey value at (px, py) of that level's image */
  uint8_t  support;     /* supporting 8-neighbours, 0..8 (rule below) */
  uint16_t source;      /* index b of the request inside this call */
} ellc_map_point;       /* 24 bytes, every field naturally aligned */

typedef struct {
  float max_var;        /* keep var <= max_var; <= 0: no variance test */
  int   min_support;    /* 0..8: keep support >= min_support */
  float support_k2;     /* >= 0, finite: neighbour n supports c iff (1/Zn - 1/Zc)^2 <= support_k2 * (Vc + Vn) */
  int   stride;         /* >= 1: keep only pixels with px % stride == 0 and py % stride == 0 */
} ellc_map_filter;

/* B requests: request b exports keyframe slot kf_slots[b] on pyramid level `level` from the slot's depth, variance and image planes of
 * that level; slots may repeat within a call. T = T12 + 12 * b is a row-major 3x4 f32 that takes the keyframe's camera coordinates
 * into the caller's frame (a caller folds any scale into the 3x3 block).
 *   A pixel is OK iff Z > 0 && Z <= FLT_MAX && V >= 0 (NaN fails all three; updateDepthImage writes 1 / invDepthSmoothed for any
 * invDepthSmoothed >= -0.05, DepthPropagation.cpp:1285-1289, so +inf and negative depths do occur). Its SUPPORT counts the
 * 8-neighbours that lie inside cols x rows of the level, are ok and satisfy (1/Zn - 1/Zc)^2 <= support_k2 * (Vc + Vn) — always the
 * level's full-resolution neighbourhood, whatever `stride` is, and always computed. A pixel is KEPT iff it is ok, px % stride == 0 and
 * py % stride == 0, max_var <= 0 || V <= max_var, and support >= min_support.
 *   The point of a kept pixel, in the reference's order (PixelWisePyramid.cpp:236-238, :244): X = ((px - cx) * Z) / fx,
 * Y = ((py - cy) * Z) / fy with the level's intrinsics (float)((double)fx / 2^level), then x = ((T[0]*X + T[1]*Y) + T[2]*Z) + T[3],
 * rows 1 and 2 likewise. All of it is IEEE f32 with correctly rounded divisions (1/Z too) and no contraction: a record is a function
 * of the configuration's intrinsics, the level, the slot's three planes, T and the filter ALONE — cfg.arith, cfg.grid_batch, B and
 * whatever else is in flight do not enter it. Coordinates that overflow f32 are the caller's business.
 *   Records come request-major, in raster order within a request. counts[b] (may be NULL) receives the number of points of request b,
 * *total (may be NULL) their sum. out == NULL is the sizing call: only counts and total are produced and capacity is ignored.
 * Otherwise, if the sum exceeds capacity the call returns ELLC_ERR_CAPACITY, nothing is written to out, counts and total are still
 * filled; on success exactly *total records are written.
 *   Synchronous, ordered like every other non-batch entry point (behind the batches in flight, before later ones). Reads the slots'
 * planes only and writes nothing that belongs to a slot (no tile count, list count, compact list, validity mark or dense hint); its
 * scratch is its own, allocated by the first call.
 * ELLC_ERR_BAD_ARG: B < 1, B > max_keyframes (or > 65535, or B x the pixels of the level beyond INT_MAX: the total is an int), a slot
 * or the level out of range, kf_slots, T12 or filter NULL, capacity < 0 with out non-NULL, min_support outside 0..8, stride < 1,
 * support_k2 negative or not finite, max_var NaN;
 * ELLC_ERR_NOT_READY: a slot without image or depth. */
ellc_status ellc_keyframe_map_points(ellc_ctx* ctx, int B, const int* kf_slots, const float* T12, int level,
                                     const ellc_map_filter* filter, ellc_map_point* out, int capacity, int* counts, int* total);

/* ---- the map rendered into a view (v13) -----------------------------------------------------------------------
 * A forward splat of B keyframe slots into ONE camera view: the depth and variance a frame at that view would be predicted to have.
 * Request b reads keyframe slot kf_slots[b] on pyramid level `level`; slots may repeat. T = T12 + 12 * b is a row-major 3x4 f32 that
 * takes the keyframe's camera coordinates into the VIEW's camera coordinates. The view has the context's camera at `level` (the
 * level's intrinsics (float)((double)fx / 2^level), as above).
 *   A source pixel takes part iff ellc_keyframe_map_points would KEEP it under `filter` (ok, stride, max_var, support — the rule above).
 * The CANDIDATE of a kept pixel (px, py, Z, V), all IEEE f32 in this order, no contraction, correctly rounded divisions:
 *   X, Y and P' = (x', y', z') as the point of ellc_keyframe_map_points (PixelWisePyramid.cpp:236-244);
 *   dropped unless z' > 0 && z' <= FLT_MAX;
 *   nid = 1 / z';  u = (x' * nid) * fx + cx;  v = (y' * nid) * fy + cy  (DepthPropagation.cpp:1050-1054);  ux = u + 0.5f;  vy = v + 0.5f;
 *   dropped unless ux >= 0 && ux < (float)cols && vy >= 0 && vy < (float)rows (NaN fails); the target is ((int)ux, (int)vy) (:1065);
 *   r = nid / (1 / Z);  r *= r;  r *= r;  nvar = r * V  (:1082-1086, applied to the variance);  dropped unless nvar >= 0 && nvar <= FLT_MAX.
 * The WINNER of a target is the candidate with the smallest 64-bit key (bits(z') << 32) | (b << 24) | i, i the source pixel's raster
 * index on the level: the nearest surface wins, exact ties go to the lower request, then to the lower raster index. Candidates are
 * not fused (the merge of :1124-1148 is not applied) and there is no photometric gate (:1066-1076). agree[target] counts the
 * candidates of that target, the winner included, for which d = nid - nid_winner satisfies d * d <= agree_k2 * (nvar + nvar_winner).
 *   Outputs are host pointers, dense cols x rows of the level, each may be NULL:
 *     depth      z' of the winner                                   0 without a winner
 *     var        nvar of the winner                                 -1
 *     source     (b << 24) | i of the winner                        -1
 *     agree      the count above (>= 1)                             0
 *     intensity  the winner's grey value on that level's image      0
 * (0 / -1 are what ellc_keyframe_set_depth takes for "no hypothesis".) *n_valid (may be NULL) receives the number of targets with a
 * winner. A result is a function of the intrinsics, the level, the slots' three planes, the T's, the filter and agree_k2 ALONE:
 * cfg.arith, cfg.grid_batch and whatever else is in flight do not enter it, and it does not depend on the order candidates arrive in.
 *   dst_kf_slot == -1: nothing is written to any slot. dst_kf_slot >= 0 (level 0 only, not among kf_slots): afterwards the slot is in
 * every respect what ellc_keyframe_set_depth(ctx, dst_kf_slot, depth, var) with the planes this call returns would leave — pyramid
 * levels, invalidated records, validity mark, dense hint, reciprocal planes — without the planes travelling to the host and back.
 *   Synchronous, ordered like every other non-batch entry point; its scratch is its own, allocated by the first call. A refused call
 * changes nothing.
 * ELLC_ERR_BAD_ARG: B < 1, B > max_keyframes, B > 256, a slot or the level out of range, more than 2^24 pixels on the level, kf_slots,
 * T12 or filter NULL, the filter errors of ellc_keyframe_map_points, agree_k2 negative or not finite, dst_kf_slot < -1 or >=
 * max_keyframes, a destination with level != 0, a destination that is also a source;
 * ELLC_ERR_NOT_READY: a source slot without image or depth. */
ellc_status ellc_keyframe_render_depth(ellc_ctx* ctx, int B, const int* kf_slots, const float* T12, int level,
                                       const ellc_map_filter* filter, float agree_k2, int dst_kf_slot,
                                       float* depth, float* var, int32_t* source, int32_t* agree, uint8_t* intensity,
                                       int* n_valid);

/* ---- the maps fused in a view (v16) ---------------------------------------------------------------------------
 * ellc_keyframe_render_depth with the candidates that agree with a target's winner MERGED into it: the EKF-style merge the reference
 * applies when it propagates a map (DepthPropagation.cpp:1124-1148, behind the occlusion test of :1090-1107), in a fixed order, so
 * that the result stays a function of the inputs alone. The arguments are the render's, with max_merge (0 .. ELLC_FUSE_MAX_MERGE), the
 * `merged` plane and n_fused added. Once a loop closure's Sim(3) is known, this is how the candidates' hypotheses tighten a keyframe's map.
 *   1. Candidates and winner. A kept source pixel, its candidate (target, z', nid, nvar) and the winner of a target are exactly
 *      ellc_keyframe_render_depth's: for the same arguments source, agree, intensity and *n_valid are byte for byte the render's.
 *   2. Members. The MEMBERS of a target are its candidates other than the winner that agree with the winner in the render's sense: with
 *      d = nid - nid_w, d * d <= agree_k2 * (nvar + nvar_w), taken against the winner's own, unmerged values (membership does not depend
 *      on the merge). Members are ordered by ascending 32-bit id (b << 24) | i: the request first, then the source's raster index. Only
 *      the first max_merge members in that order are VISITED; agree - 1 > max_merge tells a caller that a target was truncated.
 *   3. Merge. All IEEE f32 in this order, no contraction, correctly rounded divisions (:1128, :1129, :1139). The state starts at
 *      id_t = nid_w, var_t = nvar_w, m = 1. For each visited member (nid, nvar):  s = var_t + nvar;  a member with
 *      !(s > 0 && s <= FLT_MAX) is skipped: it changes nothing and is not counted;  otherwise  w = nvar / s;
 *      id_t = (w * id_t) + ((1.0f - w) * nid);  var_t = 1.0f / ((1.0f / var_t) + (1.0f / nvar)) with the old var_t;  m += 1.
 *      A zero variance on one side goes through IEEE infinities to a fused variance of 0.
 *   4. Outputs: host pointers, dense cols x rows of the level, each may be NULL, as the render's, and
 *        merged     m                                                  0 without a winner
 *      (a target has a winner iff its depth is > 0; source is a negative int32 from request 128 on, as in the render)
 *      Where m == 1, depth and var are the winner's z' and nvar, bit for bit the render's; where m >= 2, depth = 1.0f / id_t and
 *      var = var_t (a fused inverse depth so small that its reciprocal overflows f32 is the caller's business; no NaN can arise:
 *      0 <= w <= 1 and every term is non-negative). Targets without a winner hold 0 / -1 / -1 / 0 / 0 / 0. *n_fused (may be NULL)
 *      receives the number of targets with merged >= 2. With max_merge == 0 the call returns the render's five planes, byte for byte.
 *   5. A result is a function of the intrinsics, the level, the slots' three planes, the T's, the filter, agree_k2 and max_merge
 *      ALONE: cfg.arith, cfg.grid_batch, whatever else is in flight and the order candidates arrive in do not enter it, and a second
 *      call gives the same bytes (no floating-point atomics: every target merges its members itself, in the order above).
 *   6. dst_kf_slot as in the render (level 0 only, -1 for none: afterwards the slot is what ellc_keyframe_set_depth with the returned
 *      depth and var would leave), with one difference: the destination MAY be one of the sources. Fusing loop-closure candidates into
 *      a keyframe's own map is the main use: request 0 is the keyframe itself at the identity, the others are the candidates at their
 *      refined Sim(3). Every kernel has read the slots before the planes are copied into the destination, in stream order.
 *   7. Synchronous, ordered like every other non-batch entry point; a refused call changes nothing. Its scratch (the render's, and of its own a
 *      bit per source pixel of every request and a list of 4 bytes per agreeing candidate) is allocated by the first call and grown by
 *      the largest.
 * ELLC_ERR_BAD_ARG, ELLC_ERR_NOT_READY: as ellc_keyframe_render_depth, except that a destination among the sources is no error; also
 * ELLC_ERR_BAD_ARG for max_merge outside 0 .. ELLC_FUSE_MAX_MERGE;
 * ELLC_ERR_CAPACITY: the candidates that agree (the sum of the agree plane) exceed 2^31 - 1; nothing has been changed. */
#define ELLC_FUSE_MAX_MERGE 64
ellc_status ellc_keyframe_fuse_depth(ellc_ctx* ctx, int B, const int* kf_slots, const float* T12, int level,
                                     const ellc_map_filter* filter, float agree_k2, int max_merge, int dst_kf_slot,
                                     float* depth, float* var, int32_t* source, int32_t* agree, int32_t* merged,
                                     uint8_t* intensity, int* n_valid, int* n_fused);

/* ---- keyframe maps folded into the live depth map (v17) ----------------------------------------------------------
 * Everything above ends in planes of a keyframe slot. This call reaches the hypothesis STATE the depth map refines (the seven planes of
 * ellc_depth_set_state): depthMap::propagateDepth's per-hypothesis rule (DepthPropagation.cpp:1003-1157) from B keyframe slots, each at
 * a transform of its own, into the live map - without propagateDepth's wipe of the destination, and in a fixed order. The destination
 * is the context's depth map and its keyframe slot K (ellc_depth_set_keyframe), level 0 only. Request b reads keyframe slot kf_slots[b]
 * at level 0 (depth Z, variance V, the image); T = T12 + 12 * b takes that slot's camera coordinates into K's (a caller folds a Sim(3)'s
 * scale into all twelve entries). Slots may repeat, and K itself may be among them. Every operation is IEEE f32 in the stated order, no
 * contraction, correctly rounded divisions.
 *   1. A source pixel takes part iff ellc_keyframe_map_points would KEEP it under `filter` (n_kept).
 *   2. Its candidate (target, z', nid, u, v, nvar) is ellc_keyframe_render_depth's, with the same drops (n_in_view).
 *   3. Interior bound (:1059): dropped unless u > 2.1f && v > 2.1f && u < (float)cols - 3.1f && v < (float)rows - 3.1f (n_interior).
 *   4. Photometric gate (:1066-1076), only with photo_gate == 1. g is K's maxAbsGradient (the plane of ellc_get_max_gradient) at the
 *      TARGET pixel - the reference reads it at the SOURCE's coordinates (a quirk its propagation is held to elsewhere); this call has no
 *      reference output to match and reads it where it belongs. Iw is the bilinear value of K's level-0 image at (u, v) by the formulas
 *      of ellc_keyframe_sim3_step step 3 (x0 = (int)u, ax, dx0, top, bot, Iw = top + ay * (bot - top); the four taps exist because of
 *      step 3 above), Is the source's grey value, r = Iw - Is. Dropped iff (r * r) / (1600.0f + (0.25f * g) * g) > 1.0f || g < 5.0f
 *      (MAX_DIFF_CONSTANT, MAX_DIFF_GRAD_MULT, MIN_ABS_GRAD_DECREASE). The survivors of 1-4 are the CANDIDATES (n_candidates).
 *   5. Fold. A target's candidates are taken in ascending 32-bit id (b << 24) | i; only the first max_fold are VISITED (a target with
 *      more is counted in targets_truncated). The state of a target starts as the live hypothesis: valid = isValid != 0, id = invDepth,
 *      var = variance, val = validity_counter. Each visited candidate (nid, nvar) ends in exactly one of five outcomes:
 *        target valid, conflict - with d = nid - id, !(d * d <= agree_k2 * (nvar + var)), so a NaN is a conflict:
 *          d < 0: OCCLUDED, changes nothing (:1096-1099);  otherwise REPLACED: id = nid, var = nvar, val = src_validity (:1101-1121);
 *        target valid, agreeing - with s = var + nvar:  SKIPPED iff !(s > 0 && s <= FLT_MAX) (the fusion's rule);  otherwise MERGED:
 *          w = nvar / s;  id = (w * id) + ((1.0f - w) * nid);  var = 1.0f / ((1.0f / var) + (1.0f / nvar)) with the old var;
 *          val = min(val + src_validity, 255) (:1128-1140);
 *        target not valid - CREATED: id = nid, var = nvar, val = src_validity, valid = true.
 *      A target with at least one created, replaced or merged candidate is TOUCHED: invDepth = id, variance = var, validity_counter = val,
 *      isValid = 1, blacklisted = 0, invDepthSmoothed = varianceSmoothed = -1.0f (:1112-1118, :1138-1145). Every other hypothesis keeps
 *      every byte.
 *   6. Stats: n_visited == n_created + n_merged + n_replaced + n_occluded + n_skipped; targets_hit counts the targets with at least one
 *      candidate; n_valid_before / n_valid_after count isValid around the fold, before `finalise`.
 *   7. finalise == 1: afterwards the state and K's planes are, bit for bit, what the same call with finalise == 0 followed by
 *      ellc_depth_do_regularization(ctx, 0) and ellc_depth_update_depth_image(ctx) leaves. With finalise == 0 the smoothed fields of
 *      touched targets are -1, as after propagateDepth: the caller MUST regularise before anything observes or exports the map.
 *   8. Whatever ellc_depth_set_state leaves for the rest of the library, this call leaves too: ellc_depth_seeds and ellc_track_frame count
 *      and read the state as it then stands.
 *   9. The result is a function of the intrinsics, the sources' three planes, K's image and maxAbsGradient, the state, the T's, the
 *      filter and the parameters ALONE: cfg.arith, cfg.grid_batch, whatever else is in flight and the order candidates arrive in do not
 *      enter it, and a second call on the same inputs gives the same bytes (no floating-point atomics: every target folds its
 *      candidates itself, in the order above).
 *  10. Synchronous, ordered like every other non-batch entry point. A refused call changes nothing and writes nothing to `out`.
 * ELLC_ERR_BAD_ARG: B < 1, B > max_keyframes, B > 256, a slot out of range, more than 2^24 pixels, kf_slots, T12, filter or params NULL,
 * the filter errors of ellc_keyframe_map_points, agree_k2 negative or not finite, max_fold outside 1 .. ELLC_FUSE_MAX_MERGE, src_validity
 * outside 0..255, photo_gate or finalise outside 0..1;
 * ELLC_ERR_NOT_READY: no depth-map keyframe or state, a source slot without image or depth;
 * ELLC_ERR_CAPACITY: more than 2^31 - 1 candidates; nothing has been changed. */
typedef struct {
  float agree_k2;     /* >= 0, finite */
  int   max_fold;     /* 1 .. ELLC_FUSE_MAX_MERGE: candidates VISITED per target */
  int   photo_gate;   /* 0 / 1: the photometric gate of :1066-1076 */
  int   src_validity; /* 0 .. 255: validity_counter a candidate carries (keyframe slots keep none) */
  int   finalise;     /* 0 / 1: behind the fold, ellc_depth_do_regularization(ctx, 0) and ellc_depth_update_depth_image(ctx) */
} ellc_absorb_params;
void ellc_absorb_default_params(ellc_absorb_params* params);   /* {1.0f, 64, 1, 20, 1}; 20 is initializeRandomly's counter */

typedef struct {      /* 16 x int32 = 64 bytes */
  int32_t n_kept, n_in_view, n_interior, n_candidates;
  int32_t n_visited, n_created, n_merged, n_replaced, n_occluded, n_skipped;
  int32_t targets_hit, targets_touched, targets_truncated;
  int32_t n_valid_before, n_valid_after, reserved;   /* reserved = 0 */
} ellc_absorb_stats;

ellc_status ellc_depth_absorb_keyframes(ellc_ctx* ctx, int B, const int* kf_slots, const float* T12, const ellc_map_filter* filter,
                                        const ellc_absorb_params* params, ellc_absorb_stats* out /* may be NULL */);

/* ---- trial propagation records and a map restart (v18) -------------------------------------------------------------
 * What a tracker that has LOST its map needs (main.cpp:252-324, GlobalOptimize.cpp:717-943): a score per candidate keyframe, and the
 * live map re-seated on a new keyframe from keyframe slots, starting empty.
 *
 * ellc_keyframe_trial_propagate answers, for B (source, destination, transform) triples in one call and without touching the live
 * map: "if this keyframe slot's map were propagated into that image at this transform, how much map would there be?" Request b reads
 * keyframe slot src_kf_slots[b] at level 0 (depth, variance, image); the destination is slot dst_slots[b], a keyframe slot if
 * dst_is_keyframe == 1 and a frame slot if 0, of which only the level-0 image is needed (no depth); T = T12 + 12 * b takes the source's
 * camera coordinates into the destination's. Slots may repeat. The rule is steps 1-4 of ellc_depth_absorb_keyframes with the
 * destination's level-0 image and maxAbsGradient plane (ellc_get_max_gradient) in the place of K's: a source pixel takes part iff
 * ellc_keyframe_map_points would keep it (n_kept); its candidate is ellc_keyframe_render_depth's, with the same drops (n_in_view); the
 * interior bound of step 3 (n_interior). For EVERY interior pixel - the four taps exist there - g is the destination's maxAbsGradient
 * at the TARGET, Iw the bilinear value of step 4 and r = Iw - Is: n_low_grad counts g < 5.0f, sum_r2 adds (double)(r * r) and
 * sum_abs_r adds (double)|r|, whether or not the gate is on. photo_gate only decides whether step 4 drops candidates: n_candidates
 * counts the survivors of steps 1-4, n_targets the DISTINCT target pixels among them.
 *   n_targets is the number of hypotheses the fold would CREATE from this request alone in an empty map: n_created == targets_hit ==
 * n_valid_after of ellc_depth_absorb_keyframes of this one request, same gate and filter, into a wiped state. 100 * n_targets / (W * H)
 * is the seeds figure before regularisation.
 *   Record b is a function of the intrinsics, the two slots' planes, T, the filter and photo_gate ALONE: the pixels are partitioned by
 * the level's size (2048-pixel tiles, 256 threads, eight pixels a thread), partial sums are combined in a fixed order in double; B,
 * the position in the batch, the other requests, cfg.arith, cfg.grid_batch and whatever else is in flight do not enter it, and a shard
 * of a batch gives the bytes of the whole batch. Distinct targets are counted through one bit per destination pixel and request in
 * device scratch (an integer atomic OR: the count does not depend on the arrival order); requests go to the device in groups whose
 * bitmaps fit 64 MB, which cannot enter a record either.
 *   Synchronous, ordered like every other non-batch entry point. Builds the destination's maxAbsGradient plane where it is not built
 * yet, as the absorb does for K, and writes nothing else that belongs to a slot. 1 <= B <= 2048 (not bounded by max_keyframes). A
 * refused call changes nothing and leaves `out` untouched.
 * ELLC_ERR_BAD_ARG: B out of range, a slot out of range, a NULL pointer, more than 2^24 pixels, the filter errors of
 * ellc_keyframe_map_points, photo_gate or dst_is_keyframe outside 0..1;
 * ELLC_ERR_NOT_READY: a source without image or depth, a destination without image. */
typedef struct {            /* 48 bytes, every field naturally aligned */
  double  sum_r2;           /* sum of (double)(r * r) over the pixels counted in n_interior */
  double  sum_abs_r;        /* sum of (double)|r| over the same pixels */
  int32_t n_kept;           /* source pixels ellc_keyframe_map_points would keep under `filter` */
  int32_t n_in_view;        /* of those, pixels with a candidate (ellc_keyframe_render_depth's rule and drops) */
  int32_t n_interior;       /* of those, inside the bound of ellc_depth_absorb_keyframes step 3 */
  int32_t n_low_grad;       /* of those, g < 5.0f (counted whether or not the gate is on) */
  int32_t n_candidates;     /* survivors of absorb's steps 1-4 with this destination in the role of K */
  int32_t n_targets;        /* DISTINCT target pixels among the candidates */
  int32_t reserved[2];      /* 0 */
} ellc_trial_propagation;

ellc_status ellc_keyframe_trial_propagate(ellc_ctx* ctx, int B, const int* src_kf_slots, int dst_is_keyframe, const int* dst_slots,
                                          const float* T12, const ellc_map_filter* filter, int photo_gate, ellc_trial_propagation* out);

/* ellc_depth_restart_from_keyframes: depthMap::createKeyFrame (DepthPropagation.cpp:1765-1782) with propagateDepth replaced by the
 * fold of ellc_depth_absorb_keyframes from B keyframe slots into an EMPTY map. new_kf_slot holds an image, is NOT among kf_slots and
 * becomes the depth map's keyframe K; T = T12 + 12 * b takes slot kf_slots[b]'s camera coordinates into new_kf_slot's. The context
 * needs no state and no depth-map keyframe beforehand: the call can START a map.
 *   1. Wipe. Every hypothesis becomes isValid = 0, blacklisted = 0, validity_counter = 0, invDepth = 0, variance = 0, both smoothed
 *      fields -1.0f (all seven fields, unlike propagateDepth's two): nothing of an earlier state, NaNs included, reaches the result.
 *   2. Fold. The B requests are folded exactly as ellc_depth_absorb_keyframes folds them (steps 1-6 there: same rule, same order, same
 *      stats; n_valid_before == 0).
 *   3. params->finalise == 0: that is all; the smoothed fields of touched targets are -1, the caller regularises, *rescale_factor = 1.
 *      finalise == 1: createKeyFrame's tail as ellc_depth_create_keyframe runs it - regularise with occlusion removal, fill + regularise,
 *      makeInvDepthOne, the export into new_kf_slot's planes; *rescale_factor (may be NULL) receives makeInvDepthOne's factor.
 *   With finalise == 1 the state, new_kf_slot's planes on every level and the factor are, bit for bit, what ellc_depth_set_keyframe(
 * new_kf_slot), ellc_depth_set_state(the wiped planes), ellc_depth_absorb_keyframes(finalise = 0), ellc_depth_regularize(1),
 * ellc_depth_fill_holes, ellc_depth_regularize(0), ellc_depth_make_inv_depth_one and ellc_depth_update_depth_image leave; with
 * finalise == 0, what the first three leave - without seven planes travelling from the host.
 *   Validation, the pass that counts the candidates and the host's read of their number all come BEFORE anything of the state or of the
 * depth map's keyframe is touched: a refused call changes nothing, ELLC_ERR_CAPACITY included. A device error part-way leaves the depth
 * map not ready, as in ellc_depth_create_keyframe. Synchronous, ordered like every other non-batch entry point.
 * ELLC_ERR_BAD_ARG: everything ellc_depth_absorb_keyframes refuses, new_kf_slot out of range or among the sources;
 * ELLC_ERR_NOT_READY: a source slot without image or depth, new_kf_slot without an image;
 * ELLC_ERR_CAPACITY: more than 2^31 - 1 candidates. */
ellc_status ellc_depth_restart_from_keyframes(ellc_ctx* ctx, int new_kf_slot, int B, const int* kf_slots, const float* T12,
                                              const ellc_map_filter* filter, const ellc_absorb_params* params,
                                              float* rescale_factor /* may be NULL */, ellc_absorb_stats* out /* may be NULL */);

/* ---- one keyframe's map against another's (v14) ------------------------------------------------------------------
 * The geometric check of a loop closure, and the scale between two maps: request b compares keyframe slot src_kf_slots[b] with slot
 * dst_kf_slots[b] on pyramid level `level`. T = T12 + 12 * b is a row-major 3x4 f32 that takes the SOURCE's camera coordinates into
 * the DESTINATION's (a caller folds a scale into all twelve entries). Source and destination may be the same slot, slots may repeat
 * across requests. Per source pixel, all arithmetic IEEE f32 in this order, no contraction, correctly rounded divisions:
 *   1. it takes part iff ellc_keyframe_map_points would KEEP it under `filter` (n_kept);
 *   2. its candidate (target, z', nid, nvar) is ellc_keyframe_render_depth's, with the same drops (n_in_view);
 *   3. at the target pixel of the destination slot's level: Zt, Vt and the grey value It (the image is read with its stored pitch);
 *   4. it overlaps iff Zt > 0 && Zt <= FLT_MAX && Vt >= 0 (n_overlap); `filter` is not applied to the destination;
 *   5. idt = 1 / Zt;  d = nid - idt;  s = nvar + Vt;
 *   6. it agrees iff d * d <= agree_k2 * s; it is in front iff it does not agree and d > 0; it is behind otherwise;
 *   7. Is is the source's grey value at the pixel; |Is - It| and its square are added as integers;
 *   8. it is weighted iff s > 0 && s <= FLT_MAX; then w = 1 / s, q = (d * d) * w, ss = (nid * nid) * w, st = (nid * idt) * w, each
 *      converted to double and added to its sum (terms that overflow f32 are the caller's business).
 * sum_w_st / sum_w_ss is the least-squares factor that takes the source's inverse depths, as seen in the destination, onto the
 * destination's: to bring the maps to one scale a caller divides all twelve entries of T by it and calls again.
 *   Record b is a function of the intrinsics, the level, the two slots' planes, T, the filter and agree_k2 ALONE: the pixels are
 * partitioned by the level's size (2048-pixel tiles), partial sums are combined in a fixed order in double; B, the position in the
 * batch, the other requests, cfg.arith, cfg.grid_batch and whatever else is in flight do not enter it, and a shard of a batch gives
 * the bytes of the whole batch.
 *   Synchronous, ordered like every other non-batch entry point. Reads planes only: nothing that belongs to a slot is written. Its
 * scratch and staging are its own, allocated by the first call and grown by the largest. 1 <= B <= 2048 (not bounded by
 * max_keyframes: all ordered pairs of a ring are one call). A refused call changes nothing and writes nothing to `out`.
 * ELLC_ERR_BAD_ARG: B out of range, a slot or the level out of range, more than 2^24 pixels on the level, a NULL pointer, the filter
 * errors of ellc_keyframe_map_points, agree_k2 negative or not finite;
 * ELLC_ERR_NOT_READY: a source or destination slot without image or depth. */
typedef struct {
  double  sum_chi2;    /* sum of (double)q over the weighted pixels */
  double  sum_w_ss;    /* sum of (double)((nid * nid) * w) */
  double  sum_w_st;    /* sum of (double)((nid * idt) * w) */
  int64_t sum_abs_di;  /* sum of |Is - It| over the overlap pixels (grey values of the level's images) */
  int64_t sum_di2;     /* sum of (Is - It)^2 over the overlap pixels */
  int32_t n_kept;      /* source pixels ellc_keyframe_map_points would keep under `filter` */
  int32_t n_in_view;   /* of those, pixels with a candidate (ellc_keyframe_render_depth's rule) */
  int32_t n_overlap;   /* of those, pixels whose target in the destination slot holds a hypothesis */
  int32_t n_agree;     /* of the overlap */
  int32_t n_in_front;  /* of the overlap: not agreeing, source surface nearer than the destination's */
  int32_t n_behind;    /* of the overlap: the rest (n_overlap == n_agree + n_in_front + n_behind, always) */
  int32_t n_weighted;  /* overlap pixels that enter the three double sums */
} ellc_depth_consistency;   /* 72 bytes, every field naturally aligned */

ellc_status ellc_keyframe_depth_consistency(ellc_ctx* ctx, int B, const int* src_kf_slots, const int* dst_kf_slots,
                                            const float* T12, int level, const ellc_map_filter* filter, float agree_k2,
                                            ellc_depth_consistency* out);

/* ---- Sim(3) refinement of a loop-closure pair (v15) ----------------------------------------------------------------
 * makeInvDepthOne rescales every keyframe's map on its own (DepthPropagation.cpp:1546-1587), so two ring keyframes never share a
 * scale; the reference states the intent (frame::calculateSim3poseOtherWrtThis, Frame.cpp:419-439; Sim3_R, Frame.h:124) and has no
 * implementation. ellc_keyframe_sim3_step gives the normal equations of ONE Gauss-Newton step over seven parameters, in the order
 * (wx, wy, wz, vx, vy, vz, sigma): rotation first, as everywhere in this interface, then translation, then the log-scale.
 * ellc_keyframe_sim3_align runs the loop. The photometric residual fixes rotation and translation, the inverse-depth residual between
 * the two maps fixes the scale and strengthens the motion along the optical axis (alone its H is singular: no entry for wz, vx, vy).
 *   Request b compares keyframe slot src_kf_slots[b] with slot dst_kf_slots[b] on pyramid level `level` at T = T12 + 12 * b, a
 * row-major 3x4 f32 that takes the SOURCE's camera coordinates into the DESTINATION's, the scale folded into the 3x3 block. Source
 * and destination may be the same slot, slots may repeat. Per source pixel, all arithmetic IEEE f32 in this order, no contraction,
 * correctly rounded divisions:
 *   1. it takes part iff ellc_keyframe_map_points would KEEP it under `filter` (n_kept);
 *   2. its point P' = (x', y', z'), nid, u, v, target and nvar are ellc_keyframe_render_depth's candidate, with the same drops
 *      (n_in_view); fx, fy are the level's intrinsics;
 *   3. PHOTOMETRIC TERM. It takes part iff u >= 0 && v >= 0 (NaN fails) and, with x0 = (int)u, y0 = (int)v, x0 + 1 < cols &&
 *      y0 + 1 < rows (n_photo). I00 = image(y0, x0), I01 = (y0, x0 + 1), I10 = (y0 + 1, x0), I11 = (y0 + 1, x0 + 1) of the destination
 *      slot's level (read with its stored pitch) and Is, the source's grey value at the pixel, are converted to f32;
 *        ax = u - (float)x0;  ay = v - (float)y0;  dx0 = I01 - I00;  dx1 = I11 - I10;
 *        top = I00 + ax * dx0;  bot = I10 + ax * dx1;  gy = bot - top;  Iw = top + ay * gy;  gx = dx0 + ay * (dx1 - dx0);
 *      (gx, gy are the exact derivatives of the bilinear interpolant Iw);  rp = Iw - Is;
 *        A = (gx * fx) * nid;  Bv = (gy * fy) * nid;  Cq = -(((A * x') + (Bv * y')) * nid);
 *        Jp = [Cq * y' - Bv * z',  A * z' - Cq * x',  Bv * x' - A * y',  A,  Bv,  Cq,  0]
 *      (each product rounded, then the difference; the projection does not see the scale: the seventh entry is structurally zero);
 *      w0 = 1 / sigma_i2 and sp = sqrtf(w0) are computed once on the host in f32;  e = |rp| * sp;  wp = w0 if e <= huber_k,
 *      otherwise wp = w0 * (huber_k / e) (n_photo_huber);  chi2_photo += (double)((rp * rp) * wp);
 *   4. DEPTH TERM. At the target pixel of the destination slot's level: Zt, Vt. It takes part iff Zt > 0 && Zt <= FLT_MAX && Vt >= 0
 *      (v14's overlap rule; `filter` is not applied to the destination), s = nvar + Vt satisfies s > 0 && s <= FLT_MAX, and, with
 *      rd = nid - 1 / Zt, rd * rd <= gate_k2 * s (n_depth); a pixel that fails the last test only is counted in n_depth_gated;
 *        wd = depth_weight * (1 / s);  a2 = nid * nid;  Jd = [-(a2 * y'),  a2 * x',  0,  0,  0,  -a2,  -nid];
 *      chi2_depth += (double)((rd * rd) * wd);
 *   5. SUMS. For either term with weight w, residual r and Jacobian J: wJ_i = w * J_i in f32, H_ij += (double)wJ_i * (double)J_j for
 *      i <= j, b_i += (double)wJ_i * (double)r. Both products are exact in double: every term is known exactly. A structurally zero
 *      entry of J contributes no term (for finite values: the exact zero it would contribute), so H[2][6], H[3][6] and H[4][6] are
 *      always 0. A step solves H xi = -b; T <- exp(xi^) * T with the generator [[w]x + sigma I, v; 0 0]. Terms that overflow f32
 *      are the caller's business.
 *   Record b is a function of the intrinsics, the level, the two slots' planes, T, the filter and the parameters ALONE: the pixels
 * are partitioned by the level's size (2048-pixel tiles), partial sums are combined in a fixed order in double; B, the position in
 * the batch, the other requests, cfg.arith, cfg.grid_batch and whatever else is in flight do not enter it.
 *   Synchronous, ordered like every other non-batch entry point. Reads planes only: nothing that belongs to a slot is written. Its
 * scratch and staging are its own, allocated by the first call and grown by the largest. 1 <= B <= 2048. A refused call changes
 * nothing and writes nothing to its outputs.
 * ELLC_ERR_BAD_ARG: the errors of ellc_keyframe_depth_consistency (B, a slot or the level out of range, more than 2^24 pixels on the
 * level, a NULL pointer, the filter errors), a parameter that is not finite, sigma_i2 <= 0, huber_k <= 0, gate_k2 < 0,
 * depth_weight < 0;  ELLC_ERR_NOT_READY: a source or destination slot without image or depth. */
typedef struct {
  float sigma_i2;      /* > 0: variance of a grey value; the photometric weight is 1 / sigma_i2 inside the Huber threshold */
  float huber_k;       /* > 0: Huber threshold on |rp| / sigma_i */
  float gate_k2;       /* >= 0: the depth term takes rd * rd <= gate_k2 * (nvar + Vt) only */
  float depth_weight;  /* >= 0: factor on the depth term's weight 1 / (nvar + Vt) */
} ellc_sim3_params;
void ellc_sim3_default_params(ellc_sim3_params* params);   /* {16, 1.345, 9, 1} */

typedef struct {
  double  H[28];          /* upper triangle of the 7 x 7, row-major: H[0][0..6], H[1][1..6], ..., H[6][6] */
  double  b[7];
  double  chi2_photo;     /* sum of (double)((rp * rp) * wp) over the photometric pixels */
  double  chi2_depth;     /* sum of (double)((rd * rd) * wd) over the depth pixels */
  int32_t n_kept;         /* source pixels ellc_keyframe_map_points would keep under `filter` */
  int32_t n_in_view;      /* of those, pixels with a candidate (ellc_keyframe_render_depth's rule) */
  int32_t n_photo;        /* of those, pixels with four taps: the photometric term */
  int32_t n_photo_huber;  /* of those, pixels beyond the Huber threshold */
  int32_t n_depth;        /* pixels in view that enter the depth term */
  int32_t n_depth_gated;  /* pixels in view whose target holds a hypothesis and a usable s, but beyond the gate */
} ellc_sim3_normal;       /* 320 bytes, every field naturally aligned */

ellc_status ellc_keyframe_sim3_step(ellc_ctx* ctx, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, int level,
                                    const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_sim3_normal* out);

/* Host only, no device work (like ellc_se3_exp). ellc_sim3_solve: L D L^T in double without pivoting on the mirrored 7 x 7 of `n`,
 * then H xi = -b. The system is singular iff some pivot fails d_i > 1e-10 * max_j H_jj (NaN fails): then xi7 is all zero and the
 * return value is 1, otherwise 0. ellc_sim3_apply: T12_out = float(exp(xi^) * T12_in) with the generator [[w]x + sigma I, v; 0 0] -
 * the exponential in double, then the product in double, then ONE rounding to f32 per entry; xi = 0 returns T12_in's bits. T12_out
 * may be T12_in. */
int  ellc_sim3_solve(const ellc_sim3_normal* n, double* xi7);
void ellc_sim3_apply(const double* xi7, const float* T12_in, float* T12_out);

/* The loop, coarse to fine over the levels level_from, level_from - 1, ..., level_to (level_from >= level_to; n_levels of them).
 * Pair b starts at T12_in + 12 * b. Per level, every pair still ACTIVE on it is evaluated at its T (ellc_keyframe_sim3_step's
 * record), solved on the host (ellc_sim3_solve) and updated, T <- ellc_sim3_apply(xi, T); a pair leaves the level when its solve is
 * singular (no update, T unchanged), when max_i |xi_i| <= eps after an update, or when it has made max_iter updates on the level.
 * Pairs that have left a level are not part of that level's later launches. After the last level one more evaluation of every pair
 * at the T it ends with fills out[b]; that T goes to T12_out + 12 * b. iters_out[b * n_levels + k] (may be NULL) receives the updates
 * pair b made on the k-th visited level. A pair's sequence of T's depends on nothing but its own inputs.
 *   trace_T12 / trace_rec (each may be NULL): for pair b, entry b * trace_capacity + e receives, in order of evaluation, the T that
 * evaluation e was made at and its record, the final one included - at most n_levels * max_iter + 1 entries; trace_capacity must be
 * at least that when either pointer is given. The entries a pair does not use are marked: twelve zeros, and a record that is all
 * zero but for n_kept = -1.
 *   Synchronous; everything else as ellc_keyframe_sim3_step, whose errors it shares. Also ELLC_ERR_BAD_ARG: level_from < level_to,
 * max_iter outside 1..64, eps negative or not finite, T12_out or out NULL, a trace_capacity too small for a given trace. A refused
 * call writes nothing. */
ellc_status ellc_keyframe_sim3_align(ellc_ctx* ctx, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12_in,
                                     int level_from, int level_to, const ellc_map_filter* filter, const ellc_sim3_params* params,
                                     int max_iter, float eps, float* T12_out, ellc_sim3_normal* out, int* iters_out,
                                     float* trace_T12, ellc_sim3_normal* trace_rec, int trace_capacity);

/* ---- affine brightness in the Sim(3) refinement (v19) --------------------------------------------------------------
 * Everything above takes a surface to have the same grey value in both keyframes. Between the two ends of a loop closure the
 * camera's exposure has usually moved. The model here is Ip = gain * Is + offset in f32 (the product rounded, then the sum: two
 * roundings, no contraction), Is the source's grey value as f32; the photometric residual becomes rp = Iw - Ip. A light of (1, 0)
 * gives Ip == Is bit for bit. A LIGHT is two f32 per pair, light[2 * b] the gain and light[2 * b + 1] the offset; a NULL light
 * means (1, 0) for every pair; a given light must be finite.
 *
 * ellc_keyframe_light_step: the normal equations of the weighted straight-line fit of Iw on Is for request b at T = T12 + 12 * b
 * and light_in, over exactly the photometric pixels of ellc_keyframe_sim3_step: rules 1 to 3 of its comment apply word for word
 * (n_kept, n_in_view, n_photo; Iw, Is). rp = Iw - Ip at light_in; e, wp and n_photo_huber as in rule 3 with that rp; of `params`
 * only sigma_i2 and huber_k are read (all four are validated). wIs = wp * Is and wIw = wp * Iw in f32; the six products below
 * are exact in double, so every term is known exactly. The record is a function of its own request alone, in the sense and by the
 * means of ellc_keyframe_sim3_step (2048-pixel tiles, fixed order, double); its scratch and staging are its own. Synchronous;
 * 1 <= B <= 2048; a refused call changes nothing and writes nothing. Errors: those of ellc_keyframe_sim3_step, and
 * ELLC_ERR_BAD_ARG for a given light with a value that is not finite. */
typedef struct {
  double  sum_w;          /* sum (double)wp */
  double  sum_w_s;        /* sum (double)wIs,             wIs = wp * Is in f32 */
  double  sum_w_t;        /* sum (double)wIw,             wIw = wp * Iw in f32 */
  double  sum_w_ss;       /* sum (double)wIs * (double)Is   (exact product) */
  double  sum_w_st;       /* sum (double)wIs * (double)Iw   (exact product) */
  double  sum_w_tt;       /* sum (double)wIw * (double)Iw   (exact product) */
  double  chi2_photo;     /* sum (double)((rp * rp) * wp) at light_in */
  int32_t n_kept, n_in_view, n_photo, n_photo_huber;   /* as in ellc_sim3_normal, n_photo_huber at light_in */
} ellc_light_normal;      /* 72 bytes, every field naturally aligned */

ellc_status ellc_keyframe_light_step(ellc_ctx* ctx, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12,
                                     const float* light_in, int level, const ellc_map_filter* filter, const ellc_sim3_params* params,
                                     ellc_light_normal* out);

/* ellc_keyframe_sim3_step with rule 3's residual replaced by rp = Iw - Ip at `light`; nothing else differs (the Jacobian is that
 * of Iw). light NULL, or (1, 0) for a pair, gives that pair the bytes of ellc_keyframe_sim3_step. Errors: those of
 * ellc_keyframe_sim3_step, and ELLC_ERR_BAD_ARG for a given light with a value that is not finite. */
ellc_status ellc_keyframe_sim3_step_lit(ellc_ctx* ctx, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12,
                                        const float* light, int level, const ellc_map_filter* filter, const ellc_sim3_params* params,
                                        ellc_sim3_normal* out);

/* Host only, no device work (like ellc_sim3_solve). The fit of one record, in double:
 *   det = sum_w * sum_w_ss - sum_w_s^2;  gain = (sum_w * sum_w_st - sum_w_s * sum_w_t) / det;
 *   offset = (sum_w_t - gain * sum_w_s) / sum_w.
 * It is ACCEPTED iff n_photo >= min_pixels, det > 1e-10 * sum_w * sum_w_ss, gain_min <= gain <= gain_max and |offset| <= 255
 * (NaN fails every test). An accepted solve rounds both values to f32 once, stores them in light_out[0..1] and returns 0; a
 * refused one stores light_in's bits and returns 1. light_in may be NULL, meaning (1, 0); light_out may be light_in. The
 * defaults are design choices: a factor of four either way is more than the histogram gate of a loop closure lets through.
 * The device entry points that take an ellc_light_params refuse (ELLC_ERR_BAD_ARG) a value that is not finite,
 * !(0 < gain_min <= 1 <= gain_max) and min_pixels outside 2..2^30; ellc_light_solve itself checks nothing. */
typedef struct {
  float   gain_min, gain_max;   /* 0 < gain_min <= 1 <= gain_max */
  int32_t min_pixels;           /* 2..2^30: photometric pixels a fit needs; 2^30 refuses every fit (at most 2^24 pixels a level) */
} ellc_light_params;            /* 12 bytes */
void ellc_light_default_params(ellc_light_params* params);   /* {0.25f, 4.0f, 16} */
int  ellc_light_solve(const ellc_light_normal* n, const ellc_light_params* params, const float* light_in, float* light_out);

/* ellc_keyframe_sim3_align's loop with the light fitted before every Gauss-Newton step. Pair b starts at T12_in + 12 * b and the
 * light light_in + 2 * b (light_in NULL: (1, 0)). ONE EVALUATION of an active pair at (T, l) is, in this order:
 *   1. the light record at (T, l)                 (ellc_keyframe_light_step);
 *   2. l' = ellc_light_solve of it with light_params and l (a refused solve keeps l);
 *   3. the Sim(3) record at (T, l')               (ellc_keyframe_sim3_step_lit);
 *   4. the trace entry: T, l', the light record, the Sim(3) record.
 * The pair carries l' on, across levels too. The solve of the Sim(3) record, the update of T, when a pair leaves a level, the
 * launches without the pairs that have left, the final evaluation (it fills out[b], light_rec_out[b], and its l' goes to
 * light_out + 2 * b) and iters_out are ellc_keyframe_sim3_align's. A pair's sequence of T's and lights depends on nothing but
 * its own inputs. With min_pixels = 2^30 (every fit refused) and light_in NULL, the T's, the Sim(3) records and the iteration
 * counts are ellc_keyframe_sim3_align's bit for bit.
 *   trace_T12 / trace_rec / trace_light / trace_light_rec (each may be NULL): as in ellc_keyframe_sim3_align, entry
 * b * trace_capacity + e; trace_light holds two f32 an entry. Unused entries: twelve zeros, two zeros, and records that are all
 * zero but for n_kept = -1. trace_capacity must be at least n_levels * max_iter + 1 when any of the four is given.
 *   light_rec_out may be NULL; T12_out, out and light_out may not. Everything is kept aside until the call has succeeded: a
 * refused or failed call writes nothing. Errors: those of ellc_keyframe_sim3_align, a light_in with a value that is not finite,
 * the refusals of ellc_light_params above, light_params or light_out NULL. */
ellc_status ellc_keyframe_sim3_align_lit(ellc_ctx* ctx, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12_in,
                                         const float* light_in, int level_from, int level_to, const ellc_map_filter* filter,
                                         const ellc_sim3_params* params, const ellc_light_params* light_params, int max_iter, float eps,
                                         float* T12_out, float* light_out, ellc_sim3_normal* out, ellc_light_normal* light_rec_out,
                                         int* iters_out, float* trace_T12, ellc_sim3_normal* trace_rec, float* trace_light,
                                         ellc_light_normal* trace_light_rec, int trace_capacity);

/* ---- affine brightness in the absorb, the trial propagation and the restart (v24) ------------------------------------
 * The light of v19 in the last link of a loop closure: the photometric gate of ellc_depth_absorb_keyframes step 4, which
 * ellc_keyframe_trial_propagate and ellc_depth_restart_from_keyframes share. light[2 * b] is the gain and light[2 * b + 1] the offset of
 * request b; they map the SOURCE's grey value into the destination's (K's, the trial's destination, the new keyframe's), the direction
 * of T = T12 + 12 * b: Ip = gain * Is + offset in f32, the product rounded, then the sum (two roundings, no contraction). ONLY the
 * residual changes: r = Iw - Ip. g, the constants 1600.0f and 0.25f and the test g < 5.0f stay in the destination's units, so a DARKER
 * destination still loses its low-gradient candidates to g < 5.0f (MIN_ABS_GRAD_DECREASE, the reference's constant): no light repairs
 * that. light NULL means (1, 0) for every request; (1, 0) gives Ip == Is bit for bit (Is >= 0). A given light with a value that is not
 * finite is ELLC_ERR_BAD_ARG.
 *
 * ellc_depth_absorb_keyframes_lit / ellc_depth_restart_from_keyframes_lit: everything of the unlit calls applies word for word - rule,
 * order, stats, refusals, finalise, "a refused call changes nothing" - with step 4's residual taken against Ip at the request's light.
 * With light NULL, or (1, 0) for a request, that request's candidates are the unlit call's; with that for every request the state
 * planes, K's planes, the sixteen counts and the factor are the unlit call's bytes. The unlit entry points run the same kernels at (1, 0). */
ellc_status ellc_depth_absorb_keyframes_lit(ellc_ctx* ctx, int B, const int* kf_slots, const float* T12, const float* light /* may be NULL */,
                                            const ellc_map_filter* filter, const ellc_absorb_params* params,
                                            ellc_absorb_stats* out /* may be NULL */);
ellc_status ellc_depth_restart_from_keyframes_lit(ellc_ctx* ctx, int new_kf_slot, int B, const int* kf_slots, const float* T12,
                                                  const float* light /* may be NULL */, const ellc_map_filter* filter,
                                                  const ellc_absorb_params* params, float* rescale_factor /* may be NULL */,
                                                  ellc_absorb_stats* out /* may be NULL */);

/* ellc_keyframe_trial_propagate_lit: ellc_keyframe_trial_propagate with r = Iw - Ip at the request's light, and the sums a caller needs
 * to FIT that light. The first 48 bytes of a record are an ellc_trial_propagation evaluated at `light`: sum_r2, sum_abs_r, the gate,
 * n_candidates and n_targets all use r = Iw - Ip; at light NULL or (1, 0) they are ellc_keyframe_trial_propagate's bytes. The five sums
 * behind them run over EVERY pixel counted in n_interior (n_fit == n_interior), with Is the source's grey value and Iw the bilinear
 * value of step 4, both f32: they do not depend on `light` or on photo_gate. Each term of sum_ss, sum_st, sum_tt is the exact double
 * product of two f32 values; the terms are added in double in the record's own fixed order and partition (no floating-point atomics).
 * A record is a function of its own request alone, as before. Its scratch and staging are its own. Errors: those of
 * ellc_keyframe_trial_propagate, and ELLC_ERR_BAD_ARG for a given light with a value that is not finite. */
typedef struct {            /* 96 bytes, every field naturally aligned */
  double  sum_r2;           /* as in ellc_trial_propagation, with r = Iw - Ip */
  double  sum_abs_r;
  int32_t n_kept, n_in_view, n_interior, n_low_grad, n_candidates, n_targets;
  int32_t reserved[2];      /* 0 */
  double  sum_s;            /* sum (double)Is over the pixels counted in n_interior */
  double  sum_t;            /* sum (double)Iw */
  double  sum_ss;           /* sum (double)Is * (double)Is   (exact product) */
  double  sum_st;           /* sum (double)Is * (double)Iw   (exact product) */
  double  sum_tt;           /* sum (double)Iw * (double)Iw   (exact product) */
  int32_t n_fit;            /* == n_interior */
  int32_t reserved2;        /* 0 */
} ellc_trial_propagation_lit;

ellc_status ellc_keyframe_trial_propagate_lit(ellc_ctx* ctx, int B, const int* src_kf_slots, int dst_is_keyframe, const int* dst_slots,
                                              const float* T12, const float* light /* may be NULL */, const ellc_map_filter* filter,
                                              int photo_gate, ellc_trial_propagation_lit* out);

/* Host only, no device work. ellc_light_solve's rule (above) with weight 1 over the record's interior pixels: the ellc_light_normal with
 * sum_w = n_fit, sum_w_s = sum_s, sum_w_t = sum_t, sum_w_ss = sum_ss, sum_w_st = sum_st, sum_w_tt = sum_tt and n_photo = n_fit is handed
 * to ellc_light_solve: the same acceptance tests, roundings and return convention (0 accepted, 1 refused: light_in's bits, NULL meaning
 * (1, 0)); every other field of the normal is zero. An unweighted one-shot fit: no Huber weight, no iteration. A NULL rec, params or
 * light_out returns 1 and writes nothing (ellc_light_solve itself checks no pointer). */
int ellc_trial_light_solve(const ellc_trial_propagation_lit* rec, const ellc_light_params* params, const float* light_in, float* light_out);

/* ---- a keyframe's map refined against other views (v20) -------------------------------------------------------------
 * The structure step beside the motion step above: a per-pixel photometric Gauss-Newton on the INVERSE DEPTH of keyframe slot
 * kf_slot (K) against the images of B other views at known transforms and lights. K's depth Z0, variance V0 and image are read on
 * `level`. View b is slot view_slots[b], a keyframe slot if views_are_keyframes == 1 and a frame slot if 0 (as in
 * ellc_keyframe_trial_propagate); only its image on `level` is read, so a view needs no depth. Slots may repeat and K may be among
 * the views. T = T12 + 12 * b is a row-major 3x4 f32 that takes K's camera coordinates into view b's, the scale folded into the 3x3
 * block; light + 2 * b is (gain, offset) in v19's sense with K as the source, Ip = gain * Is + offset (two roundings), NULL meaning
 * (1, 0): exactly what ellc_keyframe_sim3_align_lit(src = K, dst = view) returned. Per pixel of K, all arithmetic IEEE f32 in this
 * order, no contraction, correctly rounded divisions:
 *   1. TAKING PART. Iff ellc_keyframe_map_points would KEEP the pixel under `filter` (n_kept) and prior_weight == 0 || V0 > 0
 *      (n_taking_part). d0 = 1 / Z0;  hp = prior_weight / V0, hp = 0 when prior_weight == 0.
 *   2. EVALUATION at an inverse depth d, Z = 1 / d: H = g = E = 0, n = 0, then the views in ascending b. The candidate (P' = (x', y',
 *      z'), nid, u, v) is ellc_keyframe_render_depth's for (px, py, Z, V0) at view b's T, with the same drops. The photometric pixel
 *      is rule 3 of ellc_keyframe_sim3_step word for word (the four-tap condition, Iw, gx, gy, A, Bv, Cq, rp = Iw - Ip, e and wp with
 *      the host-rounded w0 and sp). A view without a candidate or without four taps contributes nothing. Otherwise
 *        qx = x' - T[3];  qy = y' - T[7];  qz = z' - T[11];  J = -(Z * (((A * qx) + (Bv * qy)) + (Cq * qz)));
 *      (the exact derivative of Iw by d, since dP'/dd = -Z (P' - t));
 *        wJ = wp * J;  H = H + wJ * J;  g = g + wJ * rp;  E = E + (rp * rp) * wp;  n += 1.
 *   3. LOOP. d = d0; for it = 0 .. n_iter - 1: evaluate at d (the first evaluation's E and n are E0 and n0); stop with TOO_FEW_VIEWS
 *      if n < min_views;  Ht = H + hp;  gt = g + hp * (d - d0);  stop with NO_INFORMATION unless Ht > 0 && Ht <= FLT_MAX;
 *      step = gt / Ht;  dn = d - step;  stop with BAD_STEP unless dn > 0 && dn <= FLT_MAX && fabsf(step) <= max_step_rel * d (NaN
 *      fails);  d = dn.
 *   4. ACCEPTANCE. One more evaluation at the final d gives (H1, E1, n1): VIEWS_CHANGED unless n1 == n0; NO_INFORMATION unless
 *      Ht1 = H1 + hp is in (0, FLT_MAX];  c1 = E1 + (hp * (d - d0)) * (d - d0), COST_ROSE unless c1 <= E0; otherwise REFINED.
 *   5. OUTPUTS (host pointers, dense cols x rows of the level, each may be NULL). REFINED pixels get depth = 1 / d, var = 1 / Ht1,
 *      views = n1. Every other pixel keeps K's own depth and variance BITS (pixels not taking part and K's inf / NaN / negative
 *      pixels included); its `views` is n of the last evaluation made, 0 where none was made. `status` is an ellc_refine_status.
 *   6. STATS. The integers are exact. sum_cost_before / sum_cost_after add (double)E0 / (double)c1 over the refined pixels: the
 *      pixels are partitioned by the level's size (256-pixel blocks), partial sums are combined in a fixed order in double.
 *   7. dst_kf_slot is -1 or a keyframe slot, at level 0 only, exactly as in ellc_keyframe_fuse_depth: afterwards the slot is what
 *      ellc_keyframe_set_depth(dst_kf_slot, depth, var) with the returned planes would leave. It may be K itself (the main use) or
 *      a view: every kernel has read its inputs before the copy, in stream order.
 *   The result is a function of the intrinsics, the level, K's three planes, the views' images, the T's, the lights, the filter and
 *   the params ALONE; cfg.arith, cfg.grid_batch and whatever else is in flight do not enter it. THE ORDER OF THE VIEWS DOES: H, g and
 *   E are f32 sums in ascending b. A view from which no pixel gets four taps changes no byte.
 *   Synchronous, ordered like every other non-batch entry point. A refused call changes nothing and writes nothing.
 * ELLC_ERR_BAD_ARG: B outside 1..ELLC_REFINE_MAX_VIEWS, a slot or the level out of range, more than 2^24 pixels on the level; a NULL
 * view_slots, T12, filter or params; the filter errors of ellc_keyframe_map_points; a value of T, light or params that is not
 * finite; sigma_i2 <= 0, huber_k <= 0, prior_weight < 0, max_step_rel <= 0; n_iter outside 1..8, min_views outside 1..B,
 * views_are_keyframes outside 0..1; the destination errors of the fusion.
 * ELLC_ERR_NOT_READY: K without image or depth, a view without image. */
#define ELLC_REFINE_MAX_VIEWS 64

typedef enum {
  ELLC_REFINE_NOT_TAKING_PART = 0,
  ELLC_REFINE_REFINED = 1,
  ELLC_REFINE_TOO_FEW_VIEWS = 2,
  ELLC_REFINE_NO_INFORMATION = 3,
  ELLC_REFINE_BAD_STEP = 4,
  ELLC_REFINE_VIEWS_CHANGED = 5,
  ELLC_REFINE_COST_ROSE = 6
} ellc_refine_status;

typedef struct {
  float sigma_i2;      /* > 0: variance of a grey value, as in ellc_sim3_params */
  float huber_k;       /* > 0: Huber threshold on |rp| / sigma_i */
  float prior_weight;  /* >= 0: factor on the prior's information 1 / V0; 0 switches the prior off */
  float max_step_rel;  /* > 0: a step beyond max_step_rel * d ends the pixel with BAD_STEP */
  int   n_iter;        /* 1..8 Gauss-Newton steps */
  int   min_views;     /* 1..B views with four taps an evaluation needs */
} ellc_refine_params;  /* 24 bytes */
void ellc_refine_default_params(ellc_refine_params* params);   /* {16, 1.345, 1, 0.5, 3, 2} */

typedef struct {
  int32_t n_kept;            /* pixels ellc_keyframe_map_points would keep under `filter` */
  int32_t n_taking_part;     /* of those, prior_weight == 0 || V0 > 0: the sum of the six counts below */
  int32_t n_refined, n_too_few_views, n_no_information, n_bad_step, n_views_changed, n_cost_rose;
  int64_t sum_views;         /* sum of n1 over the refined pixels */
  double  sum_cost_before;   /* sum of (double)E0 over the refined pixels */
  double  sum_cost_after;    /* sum of (double)c1 over the refined pixels */
  int32_t reserved[2];       /* 0 */
} ellc_refine_stats;         /* 64 bytes, every field naturally aligned */

ellc_status ellc_keyframe_refine_depth(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                       const float* T12, const float* light /* may be NULL */, const ellc_map_filter* filter,
                                       const ellc_refine_params* params, int dst_kf_slot, float* depth, float* var, uint8_t* views,
                                       uint8_t* status, ellc_refine_stats* out /* each may be NULL */);

/* Host only, no device work. The inverse of a similarity and of its light, for a caller that holds view -> keyframe transforms
 * (ellc_keyframe_sim3_align_lit(src = view, dst = K)) and needs keyframe -> view: the 3x3 block M is inverted in double as a general
 * matrix (adjugate over determinant), t' = -(M^-1 t), each of the twelve entries rounded to f32 once; the light becomes
 * (1 / gain, -offset / gain), computed in double and rounded once. light_in NULL means (1, 0); light_out may be NULL; the outputs
 * may be the inputs. Nothing is checked: a singular block or a zero gain gives inf / NaN. */
void ellc_sim3_invert(const float* T12_in, const float* light_in /* may be NULL */, float* T12_out, float* light_out /* may be NULL */);

/* ---- hypotheses created by a depth sweep (v21) ----------------------------------------------------------------------
 * The structure-CREATION step beside the refinement above: the pixels of keyframe slot kf_slot (K) that hold no hypothesis and have
 * texture get one from a sweep over n_samples inverse depths against the images of B other views. K, `level`, the views,
 * views_are_keyframes, T12, light and dst_kf_slot mean what they mean in ellc_keyframe_refine_depth: K's camera goes into view b's
 * through T12 + 12 * b, light + 2 * b is (gain, offset) with K as the source (NULL: (1, 0)), only a view's image on `level` is read.
 * K's depth Z0, variance V0 and image I (grey values as f32) are read on `level`. Per pixel (px, py) of K, all arithmetic IEEE f32
 * in this order, no contraction, correctly rounded divisions:
 *   1. SWEPT PIXELS. A pixel is OK iff Z0 > 0 && Z0 <= FLT_MAX && V0 >= 0 (ellc_keyframe_map_points' rule; n_ok). It is SWEPT iff it
 *      is not OK, 1 <= px <= cols - 2 and 1 <= py <= rows - 2, and with gxc = I(px+1,py) - I(px-1,py), gyc = I(px,py+1) - I(px,py-1):
 *      (gxc*gxc) + (gyc*gyc) >= min_grad2 (n_swept). No ellc_map_filter takes part.
 *   2. SAMPLES. dstep = (d_max - d_min) / (float)(n_samples - 1), computed once on the host in f32;
 *      d_k = d_min + (float)k * dstep;  Z = 1 / d_k,  k = 0 .. n_samples - 1.
 *   3. COST OF SAMPLE k. E = 0, n = 0, then the views in ascending b. For the five pattern pixels j = 0..4 at the offsets (0,0),
 *      (1,0), (-1,0), (0,1), (0,-1) in this order: the candidate is ellc_keyframe_render_depth's for (px+dx, py+dy, Z, V = 0.0f) at
 *      view b's T, with its drops; then rule 3 of ellc_keyframe_sim3_step word for word (the four-tap condition, Iw, e and wp with the
 *      host-rounded w0 and sp);  rp = Iw - (gain * Is_j + offset), Is_j K's grey value at the pattern pixel;  c_j = (rp * rp) * wp.
 *      A view counts iff all five pattern pixels have a candidate and four taps: then E = E + ((((c_0 + c_1) + c_2) + c_3) + c_4),
 *      n += 1; otherwise it contributes nothing.  cost = E / (float)n.  The sample is VALID iff n >= min_views && cost <= FLT_MAX
 *      (NaN fails).
 *   4. DECISION, in this order. No valid sample: NO_VALID_SAMPLE. k1 is the lowest k among the valid samples of smallest cost, c1
 *      and n1 its cost and n. k1 == 0, k1 == n_samples - 1 or a neighbour k1 - 1 / k1 + 1 not valid: AT_RANGE_END; cm and cp are the
 *      neighbours' costs. max_cost > 0 && !(c1 <= max_cost): COST_TOO_HIGH. c2 is the smallest valid cost among the samples with
 *      |k - k1| >= 2: !(c1 <= distinct_ratio * c2): NOT_DISTINCT; with no such sample the test passes.
 *        curv = (cm - (2.0f * c1)) + cp;                                  !(curv > 0 && curv <= FLT_MAX): FLAT
 *        off = (0.5f * (cm - cp)) / curv;  d = d_k1 + off * dstep;
 *        v = var_scale * ((2.0f * (dstep * dstep)) / ((float)n1 * curv));
 *        !(d > 0 && d <= FLT_MAX && v >= 0 && v <= FLT_MAX): FLAT;  otherwise CREATED.
 *      v is the inverse of half the second difference of the summed chi-square of the n1 views at the parabola's vertex: a MODEL
 *      figure, conservative where the images are cleaner than sigma_i2 says.
 *   5. OUTPUTS (host pointers, dense cols x rows of the level, each may be NULL). CREATED pixels get depth = 1 / d, var = v,
 *      views = n1. Every other pixel keeps K's own depth and variance BITS (OK pixels, NaN, inf and negative ones included); its
 *      `views` is n1 where a k1 exists and 0 otherwise. `status` is an ellc_sweep_status. The integer stats are exact; sum_views adds
 *      n1 and sum_cost (double)c1 over the created pixels, sum_cost in the fixed order of the refinement's sums (256-pixel blocks by
 *      the level's size, then the blocks): its bytes are a function of the inputs alone.
 *   6. dst_kf_slot is -1 or a keyframe slot, at level 0 only: afterwards the slot is what ellc_keyframe_set_depth(dst_kf_slot,
 *      depth, var) with the returned planes would leave. It may be K itself (the main use) or a view.
 *   The result is a function of the intrinsics, the level, K's three planes, the views' images, the T's, the lights and the params
 *   ALONE; cfg.arith, cfg.grid_batch and whatever else is in flight do not enter it. The order of the views enters through the f32
 *   sum E only. A view in which no pattern gets its taps changes no byte. A second call gives the same bytes.
 *   Synchronous, ordered like every other non-batch entry point. A refused call changes nothing and writes nothing.
 * The defaults {16, 1.345, 0.125, 4, 100, 0, 0.7, 1, 64, 2} are DESIGN CHOICES, not measured optima: a depth range of 0.25 .. 8 in the
 * keyframe's own units (the reference scales a new keyframe's mean inverse depth to 1), a central difference of 10 grey values, a
 * best cost at most 0.7 of the best one two steps away.
 * ELLC_ERR_BAD_ARG, in this order: a NULL view_slots, T12 or params; B outside 1..ELLC_REFINE_MAX_VIEWS; views_are_keyframes outside
 * 0..1; the level out of range or more than 2^24 pixels on it; a value of T12 or light that is not finite; a value of params that is
 * not finite; sigma_i2 <= 0, huber_k <= 0, !(0 < d_min < d_max) or 1 / d_min not finite, min_grad2 < 0, distinct_ratio outside
 * (0, 1], var_scale <= 0, n_samples outside 3..ELLC_SWEEP_MAX_SAMPLES, min_views outside 1..B; the destination errors of the fusion;
 * a slot out of range.
 * ELLC_ERR_NOT_READY: K without image or depth, a view without image. */
#define ELLC_SWEEP_MAX_SAMPLES 64

typedef enum {
  ELLC_SWEEP_NOT_SWEPT = 0,
  ELLC_SWEEP_CREATED = 1,
  ELLC_SWEEP_NO_VALID_SAMPLE = 2,
  ELLC_SWEEP_AT_RANGE_END = 3,
  ELLC_SWEEP_COST_TOO_HIGH = 4,
  ELLC_SWEEP_NOT_DISTINCT = 5,
  ELLC_SWEEP_FLAT = 6
} ellc_sweep_status;

typedef struct {
  float sigma_i2;        /* > 0: variance of a grey value, as in ellc_refine_params */
  float huber_k;         /* > 0: Huber threshold on |rp| / sigma_i */
  float d_min, d_max;    /* the inverse-depth range: 0 < d_min < d_max, finite, 1 / d_min finite */
  float min_grad2;       /* >= 0: squared central-difference gradient a swept pixel needs */
  float max_cost;        /* <= 0: no test; otherwise the best sample's cost may not exceed it */
  float distinct_ratio;  /* in (0, 1]: c1 <= distinct_ratio * c2 */
  float var_scale;       /* > 0: factor on the model variance */
  int   n_samples;       /* 3 .. ELLC_SWEEP_MAX_SAMPLES */
  int   min_views;       /* 1..B views with all five pattern pixels a sample needs */
} ellc_sweep_params;     /* 40 bytes */
void ellc_sweep_default_params(ellc_sweep_params* params);   /* {16, 1.345, 0.125, 4, 100, 0, 0.7, 1, 64, 2}: design choices */

typedef struct {
  int32_t n_ok;              /* pixels that hold a hypothesis already */
  int32_t n_swept;           /* pixels swept: the sum of the six counts below */
  int32_t n_created, n_no_valid_sample, n_at_range_end, n_cost_too_high, n_not_distinct, n_flat;
  int64_t sum_views;         /* sum of n1 over the created pixels */
  double  sum_cost;          /* sum of (double)c1 over the created pixels */
  int32_t reserved[4];       /* 0 */
} ellc_sweep_stats;          /* 64 bytes, every field naturally aligned */

ellc_status ellc_keyframe_sweep_depth(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                      const float* T12, const float* light /* may be NULL */, const ellc_sweep_params* params,
                                      int dst_kf_slot, float* depth, float* var, uint8_t* views, uint8_t* status,
                                      ellc_sweep_stats* out /* each may be NULL */);

/* ---- hypotheses the other views contradict, removed (v22) -----------------------------------------------------------
 * The geometric consistency filter behind the steps above: the only call that REMOVES a hypothesis. Every kept pixel of keyframe slot
 * kf_slot (K) is put to a vote of B other views, and a pixel the views contradict loses its hypothesis. K, `level`, the views,
 * views_are_keyframes, T12, light and dst_kf_slot mean what they mean in ellc_keyframe_refine_depth: K's camera goes into view b's
 * through T12 + 12 * b (a Sim(3)'s scale folded in), light + 2 * b is (gain, offset) with K as the source (NULL: (1, 0)). Slots may
 * repeat and K may be among the views: K at the identity agrees with itself, which is the caller's business. A view's depth and
 * variance planes on `level` are read iff views_are_keyframes == 1 and the slot holds a depth; every other view (a frame slot, or a
 * keyframe slot with an image only) votes photometrically only and is no error. Per pixel of K, all arithmetic IEEE f32 in this
 * order, no contraction, correctly rounded divisions:
 *   1. TAKING PART. Iff ellc_keyframe_map_points would KEEP the pixel under `filter` (n_kept).
 *   2. VOTES, the views in any order (every count is an integer). The candidate is ellc_keyframe_render_depth's for (px, py, Z0, V0)
 *      at view b's T, with its drops: target, nid, u, v, nvar. A view without a candidate votes nothing.
 *      GEOMETRIC VOTE, where the view has depth planes: steps 3-6 of ellc_keyframe_depth_consistency word for word. Zt and Vt are read
 *      at the target; the vote takes part iff Zt > 0 && Zt <= FLT_MAX && Vt >= 0;  idt = 1 / Zt;  d = nid - idt;  s = nvar + Vt;
 *      AGREE iff d * d <= agree_k2 * s; IN_FRONT iff it does not agree and d > 0 (the view sees through K's point); BEHIND otherwise
 *      (the point is hidden in that view).
 *      PHOTOMETRIC VOTE, iff photo_k > 0, the view's geometric vote was not BEHIND and the view has four taps (the four-tap condition
 *      and Iw: rule 3 of ellc_keyframe_sim3_step):  rp = Iw - (gain * Is + offset);  e = |rp| * sp, sp = sqrtf(1 / sigma_i2) rounded
 *      on the host as elsewhere. The view counts in n_photo, and in n_bad iff !(e <= photo_k).
 *   3. DECISION, a / f / h the numbers of AGREE / IN_FRONT / BEHIND votes, in this order:
 *        CULLED_FREE_SPACE   f >= min_in_front && f > a
 *        CULLED_UNSUPPORTED  a + f + h >= min_judged && a < min_support
 *        CULLED_PHOTO        photo_k > 0 && n_photo >= min_photo && 2 * n_bad > n_photo
 *        UNSEEN              a + f + h == 0 && n_photo == 0 (the pixel is kept)
 *        KEPT                otherwise
 *   4. OUTPUTS (host pointers, dense cols x rows of the level, each may be NULL). A culled pixel gets depth 0.0f and var -1.0f,
 *      ellc_keyframe_set_depth's "no hypothesis". Every other pixel keeps K's own depth and variance BITS (pixels not taking part and
 *      K's inf / NaN / negative pixels included). votes = a | f << 8 | h << 16 | n_bad << 24; photo = n_photo; `status` is an
 *      ellc_cull_status. No count can pass 64.
 *   5. STATS. n_retained + n_unseen + n_culled_free_space + n_culled_unsupported + n_culled_photo == n_kept; the five sums add a, f,
 *      h, n_photo and n_bad over the pixels taking part. Everything is an integer: nothing depends on an order of summation.
 *   6. dst_kf_slot is -1 or a keyframe slot, at level 0 only, exactly as in ellc_keyframe_refine_depth: afterwards the slot is what
 *      ellc_keyframe_set_depth(dst_kf_slot, depth, var) with the returned planes would leave. It may be K itself (the main use) or
 *      a view: the kernel has read its inputs before the copy, in stream order.
 *   The result is a function of the intrinsics, the level, K's three planes, the views' planes, the T's, the lights, the filter and
 *   the params ALONE; cfg.arith, cfg.grid_batch, whatever else is in flight and the ORDER of the views do not enter it. A view in
 *   which no point of K has a candidate changes no byte. A second call gives the same bytes.
 *   Synchronous, ordered like every other non-batch entry point. A refused call changes nothing and writes nothing.
 * The defaults {1, 16, 3, 1, 2, 1, 2} are DESIGN CHOICES, not measured optima: the agreement of ellc_keyframe_depth_consistency, the
 * grey-value variance of the refinement, a residual of three sigma, one agreeing view among at least two that judge.
 * ELLC_ERR_BAD_ARG, in this order: a NULL view_slots, T12, filter or params; B outside 1..ELLC_REFINE_MAX_VIEWS; views_are_keyframes
 * outside 0..1; the level out of range or more than 2^24 pixels on it; the filter errors of ellc_keyframe_map_points; a value of T12
 * or light that is not finite; agree_k2 negative or not finite, sigma_i2 <= 0, or a param that is not finite; min_support,
 * min_in_front or min_photo outside 1..B, or min_judged outside 1..B; the destination errors of the fusion; a slot out of range.
 * ELLC_ERR_NOT_READY: K without image or depth, a view without image. A keyframe view without depth is accepted. */
typedef enum {
  ELLC_CULL_NOT_TAKING_PART = 0,
  ELLC_CULL_KEPT = 1,
  ELLC_CULL_CULLED_FREE_SPACE = 2,
  ELLC_CULL_CULLED_UNSUPPORTED = 3,
  ELLC_CULL_CULLED_PHOTO = 4,
  ELLC_CULL_UNSEEN = 5
} ellc_cull_status;

typedef struct {
  float agree_k2;        /* >= 0: d * d <= agree_k2 * (nvar + Vt), as in ellc_keyframe_depth_consistency */
  float sigma_i2;        /* > 0: variance of a grey value, as in ellc_refine_params */
  float photo_k;         /* <= 0: no photometric vote; otherwise a view is bad iff !(|rp| / sigma_i <= photo_k) */
  int   min_support;     /* 1..B: agreeing views a judged pixel needs */
  int   min_judged;      /* 1..B: geometric votes from which the support test applies */
  int   min_in_front;    /* 1..B: views that see through the point before free space culls it */
  int   min_photo;       /* 1..B: photometric votes from which the photometric test applies */
} ellc_cull_params;      /* 28 bytes */
void ellc_cull_default_params(ellc_cull_params* params);   /* {1, 16, 3, 1, 2, 1, 2}: design choices */

typedef struct {
  int32_t n_kept;            /* pixels taking part: the sum of the five counts below */
  int32_t n_retained, n_unseen, n_culled_free_space, n_culled_unsupported, n_culled_photo;
  int64_t sum_agree, sum_in_front, sum_behind, sum_photo, sum_photo_bad;   /* over the pixels taking part (offset 24) */
} ellc_cull_stats;           /* 64 bytes, every field naturally aligned */

ellc_status ellc_keyframe_cull_depth(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                     const float* T12, const float* light /* may be NULL */, const ellc_map_filter* filter,
                                     const ellc_cull_params* params, int dst_kf_slot, float* depth, float* var, uint32_t* votes,
                                     uint8_t* photo, uint8_t* status, ellc_cull_stats* out /* each may be NULL */);

/* ---- poses and depths refined in one step (v23) ------------------------------------------------------------------------
 * The refinement above moves K's map with the transforms held fixed, ellc_keyframe_sim3_align(_lit) moves a transform with the map
 * held fixed. These calls move both: one photometric Gauss-Newton step over the SE(3) of B <= ELLC_JOINT_MAX_VIEWS views and the
 * inverse depths of K's kept pixels TOGETHER, K's own hypotheses as the prior, the depths eliminated per pixel (Schur complement), so
 * that the host solves 6 B <= 48 unknowns. step / solve / apply / refine stand to each other as ellc_keyframe_sim3_step,
 * ellc_sim3_solve, ellc_sim3_apply and ellc_keyframe_sim3_align do. K, `level`, the views, views_are_keyframes, T12, light, filter
 * and dst_kf_slot mean what they mean in ellc_keyframe_refine_depth, word for word. Per pixel of K, all arithmetic IEEE f32 in this
 * order, no contraction, correctly rounded divisions:
 *   1. TAKING PART, d0 and hp: rule 1 of ellc_keyframe_refine_depth. The pixel is evaluated at d = inv_depth_in's value where that
 *      plane is given (a host plane, dense cols x rows of the level) and the value is > 0 && <= FLT_MAX, and at d0 otherwise.
 *   2. EVALUATION at d, Z = 1 / d: rule 2 of ellc_keyframe_refine_depth word for word, the views in ascending b, which gives per
 *      view with a term rp, wp and Jd (the refinement's J), and H, g, E and n. Such a view also has the six pose entries of rule 3 of
 *      ellc_keyframe_sim3_step, rotation then translation, a left perturbation exp(xi^) T in the VIEW's camera:
 *        Jp = (Cq y' - Bv z',  A z' - Cq x',  Bv x' - A y',  A,  Bv,  Cq).
 *      TOO_FEW_VIEWS if n < min_views.  Ht = H + hp;  gd = g + hp * (d - d0);  NO_INFORMATION unless Ht > 0 && Ht <= FLT_MAX;
 *      otherwise the pixel is USED and ih = 1 / Ht.
 *   3. SUMS over the used pixels, in double; every term is the product of two f32 values, exact in double (rule 6 of
 *      ellc_keyframe_sim3_step). With wJp[k] = wp * Jp[k], c_b[k] = (wp * Jd) * Jp[k] and m_b[k] = c_b[k] * ih, per view b with a
 *      term (and per pair of views b <= c that both have one):
 *        A[b][(k,l)]      += wJp_b[k] * Jp_b[l]   k <= l, row-major upper triangle of a 6 x 6: 21 sums a view
 *        a[b][k]          += wJp_b[k] * rp_b
 *        S[(6b+k, 6c+l)]  += m_b[k] * c_c[l]      6b+k <= 6c+l, row-major upper triangle of the 6B x 6B matrix
 *        s[6b+k]          += m_b[k] * gd
 *        chi2_photo       += (double)E;    chi2_prior += (double)((hp * (d - d0)) * (d - d0)).
 *      The reduced system is H = blockdiag(A) - S, b = a - s; the record returns A, a, S and s apart, so that every sum has its own
 *      bound and the host takes the differences. The pixels are partitioned by the level's size alone, partial sums are combined in
 *      a fixed order in double, no floating-point atomics: the same bytes on every call.
 *   4. COUNTS, all exact: n_kept, n_taking_part (the sum of the next three), n_used, n_too_few_views, n_no_information; n_terms,
 *      the sum of n over the used pixels, and n_view_terms[b], view b's share of it. Entries of views >= B are zero.
 *   The record is a function of the intrinsics, the level, K's three planes, the views' images, the T's, the lights, the filter, the
 *   params and inv_depth_in ALONE; cfg.arith, cfg.grid_batch and whatever is in flight do not enter it. THE ORDER OF THE VIEWS DOES
 *   (H and g are f32 sums in ascending b). A view from which no pixel gets four taps changes no byte of the other views' sums.
 * ellc_keyframe_joint_step refuses what ellc_keyframe_refine_depth refuses, in its order (ELLC_JOINT_MAX_VIEWS for its limit, no
 * n_iter, no destination), and a NULL `out`; prior_weight == 0 is accepted here. Synchronous; a refused call writes nothing. */
#define ELLC_JOINT_MAX_VIEWS 8

typedef enum {
  ELLC_JOINT_NOT_TAKING_PART = 0,
  ELLC_JOINT_STEPPED = 1,        /* (USED, in the step's counts) */
  ELLC_JOINT_TOO_FEW_VIEWS = 2,
  ELLC_JOINT_NO_INFORMATION = 3,
  ELLC_JOINT_BAD_STEP = 4
} ellc_joint_status;

typedef struct {
  float sigma_i2;      /* > 0: variance of a grey value, as in ellc_refine_params */
  float huber_k;       /* > 0: Huber threshold on |rp| / sigma_i */
  float prior_weight;  /* >= 0: factor on the prior's information 1 / V0 (ellc_keyframe_joint_refine: > 0) */
  float max_step_rel;  /* > 0: a depth step beyond max_step_rel * d leaves the pixel where it was (BAD_STEP) */
  int   min_views;     /* 1..B views with four taps a pixel needs */
} ellc_joint_params;   /* 20 bytes */
void ellc_joint_default_params(ellc_joint_params* params);   /* {16, 1.345, 1, 0.5, 2}: the refinement's */

typedef struct {
  double  A[ELLC_JOINT_MAX_VIEWS][21];   /* offset 0 */
  double  a[ELLC_JOINT_MAX_VIEWS][6];    /* 1344 */
  double  S[1176];                       /* 1728: the first 6B (6B + 1) / 2 entries are used */
  double  s[48];                         /* 11136 */
  double  chi2_photo, chi2_prior;        /* 11520, 11528 */
  int64_t n_terms;                       /* 11536 */
  int32_t n_kept;                        /* 11544 (-1 in a trace entry that was not written) */
  int32_t n_taking_part, n_used, n_too_few_views, n_no_information;
  int32_t B;                             /* 11564: the views of the call: what ellc_joint_solve sizes the system by */
  int32_t n_view_terms[ELLC_JOINT_MAX_VIEWS];   /* 11568 */
} ellc_joint_normal;                     /* 11600 bytes, every field naturally aligned */

ellc_status ellc_keyframe_joint_step(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                     const float* T12, const float* light /* may be NULL */, const ellc_map_filter* filter,
                                     const ellc_joint_params* params, const float* inv_depth_in /* may be NULL */,
                                     ellc_joint_normal* out);

/* Host only, no device work. Forms H and b of rule 3 from the record (6 B unknowns, B = rec->B), multiplies H's diagonal by
 * (1 + lambda) and solves H xi = -b by L D L^T in double without pivoting: the routine of ellc_sim3_solve at another size. Returns
 * non-zero and writes NOTHING when B is outside 1..ELLC_JOINT_MAX_VIEWS, lambda is negative or not finite, a sum or a component of
 * the step is not finite, or a pivot is not above 1e-10 times the largest diagonal entry. xi + 6 b is view b's (rotation,
 * translation). */
int ellc_joint_solve(const ellc_joint_normal* rec, double lambda, double* xi /* [6 * rec->B] */);

/* The step taken. POSES (host): T12_out + 12 b = ellc_sim3_apply((xi_b, log-scale 0), T12 + 12 b). DEPTHS, per pixel that takes part:
 * the evaluation of rules 1 and 2 at the GIVEN T12 and inv_depth_in, and with xf = (float)xi
 *        q = 0;  q = q + c_b[k] * xf[6b+k]  for the views with a term in ascending b, k = 0 .. 5;
 *        delta = -((gd + q) * ih);  dn = d + delta;
 * BAD_STEP unless dn > 0 && dn <= FLT_MAX && fabsf(delta) <= max_step_rel * d (NaN fails); otherwise the pixel is STEPPED.
 * OUTPUTS (host pointers, dense cols x rows of the level, each may be NULL): a STEPPED pixel gets inv_depth_out = dn, depth = 1 / dn,
 * var = ih; every other pixel keeps K's own depth and variance BITS, its inv_depth_out is d where it takes part and 0 where not.
 * `views` is n (0 where the pixel does not take part), `status` an ellc_joint_status. var = ih is the variance of the inverse depth
 * CONDITIONAL on the poses: it leaves out what the poses' own uncertainty adds and is OPTIMISTIC. The stats are exact counts.
 * dst_kf_slot is -1 or a keyframe slot, at level 0 only, exactly as in ellc_keyframe_refine_depth (depth and var are stored).
 * Refusals: the step's, a NULL xi or T12_out, an xi that is not finite, the destination errors of the refinement. */
typedef struct {
  int32_t n_kept, n_taking_part;   /* as in the step */
  int32_t n_stepped, n_too_few_views, n_no_information, n_bad_step;
  int32_t reserved[2];             /* 0 */
} ellc_joint_apply_stats;          /* 32 bytes */

ellc_status ellc_keyframe_joint_apply(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                      const float* T12, const float* light /* may be NULL */, const ellc_map_filter* filter,
                                      const ellc_joint_params* params, const float* inv_depth_in /* may be NULL */, const double* xi,
                                      int dst_kf_slot, float* T12_out, float* inv_depth_out, float* depth, float* var, uint8_t* views,
                                      uint8_t* status, ellc_joint_apply_stats* out /* the six last may be NULL */);

/* The loop. State: the transforms and an inverse-depth plane (T12, inv_depth_in at the start). rec = step(state); then up to
 * max_iter times: solve(rec, lambda) - a refused solve ends the loop; max |xi_i| < eps ends it; trial = apply(state, xi);
 * rec' = step(trial); the trial is ACCEPTED iff c(rec') <= c(rec), c = (chi2_photo + chi2_prior) / (n_terms + n_used) (a c that is
 * NaN, or n_used == 0, refuses) - a refused trial ends the loop at the last accepted state; otherwise state = trial, rec = rec'.
 * The depth plane stays on the device between the iterations; records, xi and the final planes cross to the host.
 * OUTPUTS: T12_out and `out`, the accepted state's transforms and record; *iters_out, the accepted trials; the five planes of the
 * apply that made the accepted state - with no accepted trial K's own depth and variance, inv_depth_in's values where given (0
 * elsewhere) and zeros; dst_kf_slot receives depth and var as in the apply. TRACE (each may be NULL; trace_capacity >= max_iter + 1
 * where one is given): entry e is the e-th step's T12 [B][12] and record, trace_xi's entry e the xi [6 B] solved from it (zeros
 * where no solve succeeded), trace_accepted[e] whether entry e became the state (entry 0 does). Entries not written have
 * n_kept = -1. Everything is held aside until the call has succeeded.
 * Refusals: the apply's without xi, and prior_weight == 0 (the scale gauge is free without a prior and the reduced matrix singular
 * by construction), max_iter outside 1..16, eps or lambda negative or not finite, a trace_capacity that is too small. */
ellc_status ellc_keyframe_joint_refine(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                       const float* T12_in, const float* light /* may be NULL */, const ellc_map_filter* filter,
                                       const ellc_joint_params* params, const float* inv_depth_in /* may be NULL */, int max_iter,
                                       float eps, double lambda, int dst_kf_slot, float* T12_out, ellc_joint_normal* out, int* iters_out,
                                       float* inv_depth_out, float* depth, float* var, uint8_t* views, uint8_t* status,
                                       float* trace_T12, ellc_joint_normal* trace_rec, double* trace_xi, int* trace_accepted,
                                       int trace_capacity);

/* ---- semi-dense depth map: class depthMap (DepthPropagation.cpp) -----------------------------------
 * One depth map per context (the reference's currentDepthMap). State is SoA on device:
 * invDepth, invDepthSmoothed, variance, varianceSmoothed f32; validity_counter, blacklisted i32; isValid u8
 * (DepthHypothesis.h:14-40, live fields). */
typedef struct {
  float* invDepth; float* invDepthSmoothed; float* variance; float* varianceSmoothed;
  int32_t* validity_counter; int32_t* blacklisted; uint8_t* isValid;
} ellc_hypotheses;   /* seven host arrays of W*H elements */

ellc_status ellc_depth_set_state(ellc_ctx* ctx, const ellc_hypotheses* host);
ellc_status ellc_depth_get_state(ellc_ctx* ctx, const ellc_hypotheses* host);
/* depthMap::keyFrame = keyframe slot (main.cpp:232, 307; DepthPropagation.cpp:1772). */
ellc_status ellc_depth_set_keyframe(ellc_ctx* ctx, int kf_slot);
/* depthMap::propagateDepth(new_keyframe) (:1003-1157). new_kf_slot holds the new keyframe's image;
 * pose_new_wrt_old = new_keyframe->poseWrtOrigin (old keyframe is the origin). */
ellc_status ellc_depth_propagate(ellc_ctx* ctx, int new_kf_slot, const float* pose_new_wrt_old);
/* depthMap::observeDepthRowParallel (:1932-1958, :191-263, line stereo :397-885) against frame slot
 * `frame_slot` whose pose w.r.t. the keyframe is pose_frame_wrt_kf (frame::poseWrtOrigin). */
ellc_status ellc_depth_observe(ellc_ctx* ctx, int frame_slot, const float* pose_frame_wrt_kf);
ellc_status ellc_depth_fill_holes(ellc_ctx* ctx);                         /* fillDepthHoles :1317-1400 */
ellc_status ellc_depth_regularize(ellc_ctx* ctx, int remove_occlusions);  /* regularizeDepthMap :1436-1543 */
ellc_status ellc_depth_make_inv_depth_one(ellc_ctx* ctx, float* rescale_factor); /* makeInvDepthOne :1546-1587 */
/* depthMap::doRegularization (DepthPropagation.cpp:1627-1635) = fillDepthHoles + regularizeDepthMap(remove_occlusions) in ONE
 * launch; the state afterwards is that of ellc_depth_fill_holes followed by ellc_depth_regularize(remove_occlusions), bit for
 * bit (v7). */
ellc_status ellc_depth_do_regularization(ellc_ctx* ctx, int remove_occlusions);
/* regularizeDepthMap(remove_occlusions) + fillDepthHoles + regularizeDepthMap(false), the three stencil stages in the order
 * createKeyFrame runs them (DepthPropagation.cpp:1775-1777), in ONE launch; the state afterwards is that of the three calls
 * ellc_depth_regularize(remove_occlusions), ellc_depth_fill_holes, ellc_depth_regularize(0), bit for bit (v7). */
ellc_status ellc_depth_regularize_fill_regularize(ellc_ctx* ctx, int remove_occlusions);
/* depthMap::updateDepthImage (:1254-1315): exports depth / variance pyramids into the keyframe slot
 * (what GetImagePoseEstimate then reads). */
ellc_status ellc_depth_update_depth_image(ellc_ctx* ctx);
/* depthMap::createKeyFrame(new_keyframe) (:1758-1794): propagate, regularise(occlusions), fill+regularise,
 * rescale, export; the new slot becomes the depth map's keyframe. */
ellc_status ellc_depth_create_keyframe(ellc_ctx* ctx, int new_kf_slot, const float* pose_new_wrt_old, float* rescale_factor);
ellc_status ellc_depth_seeds(ellc_ctx* ctx, float* percent);              /* calculate_no_of_Seeds :1804-1830 */
/* One tracked frame that does not switch the keyframe, main.cpp:330 + :499-502, as ONE device sequence: GetImagePoseEstimate
 * (ImageFunc.cpp:49-315; FCA) of frame slot `frame_slot` against the depth map's keyframe from init_pose, then — behind it on the
 * device, the pose never travelling to the host and back in between — observeDepthRowParallel with poseWrtOrigin =
 * concatenateRelativePose(pose, 0) (ImageFunc.cpp:305), doRegularization(false) and updateDepthImage. The call returns once the
 * POSE is there; the depth stages are still running (every later call is ordered behind them). seeds_percent (may be NULL):
 * calculate_no_of_Seeds of the map BEFORE this frame's observation (what main.cpp:368-373 writes beside the pose). Results are
 * those of ellc_align + ellc_depth_seeds + ellc_depth_observe + ellc_depth_fill_holes + ellc_depth_regularize(0) +
 * ellc_depth_update_depth_image. */
ellc_status ellc_track_frame(ellc_ctx* ctx, int frame_slot, const float* init_pose, int save_weights, float* out_pose, int* out_iters,
                             float* out_weighted, float* seeds_percent);

/* ---- multi-GPU: the loop-closure batch sharded over the ranks of one node, one gather of the results ------
 * The batch loop of globalOptimize::findMatchParallel (GlobalOptimize.cpp:480-610) runs B independent alignments; rank r of
 * `world` (one process per GPU) aligns the contiguous block ellc_shard_range gives it on its own context and the ONLY
 * exchange is one gather per batch of 8 floats per alignment: [pose(6), weightedPose, iterations executed]. A communicator
 * is independent of any ellc_ctx. Transports: RCCL (ncclAllGather over xGMI on a stream of its own; libellc_hip.so) and TCP
 * through rank 0 (host memory only: CPU tests of the sharded path, hosts without xGMI; also in libellc_comm.so, which is
 * csrc/ellc_comm.cpp alone). Up to 4 gathers may be outstanding (start / finish), so the exchange of one batch overlaps the
 * kernels of the next; ellc_gather_results = start + finish. Every rank passes the same `total`; n_local must be the size
 * of the rank's block; out8 receives `total` records in global order on every rank. */
typedef struct ellc_comm ellc_comm;
void ellc_shard_range(int total, int world, int rank, int* lo, int* hi);
ellc_status ellc_comm_unique_id(unsigned char* id128);   /* rank 0 creates it (ncclGetUniqueId); the host program hands the 128 bytes to the other ranks */
ellc_status ellc_comm_init_rccl(int device, const unsigned char* id128, int world, int rank, int max_total, ellc_comm** out);
ellc_status ellc_comm_init_tcp(const char* host_ipv4, int port, int world, int rank, int max_total, ellc_comm** out);
/* What the TRANSPORT itself reports, for the self-check of a multi-rank run: transport (1 RCCL, 2 TCP); the number of ranks and this
 * process's rank as RCCL sees them (ncclCommCount / ncclCommUserRank; TCP: the ranks that joined rank 0 / the rank announced) — both
 * init calls fail unless they equal `world` / `rank`; the PCI bus id of the communicator's device (RCCL; "" for TCP). */
ellc_status ellc_comm_info(const ellc_comm* comm, int* transport, int* world_seen, int* rank_seen, char* pci_bus_id, int pci_capacity);
ellc_status ellc_comm_destroy(ellc_comm* comm);
const char* ellc_comm_last_error(const ellc_comm* comm);
ellc_status ellc_gather_start(ellc_comm* comm, int total, const float* local8, int n_local);
ellc_status ellc_gather_finish(ellc_comm* comm, float* out8, int out_capacity);   /* out8 holds out_capacity records: ELLC_ERR_CAPACITY (the gather stays outstanding) if the oldest gather's total is larger */
ellc_status ellc_gather_results(ellc_comm* comm, int total, const float* local8, int n_local, float* out8);

/* (Measurement hooks, device self-tests and test hooks are NOT part of this interface: include/ellc_abi_diag.h declares them and only
 * libellc_hip_diag.so — the same sources built with -DELLC_DIAG_ABI — exports them. libellc_hip.so exports exactly what this header declares.) */

#ifdef __cplusplus
}
#endif
#endif /* ELLC_ABI_H */
