/* Diagnostic extension of the ELLC C ABI (include/ellc_abi.h): measurement hooks (bench.py's roofline leg, tools/), device self-tests
 * (tests/) and test hooks of the resident schedule. NOT part of the product interface: libellc_hip.so does not export these symbols;
 * libellc_hip_diag.so — csrc/ built with -DELLC_DIAG_ABI, the same kernels and launch paths — exports them in addition to everything
 * ellc_abi.h declares. Nothing here replaces a member of the reference. */
#ifndef ELLC_ABI_DIAG_H
#define ELLC_ABI_DIAG_H
#include "ellc_abi.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement hooks (bench.py) ------------------------------------------------------------------- */
/* Launch the dominant kernel (FCA residual/Jacobian/accumulate at `level` over a batch) `reps` times on
 * the context stream between two HIP events; returns the average milliseconds per launch and the
 * algorithmic bytes one launch covers (4*N + 14*V summed over the batch). */
ellc_status ellc_profile_gn_kernel(ellc_ctx* ctx, int B, const int* kf_slots, const int* frame_slots, int level, int reps,
                                   float* avg_ms, double* algorithmic_bytes, long long* valid_pixels);
/* Time `reps` full ellc_align_enqueue passes with HIP events on the context stream (ms per pass). (A call that runs the
 * early-exit tracking schedule described above is timed without a remainder it might need.) */
ellc_status ellc_profile_align(ellc_ctx* ctx, int B, const int* kf_slots, const int* frame_slots, const float* init_pose,
                               int mode, int reps, float* avg_ms);

/* `reps` enqueues of one depth-map stage between two HIP events on the context stream (ms per call). stage 0:
 * regularizeDepthMap(false), 1: fillDepthHoles, 2: observeDepthRow against frame_slot / pose, 3: updateDepthImage, 4: createKeyFrame's
 * regularise(remove occlusions) + fill + regularise in one launch, 5: the tracked frame's fill + regularise + updateDepthImage in
 * one launch. */
ellc_status ellc_profile_depth_stage(ellc_ctx* ctx, int stage, int frame_slot, const float* pose_frame_wrt_kf, int reps, float* avg_ms);

/* ellc_keyframe_map_points with HIP events around its three launches (map_count + map_scan, then map_scatter): launches_ms receives
 * their device time, without the copy of the records to the host. Everything else as the product call. */
ellc_status ellc_profile_map_points(ellc_ctx* ctx, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* filter,
                                    ellc_map_point* out, int capacity, int* counts, int* total, float* launches_ms);

/* ellc_keyframe_render_depth with HIP events around its launches (the preset of the keys, render_min, render_resolve, render_finish,
 * render_agree): launches_ms receives their device time, without the copies that follow. Everything else as the product call. */
ellc_status ellc_profile_render_depth(ellc_ctx* ctx, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* filter,
                                      float agree_k2, int dst_kf_slot, float* depth, float* var, int32_t* source, int32_t* agree,
                                      uint8_t* intensity, int* n_valid, float* launches_ms);

/* ellc_keyframe_fuse_depth with HIP events around its launches (the preset of the keys, render_min, render_resolve, render_finish,
 * fuse_agree, fuse_tile_sums, fuse_offsets, fuse_scatter, fuse_merge, fuse_finish): launches_ms receives the device time from the first to the end of the last,
 * without the copies that follow. The host's read of the list's size behind fuse_offsets - one synchronisation, and the list's growth
 * when it has to grow - lies INSIDE that window: it is part of what the call costs. Everything else as the product call. */
ellc_status ellc_profile_fuse_depth(ellc_ctx* ctx, int B, const int* kf_slots, const float* T12, int level, const ellc_map_filter* filter,
                                    float agree_k2, int max_merge, int dst_kf_slot, float* depth, float* var, int32_t* source, int32_t* agree,
                                    int32_t* merged, uint8_t* intensity, int* n_valid, int* n_fused, float* launches_ms);

/* ellc_depth_absorb_keyframes with HIP events around its launches (the preset of the count plane, absorb_mark, fuse_tile_sums,
 * fuse_offsets, absorb_scatter, absorb_fold, absorb_finish): launches_ms receives the device time from the first to the end of the last,
 * without finalise's regularisation and export behind them. The host's read of the list's size lies INSIDE that window, as in the
 * fusion's hook. Everything else as the product call. */
ellc_status ellc_profile_depth_absorb(ellc_ctx* ctx, int B, const int* kf_slots, const float* T12, const ellc_map_filter* filter,
                                      const ellc_absorb_params* params, ellc_absorb_stats* out, float* launches_ms);

/* ellc_keyframe_trial_propagate with the number of requests per launch forced (max_group_requests >= 1; 0: as many as the bitmaps'
 * 64 MB hold, the product call's choice) and HIP events around its launches (the preset of the bitmaps, trial_pass, trial_finish, per
 * group): launches_ms receives their device time, without the staging copy in front. Everything else as the product call: the records
 * do not depend on the split. */
ellc_status ellc_profile_trial_propagate(ellc_ctx* ctx, int B, const int* src_kf_slots, int dst_is_keyframe, const int* dst_slots, const float* T12,
                                         const ellc_map_filter* filter, int photo_gate, ellc_trial_propagation* out, int max_group_requests,
                                         float* launches_ms);

/* ellc_keyframe_depth_consistency with HIP events around its launches (consist_pass, consist_finish): launches_ms receives their
 * device time, without the staging copy in front. Everything else as the product call. */
ellc_status ellc_profile_depth_consistency(ellc_ctx* ctx, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, int level,
                                           const ellc_map_filter* filter, float agree_k2, ellc_depth_consistency* out, float* launches_ms);

/* ellc_keyframe_sim3_step with HIP events around its launches (sim3_pass, sim3_finish): launches_ms receives their device time,
 * without the staging copy in front. Everything else as the product call. */
ellc_status ellc_profile_sim3_step(ellc_ctx* ctx, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12, int level,
                                   const ellc_map_filter* filter, const ellc_sim3_params* params, ellc_sim3_normal* out, float* launches_ms);

/* ellc_keyframe_light_step / ellc_keyframe_sim3_step_lit with HIP events around their launches (light_pass, light_finish;
 * sim3_pass, sim3_finish): launches_ms receives their device time, without the staging copy in front. Everything else as the
 * product calls. */
ellc_status ellc_profile_light_step(ellc_ctx* ctx, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12,
                                    const float* light_in, int level, const ellc_map_filter* filter, const ellc_sim3_params* params,
                                    ellc_light_normal* out, float* launches_ms);
ellc_status ellc_profile_sim3_step_lit(ellc_ctx* ctx, int B, const int* src_kf_slots, const int* dst_kf_slots, const float* T12,
                                       const float* light, int level, const ellc_map_filter* filter, const ellc_sim3_params* params,
                                       ellc_sim3_normal* out, float* launches_ms);

/* ellc_keyframe_refine_depth with HIP events around its launches (refine_pixels, refine_finish): launches_ms receives their device
 * time, without the staging copy in front and the downloads behind. Everything else as the product call. */
ellc_status ellc_profile_refine_depth(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                      const float* T12, const float* light, const ellc_map_filter* filter, const ellc_refine_params* params,
                                      int dst_kf_slot, float* depth, float* var, uint8_t* views, uint8_t* status, ellc_refine_stats* out,
                                      float* launches_ms);

/* ellc_keyframe_sweep_depth with HIP events around its launches (sweep_pixels, sweep_finish): launches_ms receives their device time,
 * without the staging copy in front and the downloads behind. Everything else as the product call. */
ellc_status ellc_profile_sweep_depth(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                     const float* T12, const float* light, const ellc_sweep_params* params, int dst_kf_slot, float* depth,
                                     float* var, uint8_t* views, uint8_t* status, ellc_sweep_stats* out, float* launches_ms);

/* ellc_keyframe_cull_depth with HIP events around its launches (cull_pixels, cull_finish): launches_ms receives their device time,
 * without the staging copy in front and the downloads behind. Everything else as the product call. */
ellc_status ellc_profile_cull_depth(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                    const float* T12, const float* light, const ellc_map_filter* filter, const ellc_cull_params* params,
                                    int dst_kf_slot, float* depth, float* var, uint32_t* votes, uint8_t* photo, uint8_t* status,
                                    ellc_cull_stats* out, float* launches_ms);

/* ellc_keyframe_joint_step and ellc_keyframe_joint_apply with HIP events around their launches (joint_pixels, joint_count_finish,
 * joint_pairs, joint_pair_finish; joint_apply_pixels, joint_count_finish): launches_ms receives their device time, without the
 * staging copies in front and the downloads behind. Everything else as the product calls. */
ellc_status ellc_profile_joint_step(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                    const float* T12, const float* light, const ellc_map_filter* filter, const ellc_joint_params* params,
                                    const float* inv_depth_in, ellc_joint_normal* out, float* launches_ms);
ellc_status ellc_profile_joint_apply(ellc_ctx* ctx, int kf_slot, int level, int B, int views_are_keyframes, const int* view_slots,
                                     const float* T12, const float* light, const ellc_map_filter* filter, const ellc_joint_params* params,
                                     const float* inv_depth_in, const double* xi, int dst_kf_slot, float* T12_out, float* inv_depth_out,
                                     float* depth, float* var, uint8_t* views, uint8_t* status, ellc_joint_apply_stats* out,
                                     float* launches_ms);

/* Counter calibration: stream `bytes` of device memory once per launch with 4-byte-per-lane loads (the access
 * width of the compacted pixel arrays), `reps` launches, so FETCH_SIZE can be scaled against a known byte count
 * (MI355X_MICROARCH.md, HBM section). Returns average milliseconds per launch. */
ellc_status ellc_profile_calibrate_read(ellc_ctx* ctx, size_t bytes, int reps, float* avg_ms);
/* Streaming-read rate with 16-byte lanes over `bytes` of device memory: the practical ceiling behind the nominal HBM peak;
 * bench.py reports it beside the roofline (SURVEY.md section 8d asks for the measured figure). */
ellc_status ellc_profile_stream_read(ellc_ctx* ctx, size_t bytes, int reps, float* avg_ms);

/* Device self-test: q_pair[i] from the kernels' packed two-at-a-time IEEE division, q_ref[i] = a[i] / b[i] as the
 * compiler emits it; n even. The per-pixel code relies on the two being bit-identical (tests/test_gpu_gn.py). */
ellc_status ellc_selftest_div_pair(ellc_ctx* ctx, int n, const float* a, const float* b, float* q_pair, float* q_ref);

/* Device self-test of the solve's 6x6 inverse (cv::Mat::inv(DECOMP_LU) restated, PixelWisePyramid.cpp:451): n symmetric
 * matrices, each given by its 21 upper-triangular entries by rows (f64, rounded to f32 as the solve does); inv36 receives
 * the row-major f32 inverses (all zeros for a singular matrix). */
ellc_status ellc_selftest_lu(ellc_ctx* ctx, int n, const double* tri21, float* inv36);


/* Parity hook of the level-bound schedule kernels (gn_fca_fused, gn_fca_dense, gn_fca_dense4, gn_fca_dense_x, gn_ica_fused): stages
 * the batch with pose[b] ([B][6]) as alignment b's pose, builds its compact lists (or H^-1 of the constant-weight path, or none for
 * dense maps) as ellc_align does, launches ONCE the kernel the schedule runs at `level` for this context, batch and mode — the same
 * grid, age-balanced split and XCD relabelling, nothing pending — and runs the finish kernel on its sums. sums27[b]: the blocks'
 * partial records of alignment b summed in double (21 upper-triangular H by rows, then 6 b; the constant-weight kernel writes b only,
 * H is returned as 0); new_pose[b]: the pose after that one Gauss-Newton step; ica_hinv36[b]: the row-major H^-1 of the constant-weight
 * path at `level` (0 in FCA mode). kernel: the launched kernel's name; grid: {blocks per alignment, age rounds, XCD relabelling}.
 * Output pointers may be NULL. Fails for a context or batch that runs the state-driven schedule. */
ellc_status ellc_debug_schedule_sums(ellc_ctx* ctx, int B, const int* kf_slots, const int* frame_slots, int level, int mode,
                                     const float* pose, double* sums27, float* new_pose, float* ica_hinv36, char* kernel, int kernel_len,
                                     int* grid);

/* ---- test hooks of the resident schedule (gn_fca_persist, the tracking call's one-launch form) ------------------------------ */
/* Blocks with index >= first_block of every later resident launch start `polls` sleeps (about a microsecond each) late, as if the
 * dispatcher had placed them late: what a block that writes no records at the coarse levels must survive (it is lapped by the
 * writers and re-joins through the state line). polls = 0 switches the delay off. polls = -r (1 .. 255): no delay; block 0 raises
 * the abort word at the top of round r of every later resident launch — a launch abandoned half-way, which the launch path has to
 * finish with the same bits. */
ellc_status ellc_debug_persist_delay(ellc_ctx* ctx, int first_block, int polls);
/* The call counter the records' tags are made of (24 bits are used): tests set it just below the wrap. */
ellc_status ellc_debug_set_persist_epoch(ellc_ctx* ctx, unsigned epoch);
/* Eager lists (default on in a context that tracks): the depth map's export builds the tracking call's compact lists of its keyframe
 * right behind itself, so that the next alignment against that keyframe starts without the compaction. 0 switches that off (every
 * alignment builds its lists itself, as up to r05): the results must not change by a bit (tests). */
ellc_status ellc_debug_set_eager_lists(ellc_ctx* ctx, int on);
/* A tracking call whose compact lists are already there (eager lists) has no staging launch: its resident launch builds the state
 * records from its arguments and takes the batch description and the seeds count along, and ellc_track_frame's saved weights are
 * added by further blocks of its selection launch (default on). 0: the staging kernel and gn_add_saved_weights_all run as up to r05 —
 * the results must not change by a bit (tests). */
ellc_status ellc_debug_set_fold_staging(ellc_ctx* ctx, int on);
/* Constant-weight path, tolerance mode: the per-(slot, level) H^-1 are kept while the keyframe's planes are unchanged and the
 * per-call compaction then builds the records only (default on). 0: every compaction recomputes them, as up to r05 — the results
 * must not change by a bit (tests). */
ellc_status ellc_debug_set_hinv_cache(ellc_ctx* ctx, int on);
/* The compaction's count launch (prep_count) is left out while every slot a group rebuilds still holds the tile counts of its depth
 * planes as they are (default on). 0: every compaction counts, as up to r06 - the results must not change by a bit (tests). */
ellc_status ellc_debug_set_count_cache(ellc_ctx* ctx, int on);
/* Groups of this context that compacted with a count launch, and without one because the kept counts were current. (A tracking
 * call's count-free compaction and groups that build no lists are in neither.) Either pointer may be NULL. */
ellc_status ellc_debug_count_cache_counters(ellc_ctx* ctx, long long* groups_counted, long long* groups_skipped);
/* The compaction of a launch group ranks its pixels from the valid-bit masks the count launch leaves behind the tile counts and
 * gathers the depth of the valid ones only (default on). 0: it reads the whole depth planes, as up to r09 (kept in this library
 * only) - the same pixels in the same order, so the results must not change by a bit (tests). A plan-time choice, as the packed
 * taps are. The count-free form of a tracking call reads the depth planes either way. */
ellc_status ellc_debug_set_mask_scatter(ellc_ctx* ctx, int on);
/* Scatter launches behind a count launch (now or kept) that this context has enqueued or captured in the masked form and in the
 * depth-reading form - the tests' evidence that the two sides of their comparison ran different kernels. A count-free compaction
 * is in neither. Either pointer may be NULL. */
ellc_status ellc_debug_mask_scatter_counters(ellc_ctx* ctx, long long* masked, long long* from_depth);
/* The valid-bit mask of a keyframe slot at `level`, as the last count launch left it: 64 words per tile of 2048 pixels, bit i of a
 * tile = (depth > 0) of pixel tile * 2048 + i in raster order, zeros past the end of the plane. `out` holds 64 * ceil(n / 2048)
 * words. ELLC_ERR_NOT_READY while the slot's counts are stale (a writer of its depth planes, or a count-free compaction, since). */
ellc_status ellc_debug_get_valid_mask(ellc_ctx* ctx, int kf_slot, int level, uint32_t* out);
/* Tolerance mode: the interior taps of a warped point come as ONE 16-byte load from the frame slot's row-packed plane (default on).
 * 0: as four unaligned row loads from the image plane, as up to r07 (kept in this library only) - the same twelve bytes reach the
 * same arithmetic, so the results must not change by a bit (tests). A plan-time choice: sequences captured under either are kept apart. */
ellc_status ellc_debug_set_packed_taps(ellc_ctx* ctx, int on);
/* How many kernel argument records (one per enqueued or captured pixel-pass launch, one per ellc_align_quality_at call) this context
 * has built with the row loads selected: 0 for a context that never switched the packed taps off, and rising with every kind of call
 * of one that did - the tests' evidence that the other side of their comparison ran the other path. */
ellc_status ellc_debug_row_tap_launches(ellc_ctx* ctx, long long* n);
/* The row-packed plane of a frame slot at `level`: stored_w * stored_h words (ellc_get_image_level's sizes), word (y, x) =
 * I(y-1,x) | I(y,x) << 8 | I(y+1,x) << 16 | I(y+2,x) << 24 with a zero byte for rows outside [0, rows). Tolerance-mode contexts only. */
ellc_status ellc_debug_get_packed_level(ellc_ctx* ctx, int frame_slot, int level, uint32_t* out);
/* Resident launches of this context so far, how many of them the host had to finish with launches (abandoned), and — device-wide,
 * since the library was loaded — how many blocks were lapped and re-joined through the state line. Any pointer may be NULL. */
ellc_status ellc_debug_persist_counters(ellc_ctx* ctx, long long* resident_launches, long long* abandoned_launches, long long* rejoined_blocks);

#ifdef __cplusplus
}
#endif
#endif /* ELLC_ABI_DIAG_H */
