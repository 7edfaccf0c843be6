// Host-side context behind the C ABI (include/ellc_abi.h).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <array>
#include <map>
#include <tuple>
#include "../../include/ellc_abi.h"
#ifdef ELLC_DIAG_ABI
#include "../../include/ellc_abi_diag.h"
#endif
#include "ellc_device.hpp"

namespace ellc {

struct DepthSoA {   // DepthHypothesis.h:14-40, live fields, structure of arrays
  float* invDepth = nullptr;
  float* invDepthSmoothed = nullptr;
  float* variance = nullptr;
  float* varianceSmoothed = nullptr;
  int* validity = nullptr;
  int* blacklisted = nullptr;
  uint8_t* isValid = nullptr;
};

// Everything that shapes one enqueued launch sequence of the alignment path. Whoever starts a sequence (launch_group, the untracked
// branch of align_enqueue_impl, resolve_batch for a continuation, the diagnostic hooks) builds one and passes it down by reference:
// no function of the chain reads a choice from the context, and a new launch-time choice is a new member here (and, when captured
// sequences differ by it, in GraphKey).
struct LaunchPlan {
  int B = 0;                  // alignments the sequence covers
  int nu = 0;                 // unique keyframe slots whose compact lists it (re)builds (uniq_slot_h)
  int mode = ELLC_MODE_FCA;
  int save_weights = 0;
  int set = 0;                // the batch set it runs in
  bool continuation = false;  // the rest of a state-driven schedule whose first part ended early (no staging, no compaction)
  bool dense = false;         // the list-free schedule (gn_fca_dense*)
  int need = 0;               // the record set (PrepArgs::need) the compaction builds: need_of(), or 16 where the slots' H^-1 are current
  bool skip_count = false;    // the compaction relies on the tile counts kept in the slots: no prep_count launch
  bool pollable = false;      // the sequence ends in a finish kernel the host may poll (FusedArgs::host_polls)
  bool resident = false;      // the state-driven schedule as one resident launch (gn_fca_persist)
  int adaptive_first = 0;     // launches of the first part of a state-driven schedule (0: not that schedule, or the resident form)
  bool direct = false;        // launched kernel by kernel, not replayed from a captured graph: the staging record goes through kernel arguments
  bool track = false;         // the alignment belongs to ellc_track_frame (set_track_fields)
  const void* count_valid = nullptr;   // ... whose count of the valid hypotheses the launch that stages the batch takes along
  int count_n = 0;                     //     (the plane's size; 0: none)
  bool row_taps = false;      // diagnostic library only (ellc_debug_set_packed_taps): the tolerance mode's interior taps as four row loads from
                              // FrLevelDev::img, not one load from the row-packed plane (GnArgs::row_taps)
  bool depth_scatter = false; // diagnostic library only (ellc_debug_set_mask_scatter(0)): the compaction of a launch group ranks its pixels
                              // from the depth planes, not from the valid-bit masks kept with the tile counts (prep_scatter<NEED, false>)
};

// ellc_track_frame's request to align_enqueue_impl: the alignment is its own (LaunchPlan::track), and the count it would like taken along
struct TrackRequest {
  const void* count_valid;
  int count_n;   // 0: no count
};

// What tells one captured launch sequence from another: the plan's members that change what is captured, and cfg.grid_batch (the
// grids). resident, direct and the count request are absent: such sequences are never captured.
struct GraphKey {
  int B, nu, mode, save_weights, continuation, track, pollable, adaptive_first, grid_batch, dense, need, skip_count, set, row_taps, depth_scatter;
  bool operator<(const GraphKey& o) const {
    auto t = [](const GraphKey& k) {
      return std::tie(k.B, k.nu, k.mode, k.save_weights, k.continuation, k.track, k.pollable, k.adaptive_first, k.grid_batch, k.dense, k.need, k.skip_count, k.set, k.row_taps, k.depth_scatter);
    };
    return t(*this) < t(o);
  }
};
inline GraphKey graph_key(const LaunchPlan& p, int grid_batch) {
  return GraphKey{p.B, p.nu, p.mode, p.save_weights ? 1 : 0, p.continuation, p.track, p.pollable, p.adaptive_first, grid_batch, p.dense, p.need, p.skip_count, p.set, p.row_taps, p.depth_scatter};
}

// Staging and scratch of a call that reduces B (source, destination) pairs to one record each (ellc_ring_common.hpp: pair_reserve,
// pair_run, pair_free). Not from the arena: they grow with the largest call.
struct PairScratch {
  int cap = 0;                                          // requests the staging holds
  void *stage_h = nullptr, *stage_d = nullptr;          // pinned: [cap] requests as the pass kernel reads them, and the device copy
  void *out_h = nullptr, *out_dev_alias = nullptr;      // pinned: [cap] records (the finish kernel writes them)
  void* partials_d = nullptr;                           // [requests of one launch][tiles of the level] partial records
  size_t partials_cap = 0;                              //   records it holds
};
void pair_free(PairScratch& s);

}  // namespace ellc

struct ellc_ctx {
  ellc_config cfg;
  hipStream_t stream = nullptr;
  std::string err;
  int L = 0;
  ellc::LevelGeom geom_h[ELLC_MAX_LEVELS];
  ellc::LevelGeom* geom_d = nullptr;
  std::vector<void*> allocs;                 // the arena chunks (freed on destroy)
  char* arena_base = nullptr;                // current chunk: device buffers are carved out of a few large allocations
  size_t arena_size = 0, arena_used = 0;
  bool fast = false;                         // cfg.arith == ELLC_ARITH_FAST
  bool row_taps = false;                     // ellc_debug_set_packed_taps(0), diagnostic library only: see LaunchPlan::row_taps
  long long row_tap_args = 0;                //   kernel argument records built with the row loads selected (ellc_debug_row_tap_launches)
  std::vector<void*> host_allocs;            // hipHostMalloc'ed
  std::vector<ellc::KfLevelDev> kf_tab_h;    // [L][max_kf]
  std::vector<ellc::FrLevelDev> fr_tab_h;    // [L][max_fr]
  ellc::KfLevelDev* kf_tab_d = nullptr;
  ellc::FrLevelDev* fr_tab_d = nullptr;
  std::vector<char> kf_has_image, kf_has_depth, fr_has_image;
  // dense hint: the slot's level-0 depth plane was uploaded with at least nine tenths of its pixels valid (ellc_keyframe_set_depth
  // counts them). A tolerance-mode FCA batch whose keyframes all carry the hint is aligned without compact lists (gn_fca_dense:
  // thread <-> pixel, the planes read directly). A hint, not a promise: pixels without depth are skipped where they occur.
  std::vector<char> kf_dense;
  bool dense_maps_off = false;   // ellc_ctx_set_dense_maps(1): dense maps take the list path too (bit-comparison runs)
#ifdef ELLC_NO_DENSE_QUADS
  bool dense_quads = false;   // (A/B builds: the r05 kernel, one pixel per thread)
#else
  bool dense_quads = true;    // list-free launches take four adjacent pixels per thread (gn_fca_dense4) at levels whose width allows
#endif
  // cfg.cache_records: which record set (PrepArgs::need) the compact lists of a keyframe slot hold, 0 = none / stale. The lists
  // are a pure function of the slot's image, depth pyramid and weight planes: every entry point that writes one of those
  // clears the tag (ellc::invalidate_records); a batch rebuilds only the slots whose tag differs from what it needs.
  std::vector<int> kf_rec_tag;
  std::vector<char> kf_rec_eager;   // the slot's lists were built behind the depth map's export and are valid whatever cfg.cache_records says (enqueue_eager_lists)
  bool eager_lists = true;
  bool fold_staging = true;   // a tracking call whose lists are there leaves its staging to the resident launch (PersistStage, stage_folds)
  // ICA, tolerance mode: H^-1 per (slot, level) — the inverse of sum W J^T J over the keyframe's valid pixels (PixelWisePyramid.cpp:938-939)
  // — is a function of the keyframe's planes alone. kf_hinv_ok[slot]: the inverses the last compaction of the slot left are still
  // current (every writer of the planes clears it through invalidate_records): the next compaction builds the records only (r06)
  std::vector<char> kf_hinv_ok;
  bool hinv_cache = true;
  // The compaction's count launch (prep_count) reads every level's depth plane of a slot to leave one integer per tile. Those
  // integers depend on the depth planes alone. kf_counts_ok[slot]: KfLevelDev::tile_count of every level of the slot holds the plain
  // counts a prep_count launch left, and the depth planes have not been written since (every writer clears it through
  // invalidate_records; the count-free form, which stores tagged words there, clears it too): a group whose rebuilt slots all
  // carry the mark launches prep_scatter alone, which reads the kept counts as it reads fresh ones.
  // Behind the counts, in the same allocation, prep_count leaves one valid bit per pixel (prep_mask_offset): same inputs, same only
  // writer, so the same mark covers it. prep_scatter of a launch group ranks its pixels from those bits and never reads a depth
  // plane for its validity.
  std::vector<char> kf_counts_ok;
  bool count_cache = true;
  bool depth_scatter = false;   // ellc_debug_set_mask_scatter(0), diagnostic library only: see LaunchPlan::depth_scatter
  long long scatters_masked = 0, scatters_from_depth = 0;   //   scatter launches behind a count, enqueued or captured, of either form (ellc_debug_mask_scatter_counters)
  long long groups_counted = 0, groups_count_skipped = 0;   // groups launch_group launched with / without a count launch (those that compact at all; the count-free form is neither)
  bool cache_records = false;
  std::vector<std::array<int, ELLC_MAX_LEVELS>> kf_num_weights;
  std::vector<float*> kf_maxgrad, fr_maxgrad;
  std::vector<int*> kf_maxgrad_count, fr_maxgrad_count;
  std::vector<char> kf_maxgrad_valid, fr_maxgrad_valid;
  // alignment work buffers
  int *kf_slot_d = nullptr, *fr_slot_d = nullptr, *uniq_slot_d = nullptr;
  int *kf_slot_h = nullptr, *fr_slot_h = nullptr, *uniq_slot_h = nullptr;   // pinned
  float *init_pose_d = nullptr, *init_pose_h = nullptr;
  ellc::AlignState *state_d = nullptr, *state_h = nullptr;
  ellc::AlignResult* result_h = nullptr;            // pinned; written by the last kernel of a schedule through result_dev_alias
  ellc::AlignResult* result_dev_alias = nullptr;
  const int* stage_dev_alias = nullptr;             // device-side address of the pinned staging record (kf_slot_h ...)
  // Batches in flight (ellc_align_enqueue several times before ellc_align_fetch). The unit that runs on the device is a GROUP:
  // up to cfg.coalesce full batches (B == max_batch) staged side by side in one set of buffers and launched as ONE sequence
  // over all their alignments — a launch over 96 alignments costs little more than one over 32 (the per-launch costs of the
  // dependent chain: launch gap, cold loads, solve, reduction, and the latency-bound coarse levels that do not fill the
  // device, are paid once), r02: 4.7 -> 6.5 M iterations/s at three groups of three in flight. With cfg.coalesce = 1 (default)
  // a group is one batch and everything is as before. Every group has its own pinned staging / result records and device work
  // buffers (staged slots, AlignState, block partials), sized for coalesce x max_batch alignments; launched groups take one of
  // three streams (the main stream first: a caller with one batch at a time never leaves it; a process holds few hardware
  // queues, and streams that end up on the same one do not overlap), so up to three groups run CONCURRENTLY: the latency-bound
  // coarse iterations of one overlap the throughput-bound fine iterations of another. Groups that share a keyframe slot are
  // ordered one after the other (the compaction, H^-1 and the saved weights live in the keyframe slot). There is one set more than
  // batches may be in flight (max_inflight): it takes the batches that arrive while the oldest group is being fetched. The members above point at the set / slice of the batch being
  // staged or the group being launched. All other entry points work on `stream`, launch a group that is still open and make
  // the stream wait for the groups in flight, so a caller sees one in-order queue per context as before.
  static constexpr int MAX_COALESCE = 4;
#ifndef ELLC_STREAMS
#define ELLC_STREAMS 3
#endif
  static constexpr int STREAMS = ELLC_STREAMS;
  static constexpr int SETS = (STREAMS + 1) * MAX_COALESCE + 1;   // of which max_inflight + 1 are used (n_sets): every batch in flight may be a group of its own
  struct BatchSet {
    int* stage_h = nullptr;                         // 9 * cap ints: kf slots, frame slots, unique slots, initial poses (cap = coalesce * max_batch)
    const int* stage_dev_alias = nullptr;
    ellc::AlignResult* result_h = nullptr;
    ellc::AlignResult* result_dev_alias = nullptr;
    hipEvent_t done = nullptr;
    int* stage_d = nullptr;                         // device copy of the staging record
    ellc::AlignState* state_d = nullptr;            // two launch-parity buffers
    float* partials_d = nullptr;
    unsigned* persist_bar_d = nullptr;              // gn_fca_persist's abort words (two alignments; zero between calls)
    // the group staged / in flight in this set
    int fill = 0;                                   // batches staged side by side: batch j = alignments [j * max_batch, ...)
    int fetched = 0;                                // of which fetched (the set is free again when fetched == fill)
    bool launched = false;
    bool coalescable = false;                       // further full batches of the same mode may join until it is launched
    int slice_B[MAX_COALESCE] = {0, 0, 0, 0};       // size of each staged batch
    int stream_idx = 0;                             // the batch stream it was launched on (0: the context's main stream)
    std::vector<int> kf_slots;                      // unique keyframe slots of the group (all of them: the slots it reads)
    std::vector<int> built_slots;                   // of which it rebuilds the compact lists (or accumulates saved weights into)
    int B = 0;                                      // alignments the launch covers
    bool joined = true;                             // the main stream already waits for `done`
    int mode = 0, save_weights = 0;
    bool adaptive = false;                          // the group (one batch) runs the state-driven schedule (gn_fca_adaptive)
    bool resident = false;                          //   as one resident launch (gn_fca_persist)
    int adaptive_first = 0;                         //   whose first graph holds this many launches
    bool pollable = false;                          // its finish kernel ordered its result records for a polling host (FusedArgs::host_polls)
    // ellc_track_frame's alignment: the request (align_enqueue_impl) ...
    bool track = false;                             // its finish kernel builds the observation's matrices and sets the depth stages' gate
    const void* count_valid = nullptr;              // the validity plane whose count the launch that stages the batch is asked to take along
    int count_n = 0;                                //   and its size (0: no count asked for)
    // ... and what launch_group answers
    bool count_rode = false;                        // that launch took the count along (a sequence launched kernel by kernel does)
    bool done_by_caller = false;                    // `done` is left to the caller, who records it behind the depth stages
    bool ride_weights = false;                      // the saved weights wait for the observation's selection launch (launch_observe)
    bool resolved = true;                           // `done` has been waited for and the continuation, if one was needed, has run
  } batch_set[SETS];
  hipStream_t batch_stream[STREAMS] = {};   // [0] = stream; the others are created when first needed
  int stream_waited_mark[STREAMS] = {};      // the main-stream mark each batch stream has been ordered after
  int coalesce = 1;                                 // cfg.coalesce clamped to 1..MAX_COALESCE
  int max_inflight = 3;                             // batches in flight: 3 with coalesce = 1; 4 x coalesce otherwise (three groups
                                                    // running and a fourth queued behind the oldest, so that the device never waits
                                                    // for the host to gather the next group)
  int n_sets = 4;                                   // sets in use: max_inflight + 1
  int group_cap = 0;                                // alignments per set: coalesce * max_batch
  int open_set = -1;                                // the set whose group is staged but not launched yet (-1: none)
  hipEvent_t ev_main = nullptr;                     // marks the main stream behind the last non-batch call
  hipEvent_t ev_xfer = nullptr;                     // ellc_copy_slot_across: orders this context's stream against another context's
  bool main_dirty = false;                          // a non-batch entry point ran since ev_main was recorded
  int main_mark = 0;
  int inflight[SETS * MAX_COALESCE] = {0};         // FIFO of the batches in flight: set * MAX_COALESCE + slice
  int n_inflight = 0;
  int cur_set = 0;                                  // the batch set the per-batch pointers below refer to (select_batch_set)
  float* partials_d = nullptr;
  unsigned* persist_bar_d = nullptr;
  unsigned persist_spin_limit = 1u << 15;           // polls of a missing record before gn_fca_persist gives a launch up (0: at once — test hook)
  unsigned prep_tag = 0;                            // tag of the last compaction without a count launch (PrepArgs::lb_tag)
  unsigned persist_epoch = 0;                       // calls of gn_fca_persist so far (tags of its partial records)
  int persist_delay_from = 0, persist_delay_polls = 0;   // test hook (ellc_debug_persist_delay): blocks from this index on start late
  int persist_backoff = 0;                          // calls that still run as launches after a resident launch had to be abandoned
  long long persist_launches = 0, persist_abandoned = 0;   // resident launches so far / those the host had to finish with launches
  int persist_capacity = 0;                         // blocks of gn_fca_persist the device holds at once (occupancy x CUs)
  bool use_persist = true;                          // the state-driven schedule as one resident launch (gn_fca_persist)
  float* planes_d = nullptr;
  // ellc_align_quality_at: scratch of its own, allocated by the first call (a context that never calls it holds none)
  int* quality_stage_h = nullptr;                               // [max_batch] keyframe slots, [max_batch] frame slots, [max_batch][6] poses; pinned,
  const int* quality_stage_dev_alias = nullptr;                 //   read by the kernel through its device-side address
  float* quality_partials_d = nullptr;                          // [max_batch][blocks of level 0][ELLC_PART_STRIDE]
  int* quality_counts_d = nullptr;                              // [max_batch][blocks of level 0][2]
  ellc_align_quality *quality_out_h = nullptr, *quality_out_dev_alias = nullptr;   // pinned: the finish kernel writes the records
  // ellc_keyframe_map_points: scratch of its own, allocated by the first call
  int* map_stage_h = nullptr;               // pinned: [max_keyframes] slot of every request, [max_keyframes][12] f32 transforms
  int* map_stage_d = nullptr;               //   and its device copy
  int* map_tile_counts_d = nullptr;         // [max_keyframes][tiles of level 0] kept pixels per tile
  unsigned* map_tile_offsets_d = nullptr;   // [max_keyframes][tiles of level 0] records in front of each tile
  int *map_totals_h = nullptr, *map_totals_dev_alias = nullptr;   // pinned: [max_keyframes] points per request, then their sum (map_scan writes them)
  void* map_out_d = nullptr;                // device staging of the records: an allocation of its own that grows with the largest call
  size_t map_out_cap = 0;                   //   records it holds
  // ellc_keyframe_render_depth: scratch of its own, allocated by the first call
  int* render_stage_h = nullptr;            // pinned: [max_keyframes] slot of every request, [max_keyframes][12] f32 transforms, [max_keyframes][2] f32 lights
  void* render_block_d = nullptr;           // one device allocation of its own (several MB at 640x480: not carved from the arena) that holds:
  int* render_stage_d = nullptr;            //   the device copy of the record above
  unsigned long long* render_keys_d = nullptr;   // [W*H] smallest candidate key per target
  float *render_depth_d = nullptr, *render_var_d = nullptr;   // [W*H] the view's planes
  int32_t *render_source_d = nullptr, *render_agree_d = nullptr;
  uint8_t* render_intensity_d = nullptr;
  int* render_block_counts_d = nullptr;     // [ceil(W*H / 256)] targets with a winner per block of render_resolve
  int *render_nvalid_h = nullptr, *render_nvalid_dev_alias = nullptr;   // pinned: their sum (render_finish writes it)
  // ellc_keyframe_fuse_depth: the render's scratch above (its kernels run first) and, of its own, allocated by the first call:
  void* fuse_block_d = nullptr;             // one device allocation that holds:
  unsigned* fuse_cursor_d = nullptr;        //   [W*H] begin, then end, of every target's segment of the list
  int32_t* fuse_merged_d = nullptr;         //   [W*H] the merged plane
  unsigned long long* fuse_tile_sums_d = nullptr;   // [tiles of level 0] agreeing candidates per tile
  int* fuse_block_counts_d = nullptr;       //   [ceil(W*H / 256)] fused targets per block of fuse_merge
  long long *fuse_totals_h = nullptr, *fuse_totals_dev_alias = nullptr;   // pinned: the list's size (fuse_offsets), n_fused (fuse_finish)
  unsigned long long* fuse_mask_d = nullptr;   // one bit per source pixel of every request (fuse_agree): grows with the largest requests x tiles
  size_t fuse_mask_cap = 0;                 //   words it holds
  uint32_t* fuse_list_d = nullptr;          // the candidate ids, segment after segment: an allocation of its own that grows with the largest call
  size_t fuse_list_cap = 0;                 //   entries it holds
  // ellc_depth_absorb_keyframes: the render's and the fusion's scratch above and, of its own, allocated by the first call:
  void* absorb_block_d = nullptr;           // [64] words for absorb_mark's four counts, then [ceil(W*H / 256)][11] outcome counts per block of absorb_fold
  int32_t *absorb_stats_h = nullptr, *absorb_stats_dev_alias = nullptr;   // pinned: the sixteen words of ellc_absorb_stats (absorb_finish)
  // ellc_keyframe_depth_consistency, ellc_keyframe_sim3_step / _step_lit / _align / _align_lit, ellc_keyframe_trial_propagate,
  // ellc_keyframe_light_step (through ellc_keyframe_sim3_align_lit too): a PairScratch each, and the trial call's bitmaps
  ellc::PairScratch consist, sim3, trial, light;
  ellc::PairScratch trial_lit;              // ellc_keyframe_trial_propagate_lit: its records are twice as wide
  unsigned* trial_bits_d = nullptr;         // [requests of one launch][ceil(W*H / 32)] one bit per target pixel
  size_t trial_bits_cap = 0;                //   words it holds
  // ellc_keyframe_refine_depth: a PairScratch (the views' staging, one record, the blocks' partial records) and the four planes it returns
  ellc::PairScratch refine;
  void* refine_planes_d = nullptr;          // [n] f32 depth, [n] f32 variance, [n] u8 views, [n] u8 status of the largest level asked for
  size_t refine_planes_cap = 0;             //   pixels it holds
  // ellc_keyframe_sweep_depth: a PairScratch of its own; the four planes it returns are the refinement's (both calls are synchronous)
  ellc::PairScratch sweep;
  // ellc_keyframe_cull_depth: a PairScratch of its own (a staged view carries two more pointers) and its five planes
  ellc::PairScratch cull;
  void* cull_planes_d = nullptr;            // [n] f32 depth, [n] f32 variance, [n] u32 votes, [n] u8 photo, [n] u8 status of the largest level asked for
  size_t cull_planes_cap = 0;               //   pixels it holds
  // ellc_keyframe_joint_step / _apply / _refine: a PairScratch for the views' staging and the records of joint_pairs, one for the counts of
  // the per-pixel kernels, and the family's planes
  ellc::PairScratch joint, joint_count;
  void* joint_planes_d = nullptr;           // ten f32 and five u8 planes of the largest level asked for (ellc_joint_impl.hpp names them)
  size_t joint_planes_cap = 0;              //   pixels each holds
  float *scratch_a = nullptr, *scratch_b = nullptr;   // W*H f32 each
  int tile_begin[ELLC_MAX_LEVELS + 1];
  int cap[ELLC_MAX_LEVELS];                            // compact capacity per level (= n)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // captured launch sequences, one per GraphKey (ellc::graph_key of the LaunchPlan): launch_align_graph
  std::map<ellc::GraphKey, hipGraphExec_t> graphs;
  long long counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // ELLC_CTR_* (ellc_abi.h): ellc_ctx_counters
  int poll_timeout_us = 2000;   // resolve_batch polls this long before it falls back to the event
  bool poll_results = true;     // resolve_batch polls the pinned result records of small single-stream batches; ELLC_NO_POLL=1 (diag)
  bool use_graph = true;
  int direct_max_batch = 0;     // level-bound launch sequences over at most this many alignments are launched kernel by kernel too (measured for B = 1: 0.225 ms either way)
  bool graph_adaptive = false;  // the state-driven (tracking) schedule as a captured graph too; ELLC_GRAPH_ADAPTIVE=1 (diag)
  bool age_balance = true;      // age-balanced split of full-round grids (FusedArgs::age_rounds); ELLC_NO_AGE_BALANCE=1 disables
  double age_weight[5][4] = {{1, 1, 1, 1}, {1, 1, 1, 1}, {1.15, 0.85, 1, 1}, {1.2, 1.0, 0.8, 1}, {1.35, 1.15, 0.9, 0.6}};   // [rounds][round], ELLC_AGE_W (r01 sweep at 640x480, batch 32)
  double age_min_px_per_thread = 5.0;   // ELLC_AGE_MIN_PX
  bool use_adaptive = true;             // early-exit FCA schedules are state-driven (gn_fca_adaptive); ELLC_NO_ADAPTIVE=1 (diag) turns it off
  int adaptive_max_batch = 2;           //   for batches of at most this many alignments; ELLC_ADAPTIVE_MAX_BATCH (diag)
  int adaptive_hint = 0;                //   launches of the next first graph, from what the previous call needed (0: none yet)
  int adaptive_first_override = 0;      //   launches of the first graph; ELLC_ADAPTIVE_FIRST (diag)
  bool pipe = true;             // software-pipelined record loads in the fused FCA kernel (ELLC_PIPE=0 disables; r01: -10 % per launch at
                                // 1280x960 dense where the records stream from HBM, neutral at 640x480 semi-dense)
  bool use_fused = true;        // the production schedules (ELLC_NO_FUSE=1, diagnostic builds: one accumulate + one solve launch per iteration)
  int nblk_override[ELLC_MAX_LEVELS] = {0};
  int resident_blocks = 1280;   // 256-thread blocks of the accumulate kernel resident on the device at once
  // image uploads: ring of pinned staging buffers, so an upload only enqueues (ellc_hip.hip: upload_pyramid)
  static constexpr int UPLOAD_RING = 4;
  uint8_t* upload_stage[UPLOAD_RING] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t upload_done[UPLOAD_RING] = {nullptr, nullptr, nullptr, nullptr};
  int upload_cursor = 0;
  // frame uploads run on a stream of their own (created by the first ellc_frame_upload): per frame slot the event of its last
  // main-stream reader (mark_frame_use) and of its last upload
  hipStream_t upload_stream = nullptr;
  std::vector<hipEvent_t> fr_use_ev, fr_ready_ev;
  // frame ingest (ellc_ingest_configure): fixed-point undistortion map of the 2x2 source pixels of every output pixel
  void* ingest_map = nullptr;
  uint8_t* ingest_bgr = nullptr;    // staging for one full-size BGR frame
  int ingest_w = 0, ingest_h = 0;
  // depth map (one per context)
  ellc::DepthSoA dm_cur, dm_oth;
  int dm_kf_slot = -1;
  bool dm_ready = false;
  float dm_depth_scale = 1.0f, dm_global_scale = 1.0f;
  float *dm_deptharr0 = nullptr, *dm_vararr0 = nullptr;     // level-0 arrays in the reference's array convention
  // propagate scratch
  int *pr_tgt = nullptr, *pr_cnt = nullptr, *pr_slots = nullptr, *pr_val = nullptr, *pr_remaining = nullptr;   // pr_remaining: a counter word (ellc_depth_seeds)
  float *pr_id = nullptr, *pr_var = nullptr;
  double* red_scratch = nullptr;                            // reductions (rescale factor)
  double* sum_parts = nullptr;                              // per-tile (sum, count) of dm_reg_fill_reg for the rescale in the export's launch
  // ellc_track_frame: the observation's matrices and the gate, built on the device behind the alignment; a host-visible record
  void* track_mats_d = nullptr;
  int* track_gate_d = nullptr;
  int* seed_acc = nullptr;   // dm_count_valid_block: sum and arrival ticket (zero between calls)
  int obs_parity = 0;              // which of the two counter sets the next observation uses
  float2* obs_list_ep = nullptr;   // the epipolar direction of every list entry
  int *obs_list = nullptr, *obs_ctr = nullptr;   // work list of dm_observe_select / dm_observe_walk and its counters (zero between calls)
  int* track_h = nullptr;    // host-visible: [0] the valid hypotheses before the observation, [1] the number of the count that wrote it
  bool ride_saved_weights = true;   // a tracking call's saved weights wait for its selection launch (BatchSet::ride_weights; ellc_debug_set_fold_staging(0): a launch of their own)
  int track_counts = 0;      // counts launched so far (ellc_track_frame waits for [1] to say this one)
  int* track_dev_alias = nullptr;
  float Kinv[9], Kmat[9];
};

namespace ellc {
ellc_status fail(ellc_ctx* c, ellc_status s, const std::string& msg);
ellc_status enqueue_eager_lists(ellc_ctx* c, int slot);   // the tracking call's lists of a keyframe slot, built behind the export of its planes
void invalidate_records(ellc_ctx* c, int slot);   // the slot's planes are about to change: its compact lists, H^-1 and tile counts no longer match them
void invalidate_lists(ellc_ctx* c, int slot);     // ... its weight planes only: the lists and H^-1, not the tile counts (they depend on the depth alone)
#define ELLC_HIP(ctx, expr)                                                                               \
  do {                                                                                                    \
    hipError_t e__ = (expr);                                                                              \
    if (e__ != hipSuccess) return ellc::fail(ctx, ELLC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
  } while (0)

// Every entry point makes the context's device current for the calling thread first: HIP's current device is per
// thread, and the reference calls GetImagePoseEstimate from a second (loop-closure) thread (GlobalOptimize.cpp:241).
ellc_status enter(ellc_ctx* c, bool join);
#define ELLC_ENTER_IMPL(ctx, join)                      \
  do {                                                  \
    if (ctx) {                                          \
      const ellc_status s__ = ellc::enter(ctx, join);   \
      if (s__ != ELLC_OK) return s__;                   \
    }                                                   \
  } while (0)
#define ELLC_ENTER(ctx) ELLC_ENTER_IMPL(ctx, true)          // runs on the main stream, behind the batches in flight
#define ELLC_ENTER_BATCH(ctx) ELLC_ENTER_IMPL(ctx, false)   // ellc_align_enqueue / ellc_align_fetch

int choose_nblk(const ellc_ctx* c, int level, int B, bool dense);   // dense: the grid of a list-free launch (callers outside the alignment path: false)
ellc_status run_prep(ellc_ctx* c, const LaunchPlan& p);
ellc_status build_depth_pyramid(ellc_ctx* c, int slot);
ellc_status build_depth_pyramid_from(ellc_ctx* c, int slot, int first_level);
ellc_status build_maxgrad(ellc_ctx* c, bool is_kf, int slot);
ellc_status build_image_pyramid(ellc_ctx* c, uint8_t* const* img, hipStream_t st);
ellc_status pack_frame_taps(ellc_ctx* c, int slot, hipStream_t st);
ellc_status mark_frame_use(ellc_ctx* c, int slot);
}  // namespace ellc
