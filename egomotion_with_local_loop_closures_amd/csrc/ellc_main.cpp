// ellc_main — a main.cpp-shaped driver over the facade (reference: src/main.cpp:199-505): tracks a sequence of
// grey frames against the active keyframe, refines / propagates the semi-dense depth map, switches keyframe every
// KEYFRAME_PROPAGATE_INTERVAL frames and writes the reference's result files:
//   poses_orig.txt   frameId kfId wx wy wz vx vy vz(poseWrtWorld) rescaleFactor seeds%        (main.cpp:373)
//   matchframes.txt  frameId kfId pose6(poseWrtOrigin) rescaleFactor seeds% 0 0 0               (main.cpp:382)
//   matchframes_globalopt.txt (LC mode)  testId matchId pose6 rescale seeds matchValue rms_error view_angle   (GlobalOptimize.cpp:580)
//   <id>_{Depth,Depth_pyr0,DepthVarArr_pyr0}.txt (--save-mats DIR)  text checkpoints of the active keyframe at every
//                    keyframe switch (ImageFunc.cpp:73-87, Frame.cpp:697-871); --replicate DIR reads them back (:58-66)
// --init-poses FILE  FLAG_INITIALIZE_NONZERO_POSE (main.cpp:207-225): one line "frameNo wx wy wz vx vy vz" (world pose,
//                    the so3poses7.txt of the rotation-averaging step) per tracked frame; supplies the initial rotation
// --no-fused         every stage of a tracked frame as its own call, the pose through the host (GetImagePoseEstimate, then observe /
//                    regularise / export). Default (--fused): tracked frames through ellc_track_frame — the depth stages are enqueued
//                    behind the alignment and read its pose on the device (same files, same bits); since r04 (fill + regularise +
//                    export in one launch behind the observation) 0.207-0.209 against 0.213-0.217 ms per frame in bench.py's loop
// --bgr              the input holds decoded full-size BGR frames (4W x 4H x 3 bytes each): grey conversion, undistortion with
//                    the reference's hard-coded camera (ExternVariable.h:53-62, scaled to the input size) and the 1/4
//                    resize run on the device (Frame.cpp:45-75); --no-undistort = FLAG_DO_UNDISTORTION off
// --world N --rank r [--device d] with --comm-id FILE (RCCL: rank 0 writes its 128-byte unique id there, the others read it)
//                    or --comm-tcp PORT (TCP on 127.0.0.1 through rank 0): one process per GPU, every process tracks the whole
//                    sequence, the loop-closure batch (GlobalOptimize.cpp:480-610) is sharded over the ranks by
//                    ellc_shard_range and its poses are gathered once per batch (ellc_gather_results); every rank writes
//                    the same files into its own out_dir
// --match-quality PATH  (LC mode) one line per line of matchframes_globalopt.txt: "frameId kfId n_depth n_used rms wrms" — how well the
//                    candidate fits at the pose the batch returned (ellc_align_quality_at, level 0); every other file is unchanged.
//                    Single process only: refused with --world > 1 (the gather record stays 8 floats)
// --match-geometry PATH  (LC mode) one line per line of matchframes_globalopt.txt: "frameId kfId n_kept n_in_view n_overlap n_agree
//                    n_in_front n_behind scale mean_chi2 mean_abs_di" — the candidate's map against the pushed keyframe's at the pose the
//                    batch returned, after the two maps were brought to one scale (ellc_keyframe_depth_consistency, level 0, the filter
//                    of --map, agree_k2 1; globalOptimize::collectMatchGeometry); every other file is unchanged. With --world > 1 every
//                    rank computes the whole batch: the ring is replicated
// --match-sim3 PATH  (LC mode) one line per line of matchframes_globalopt.txt: "frameId kfId scale tx ty tz wx wy wz n_photo n_depth
//                    chi2_photo chi2_depth iters" - the similarity transform from the candidate's camera into the pushed keyframe's,
//                    refined over seven parameters from the pose the batch returned (ellc_keyframe_sim3_align;
//                    globalOptimize::refineMatchSim3); every other file is unchanged. With --world > 1 every rank computes the whole batch
// --match-light      (LC mode, with --match-sim3 only: a usage error otherwise) the refinement fits an affine brightness between the
//                    pair before every step (ellc_keyframe_sim3_align_lit; globalOptimize::matchAffineLight) and every line of the
//                    --match-sim3 file ends in " gain offset"; without the flag every output file is as before
// --refine-matches PATH  (LC mode, with --match-sim3 only: a usage error otherwise) behind the Sim(3) refinement the pushed keyframe's
//                    ring map is refined against the images of its candidates at the inverted refined transforms and lights
//                    (ellc_keyframe_refine_depth, level 0, into the keyframe's own ring slot; globalOptimize::refineMatchDepth); PATH gets
//                    one line per push that had candidates: "frameId views n_kept n_taking_part n_refined n_too_few_views
//                    n_no_information n_bad_step n_views_changed n_cost_rose sum_views sum_cost_before sum_cost_after". Without the
//                    flag every output file is as before
// --sweep-matches PATH  (LC mode, with --match-sim3 only: a usage error otherwise) behind the Sim(3) refinement, and in front of
//                    --refine-matches' step where both are given, the pixels of the pushed keyframe's ring map that hold no hypothesis
//                    get one from a depth sweep against the images of its candidates at the inverted refined transforms and lights
//                    (ellc_keyframe_sweep_depth, level 0, default parameters, into the keyframe's own ring slot;
//                    globalOptimize::sweepMatchDepth); PATH gets one line per push that had candidates: "frameId views n_ok n_swept
//                    n_created n_no_valid_sample n_at_range_end n_cost_too_high n_not_distinct n_flat sum_views sum_cost". Without the
//                    flag every output file is as before
// --joint-matches PATH (LC mode, with --match-sim3 only: a usage error otherwise) behind the Sim(3) refinement and --sweep-matches' step,
//                    in place of --refine-matches' step where both are given and before --cull-matches' step, the transforms of the
//                    first eight candidates and the pushed keyframe's ring map are refined together (ellc_keyframe_joint_refine, level 0,
//                    the filter of --map, default parameters, six iterations at most, into the keyframe's own ring slot;
//                    globalOptimize::refineMatchJoint); the refined transforms replace the Sim(3) refinement's for what follows. PATH
//                    gets one line per push that had candidates: "frameId views iters n_kept n_taking_part n_used n_too_few_views
//                    n_no_information n_terms chi2_photo chi2_prior". Without the flag every output file is as before
// --cull-matches PATH  (LC mode, with --match-sim3 only: a usage error otherwise) behind the Sim(3) refinement, and behind
//                    --refine-matches' step where both are given, the hypotheses of the pushed keyframe's ring map that its
//                    candidates contradict at the inverted refined transforms and lights are removed (ellc_keyframe_cull_depth,
//                    level 0, every hypothesis taking part, default parameters, into the keyframe's own ring slot;
//                    globalOptimize::cullMatchDepth); PATH gets one line per push that had candidates: "frameId views n_kept
//                    n_retained n_unseen n_culled_free_space n_culled_unsupported n_culled_photo sum_agree sum_in_front sum_behind
//                    sum_photo sum_photo_bad". Without the flag every output file is as before
// --map FILE        (LC mode) at the end of the run the ring's keyframes as one world-frame point cloud (globalOptimize::exportLocalMap:
//                    level 0, no variance test, at least 3 supporting neighbours, support_k2 1, every pixel), written as binary PLY
//                    (x y z float, intensity uchar, var float); every other file is unchanged
// --render FILE      (LC mode) at the end of the run the ring's keyframes rendered into the view of the last pushed keyframe
//                    (globalOptimize::renderLocalMap: level 0, the filter of --map, agree_k2 1); the depth plane is written as a
//                    little-endian PFM ("Pf", rows bottom to top, 0 where nothing landed); every other file is unchanged
// --fuse FILE        (LC mode) the same view with the ring's agreeing hypotheses merged per target (globalOptimize::fuseLocalMap: the
//                    filter and agree_k2 of --render, at most 64 members per target), its depth plane written as such a PFM; every
//                    other file is unchanged. --fuse-inputs DIR (with --fuse) also writes what that view was made from, for a caller to
//                    fuse it again through another binding: T.bin ([requests][12] f32, keyframe camera -> view camera, request order) and
//                    slot<k>.depth / slot<k>.var (request k's level-0 planes, raw f32 rows top to bottom)
// --absorb-matches FILE  (LC mode) what every push's batch found is folded into the LIVE depth map of the pushed keyframe
//                    (globalOptimize::absorbMatches: the batch and its Sim(3) refinement run synchronously, the candidates' ring slots are
//                    copied into tracking-context keyframe slots 2, 3, ..., ellc_depth_absorb_keyframes with the default parameters), so
//                    the map createKeyFrame propagates next carries it; FILE gets "frameId B" and the fifteen stats per push. The
//                    tracking context is created with max_keyframes 2 + 43. Without the flag every output file is what it was.
//                    Together with --match-light the fold is ellc_depth_absorb_keyframes_lit at every candidate's refined light
// --restore-connection FILE  (LC mode) FLAG_RESTORE_CONNECTION (main.cpp:252-324): before a frame is tracked the live map is checked
//                    (globalOptimize::checkConnection); when it has no seeds left the frame is re-localised against the ring
//                    (globalOptimize::findConnection with restoreConnection on: one batched alignment, one ellc_keyframe_trial_propagate,
//                    ellc_depth_restart_from_keyframes from the best candidate). On success the pose and match lines of main.cpp:289 / :301
//                    are written, the frame becomes the active keyframe and the next frame is taken; otherwise the frame is dropped.
//                    FILE gets one line per lost frame, "frameId n_candidates chosen_kfId n_targets seeds_after rescale" ("frameId
//                    n_candidates -1 0 0 0" for a frame without a connection). The tracking context is created with max_keyframes 3
//                    at least. Without the flag every output file is what it was
// --restore-light    (LC mode, with --restore-connection only: a usage error otherwise) globalOptimize::restoreAffineLight: the
//                    candidates are scored by ellc_keyframe_trial_propagate_lit at (1, 0), a light is fitted per candidate
//                    (ellc_trial_light_solve), they are scored again at it, and the map restarts through
//                    ellc_depth_restart_from_keyframes_lit at the winner's light; every line of FILE ends in " gain offset" (the
//                    winner's; "1 0" for a frame without a connection)
// Input is otherwise a header-less file of W*H u8 grey frames (the decode itself always stays outside).
// In LC mode finished keyframes go through the loop-closure ring (facade class globalOptimize): matching and the batched
// alignment of a pushed keyframe run on a second thread and a second context beside tracking, joined at the next push
// (GlobalOptimize.cpp:241 / :161); tracking-loss recovery (findConnection) runs with --restore-connection only, and the MATLAB
// rotation averaging is not part of this path.
#include "../../include/ellc_facade.hpp"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>
#include <unistd.h>

using namespace ellc;

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s frames.raw W H num_frames out_dir [LC] [levels] [--save-mats DIR] [--replicate DIR] [--init-poses FILE] [--bgr] [--no-undistort] [--match-quality PATH] [--match-geometry PATH] [--match-sim3 PATH [--match-light] [--sweep-matches PATH] [--refine-matches PATH] [--joint-matches PATH] [--cull-matches PATH]] [--map FILE] [--render FILE] [--fuse FILE [--fuse-inputs DIR]] [--absorb-matches FILE] [--restore-connection FILE] [--restore-light]\n", argv[0]);
    return -1;
  }
  const std::string in = argv[1], outdir = argv[5];
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), max_frame_counter = std::atoi(argv[4]);
  bool lc = false;
  int levels = 4;
  std::string save_mats, replicate, init_poses;
  bool bgr = false, undistort = true, no_fused = false, match_light = false, restore_light = false;
  int world = 1, rank = 0, device = 0, comm_port = 0;
  std::string comm_id_file, match_quality, match_geometry, match_sim3, refine_matches, sweep_matches, cull_matches, joint_matches, map_file, render_file, fuse_file, fuse_inputs, absorb_matches, restore_connection;
  for (int i = 6; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "LC") lc = true;
    else if (a == "--save-mats" && i + 1 < argc) save_mats = argv[++i];
    else if (a == "--replicate" && i + 1 < argc) replicate = argv[++i];
    else if (a == "--init-poses" && i + 1 < argc) init_poses = argv[++i];
    else if (a == "--bgr") bgr = true;
    else if (a == "--no-undistort") undistort = false;
    else if (a == "--fused") no_fused = false;   // (default) tracked frames through ellc_track_frame (alignment + depth stages as one device sequence)
    else if (a == "--no-fused") no_fused = true;   // every stage as its own call: GetImagePoseEstimate, then observe / regularise / export
    else if (a == "--world" && i + 1 < argc) world = std::atoi(argv[++i]);
    else if (a == "--rank" && i + 1 < argc) rank = std::atoi(argv[++i]);
    else if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
    else if (a == "--comm-id" && i + 1 < argc) comm_id_file = argv[++i];
    else if (a == "--comm-tcp" && i + 1 < argc) comm_port = std::atoi(argv[++i]);
    else if (a == "--match-quality" && i + 1 < argc) match_quality = argv[++i];
    else if (a == "--match-geometry" && i + 1 < argc) match_geometry = argv[++i];
    else if (a == "--match-sim3" && i + 1 < argc) match_sim3 = argv[++i];
    else if (a == "--match-light") match_light = true;
    else if (a == "--restore-light") restore_light = true;
    else if (a == "--refine-matches" && i + 1 < argc) refine_matches = argv[++i];
    else if (a == "--sweep-matches" && i + 1 < argc) sweep_matches = argv[++i];
    else if (a == "--cull-matches" && i + 1 < argc) cull_matches = argv[++i];
    else if (a == "--joint-matches" && i + 1 < argc) joint_matches = argv[++i];
    else if (a == "--map" && i + 1 < argc) map_file = argv[++i];
    else if (a == "--render" && i + 1 < argc) render_file = argv[++i];
    else if (a == "--fuse" && i + 1 < argc) fuse_file = argv[++i];
    else if (a == "--fuse-inputs" && i + 1 < argc) fuse_inputs = argv[++i];
    else if (a == "--absorb-matches" && i + 1 < argc) absorb_matches = argv[++i];
    else if (a == "--restore-connection" && i + 1 < argc) restore_connection = argv[++i];
    else if (!a.empty() && a[0] >= '0' && a[0] <= '9') levels = std::atoi(a.c_str());
    else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return -1; }
  }
  if (match_light && match_sim3.empty()) {
    std::fprintf(stderr, "--match-light needs --match-sim3 PATH: the light is fitted inside the Sim(3) refinement and reported in its file\n");
    return -1;
  }
  if (restore_light && restore_connection.empty()) {
    std::fprintf(stderr, "--restore-light needs --restore-connection FILE: the light is fitted inside the search for a new connection and reported in its file\n");
    return -1;
  }
  if (!refine_matches.empty() && match_sim3.empty()) {
    std::fprintf(stderr, "--refine-matches needs --match-sim3 PATH: the map is refined at the transforms the Sim(3) refinement returns\n");
    return -1;
  }
  if (!sweep_matches.empty() && match_sim3.empty()) {
    std::fprintf(stderr, "--sweep-matches needs --match-sim3 PATH: the sweep runs at the transforms the Sim(3) refinement returns\n");
    return -1;
  }
  if (!cull_matches.empty() && match_sim3.empty()) {
    std::fprintf(stderr, "--cull-matches needs --match-sim3 PATH: the vote runs at the transforms the Sim(3) refinement returns\n");
    return -1;
  }
  if (!joint_matches.empty() && match_sim3.empty()) {
    std::fprintf(stderr, "--joint-matches needs --match-sim3 PATH: the joint refinement starts at the transforms the Sim(3) refinement returns\n");
    return -1;
  }
  if (!match_quality.empty() && world > 1) {
    std::fprintf(stderr, "--match-quality is for a single process: with --world > 1 the ranks exchange poses only (8 floats per alignment)\n");
    return -1;
  }
  const int KEYFRAME_PROPAGATE_INTERVAL = 8;   // ExternVariable.h:39
  std::ifstream f(in, std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", in.c_str()); return -1; }
  std::ofstream pose_file_orig(outdir + "/poses_orig.txt"), match_file(outdir + "/matchframes.txt");
  if (!pose_file_orig || !match_file) { std::fprintf(stderr, "cannot open output files in %s\n", outdir.c_str()); return -1; }
  try {
    ellc_config cfg;
    ellc_default_config(&cfg, W, H, levels);
    cfg.device = device;   // the tracking context: keyframe slots 0,1 (active / incoming), one alignment at a time; in LC mode the
                           // loop-closure ring and its batches live in a context of their own (facade class globalOptimize)
    if (lc && !absorb_matches.empty()) cfg.max_keyframes = 2 + globalOptimize::MAX_LOOP_ARRAY_LENGTH_SCALE_AVG;   // the candidates' copies (absorbMatches)
    if (lc && !restore_connection.empty() && cfg.max_keyframes < 3) cfg.max_keyframes = 3;   // the chosen candidate's copy (restoreConnection)
    Runtime rt(cfg);
    struct CommOwner {   // destroyed after the loop, before the runtime
      ellc_comm* c = nullptr;
      ~CommOwner() { if (c) ellc_comm_destroy(c); }
    } comm;
    if (world > 1) {
      if (rank < 0 || rank >= world || (comm_id_file.empty() && comm_port <= 0)) { std::fprintf(stderr, "--world needs --rank and --comm-id FILE or --comm-tcp PORT\n"); return -1; }
      const int max_total = globalOptimize::MAX_LOOP_ARRAY_LENGTH_SCALE_AVG;
      ellc_status st;
      if (!comm_id_file.empty()) {
        unsigned char id[128];
        if (rank == 0) {
          if (ellc_comm_unique_id(id) != ELLC_OK) { std::fprintf(stderr, "ellc_comm_unique_id failed\n"); return -2; }
          std::remove(comm_id_file.c_str());   // a stale id from an earlier run must not be picked up (give every run a fresh path anyway)
          std::ofstream o((comm_id_file + ".tmp").c_str(), std::ios::binary);
          o.write((const char*)id, 128);
          o.close();
          std::rename((comm_id_file + ".tmp").c_str(), comm_id_file.c_str());
        } else {
          for (int attempt = 0;; attempt++) {
            std::ifstream idf(comm_id_file.c_str(), std::ios::binary);
            if (idf && idf.read((char*)id, 128)) break;
            if (attempt > 600) { std::fprintf(stderr, "no unique id in %s after 60 s\n", comm_id_file.c_str()); return -2; }
            usleep(100000);
          }
        }
        st = ellc_comm_init_rccl(device, id, world, rank, max_total, &comm.c);
      } else {
        st = ellc_comm_init_tcp("127.0.0.1", comm_port, world, rank, max_total, &comm.c);
      }
      if (st != ELLC_OK) { std::fprintf(stderr, "communicator: %s\n", ellc_comm_last_error(comm.c)); return -2; }
      rt.comm = comm.c; rt.world = world; rt.rank = rank;
    }
    rt.FLAG_DO_LOOP_CLOSURE = lc;
    rt.KEYFRAME_PROPAGATE_INTERVAL = KEYFRAME_PROPAGATE_INTERVAL;
    if (!save_mats.empty()) { rt.FLAG_SAVE_MATS = true; rt.SAVED_MATS_PATH = save_mats; }
    if (!replicate.empty()) { rt.FLAG_REPLICATE_POSE_ESTIMATION = true; rt.SAVED_MATS_PATH = replicate; }
    std::ifstream initialize_pose_file;
    if (!init_poses.empty()) {
      initialize_pose_file.open(init_poses.c_str());
      if (!initialize_pose_file) { std::fprintf(stderr, "cannot open %s\n", init_poses.c_str()); return -1; }
    }
    depthMap currentDepthMap(rt);
    std::unique_ptr<globalOptimize> globalOptimizeLoop;
    if (lc) globalOptimizeLoop.reset(new globalOptimize(rt, outdir + "/matchframes_globalopt.txt"));
    if (lc && !match_quality.empty()) {
      globalOptimizeLoop->match_quality_file.open(match_quality.c_str());
      if (!globalOptimizeLoop->match_quality_file) { std::fprintf(stderr, "cannot open %s\n", match_quality.c_str()); return -1; }
      globalOptimizeLoop->collectMatchQuality = true;
    }
    if (lc && !match_geometry.empty()) {
      globalOptimizeLoop->match_geometry_file.open(match_geometry.c_str());
      if (!globalOptimizeLoop->match_geometry_file) { std::fprintf(stderr, "cannot open %s\n", match_geometry.c_str()); return -1; }
      globalOptimizeLoop->collectMatchGeometry = true;
    }
    if (lc && !match_sim3.empty()) {
      globalOptimizeLoop->match_sim3_file.open(match_sim3.c_str());
      if (!globalOptimizeLoop->match_sim3_file) { std::fprintf(stderr, "cannot open %s\n", match_sim3.c_str()); return -1; }
      globalOptimizeLoop->refineMatchSim3 = true;
      globalOptimizeLoop->matchAffineLight = match_light;
    }
    if (lc && !refine_matches.empty()) {
      globalOptimizeLoop->refine_matches_file.open(refine_matches.c_str());
      if (!globalOptimizeLoop->refine_matches_file) { std::fprintf(stderr, "cannot open %s\n", refine_matches.c_str()); return -1; }
      globalOptimizeLoop->refineMatchDepth = true;
    }
    if (lc && !sweep_matches.empty()) {
      globalOptimizeLoop->sweep_matches_file.open(sweep_matches.c_str());
      if (!globalOptimizeLoop->sweep_matches_file) { std::fprintf(stderr, "cannot open %s\n", sweep_matches.c_str()); return -1; }
      globalOptimizeLoop->sweepMatchDepth = true;
    }
    if (lc && !cull_matches.empty()) {
      globalOptimizeLoop->cull_matches_file.open(cull_matches.c_str());
      if (!globalOptimizeLoop->cull_matches_file) { std::fprintf(stderr, "cannot open %s\n", cull_matches.c_str()); return -1; }
      globalOptimizeLoop->cullMatchDepth = true;
    }
    if (lc && !joint_matches.empty()) {
      globalOptimizeLoop->joint_matches_file.open(joint_matches.c_str());
      if (!globalOptimizeLoop->joint_matches_file) { std::fprintf(stderr, "cannot open %s\n", joint_matches.c_str()); return -1; }
      globalOptimizeLoop->refineMatchJoint = true;
    }
    if (lc && !absorb_matches.empty()) {
      globalOptimizeLoop->absorb_file.open(absorb_matches.c_str());
      if (!globalOptimizeLoop->absorb_file) { std::fprintf(stderr, "cannot open %s\n", absorb_matches.c_str()); return -1; }
      globalOptimizeLoop->absorbMatches = true;   // (pushToArray turns the Sim(3) refinement on for its batch)
    }
    std::ofstream restore_file;
    if (lc && !restore_connection.empty()) {
      restore_file.open(restore_connection.c_str());
      if (!restore_file) { std::fprintf(stderr, "cannot open %s\n", restore_connection.c_str()); return -1; }
      globalOptimizeLoop->restoreConnection = true;
      globalOptimizeLoop->restoreAffineLight = restore_light;
    }
    std::vector<std::unique_ptr<frame>> frameptr_vector;
    frame* activeKeyFrame = nullptr;
    std::vector<uint8_t> buf(bgr ? (size_t)W * H * 48 : (size_t)W * H);
    if (bgr) {   // the reference's camera is given for 1920 x 1080 (ExternVariable.h:53-62): scale with the input width
      const float sc = (4.0f * W) / 1920.0f;
      const float dist[5] = {-0.288283f, 0.146546f, 0.003800f, -0.001690f, -0.132134f};
      rt.configureIngest(4 * W, 4 * H, 1642.405612f * sc, 1636.148027f * sc, 2.0f * W, 2.0f * H, dist, undistort);
    }
    float initial_pose[6] = {0, 0, 0, 0, 0, 0};
    for (int frame_counter = 1; frame_counter <= max_frame_counter; frame_counter++) {
      if (!f.read((char*)buf.data(), buf.size())) { std::fprintf(stderr, "short read at frame %d\n", frame_counter); return -1; }
      frameptr_vector.emplace_back(new frame(rt, buf.data(), bgr));
      frame* cur = frameptr_vector.back().get();
      if (frame_counter == 1) {   // main.cpp:228-236
        activeKeyFrame = cur;
        currentDepthMap.formDepthMap(cur);
        currentDepthMap.updateDepthImage();
        continue;
      }
      frame* tminus1 = frameptr_vector[frameptr_vector.size() - 2].get();
      const bool have_init = initialize_pose_file.is_open();
      if (have_init) {   // main.cpp:207-211
        int temp_frame_no;
        initialize_pose_file >> temp_frame_no >> initial_pose[0] >> initial_pose[1] >> initial_pose[2] >> initial_pose[3] >> initial_pose[4] >> initial_pose[5];
        if (!initialize_pose_file) { std::fprintf(stderr, "initial-pose file ends before frame %d\n", frame_counter); return -1; }
      }
      if (restore_file.is_open()) {   // main.cpp:252-324
        globalOptimize& g = *globalOptimizeLoop;
        g.checkConnection(&currentDepthMap);
        if (g.connectionLost) {
          g.findConnection(cur);
          const globalOptimize::RestoreRecord& r = g.lastRestore;
          if (!g.connectionLost) {   // a new connection: the frame becomes the active keyframe
            int n_targets = 0;
            float gain = 1.0f, offset = 0.0f;
            for (size_t b = 0; b < r.ids.size(); b++)
              if (r.ids[b] == r.chosen) {
                n_targets = r.records[b].n_targets;
                gain = r.lights[2 * b];
                offset = r.lights[2 * b + 1];
              }
            restore_file << (cur->frameId + rt.BATCH_START_ID - 1) << " " << r.ids.size() << " " << (r.chosenFrameId + rt.BATCH_START_ID - 1) << " " << n_targets
                         << " " << r.seedsAfter << " " << r.rescaleFactor;
            if (restore_light) restore_file << " " << gain << " " << offset;
            restore_file << "\n";
            restore_file.flush();
            currentDepthMap = *g.temp_depthMap;   // :267
            const float seeds_found = currentDepthMap.calculate_no_of_Seeds();
            const int id = cur->frameId + rt.BATCH_START_ID - 1, kid = activeKeyFrame->frameId + rt.BATCH_START_ID - 1;
            pose_file_orig << id << " " << kid << " " << cur->poseWrtWorld[0] << " " << cur->poseWrtWorld[1] << " " << cur->poseWrtWorld[2] << " "
                           << cur->poseWrtWorld[3] << " " << cur->poseWrtWorld[4] << " " << cur->poseWrtWorld[5] << " " << activeKeyFrame->rescaleFactor
                           << " " << seeds_found << "\n";   // :289
            if (cur->frameId % KEYFRAME_PROPAGATE_INTERVAL == 0)   // :296-301
              match_file << id << " " << kid << " " << cur->poseWrtOrigin[0] << " " << cur->poseWrtOrigin[1] << " " << cur->poseWrtOrigin[2] << " "
                         << cur->poseWrtOrigin[3] << " " << cur->poseWrtOrigin[4] << " " << cur->poseWrtOrigin[5] << " " << activeKeyFrame->rescaleFactor
                         << " " << seeds_found << " " << "0" << " " << "0" << " " << "0" << "\n";
            currentDepthMap.keyFrame = cur;   // :307-308
            activeKeyFrame = cur;
            delete g.temp_depthMap;
            g.temp_depthMap = nullptr;
            frameptr_vector.erase(frameptr_vector.begin(), frameptr_vector.end() - 1);   // keep only the new keyframe
            continue;   // :314
          }
          restore_file << (cur->frameId + rt.BATCH_START_ID - 1) << " " << r.ids.size() << " -1 0 0 0" << (restore_light ? " 1 0" : "") << "\n";
          restore_file.flush();
          frameptr_vector.pop_back();   // :319-322: the frame is of no use
          continue;
        }
      }
      // a frame that switches the keyframe (main.cpp:404) is aligned on its own; with --fused every other frame goes through the
      // fused call: alignment + observe + regularise + export as one device sequence (TrackFrameAndObserve)
      const bool kf_switch = (frame_counter % KEYFRAME_PROPAGATE_INTERVAL == 0) || (frame_counter == max_frame_counter);
      float seeds_num = 0;
      if (kf_switch || no_fused) {
        GetImagePoseEstimate(activeKeyFrame, cur, frame_counter, &currentDepthMap, tminus1, have_init ? initial_pose : nullptr);   // main.cpp:330
        seeds_num = currentDepthMap.calculate_no_of_Seeds();
      } else {
        TrackFrameAndObserve(activeKeyFrame, cur, &currentDepthMap, tminus1, have_init ? initial_pose : nullptr, &seeds_num);
      }
      const int id = cur->frameId + rt.BATCH_START_ID - 1, kid = activeKeyFrame->frameId + rt.BATCH_START_ID - 1;
      pose_file_orig << id << " " << kid << " " << cur->poseWrtWorld[0] << " " << cur->poseWrtWorld[1] << " " << cur->poseWrtWorld[2] << " "
                     << cur->poseWrtWorld[3] << " " << cur->poseWrtWorld[4] << " " << cur->poseWrtWorld[5] << " " << activeKeyFrame->rescaleFactor
                     << " " << seeds_num << "\n";
      match_file << id << " " << kid << " " << cur->poseWrtOrigin[0] << " " << cur->poseWrtOrigin[1] << " " << cur->poseWrtOrigin[2] << " "
                 << cur->poseWrtOrigin[3] << " " << cur->poseWrtOrigin[4] << " " << cur->poseWrtOrigin[5] << " " << activeKeyFrame->rescaleFactor
                 << " " << seeds_num << " " << "0" << " " << "0" << " " << "0" << "\n";
      if (kf_switch || no_fused) currentDepthMap.formDepthMap(cur);   // main.cpp:391
      if (kf_switch) {   // main.cpp:404
        if (lc) activeKeyFrame->finaliseWeights();
        currentDepthMap.finaliseKeyframe();
        if (lc) globalOptimizeLoop->pushToArray(activeKeyFrame, &currentDepthMap);   // main.cpp:462
        currentDepthMap.createKeyFrame(cur);
        activeKeyFrame = cur;
        frameptr_vector.erase(frameptr_vector.begin(), frameptr_vector.end() - 1);   // keep only the most recent frame
        continue;
      }
      if (no_fused) {
        currentDepthMap.updateKeyFrame();   // main.cpp:499-502
        currentDepthMap.observeDepthRowParallel();
        currentDepthMap.doRegularization();
        currentDepthMap.updateDepthImage();
      }
    }
    if (globalOptimizeLoop) globalOptimizeLoop->join_all();   // the last keyframe's match thread (t_group.join_all)
    if (globalOptimizeLoop && !map_file.empty()) {
      ellc_map_filter filter;
      filter.max_var = 0.0f; filter.min_support = 3; filter.support_k2 = 1.0f; filter.stride = 1;
      std::vector<ellc_map_point> cloud;
      globalOptimizeLoop->exportLocalMap(filter, 0, cloud);
      write_ply(map_file, cloud);
    }
    if (globalOptimizeLoop && !render_file.empty()) {
      if (globalOptimizeLoop->lastPushedArrayId < 0) throw std::runtime_error("--render: no keyframe was pushed into the ring");
      ellc_map_filter filter;
      filter.max_var = 0.0f; filter.min_support = 3; filter.support_k2 = 1.0f; filter.stride = 1;
      RenderedView view;
      globalOptimizeLoop->renderLocalMap(globalOptimizeLoop->loopFrameArray[globalOptimizeLoop->lastPushedArrayId].poseWrtWorld, 0, filter, 1.0f, nullptr, view);
      write_pfm(render_file, view.depth, view.cols, view.rows);
    }
    if (globalOptimizeLoop && !fuse_file.empty()) {
      if (globalOptimizeLoop->lastPushedArrayId < 0) throw std::runtime_error("--fuse: no keyframe was pushed into the ring");
      ellc_map_filter filter;
      filter.max_var = 0.0f; filter.min_support = 3; filter.support_k2 = 1.0f; filter.stride = 1;
      FusedView view;
      globalOptimizeLoop->fuseLocalMap(globalOptimizeLoop->loopFrameArray[globalOptimizeLoop->lastPushedArrayId].poseWrtWorld, 0, filter, 1.0f,
                                       ELLC_FUSE_MAX_MERGE, nullptr, view);
      write_pfm(fuse_file, view.depth, view.cols, view.rows);
      if (!fuse_inputs.empty()) {
        auto dump = [](const std::string& path, const void* p, size_t bytes) {
          std::ofstream f(path, std::ios::binary);
          f.write((const char*)p, (std::streamsize)bytes);
          if (!f) throw std::runtime_error("--fuse-inputs: cannot write " + path);
        };
        const size_t n = (size_t)view.cols * view.rows;
        std::vector<float> d(n), v(n);
        dump(fuse_inputs + "/T.bin", view.T.data(), view.T.size() * sizeof(float));
        for (size_t k = 0; k < view.slots.size(); k++) {
          globalOptimizeLoop->ring.check(ellc_keyframe_get_depth_level(globalOptimizeLoop->ring.ctx, view.slots[k], 0, d.data(), v.data()),
                                         "ellc_keyframe_get_depth_level");
          dump(fuse_inputs + "/slot" + std::to_string(k) + ".depth", d.data(), n * sizeof(float));
          dump(fuse_inputs + "/slot" + std::to_string(k) + ".var", v.data(), n * sizeof(float));
        }
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "ellc_main: %s\n", e.what());
    return -2;
  }
  return 0;
}
