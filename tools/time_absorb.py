#!/usr/bin/env python3
"""Time of one ellc_depth_absorb_keyframes call over a whole loop-closure ring, beside ellc_keyframe_fuse_depth on the same inputs in the
same run: the ring of tools/time_fuse_depth.py (43 keyframe slots at 640x480, once with semi-dense and once with dense maps), viewed from
the LAST slot, which is also the live keyframe of the depth map; the state is synth.make_depth_state of that slot's image. Filter (no
variance test, min_support 3, support_k2 1, stride 1), agree_k2 1, max_fold / max_merge 64, the photometric gate on. The state is
uploaded again in front of every absorb call (untimed); the two calls alternate, medians over --reps calls after --warmup untimed ones:
  device   HIP events around the launches inside the call (ellc_profile_depth_absorb: the preset of the count plane to the end of
           absorb_finish, the host's read of the list's size included, finalise's launches not; ellc_profile_fuse_depth likewise)
  wall     the whole call as a caller sees it, without finalise and with it (regularisation, export and pyramid behind the fold)
  list     the largest segment (candidates of one target) and the list's size (their sum, 4 bytes each)
  host     the numpy restatement of the rule (tests/absorb_reference.py) on the read-back planes and state - timed once, it takes
           seconds; the seven state planes and the stats must be identical
usage: tools/time_absorb.py [--slots N] [--reps R] [--max-fold M] [--no-host]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from egomotion_with_local_loop_closures_amd import api, synth  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # noqa: E402
import diaglib  # noqa: E402,F401  (ELLC_LIB_PATH -> _lib.use_library: diagnostic builds)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # noqa: E402
import absorb_reference as A  # noqa: E402
import render_depth_reference as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=43)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--max-fold", type=int, default=64)
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
W, H, L, B = 640, 480, 4, a.slots
FLT = dict(max_var=0.0, min_support=3, support_k2=1.0, stride=1)

for dense in (False, True):
    base = [synth.make_pair(W, H, seed=100 + k, dense=dense) for k in range(4)]   # four scenes, repeated over the slots
    fx, fy, cx, cy = base[0]["intrinsics"]
    ctx = api.Context(api.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, max_keyframes=B + 1, max_frames=1, max_batch=1), diag=True)
    for b in range(B):
        s = base[b % 4]
        ctx.keyframe_upload(b, s["kf_image"]); ctx.keyframe_set_depth(b, s["depth0"], s["var0"])
    slots = np.arange(B, dtype=np.int32)
    K = B - 1
    # keyframes a few centimetres and fractions of a degree apart, as a ring around a view holds them; the view is the last one's
    to_view = [np.vstack([R.scaled_transform(xi=(0.002 * b, -0.001 * b, 0.001, 0.01 * b, -0.005 * b, 0.002 * b), scale=1.0).reshape(3, 4).astype(np.float64),
                          [0, 0, 0, 1]]) for b in range(B)]
    Ts = np.stack([(np.linalg.inv(to_view[K]) @ to_view[b])[:3, :].astype(np.float32).reshape(12) for b in range(B)])
    state = synth.make_depth_state(W, H, 12, base[K % 4]["kf_image"], idepth_true=base[K % 4]["idepth_true"], fill=0.7)
    ctx.depth_set_keyframe(K)
    fold = dict(max_fold=a.max_fold, finalise=0)
    dev, wall, wall_fin, dev_f, wall_f = [], [], [], [], []
    out_f = ctx.fuse_depth(slots, Ts, level=0, agree_k2=1.0, max_merge=a.max_fold, **FLT)
    for i in range(a.warmup + a.reps):
        ctx.depth_set_state(state)
        t0 = time.perf_counter()
        stats = ctx.depth_absorb(slots, Ts, params=fold, **FLT)
        t1 = time.perf_counter()
        out_f = ctx.fuse_depth(slots, Ts, level=0, agree_k2=1.0, max_merge=a.max_fold, out=out_f, **FLT)
        t2 = time.perf_counter()
        ctx.depth_set_state(state)
        ms = ctx.profile_depth_absorb(slots, Ts, params=fold, **FLT)["launches_ms"]
        ms_f = ctx.profile_fuse_depth(slots, Ts, level=0, agree_k2=1.0, max_merge=a.max_fold, out=out_f, **FLT)["launches_ms"]
        ctx.depth_set_state(state)
        t3 = time.perf_counter()
        ctx.depth_absorb(slots, Ts, params=dict(max_fold=a.max_fold, finalise=1), **FLT)   # (K's planes change: K is the last request, read before)
        t4 = time.perf_counter()
        ctx.keyframe_set_depth(K, base[K % 4]["depth0"], base[K % 4]["var0"])
        if i >= a.warmup:
            wall.append(1e3 * (t1 - t0)); wall_f.append(1e3 * (t2 - t1)); dev.append(ms); dev_f.append(ms_f); wall_fin.append(1e3 * (t4 - t3))
    line = "%-10s %d slots 640x480 max_fold %d: %d candidates on %d targets, created %d merged %d replaced %d occluded %d skipped %d, truncated %d, " \
           "valid %d -> %d; absorb device %.3f ms (min %.3f), wall %.2f ms (min %.2f), with finalise %.2f ms (min %.2f); fuse device %.3f ms (min %.3f), " \
           "wall %.2f ms (min %.2f); device ratio %.2f" % (
               "dense" if dense else "semi-dense", B, a.max_fold, stats["n_candidates"], stats["targets_hit"], stats["n_created"], stats["n_merged"],
               stats["n_replaced"], stats["n_occluded"], stats["n_skipped"], stats["targets_truncated"], stats["n_valid_before"], stats["n_valid_after"],
               np.median(dev), min(dev), np.median(wall), min(wall), np.median(wall_fin), min(wall_fin), np.median(dev_f), min(dev_f), np.median(wall_f),
               min(wall_f), np.median(dev) / np.median(dev_f))
    if not a.no_host:
        ctx.depth_set_state(state)
        t0 = time.perf_counter()
        planes = [ctx.keyframe_depth_level(b, 0) + (ctx.image_level(True, b, 0)[0],) for b in range(B)]
        before = ctx.depth_get_state()
        k_img, k_mg = ctx.image_level(True, K, 0)[0], ctx.max_gradient(True, K)[0]
        t1 = time.perf_counter()
        ref = A.absorb(planes, A.level_intrinsics(fx, fy, cx, cy, 0), Ts, (0.0, 3, 1.0, 1), k_img, k_mg, before, agree_k2=1.0, max_fold=a.max_fold)
        t2 = time.perf_counter()
        got_stats = ctx.depth_absorb(slots, Ts, params=fold, **FLT)
        got = ctx.depth_get_state()
        assert not A.differing(ref, got) and ref["stats"] == got_stats, (A.differing(ref, got), ref["stats"], got_stats)
        cand, _ = A._sorted_candidates(planes, A.level_intrinsics(fx, fy, cx, cy, 0), Ts, (0.0, 3, 1.0, 1), k_img, k_mg, 1)
        line += "; largest segment %d, list %d entries; host path: read-back %.1f ms + numpy %.1f ms (state and stats identical)" % (
            int(np.bincount(cand["target"]).max()) if cand["target"].size else 0, cand["target"].size, 1e3 * (t1 - t0), 1e3 * (t2 - t1))
    print(line, flush=True)
    ctx.close()
