#!/usr/bin/env python3
"""Time of one ellc_keyframe_trial_propagate call over a whole loop-closure ring, beside what a caller had to do for the same figures
before it existed, in the same run: the ring of tools/time_absorb.py (43 keyframe slots at 640x480, semi-dense maps), every other slot as
a candidate for the LAST slot's image. Filter (no variance test, min_support 3, support_k2 1, stride 1), the photometric gate on.
  trial    one call over all candidates: device time (HIP events around its launches, ellc_profile_trial_propagate) and wall time
  today    per candidate ellc_depth_set_state of a wiped state + ellc_depth_absorb_keyframes with B = 1, finalise 0: wall time of all of them
           (the live map is destroyed each time); n_created of each must equal the trial's n_targets, the four counts in front too
  restart  ellc_depth_restart_from_keyframes from the best candidate (finalise 1) beside its eight-call twin (set_keyframe, set_state of
           the wiped planes, absorb, regularise, fill, regularise, makeInvDepthOne, export): wall time of each; the stats and factors equal
The legs alternate; medians over --reps rounds after --warmup untimed ones.
usage: tools/time_trial_propagate.py [--slots N] [--reps R]"""
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
import render_depth_reference as R  # noqa: E402
import trial_propagation_reference as TR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=44)   # 43 candidates and the view
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=30)
a = ap.parse_args()
W, H, L, N = 640, 480, 4, a.slots
B, K = N - 1, N - 1
FLT = dict(max_var=0.0, min_support=3, support_k2=1.0, stride=1)

base = [synth.make_pair(W, H, seed=100 + k) for k in range(4)]   # four scenes, repeated over the slots
fx, fy, cx, cy = base[0]["intrinsics"]
ctx = api.Context(api.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, max_keyframes=N, max_frames=1, max_batch=1), diag=True)
for b in range(N):
    s = base[b % 4]
    ctx.keyframe_upload(b, s["kf_image"]); ctx.keyframe_set_depth(b, s["depth0"], s["var0"])
to_view = [np.vstack([R.scaled_transform(xi=(0.002 * b, -0.001 * b, 0.001, 0.01 * b, -0.005 * b, 0.002 * b), scale=1.0).reshape(3, 4).astype(np.float64),
                      [0, 0, 0, 1]]) for b in range(N)]
Ts = np.stack([(np.linalg.inv(to_view[K]) @ to_view[b])[:3, :].astype(np.float32).reshape(12) for b in range(B)])
src, dst = np.arange(B, dtype=np.int32), np.full(B, K, np.int32)
wiped = TR.wiped_state(H, W)
ctx.depth_set_keyframe(K)
keep = ctx.keyframe_depth_level(K, 0)
dev, wall, wall_today, wall_restart, wall_twin = [], [], [], [], []
for i in range(a.warmup + a.reps):
    t0 = time.perf_counter()
    rec = ctx.trial_propagate(src, dst, Ts, dst_is_keyframe=True, **FLT)
    t1 = time.perf_counter()
    today = []
    for b in range(B):
        ctx.depth_set_state(wiped)
        today.append(ctx.depth_absorb([b], Ts[b:b + 1], params=dict(finalise=0), **FLT))
    t2 = time.perf_counter()
    hooked, ms = ctx.profile_trial_propagate(src, dst, Ts, dst_is_keyframe=True, **FLT)
    assert hooked.tobytes() == rec.tobytes()
    for b in range(B):
        assert rec["n_targets"][b] == today[b]["n_created"] == today[b]["targets_hit"], (b, rec[b], today[b])
        assert all(rec[k][b] == today[b][k] for k in ("n_kept", "n_in_view", "n_interior", "n_candidates")), (b, rec[b], today[b])
    best = int(np.argmax(rec["n_targets"]))
    t3 = time.perf_counter()
    stats, factor = ctx.depth_restart(K, [best], Ts[best:best + 1], **FLT)
    t4 = time.perf_counter()
    ctx.keyframe_set_depth(K, *keep)
    t5 = time.perf_counter()
    ctx.depth_set_keyframe(K)
    ctx.depth_set_state(wiped)
    stats_twin = ctx.depth_absorb([best], Ts[best:best + 1], params=dict(finalise=0), **FLT)
    ctx.depth_regularize(True)
    ctx.depth_fill_holes()
    ctx.depth_regularize(False)
    factor_twin = ctx.depth_make_inv_depth_one()
    ctx.depth_update_depth_image()
    t6 = time.perf_counter()
    ctx.keyframe_set_depth(K, *keep)
    assert stats == stats_twin and np.float32(factor) == np.float32(factor_twin), (stats, stats_twin, factor, factor_twin)
    if i >= a.warmup:
        dev.append(ms); wall.append(1e3 * (t1 - t0)); wall_today.append(1e3 * (t2 - t1)); wall_restart.append(1e3 * (t4 - t3)); wall_twin.append(1e3 * (t6 - t5))
print("%d candidates 640x480: n_targets %d .. %d (best: slot %d); trial device %.3f ms (min %.3f), wall %.2f ms (min %.2f); today's %d x (set_state + absorb) "
      "wall %.1f ms (min %.1f), ratio %.0f; restart wall %.2f ms (min %.2f), eight-call twin %.2f ms (min %.2f)" % (
          B, int(rec["n_targets"].min()), int(rec["n_targets"].max()), best, np.median(dev), min(dev), np.median(wall), min(wall), B, np.median(wall_today),
          min(wall_today), np.median(wall_today) / np.median(wall), np.median(wall_restart), min(wall_restart), np.median(wall_twin), min(wall_twin)), flush=True)
ctx.close()
