#!/usr/bin/env python3
"""Time of one ellc_keyframe_map_points call over a whole loop-closure ring: 43 keyframe slots at 640x480, level 0, once with semi-dense
and once with dense maps, filter (no variance test, min_support 3, support_k2 1, stride 1 — what ellc_main --map uses).
Three figures per map kind, medians over --reps calls after --warmup untimed ones:
  device   HIP events around the three launches (map_count + map_scan, map_scatter) inside the call (ellc_profile_map_points)
  wall     the whole call as a caller sees it: sizing call + export, records in host memory
  host     what a caller did before the entry point existed: 43 x (keyframe_depth_level + image_level) and the numpy restatement of
           the rule (tests/map_points_reference.py) on the planes — timed once, it takes seconds
usage: tools/time_map_points.py [--slots N] [--reps R] [--no-host]"""
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
import map_points_reference as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=43)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
W, H, L, B = 640, 480, 4, a.slots
FLT = dict(max_var=0.0, min_support=3, support_k2=1.0, stride=1)

for dense in (False, True):
    base = [synth.make_pair(W, H, seed=100 + k, dense=dense) for k in range(4)]   # four scenes, repeated over the slots
    fx, fy, cx, cy = base[0]["intrinsics"]
    ctx = api.Context(api.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, max_keyframes=B, max_frames=1, max_batch=1), diag=True)
    for b in range(B):
        s = base[b % 4]
        ctx.keyframe_upload(b, s["kf_image"]); ctx.keyframe_set_depth(b, s["depth0"], s["var0"])
    slots = np.arange(B, dtype=np.int32)
    Ts = np.stack([R.scaled_transform(xi=(0.01 * b, -0.02, 0.03, 0.1 * b, -0.2, 0.3), scale=1.0) for b in range(B)])
    dev, wall = [], []
    for i in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        pts, counts = ctx.map_points(slots, Ts, level=0, **FLT)
        t1 = time.perf_counter()
        _, _, ms = ctx.profile_map_points(slots, Ts, level=0, **FLT)
        if i >= a.warmup:
            wall.append(1e3 * (t1 - t0)); dev.append(ms)
    line = "%-10s %d slots 640x480 level 0: %d points (%.1f %% of the pixels, %.1f MB of records); device %.3f ms (min %.3f), wall %.2f ms (min %.2f)" % (
        "dense" if dense else "semi-dense", B, pts.size, 100.0 * pts.size / (B * W * H), pts.nbytes / 1e6, np.median(dev), min(dev), np.median(wall), min(wall))
    if not a.no_host:
        t0 = time.perf_counter()
        planes = [ctx.keyframe_depth_level(b, 0) + (ctx.image_level(True, b, 0)[0],) for b in range(B)]
        t1 = time.perf_counter()
        intr = R.level_intrinsics(fx, fy, cx, cy, 0)
        ref = [R.map_points(d, v, img, intr, Ts[b], (0.0, 3, 1.0, 1), source=b) for b, (d, v, img) in enumerate(planes)]
        t2 = time.perf_counter()
        assert R.records_equal(np.concatenate(ref), pts)
        line += "; host path: read-back %.1f ms + numpy %.1f ms (records identical)" % (1e3 * (t1 - t0), 1e3 * (t2 - t1))
    print(line, flush=True)
    ctx.close()
