#!/usr/bin/env python3
"""Time of one ellc_keyframe_fuse_depth call over a whole loop-closure ring, beside ellc_keyframe_render_depth on the same inputs in the
same run: 43 keyframe slots at 640x480 fused into one view, level 0, once with semi-dense and once with dense maps, filter (no variance
test, min_support 3, support_k2 1, stride 1 — what ellc_main --render / --fuse use), agree_k2 1, max_merge 64. The two calls alternate,
medians over --reps calls after --warmup untimed ones:
  device   HIP events around the launches inside the call (ellc_profile_fuse_depth: the preset of the keys to the end of fuse_finish, the
           host's read of the list's size included; ellc_profile_render_depth: the preset to the end of render_agree)
  wall     the whole call as a caller sees it, the planes in host memory the caller reuses from call to call
  list     the largest segment (agreeing candidates of one target) and the list's size (their sum, 4 bytes each)
  host     the numpy restatement of the rule (tests/fuse_depth_reference.py) on the read-back planes — timed once, it takes seconds; its
           planes must be identical
usage: tools/time_fuse_depth.py [--slots N] [--reps R] [--max-merge M] [--no-host]"""
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
import fuse_depth_reference as FU  # noqa: E402
import render_depth_reference as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=43)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--max-merge", type=int, default=64)
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
    # keyframes a few centimetres and fractions of a degree apart, as a ring around a view holds them
    Ts = np.stack([R.scaled_transform(xi=(0.002 * b, -0.001 * b, 0.001, 0.01 * b, -0.005 * b, 0.002 * b), scale=1.0) for b in range(B)])
    dev, wall, dev_r, wall_r = [], [], [], []
    out = ctx.fuse_depth(slots, Ts, level=0, agree_k2=1.0, max_merge=a.max_merge, **FLT)
    out_r = ctx.render_depth(slots, Ts, level=0, agree_k2=1.0, **FLT)
    for i in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        out = ctx.fuse_depth(slots, Ts, level=0, agree_k2=1.0, max_merge=a.max_merge, out=out, **FLT)
        t1 = time.perf_counter()
        out_r = ctx.render_depth(slots, Ts, level=0, agree_k2=1.0, out=out_r, **FLT)
        t2 = time.perf_counter()
        ms = ctx.profile_fuse_depth(slots, Ts, level=0, agree_k2=1.0, max_merge=a.max_merge, out=out, **FLT)["launches_ms"]
        ms_r = ctx.profile_render_depth(slots, Ts, level=0, agree_k2=1.0, out=out_r, **FLT)["launches_ms"]
        if i >= a.warmup:
            wall.append(1e3 * (t1 - t0)); wall_r.append(1e3 * (t2 - t1)); dev.append(ms); dev_r.append(ms_r)
    line = "%-10s %d slots 640x480 level 0 max_merge %d: %d of %d targets valid, %d fused (%d from 3 or more), largest segment %d, list %d entries; " \
           "fuse device %.3f ms (min %.3f), wall %.2f ms (min %.2f); render device %.3f ms (min %.3f), wall %.2f ms (min %.2f); device ratio %.2f" % (
               "dense" if dense else "semi-dense", B, a.max_merge, out["n_valid"], W * H, out["n_fused"], int((out["merged"] >= 3).sum()), out["agree"].max(),
               int(out["agree"].sum(dtype=np.int64)), np.median(dev), min(dev), np.median(wall), min(wall), np.median(dev_r), min(dev_r), np.median(wall_r),
               min(wall_r), np.median(dev) / np.median(dev_r))
    if not a.no_host:
        t0 = time.perf_counter()
        planes = [ctx.keyframe_depth_level(b, 0) + (ctx.image_level(True, b, 0)[0],) for b in range(B)]
        t1 = time.perf_counter()
        ref = FU.fuse(planes, R.level_intrinsics(fx, fy, cx, cy, 0), Ts, (0.0, 3, 1.0, 1), 1.0, a.max_merge)
        t2 = time.perf_counter()
        assert FU.planes_equal(ref, out), FU.differing(ref, out)
        line += "; host path: read-back %.1f ms + numpy %.1f ms (planes identical)" % (1e3 * (t1 - t0), 1e3 * (t2 - t1))
    print(line, flush=True)
    ctx.close()
