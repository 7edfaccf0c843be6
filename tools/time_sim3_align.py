#!/usr/bin/env python3
"""Time of ellc_keyframe_sim3_step and ellc_keyframe_sim3_align over a loop-closure ring of 43 keyframes at 640x480, semi-dense maps,
filter (no variance test, min_support 3, support_k2 1, stride 1 - what ellc_main --match-sim3 uses), the default ellc_sim3_params, in
the two shapes of tools/time_depth_consistency.py:
  batch    43 pairs on level 0: every ring keyframe against the last one (the loop-closure batch)
  matrix   all 43 x 42 = 1806 ordered pairs on level 2 (a covisibility matrix of the ring)
Figures per shape, medians over --reps calls after --warmup untimed ones:
  step device   HIP events around the launches (sim3_pass, sim3_finish) inside one ellc_keyframe_sim3_step (ellc_profile_sim3_step)
  step wall     the whole ellc_keyframe_sim3_step call as a caller sees it
  align wall    one ellc_keyframe_sim3_align call on that level (max_iter 10, eps 1e-4), with the evaluations it made
  consistency   ellc_keyframe_depth_consistency's device and wall time on the same pairs, for scale: the same walk with three double sums
  host          timed once: the two slots' planes read back and tests/sim3_reference.py's step for every --check-every'th pair, each held
                to the call's record field by field
usage: tools/time_sim3_align.py [--slots N] [--reps R] [--no-host]"""
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
import sim3_reference as S  # noqa: E402
from map_points_reference import scaled_transform  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=43)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--check-every", type=int, default=25)
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
W, H, L, N = 640, 480, 4, a.slots
FLT = dict(max_var=0.0, min_support=3, support_k2=1.0, stride=1)
FLT_T = (0.0, 3, 1.0, 1)

base = [synth.make_pair(W, H, seed=100 + k) for k in range(4)]   # four scenes, repeated over the slots
fx, fy, cx, cy = base[0]["intrinsics"]
ctx = api.Context(api.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, max_keyframes=N, max_frames=1, max_batch=1), diag=True)
for b in range(N):
    s = base[b % 4]
    ctx.keyframe_upload(b, s["kf_image"]); ctx.keyframe_set_depth(b, s["depth0"], s["var0"])


def transform(s, d):
    """keyframes a few centimetres and fractions of a degree apart, as the poses of a loop-closure batch are"""
    k = s - d
    return scaled_transform(xi=(0.002 * k, -0.001 * k, 0.001, 0.01 * k, -0.005 * k, 0.002 * k), scale=1.0)


def host_path(src, dst, Ts, level, recs):
    """read-back + numpy reference of every check_every'th pair; returns (pairs, read-back ms, numpy ms)."""
    t_read = t_numpy = 0.0
    planes = {}
    n = 0
    for b in range(0, len(src), a.check_every):
        t0 = time.perf_counter()
        for slot in (src[b], dst[b]):
            if slot not in planes:
                planes[slot] = ctx.keyframe_depth_level(slot, level) + (ctx.image_level(True, slot, level)[0],)
        t1 = time.perf_counter()
        ref = S.step(planes[src[b]], planes[dst[b]], S.level_intrinsics(fx, fy, cx, cy, level), Ts[b], FLT_T)
        t_numpy += time.perf_counter() - t1
        t_read += t1 - t0
        r = recs[b]
        for k in S.INT_FIELDS:
            assert int(r[k]) == ref[k], (src[b], dst[b], k, int(r[k]), ref[k])
        values = list(r["H"]) + list(r["b"]) + [r["chi2_photo"], r["chi2_depth"]]
        for v, (name, want, bound) in zip(values, S.sums_of(ref)):
            assert abs(float(v) - want) <= bound, (src[b], dst[b], name, float(v), want, bound)
        n += 1
    return n, 1e3 * t_read, 1e3 * t_numpy


shapes = [("batch", 0, [(s, N - 1) for s in range(N)]), ("matrix", 2, [(s, d) for s in range(N) for d in range(N) if s != d])]
for name, level, pairs in shapes:
    src = np.array([p[0] for p in pairs], np.int32); dst = np.array([p[1] for p in pairs], np.int32)
    Ts = np.stack([transform(s, d) for s, d in pairs])
    dev, wall, awall, cdev, cwall = [], [], [], [], []
    for i in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        recs = ctx.sim3_step(src, dst, Ts, level=level, **FLT)
        t1 = time.perf_counter()
        ms = ctx.profile_sim3_step(src, dst, Ts, level=level, **FLT)[1]
        t2 = time.perf_counter()
        res = ctx.sim3_align(src, dst, Ts, level_from=level, level_to=level, max_iter=10, eps=1e-4, **FLT)
        t3 = time.perf_counter()
        ctx.depth_consistency(src, dst, Ts, level=level, agree_k2=1.0, **FLT)
        t4 = time.perf_counter()
        cms = ctx.profile_depth_consistency(src, dst, Ts, level=level, agree_k2=1.0, **FLT)[1]
        if i >= a.warmup:
            wall.append(1e3 * (t1 - t0)); dev.append(ms); awall.append(1e3 * (t3 - t2)); cwall.append(1e3 * (t4 - t3)); cdev.append(cms)
    rows, cols = ctx.level_shape(level)
    line = ("%-6s %d pairs %dx%d level %d: kept %d in view %d photo %d depth %d; step device %.3f ms (min %.3f), step wall %.3f ms (min %.3f); "
            "align wall %.3f ms (min %.3f), %d updates, at most %d a pair; consistency device %.3f ms, wall %.3f ms") % (
        name, len(pairs), cols, rows, level, recs["n_kept"].sum(), recs["n_in_view"].sum(), recs["n_photo"].sum(), recs["n_depth"].sum(),
        np.median(dev), min(dev), np.median(wall), min(wall), np.median(awall), min(awall), int(res["iters"].sum()), int(res["iters"].max()),
        np.median(cdev), np.median(cwall))
    if not a.no_host:
        n, t_read, t_numpy = host_path(src.tolist(), dst.tolist(), Ts, level, recs)
        line += "; host path: %d pairs, read-back %.1f ms + numpy reference %.1f ms (records equal within the sums' bounds)" % (n, t_read, t_numpy)
    print(line, flush=True)
ctx.close()
