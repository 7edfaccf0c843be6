#!/usr/bin/env python3
"""Time of ellc_keyframe_sweep_depth over the loop-closure ring of tools/time_refine_depth.py: keyframes at 640x480 with semi-dense maps,
K the LAST keyframe with its map thinned to the pixels with (x + 2 y) % 3 == 0 (the holes a sweep is for: two of three textured pixels
hold no hypothesis), swept on level 0 against the first 1, 4 and 16 of the other keyframes at the transforms of the loop-closure batch
(inverted: keyframe -> view) and the light (0.9, 10), with 16 and 64 samples over the default range. Figures per (views, samples),
medians over --reps calls after --warmup untimed ones, the variants interleaved:
  device        HIP events around the launches (sweep_pixels, sweep_finish) inside one call (ellc_profile_sweep_depth)
  wall          the whole ellc_keyframe_sweep_depth call as a caller sees it, the four planes downloaded
  per term      device time over (swept pixel x sample x view): five pattern pixels each
  refine_depth  the same-run device and wall time of ellc_keyframe_refine_depth on the same K, views, transforms and lights (pass-all
                filter, default parameters), once per number of views: the yardstick
  compaction    ellc_keyframe_map_points' three launches over K alone (ellc_profile_map_points): what a compaction of the swept pixels
                in front of the pixel kernel would add. --empty-k gives K no hypothesis at all (every textured interior pixel is
                swept, fewer waves diverge at the swept test), so that two runs tell what the divergence of the thinned map costs
  host          once per (views, samples) with views x samples <= 64 (the numpy reference takes seconds per view and sample at this
                size) unless --no-host: tests/sweep_depth_reference.py's sweep on the planes read back; the call is held to it on every
                --check-every'th pixel (planes) and on the integer stats
usage: tools/time_sweep_depth.py [--slots N] [--reps R] [--no-host] [--empty-k] [--level L]"""
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
import sweep_depth_reference as SW  # noqa: E402
from map_points_reference import scaled_transform  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=17)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--check-every", type=int, default=7)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--empty-k", action="store_true")
ap.add_argument("--level", type=int, default=0)
a = ap.parse_args()
W, H, L, N = 640, 480, 4, a.slots
LIGHT = (0.9, 10.0)

base = [synth.make_pair(W, H, seed=100 + k) for k in range(4)]   # four scenes, repeated over the slots
fx, fy, cx, cy = base[0]["intrinsics"]
ctx = api.Context(api.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, max_keyframes=N, max_frames=1, max_batch=1), diag=True)
for b in range(N):
    s = base[b % 4]
    ctx.keyframe_upload(b, s["kf_image"]); ctx.keyframe_set_depth(b, s["depth0"], s["var0"])
K = N - 1
yy, xx = np.mgrid[0:H, 0:W]
keep = np.zeros((H, W), bool) if a.empty_k else (xx + 2 * yy) % 3 == 0
ctx.keyframe_set_depth(K, np.where(keep, base[K % 4]["depth0"], 0).astype(np.float32), base[K % 4]["var0"])


def transform(s, d):
    """keyframes a few centimetres and fractions of a degree apart, as the poses of a loop-closure batch are (tools/time_sim3_align.py)"""
    k = s - d
    return scaled_transform(xi=(0.002 * k, -0.001 * k, 0.001, 0.01 * k, -0.005 * k, 0.002 * k), scale=1.0)


Ts_all = np.stack([api.sim3_invert(transform(s, K))[0] for s in range(N - 1)])
counts = [v for v in (1, 4, 16) if v <= N - 1]
variants = [(v, ns) for v in counts for ns in (16, 64)]
dev = {k: [] for k in variants}; wall = {k: [] for k in variants}
rdev = {v: [] for v in counts}; rwall = {v: [] for v in counts}
last = {}
for i in range(a.warmup + a.reps):
    for v in counts:   # interleaved: a drift of the clocks reaches every variant alike
        views = list(range(v)); Ts = Ts_all[:v]; lights = [LIGHT] * v
        for ns in (16, 64):
            prm = dict(n_samples=ns, min_views=min(2, v))
            t0 = time.perf_counter()
            res = ctx.sweep_depth(K, views, Ts, lights, level=a.level, params=prm)
            t1 = time.perf_counter()
            ms = ctx.profile_sweep_depth(K, views, Ts, lights, level=a.level, params=prm)[1]
            last[(v, ns)] = res
            if i >= a.warmup:
                wall[(v, ns)].append(1e3 * (t1 - t0)); dev[(v, ns)].append(ms)
        t0 = time.perf_counter()
        ctx.refine_depth(K, views, Ts, lights, level=a.level, params=dict(min_views=min(2, v)))
        t1 = time.perf_counter()
        rms = ctx.profile_refine_depth(K, views, Ts, lights, level=a.level, params=dict(min_views=min(2, v)))[1]
        if i >= a.warmup:
            rwall[v].append(1e3 * (t1 - t0)); rdev[v].append(rms)
for v, ns in variants:
    depth, var, nviews, status, st = last[(v, ns)]
    terms = st["n_swept"] * ns * v
    line = ("%2d views %2d samples %dx%d level %d: ok %d swept %d created %d (no valid sample %d, at range end %d, cost too high %d, not distinct %d, flat %d); "
            "device %.3f ms (min %.3f), wall %.3f ms (min %.3f); %d pixel-sample-views: %.4f ns each; refine_depth on the same inputs: device %.3f ms "
            "(min %.3f), wall %.3f ms") % (
        v, ns, W >> a.level, H >> a.level, a.level, st["n_ok"], st["n_swept"], st["n_created"], st["n_no_valid_sample"], st["n_at_range_end"],
        st["n_cost_too_high"], st["n_not_distinct"], st["n_flat"], np.median(dev[(v, ns)]), min(dev[(v, ns)]), np.median(wall[(v, ns)]),
        min(wall[(v, ns)]), terms, 1e6 * np.median(dev[(v, ns)]) / max(terms, 1), np.median(rdev[v]), min(rdev[v]), np.median(rwall[v]))
    if not a.no_host and v * ns <= 64:
        t0 = time.perf_counter()
        kf = ctx.keyframe_depth_level(K, a.level) + (ctx.image_level(True, K, a.level)[0],)
        imgs = [ctx.image_level(True, s, a.level)[0] for s in range(v)]
        t1 = time.perf_counter()
        ref = SW.sweep(kf, imgs, SW.level_intrinsics(fx, fy, cx, cy, a.level), Ts_all[:v], [LIGHT] * v, dict(n_samples=ns, min_views=min(2, v)))
        t2 = time.perf_counter()
        for name, g in zip(SW.PLANES, (depth, var, nviews, status)):
            assert g.reshape(-1)[::a.check_every].tobytes() == ref[name].reshape(-1)[::a.check_every].tobytes(), (v, ns, name)
        for k in SW.INT_FIELDS:
            assert int(st[k]) == ref[k], (v, ns, k, st[k], ref[k])
        line += "; host path: read-back %.1f ms + numpy reference %.1f ms (planes equal on every %dth pixel, integer stats equal)" % (
            1e3 * (t1 - t0), 1e3 * (t2 - t1), a.check_every)
    print(line, flush=True)
cms = [ctx.profile_map_points([K], [np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)], level=a.level)[2] for _ in range(a.warmup + a.reps)][a.warmup:]
print("compaction launches over K alone (map_count, map_scan, map_scatter): device %.3f ms (min %.3f)%s" % (
    np.median(cms), min(cms), "; K without hypotheses" if a.empty_k else ""), flush=True)
ctx.close()
