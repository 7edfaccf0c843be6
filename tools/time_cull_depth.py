#!/usr/bin/env python3
"""Time of ellc_keyframe_cull_depth over the loop-closure ring of tools/time_refine_depth.py: keyframes at 640x480 with semi-dense maps,
K the LAST keyframe, put to the vote of the first 1, 4, 16 and 42 of the other keyframes on level 0 at the transforms of the
loop-closure batch (inverted: keyframe -> view) and the light (0.9, 10), with the photometric vote on (photo_k 3) and off (photo_k 0),
the pass-all filter and the other parameters at their defaults (the four counts lowered to the number of views). Figures per (views,
photometric vote), medians over --reps calls after --warmup untimed ones, the variants interleaved:
  device        HIP events around the launches (cull_pixels, cull_finish) inside one call (ellc_profile_cull_depth)
  wall          the whole ellc_keyframe_cull_depth call as a caller sees it, the five planes downloaded
  per vote      device time over (pixel taking part x view)
  refine_depth  the same-run device and wall time of ellc_keyframe_refine_depth at n_iter = 1 on the same K, views, transforms and lights
                (pass-all filter, the other parameters at their defaults), once per number of views: the yardstick. It evaluates every
                (pixel, view) twice with four taps each; the cull projects once and gathers two values, and four taps where the
                photometric vote is on
  host          with at most --host-views views unless --no-host: tests/cull_depth_reference.py's cull on the planes read back; the
                call is held to it byte for byte (planes) and on every stat
usage: tools/time_cull_depth.py [--slots N] [--reps R] [--no-host] [--level L]"""
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
import cull_depth_reference as Q  # noqa: E402
from map_points_reference import scaled_transform  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=43)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--host-views", type=int, default=4)
ap.add_argument("--no-host", action="store_true")
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


def transform(s, d):
    """keyframes a few centimetres and fractions of a degree apart, as the poses of a loop-closure batch are (tools/time_sim3_align.py)"""
    k = s - d
    return scaled_transform(xi=(0.002 * k, -0.001 * k, 0.001, 0.01 * k, -0.005 * k, 0.002 * k), scale=1.0)


Ts_all = np.stack([api.sim3_invert(transform(s, K))[0] for s in range(N - 1)])
counts = [v for v in (1, 4, 16, 42) if v <= N - 1]
variants = [(v, pk) for v in counts for pk in (3.0, 0.0)]
dev = {k: [] for k in variants}; wall = {k: [] for k in variants}
rdev = {v: [] for v in counts}; rwall = {v: [] for v in counts}
last = {}


def params_of(v, pk):
    return Q.case_params(v, photo_k=pk)


for i in range(a.warmup + a.reps):
    for v in counts:   # interleaved: a drift of the clocks reaches every variant alike
        views = list(range(v)); Ts = Ts_all[:v]; lights = [LIGHT] * v
        for pk in (3.0, 0.0):
            t0 = time.perf_counter()
            res = ctx.cull_depth(K, views, Ts, lights, level=a.level, params=params_of(v, pk))
            t1 = time.perf_counter()
            ms = ctx.profile_cull_depth(K, views, Ts, lights, level=a.level, params=params_of(v, pk))[1]
            last[(v, pk)] = res
            if i >= a.warmup:
                wall[(v, pk)].append(1e3 * (t1 - t0)); dev[(v, pk)].append(ms)
        rp = dict(n_iter=1, min_views=min(2, v))
        t0 = time.perf_counter()
        ctx.refine_depth(K, views, Ts, lights, level=a.level, params=rp)
        t1 = time.perf_counter()
        rms = ctx.profile_refine_depth(K, views, Ts, lights, level=a.level, params=rp)[1]
        if i >= a.warmup:
            rwall[v].append(1e3 * (t1 - t0)); rdev[v].append(rms)
for v, pk in variants:
    st = last[(v, pk)]["stats"]
    votes = st["n_kept"] * v
    line = ("%2d views photo_k %g %dx%d level %d: kept %d retained %d unseen %d culled (free space %d, unsupported %d, photo %d); votes agree %d in front %d "
            "behind %d photo %d bad %d; device %.3f ms (min %.3f), wall %.3f ms (min %.3f); %d pixel-views: %.4f ns each; refine_depth n_iter 1 on the "
            "same inputs: device %.3f ms (min %.3f), wall %.3f ms") % (
        v, pk, W >> a.level, H >> a.level, a.level, st["n_kept"], st["n_retained"], st["n_unseen"], st["n_culled_free_space"], st["n_culled_unsupported"],
        st["n_culled_photo"], st["sum_agree"], st["sum_in_front"], st["sum_behind"], st["sum_photo"], st["sum_photo_bad"], np.median(dev[(v, pk)]),
        min(dev[(v, pk)]), np.median(wall[(v, pk)]), min(wall[(v, pk)]), votes, 1e6 * np.median(dev[(v, pk)]) / max(votes, 1), np.median(rdev[v]),
        min(rdev[v]), np.median(rwall[v]))
    if not a.no_host and v <= a.host_views:
        t0 = time.perf_counter()
        kf = ctx.keyframe_depth_level(K, a.level) + (ctx.image_level(True, K, a.level)[0],)
        vws = [ctx.keyframe_depth_level(s, a.level) + (ctx.image_level(True, s, a.level)[0],) for s in range(v)]
        t1 = time.perf_counter()
        ref = Q.cull(kf, vws, Q.level_intrinsics(fx, fy, cx, cy, a.level), Ts_all[:v], [LIGHT] * v, Q.NO_FILTER, params_of(v, pk))
        t2 = time.perf_counter()
        for name in Q.PLANES:
            assert last[(v, pk)][name].tobytes() == ref[name].tobytes(), (v, pk, name)
        for k in Q.INT_FIELDS:
            assert int(st[k]) == ref[k], (v, pk, k, st[k], ref[k])
        line += "; host path: read-back %.1f ms + numpy reference %.1f ms (planes and stats equal)" % (1e3 * (t1 - t0), 1e3 * (t2 - t1))
    print(line, flush=True)
ctx.close()
