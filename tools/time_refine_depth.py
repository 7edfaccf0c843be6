#!/usr/bin/env python3
"""Time of ellc_keyframe_refine_depth over the loop-closure ring of tools/time_sim3_align.py: 43 keyframes at 640x480, semi-dense maps,
filter (no variance test, min_support 3, support_k2 1, stride 1 - what ellc_main --refine-matches uses), the default
ellc_refine_params (n_iter 3: four evaluations a pixel that runs to the end). K is the LAST keyframe; it is refined on level 0 against
the first 1, 4, 16 and 42 of the other keyframes at the transforms of the loop-closure batch (inverted: keyframe -> view) and the
light (0.9, 10). Figures per number of views, medians over --reps calls after --warmup untimed ones, the variants interleaved:
  device        HIP events around the launches (refine_pixels, refine_finish) inside one call (ellc_profile_refine_depth)
  wall          the whole ellc_keyframe_refine_depth call as a caller sees it, the four planes downloaded
  per eval      device time over (kept pixel x view x evaluation). The call does not return the evaluations it made, so the count is
                bracketed from the statuses: refined, views-changed and cost-rose pixels made n_iter + 1 evaluations, every other pixel
                that takes part at least one and at most n_iter + 1
  compaction    ellc_keyframe_map_points' three launches (count, scan, scatter) over K alone (ellc_profile_map_points): what a
                compaction of the kept pixels in front of the pixel kernel would add. --dense-k gives K a dense map (every interior
                pixel kept: no wave diverges at map_keep), so that two runs tell what the divergence of the semi-dense map costs
  sim3_step_lit the same-run device time of ellc_keyframe_sim3_step_lit over the same pairs (K as the source, the views as the
                destinations), and that over its n_kept (kept pixel x view, one evaluation): the yardstick
  host          timed once per number of views: the planes read back and tests/refine_depth_reference.py's refine; every call is held to
                it on every --check-every'th pixel (planes) and on the integer stats
                --level L runs everything on pyramid level L (a quarter of the waves per level, the same work per wave): whether the
                device time follows the number of waves or the length of one wave's loop
usage: tools/time_refine_depth.py [--slots N] [--reps R] [--no-host] [--dense-k] [--level L]"""
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
import refine_depth_reference as R  # noqa: E402
from map_points_reference import scaled_transform  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=43)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--check-every", type=int, default=7)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--dense-k", action="store_true")
ap.add_argument("--level", type=int, default=0)
a = ap.parse_args()
W, H, L, N = 640, 480, 4, a.slots
FLT = dict(max_var=0.0, min_support=3, support_k2=1.0, stride=1)
FLT_T = (0.0, 3, 1.0, 1)
LIGHT = (0.9, 10.0)
N_ITER = R.DEFAULT_PARAMS["n_iter"]

base = [synth.make_pair(W, H, seed=100 + k) for k in range(4)]   # four scenes, repeated over the slots
fx, fy, cx, cy = base[0]["intrinsics"]
ctx = api.Context(api.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, max_keyframes=N, max_frames=1, max_batch=1), diag=True)
for b in range(N):
    s = base[b % 4]
    ctx.keyframe_upload(b, s["kf_image"]); ctx.keyframe_set_depth(b, s["depth0"], s["var0"])
K = N - 1
if a.dense_k:
    s = synth.make_pair(W, H, seed=100 + K % 4, dense=True)
    ctx.keyframe_upload(K, s["kf_image"]); ctx.keyframe_set_depth(K, s["depth0"], s["var0"])


def transform(s, d):
    """keyframes a few centimetres and fractions of a degree apart, as the poses of a loop-closure batch are (tools/time_sim3_align.py)"""
    k = s - d
    return scaled_transform(xi=(0.002 * k, -0.001 * k, 0.001, 0.01 * k, -0.005 * k, 0.002 * k), scale=1.0)


# the batch holds view -> K; the refinement wants K -> view
Ts_all = np.stack([api.sim3_invert(transform(s, K))[0] for s in range(N - 1)])
counts = [v for v in (1, 4, 16, 42) if v <= N - 1]
dev = {v: [] for v in counts}; wall = {v: [] for v in counts}; sdev = {v: [] for v in counts}
last = {}
for i in range(a.warmup + a.reps):
    for v in counts:   # interleaved: a drift of the clocks reaches every variant alike
        views = list(range(v)); Ts = Ts_all[:v]; lights = [LIGHT] * v
        prm = dict(min_views=min(2, v))
        t0 = time.perf_counter()
        res = ctx.refine_depth(K, views, Ts, lights, level=a.level, params=prm, **FLT)
        t1 = time.perf_counter()
        ms = ctx.profile_refine_depth(K, views, Ts, lights, level=a.level, params=prm, **FLT)[1]
        recs, sms = ctx.profile_sim3_step_lit([K] * v, views, Ts, lights, level=a.level, **FLT)
        last[v] = (res, recs)
        if i >= a.warmup:
            wall[v].append(1e3 * (t1 - t0)); dev[v].append(ms); sdev[v].append(sms)
for v in counts:
    res, recs = last[v]
    st = res["stats"]
    evals = st["n_taking_part"] * v * (N_ITER + 1)
    full = st["n_refined"] + st["n_views_changed"] + st["n_cost_rose"]
    evals_lo = (full * (N_ITER + 1) + (st["n_taking_part"] - full)) * v
    kept_pairs = int(recs["n_kept"].sum())
    line = ("%2d views %dx%d level %d: kept %d taking part %d refined %d (too few %d, no information %d, bad step %d, views changed %d, cost rose %d); "
            "device %.3f ms (min %.3f), wall %.3f ms (min %.3f); %d to %d pixel-view-evaluations: %.4f to %.4f ns each; sim3_step_lit over the same %d pairs: "
            "device %.3f ms (min %.3f), %d kept pixel-views: %.3f ns each") % (
        v, W >> a.level, H >> a.level, a.level, st["n_kept"], st["n_taking_part"], st["n_refined"], st["n_too_few_views"], st["n_no_information"], st["n_bad_step"], st["n_views_changed"],
        st["n_cost_rose"], np.median(dev[v]), min(dev[v]), np.median(wall[v]), min(wall[v]), evals_lo, evals, 1e6 * np.median(dev[v]) / max(evals, 1), 1e6 * np.median(dev[v]) / max(evals_lo, 1), v,
        np.median(sdev[v]), min(sdev[v]), kept_pairs, 1e6 * np.median(sdev[v]) / max(kept_pairs, 1))
    if not a.no_host:
        t0 = time.perf_counter()
        kf = ctx.keyframe_depth_level(K, a.level) + (ctx.image_level(True, K, a.level)[0],)
        imgs = [ctx.image_level(True, s, a.level)[0] for s in range(v)]
        t1 = time.perf_counter()
        ref = R.refine(kf, imgs, R.level_intrinsics(fx, fy, cx, cy, a.level), Ts_all[:v], [LIGHT] * v, FLT_T, dict(min_views=min(2, v)))
        t2 = time.perf_counter()
        for name in R.PLANES:
            g, w = res[name].reshape(-1)[::a.check_every], ref[name].reshape(-1)[::a.check_every]
            assert g.tobytes() == w.tobytes(), (v, name)
        for k in R.INT_FIELDS:
            assert int(st[k]) == ref[k], (v, k, st[k], ref[k])
        line += "; host path: read-back %.1f ms + numpy reference %.1f ms (planes equal on every %dth pixel, integer stats equal)" % (
            1e3 * (t1 - t0), 1e3 * (t2 - t1), a.check_every)
    print(line, flush=True)
cms = [ctx.profile_map_points([K], [np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)], level=a.level, **FLT)[2] for _ in range(a.warmup + a.reps)][a.warmup:]
print("compaction launches over K alone (map_count, map_scan, map_scatter): device %.3f ms (min %.3f)%s" % (
    np.median(cms), min(cms), "; K dense" if a.dense_k else ""), flush=True)
ctx.close()
