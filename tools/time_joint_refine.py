#!/usr/bin/env python3
"""Time of ellc_keyframe_joint_step / _apply / _refine over the loop-closure ring of tools/time_refine_depth.py: nine keyframes at
640x480, semi-dense maps, the filter ellc_main --joint-matches uses (no variance test, min_support 3, support_k2 1, stride 1), the
default ellc_joint_params. K is the LAST keyframe; its map and the transforms of the first 1, 3 and 8 other keyframes are refined on
level 0, from the transforms of the loop-closure batch (inverted: keyframe -> view) and the light (0.9, 10). Figures per number of
views, medians over --reps calls after --warmup untimed ones, the variants interleaved:
  step device     HIP events around the four launches of one ellc_keyframe_joint_step (ellc_profile_joint_step)
  apply device    HIP events around the two launches of one ellc_keyframe_joint_apply at the step's own solve (ellc_profile_joint_apply)
  solve           ellc_joint_solve of the step's record, host wall time
  loop wall       the whole ellc_keyframe_joint_refine call (max_iter 6, eps 1e-6, lambda 0) as a caller sees it, the five planes
                  downloaded, and the iterations it accepted
  sim3_step_lit   the same-run device time of ellc_keyframe_sim3_step_lit over the same pairs (K as the source)
  refine_depth    the same-run device time of ellc_keyframe_refine_depth at n_iter = 1 over the same views
usage: tools/time_joint_refine.py [--reps R] [--warmup W] [--level L]"""
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
from map_points_reference import scaled_transform  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--level", type=int, default=0)
a = ap.parse_args()
W, H, L, N = 640, 480, 4, 9
FLT = dict(max_var=0.0, min_support=3, support_k2=1.0, stride=1)
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
counts = (1, 3, 8)
names = ("step", "apply", "solve", "loop", "sim3", "refine")
t = {v: {k: [] for k in names} for v in counts}
last = {}
for i in range(a.warmup + a.reps):
    for v in counts:   # interleaved: a drift of the clocks reaches every variant alike
        views = list(range(v)); Ts = Ts_all[:v]; lights = [LIGHT] * v
        prm = dict(min_views=min(2, v))
        rec, step_ms = ctx.profile_joint_step(K, views, Ts, lights, level=a.level, params=prm, **FLT)
        t0 = time.perf_counter()
        xi, refused = api.joint_solve(rec)
        t1 = time.perf_counter()
        out, apply_ms = ctx.profile_joint_apply(K, views, Ts, xi, lights, level=a.level, params=prm, **FLT)
        t2 = time.perf_counter()
        res = ctx.joint_refine(K, views, Ts, lights, level=a.level, max_iter=6, eps=1e-6, lam=0.0, params=prm, **FLT)
        t3 = time.perf_counter()
        sim3_ms = ctx.profile_sim3_step_lit([K] * v, views, Ts, lights, level=a.level, **FLT)[1]
        refine_ms = ctx.profile_refine_depth(K, views, Ts, lights, level=a.level, params=dict(n_iter=1, min_views=min(2, v)), **FLT)[1]
        last[v] = (rec, refused, out, res)
        if i >= a.warmup:
            for k, x in zip(names, (step_ms, apply_ms, 1e3 * (t1 - t0), 1e3 * (t3 - t2), sim3_ms, refine_ms)):
                t[v][k].append(x)
for v in counts:
    rec, refused, out, res = last[v]
    m = {k: (np.median(x), min(x)) for k, x in t[v].items()}
    print(("%d views %dx%d level %d: kept %d used %d terms %d (solve %s; apply stepped %d, bad step %d); step device %.3f ms (min %.3f), apply device %.3f ms "
           "(min %.3f), solve %.3f ms (min %.3f); loop wall %.3f ms (min %.3f) with %d accepted iterations; sim3_step_lit over the same %d pairs: device "
           "%.3f ms (min %.3f); refine_depth at n_iter 1: device %.3f ms (min %.3f)") % (
        v, W >> a.level, H >> a.level, a.level, rec["n_kept"], rec["n_used"], rec["n_terms"], "refused" if refused else "ok", out["stats"]["n_stepped"],
        out["stats"]["n_bad_step"], m["step"][0], m["step"][1], m["apply"][0], m["apply"][1], m["solve"][0], m["solve"][1], m["loop"][0], m["loop"][1],
        res["iters"], v, m["sim3"][0], m["sim3"][1], m["refine"][0], m["refine"][1]), flush=True)
ctx.close()
