#!/usr/bin/env python3
"""Device time of one ellc_align_quality_at call (its staging copy, the pixel pass gn_fca_quality and gn_quality_finish) at B = 32,
640x480, level 0, on the scenes of bench.py's workload, in both arithmetic modes: HIP events on the context's stream around the
call, 50 untimed calls, then the median of 200. Beside it, from the same context, the level-0 launch of the alignment's own list
kernel over the same 32 alignments (ellc_profile_gn_kernel), which reads only the pixels that carry a depth.
usage: tools/time_align_quality.py [--level L] [--batch B]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from egomotion_with_local_loop_closures_amd import api, synth  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # noqa: E402
import diaglib  # noqa: E402,F401  (ELLC_LIB_PATH -> _lib.use_library: diagnostic builds)

ap = argparse.ArgumentParser()
ap.add_argument("--level", type=int, default=0)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--reps", type=int, default=200)
a = ap.parse_args()
W, H, L, B = 640, 480, 4, a.batch
hip = C.CDLL("libamdhip64.so")


def ck(st, what):
    if st != 0:
        raise RuntimeError("%s -> %d" % (what, st))


scenes = synth.make_shared_frame_batch(W, H, B, seed=0x5EED)   # bench.py's default workload, rank 0
fx, fy, cx, cy = scenes[0]["intrinsics"]
for arith, name in ((api.ARITH_FAST, "fast"), (api.ARITH_EXACT, "exact")):
    ctx = api.Context(api.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, early_exit=0, max_keyframes=B, max_frames=1, max_batch=B, arith=arith), diag=True)
    ctx.frame_upload(0, scenes[0]["cur_image"])
    for b, s in enumerate(scenes):
        ctx.keyframe_upload(b, s["kf_image"]); ctx.keyframe_set_depth(b, s["depth0"], s["var0"])
    kf = np.arange(B, dtype=np.int32); fr = np.zeros(B, np.int32)
    poses, _, _ = ctx.align(kf, fr)
    stream = C.c_void_p(ctx._l.ellc_stream(ctx.h))
    e0, e1 = C.c_void_p(), C.c_void_p()
    ck(hip.hipEventCreate(C.byref(e0)), "hipEventCreate"); ck(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    for _ in range(a.warmup):
        q = ctx.align_quality(kf, fr, poses, level=a.level)
    ms = []
    for _ in range(a.reps):
        ck(hip.hipEventRecord(e0, stream), "hipEventRecord")
        ctx.align_quality(kf, fr, poses, level=a.level)
        ck(hip.hipEventRecord(e1, stream), "hipEventRecord")
        ck(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        t = C.c_float(0)
        ck(hip.hipEventElapsedTime(C.byref(t), e0, e1), "hipEventElapsedTime")
        ms.append(t.value)
    ms = np.array(ms)
    list_ms, _, valid = ctx.profile_gn_kernel(kf, fr, a.level, reps=50)
    n = (W >> a.level) * (H >> a.level)
    print("%-5s B %d level %d: ellc_align_quality_at %.1f us (median of %d; min %.1f, p90 %.1f); list kernel launch over the same alignments %.1f us; "
          "%.1f %% of the %d pixels carry a depth; mean overlap %.3f, mean rms %.2f" %
          (name, B, a.level, 1e3 * np.median(ms), a.reps, 1e3 * ms.min(), 1e3 * np.percentile(ms, 90), 1e3 * list_ms,
           100.0 * valid / (B * n), n, q["overlap"].mean(), q["rms"].mean()))
    ck(hip.hipEventDestroy(e0), "hipEventDestroy"); ck(hip.hipEventDestroy(e1), "hipEventDestroy")
    ctx.close()
