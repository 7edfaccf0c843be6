"""Records tests/golden/pixel_step_bits.npz: H, b and the stepped pose of ONE launch of the tolerance mode's schedule kernel at every
level (ellc_debug_schedule_sums, diagnostic library), as bytes, for the cases of tests/test_gpu_pixel_step_bits.py.

The fixture is what the build of the commit BEFORE a change to the pixel step computes; the test holds every later build to it bit for
bit. So this file is run once, on an MI355X, against that parent build:

    python tests/golden/make_pixel_step_bits.py --lib /path/to/parent/libellc_hip_diag.so [--out tests/golden/pixel_step_bits.npz]

(--lib: a library of the diagnostic ABI WITH the row loads, i.e. the parent's own libellc_hip_diag.so; without --lib the tree's.)
The test imports the case list from here, so generator and test cannot drift apart.

Before it records anything the generator warps every case's points in numpy and asserts that the cases, taken together, put waves on
each path of the step: waves whose lanes are all interior, waves with a lane on the border (the packed window at the clamped origin,
or the per-tap gathers under the row loads), and lanes with none of their four taps in the image.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pixel_step_bits.npz")
SHAPES = [(72, 52, 3), (64, 32, 2)]
MAPS = ["semi_dense", "all", "none", "last_pixel", "chunk256", "chunk256p1"]
TAPS = [1, 0]   # packed taps, then ellc_debug_set_packed_taps(0): the row loads
THREADS = 256   # a block of the schedule's kernels; a wave is 64 consecutive threads, thread t takes records begin + t + 256 k
# [rotation, translation]: zero; a small twist; a shift of about 3 pixels (lanes on the border); a shift that sends about a third of
# the points out of the image. The depths are around 1, so a translation tx moves a point by about fx tx = 0.855 w tx pixels.
POSES = {
    72: np.array([[0, 0, 0, 0, 0, 0], [0.004, -0.003, 0.002, 0.01, -0.008, 0.006], [0, 0, 0, 0.05, -0.045, 0], [0, 0, 0, 0.42, 0, 0]], np.float32),
    64: np.array([[0, 0, 0, 0, 0, 0], [0.004, -0.003, 0.002, 0.01, -0.008, 0.006], [0, 0, 0, 0.055, -0.05, 0], [0, 0, 0, 0.42, 0, 0]], np.float32),
}


def make_pair(w, h):
    from egomotion_with_local_loop_closures_amd import synth
    return synth.make_pair(w, h, seed=1100 + w, rot=0.004, trans=0.012)


def pattern(name, h, w, valid0, level, nblk0):
    """which pixels of an (h, w) level carry a depth hypothesis; nblk0: the blocks per alignment of the level-0 launch"""
    n = h * w
    i = np.arange(n)
    if name == "all":
        m = np.ones(n, bool)
    elif name == "none":
        m = np.zeros(n, bool)
    elif name == "last_pixel":
        m = i == n - 1
    elif name in ("chunk256", "chunk256p1"):
        # level 0: the first V pixels in raster order, V = 256 nblk (every block's chunk is exactly one full step of its 256 threads)
        # or 256 nblk + 1 (ceil(V / nblk) = 257: a second step with one live thread); the coarser levels: the same share of the level
        v0 = THREADS * nblk0 + (1 if name == "chunk256p1" else 0)
        m = i < (v0 if level == 0 else max(1, v0 >> (2 * level)))
    else:   # the semi-dense map of synth (gradient threshold), subsampled for the coarser levels
        m = valid0[:: 1 << level, :: 1 << level][:h, :w].ravel()
    return m.reshape(h, w)


def level_maps(pair, name, L, nblk0):
    """(mask, depth, variance) of every level, each level written by itself (no dense hint: the lists are built)"""
    full = (1.0 / pair["idepth_true"]).astype(np.float32)
    h0, w0 = full.shape
    out = []
    for l in range(L):
        h, w = h0 >> l, w0 >> l
        m = pattern(name, h, w, pair["valid"], l, nblk0)
        d = full[:: 1 << l, :: 1 << l][:h, :w]
        var = np.float32(0.0125) * (1.0 + 0.25 * ((np.arange(h * w).reshape(h, w) % 7) / np.float32(7.0))).astype(np.float32)
        out.append((m, np.where(m, d, 0.0).astype(np.float32), np.where(m, var, -1.0).astype(np.float32)))
    return out


def context(ellc, w, h, L, pair, packed):
    fx, fy, cx, cy = pair["intrinsics"]
    cfg = ellc.default_config(w, h, L, fx=fx, fy=fy, cx=cx, cy=cy, max_iter=(3, 4, 5)[:L], max_keyframes=2, max_frames=2, max_batch=4,
                              early_exit=0, arith=ellc.ARITH_FAST)
    ctx = ellc.Context(cfg, diag=True)
    ctx.keyframe_upload(0, pair["kf_image"])
    ctx.keyframe_set_depth(0, pair["depth0"], pair["var0"])
    ctx.frame_upload(0, pair["cur_image"])
    if not packed:
        ctx.debug_set_packed_taps(False)
    return ctx


def set_map(ctx, maps):
    for l, (_, d, var) in enumerate(maps):
        ctx.keyframe_set_depth_level(0, l, d, var)


def key(w, name, packed, level, field):
    return "w%d/%s/taps%d/l%d/%s" % (w, name, packed, level, field)


def run_cases(ellc, w, h, L, emit):
    """every case of one shape: emit(key, value) for H, b, pose (arrays), kernel (str) and grid (tuple) of each launch"""
    pair = make_pair(w, h)
    batch = [0, 0, 0, 0]   # one keyframe and one frame, four poses
    for packed in TAPS:
        ctx = context(ellc, w, h, L, pair, packed)
        nblk0 = ctx.debug_schedule_sums(batch, batch, 0, POSES[w])["grid"][0]
        for name in MAPS:
            set_map(ctx, level_maps(pair, name, L, nblk0))
            for l in range(L):
                s = ctx.debug_schedule_sums(batch, batch, l, POSES[w])
                for f in ("H", "b", "pose"):
                    emit(key(w, name, packed, l, f), np.ascontiguousarray(s[f]))
                emit(key(w, name, packed, l, "kernel"), s["kernel"])
                emit(key(w, name, packed, l, "grid"), np.array(s["grid"], np.int32))
        ctx.close()
    return nblk0


def path_census(w, h, L, nblk0, grids):
    """numpy warp of every case's records: counts of (interior-only waves, waves with a border lane, lanes without a tap in bounds).
    A wave holds the records begin + 64 j .. begin + 64 j + 63 (+ 256 k) of a block's contiguous chunk [begin, begin + ceil(V / nblk))."""
    from egomotion_with_local_loop_closures_amd import synth
    pair = make_pair(w, h)
    fx0, fy0, cx0, cy0 = pair["intrinsics"]
    interior_waves = border_waves = oob_lanes = 0
    for name in MAPS:
        maps = level_maps(pair, name, L, nblk0)
        for l, (m, d, _) in enumerate(maps):
            s = 2.0 ** l
            fx, fy, cx, cy = np.float32(fx0 / s), np.float32(fy0 / s), np.float32(cx0 / s), np.float32(cy0 / s)
            rows, cols = m.shape
            ys, xs = np.nonzero(m)
            V = xs.size
            if V == 0:
                continue
            nblk = grids[(name, l)][0]
            chunk = (V + nblk - 1) // nblk
            Z = d[ys, xs].astype(np.float64)
            P0 = np.stack([(xs - cx) / fx * Z, (ys - cy) / fy * Z, Z])
            for pose in POSES[w]:
                T = synth.se3_exp(pose)
                P = T[:3, :3] @ P0 + T[:3, 3:4]
                x1 = fx * P[0] / P[2] + cx
                y1 = fy * P[1] / P[2] + cy
                x0, y0 = np.floor(x1), np.floor(y1)
                inter = (x0 >= 1) & (x0 <= cols - 3) & (y0 >= 1) & (y0 <= rows - 3)
                # all four taps outside: both columns x0, x0 + 1 or both rows y0, y0 + 1 (the kernels' bounds tests)
                none = ((x0 < 0) | (x0 > cols - 1)) & ((x1 < 0) | (x1 > cols - 1)) | ((y0 < 0) | (y0 > rows - 1)) & ((y1 < 0) | (y1 > rows - 1))
                oob_lanes += int(none.sum())
                for b in range(nblk):
                    lo, hi = b * chunk, min(V, (b + 1) * chunk)
                    for s0 in range(lo, hi, 64):
                        lanes = inter[s0:min(hi, s0 + 64)]
                        # well inside or well outside the border only: a lane within 0.02 px of an integer could fall either way in f32
                        frac = np.minimum(np.abs(x1[s0:s0 + lanes.size] - np.rint(x1[s0:s0 + lanes.size])),
                                          np.abs(y1[s0:s0 + lanes.size] - np.rint(y1[s0:s0 + lanes.size])))
                        if (frac < 0.02).any():
                            continue
                        if lanes.all():
                            interior_waves += 1
                        else:
                            border_waves += 1
    return interior_waves, border_waves, oob_lanes


FIELDS = ("H", "b", "pose", "kernel", "grid")


def save_fixture(path, out):
    """one array per field, the launches stacked in the order of `case` (a handful of members compresses far better than 300)"""
    cases = sorted({k.rsplit("/", 1)[0] for k in out})
    np.savez_compressed(path, case=np.array(cases), **{f: np.stack([np.asarray(out[c + "/" + f]) for c in cases]) for f in FIELDS})


def load_fixture(path=FIXTURE):
    """{key(...): value} as run_cases emits them"""
    with np.load(path) as z:
        return {str(c) + "/" + f: z[f][i] for i, c in enumerate(z["case"]) for f in FIELDS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="a diagnostic-ABI build of the parent commit (with the row loads)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    from egomotion_with_local_loop_closures_amd import _lib, api
    if args.lib:
        _lib.use_library(args.lib)
    out = {}
    for w, h, L in SHAPES:
        nblk0 = run_cases(api, w, h, L, lambda k, v: out.__setitem__(k, np.array(v) if isinstance(v, str) else v))
        grids = {(name, l): tuple(out[key(w, name, 1, l, "grid")]) for name in MAPS for l in range(L)}
        iw, bw, ol = path_census(w, h, L, nblk0, grids)
        print("%dx%d: nblk at level 0 %d; interior-only waves %d, waves with a border lane %d, lanes without a tap in bounds %d" % (w, h, nblk0, iw, bw, ol))
        assert iw > 0 and bw > 0 and ol > 0, "the cases of this shape leave a path of the pixel step unvisited"
        for name in ("chunk256", "chunk256p1"):
            g = grids[(name, 0)]
            assert g[0] == nblk0 and g[1] <= 1, ("the level-0 launch is not an even split over nblk0 blocks", name, g)
        kernels = sorted({str(out[key(w, name, p, l, "kernel")]) for name in MAPS for p in TAPS for l in range(L)})
        print("   kernels:", ", ".join(kernels))
    save_fixture(args.out, out)
    print("wrote %s: %d launches, %d bytes" % (args.out, len(out) // len(FIELDS), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
