"""The fused view above the C ABI: globalOptimize::fuseLocalMap / write_pfm of the facade against the Python binding's fuse_depth of the
same planes and transforms, and ellc_main --fuse on a tracked sequence against the binding's fuse of the ring the driver fused
(--fuse-inputs), every other output file byte-identical."""
import os
import subprocess
import numpy as np
import pytest
from egomotion_with_local_loop_closures_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egomotion_with_local_loop_closures_amd", "csrc")
W, H, LEVELS = 160, 120, 4
FILTER = dict(max_var=0.0, min_support=2, support_k2=1.0, stride=1)
AGREE_K2 = 0.75
PLANES = (("depth", np.float32), ("var", np.float32), ("source", np.int32), ("agree", np.int32), ("merged", np.int32), ("intensity", np.uint8))


def make_sequence(n_frames):
    rng = np.random.default_rng(42)
    tex = synth.value_noise_texture(W, H, rng)
    idepth = synth.smooth_field(W, H, rng, cell=64, lo=0.7, hi=1.3)
    fx, fy, cx, cy = synth.default_intrinsics(W, H)
    step = np.array([0.0008, -0.0005, 0.0004, 0.004, 0.0015, -0.001])
    return [tex] + [synth.render_current(tex, idepth, synth.se3_exp(step * n), fx, fy, cx, cy) for n in range(1, n_frames)]


FUSE_PROGRAM = r"""
// Three keyframes in the loop-closure ring, each with a world pose of its own, fused into a fourth pose: the planes, the transforms and
// the ring slots' level-0 depth / variance go to files for the caller to fuse again through another binding.
#include "ellc_facade.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace ellc;
static bool dump(const std::string& path, const void* p, size_t bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
  std::fclose(f);
  return ok;
}
int main(int argc, char** argv) {
  const int W = 160, H = 120;
  const size_t n = (size_t)W * H;
  if (argc < 3) return 1;
  const std::string dir = argv[2];
  std::vector<uint8_t> img(n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(img.data(), 1, img.size(), f) != img.size()) return 2;
  std::fclose(f);
  ellc_config cfg;
  ellc_default_config(&cfg, W, H, 4);
  Runtime rt(cfg);
  globalOptimize loop(rt, dir + "/matchframes_globalopt.txt");
  frame f1(rt, img.data());
  depthMap dm(rt);
  dm.formDepthMap(&f1);
  dm.updateDepthImage();
  const float poses[3][6] = {{0, 0, 0, 0, 0, 0}, {0.002f, -0.001f, 0.003f, 0.01f, -0.02f, 0.005f}, {-0.005f, 0.004f, 0.001f, -0.02f, 0.01f, 0.03f}};
  const float view_pose[6] = {0.001f, 0.002f, -0.001f, 0.005f, 0.005f, -0.01f};
  for (int k = 0; k < 3; k++) {
    std::memcpy(f1.poseWrtWorld, poses[k], 24);
    loop.pushToArray(&f1, &dm);
  }
  if (loop.lastPushedArrayId != 2) return 3;
  ellc_map_filter flt;
  flt.max_var = 0.0f; flt.min_support = 2; flt.support_k2 = 1.0f; flt.stride = 1;
  FusedView v;
  loop.fuseLocalMap(view_pose, 0, flt, 0.75f, ELLC_FUSE_MAX_MERGE, NULL, v);
  if (v.ids.size() != 3 || v.ids[0] != 0 || v.ids[1] != 1 || v.ids[2] != 2 || v.T.size() != 36 || v.max_merge != ELLC_FUSE_MAX_MERGE) return 4;
  if (v.cols != W || v.rows != H || v.depth.size() != n || v.merged.size() != n || v.intensity.size() != n) return 5;
  std::vector<float> d(n), var(n);
  for (int k = 0; k < 3; k++) {
    if (ellc_keyframe_get_depth_level(loop.ring.ctx, v.slots[k], 0, d.data(), var.data()) != ELLC_OK) return 6;
    if (!dump(dir + "/slot" + std::to_string(k) + ".depth", d.data(), n * 4) || !dump(dir + "/slot" + std::to_string(k) + ".var", var.data(), n * 4)) return 7;
  }
  if (!dump(dir + "/T.bin", v.T.data(), 36 * 4) || !dump(dir + "/view.depth", v.depth.data(), n * 4) || !dump(dir + "/view.var", v.var.data(), n * 4) ||
      !dump(dir + "/view.source", v.source.data(), n * 4) || !dump(dir + "/view.agree", v.agree.data(), n * 4) ||
      !dump(dir + "/view.merged", v.merged.data(), n * 4) || !dump(dir + "/view.intensity", v.intensity.data(), n))
    return 8;
  write_pfm(dir + "/view.pfm", v.depth, v.cols, v.rows);
  std::printf("n_valid %d\nn_fused %d\n", v.n_valid, v.n_fused);
  // the render of the same view: what the render decides is the same
  RenderedView r;
  loop.renderLocalMap(view_pose, 0, flt, 0.75f, NULL, r);
  if (r.n_valid != v.n_valid || std::memcmp(r.source.data(), v.source.data(), n * 4) != 0 || std::memcmp(r.agree.data(), v.agree.data(), n * 4) != 0) return 9;
  // level 1 goes through as well, with planes of its size; max_merge 0 is the render
  FusedView v1;
  loop.fuseLocalMap(view_pose, 1, flt, 0.75f, 0, NULL, v1);
  if (v1.cols != W / 2 || v1.rows != H / 2 || v1.depth.size() != n / 4 || v1.merged.size() != n / 4 || v1.n_valid <= 0 || v1.n_fused != 0) return 10;
  // into: the tracking runtime's keyframe receives the fused planes
  FusedView v2;
  loop.fuseLocalMap(view_pose, 0, flt, 0.75f, ELLC_FUSE_MAX_MERGE, &f1, v2);
  if (std::memcmp(v2.depth.data(), v.depth.data(), n * 4) != 0 || v2.n_valid != v.n_valid || v2.n_fused != v.n_fused) return 11;
  if (ellc_keyframe_get_depth_level(rt.ctx, f1.kf_slot, 0, d.data(), var.data()) != ELLC_OK) return 12;
  if (std::memcmp(d.data(), v.depth.data(), n * 4) != 0 || std::memcmp(var.data(), v.var.data(), n * 4) != 0) return 13;
  return 0;
}
"""


def read_pfm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    assert parts[0] == b"Pf" and float(parts[2]) < 0   # greyscale, little-endian
    cols, rows = (int(v) for v in parts[1].split())
    assert len(parts[3]) == 4 * cols * rows
    return np.frombuffer(parts[3], "<f4").reshape(rows, cols)[::-1]   # PFM stores its scanlines bottom to top


def test_fuse_local_map_equals_the_python_bindings_fuse(tmp_path, ellc):
    frames = make_sequence(1)
    image = np.ascontiguousarray(frames[0], np.uint8)
    raw = tmp_path / "f.raw"
    raw.write_bytes(image.tobytes())
    src = tmp_path / "fuse.cpp"
    src.write_text(FUSE_PROGRAM)
    exe = tmp_path / "fuse"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L", CSRC, "-lellc_hip",
                    "-Wl,-rpath," + CSRC], check=True)
    r = subprocess.run([str(exe), str(raw), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stdout.decode()
    n_valid, n_fused = (int([l for l in r.stdout.decode().split("\n") if l.startswith(k + " ")][0].split()[1]) for k in ("n_valid", "n_fused"))
    view = {name: np.fromfile(tmp_path / ("view." + name), dt).reshape(H, W) for name, dt in PLANES}
    assert n_valid == int((view["source"] >= 0).sum()) > 0 and n_fused == int((view["merged"] >= 2).sum()) > 0
    # the same planes in a context of the binding's, the same transforms
    ctx = ellc.Context(ellc.default_config(W, H, LEVELS, max_keyframes=3))
    try:
        for k in range(3):
            ctx.keyframe_upload(k, image)
            ctx.keyframe_set_depth(k, np.fromfile(tmp_path / ("slot%d.depth" % k), np.float32).reshape(H, W),
                                   np.fromfile(tmp_path / ("slot%d.var" % k), np.float32).reshape(H, W))
        T = np.fromfile(tmp_path / "T.bin", np.float32).reshape(3, 12)
        got = ctx.fuse_depth([0, 1, 2], T, level=0, agree_k2=AGREE_K2, max_merge=64, **FILTER)
    finally:
        ctx.close()
    assert got["n_valid"] == n_valid and got["n_fused"] == n_fused
    for name, _ in PLANES:
        assert got[name].tobytes() == view[name].tobytes(), name
    assert (view["merged"] >= 3).sum() > 0   # more than one ring entry is merged into a target
    assert read_pfm(tmp_path / "view.pfm").tobytes() == view["depth"].tobytes()


def test_ellc_main_writes_the_fused_view_and_nothing_else_changes(tmp_path, ellc):
    n_frames = 17
    frames = make_sequence(n_frames)
    raw = tmp_path / "frames.raw"
    raw.write_bytes(b"".join(np.ascontiguousarray(f, np.uint8).tobytes() for f in frames))
    exe = os.path.join(CSRC, "ellc_main")
    assert os.path.exists(exe), "ellc_main not built (run __graft_entry__.build())"
    plain, fused, inputs = tmp_path / "plain", tmp_path / "fused", tmp_path / "inputs"
    plain.mkdir(); fused.mkdir(); inputs.mkdir()
    pfm, rendered_pfm = tmp_path / "fused.pfm", tmp_path / "rendered.pfm"
    for out, extra in ((plain, []), (fused, ["--render", str(rendered_pfm), "--fuse", str(pfm), "--fuse-inputs", str(inputs)])):
        r = subprocess.run([exe, str(raw), str(W), str(H), str(n_frames), str(out), "LC"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode()
    head = pfm.read_bytes().split(b"\n", 3)
    assert head[:3] == [b"Pf", b"%d %d" % (W, H), b"-1.0"] and len(head[3]) == 4 * W * H
    depth, rendered = read_pfm(pfm), read_pfm(rendered_pfm)
    assert depth.shape == (H, W) and np.isfinite(depth).all() and (depth >= 0).all() and (depth > 0).sum() > 0
    # the ring as the driver fused it (--fuse-inputs), fused again through the binding: the filter and agree_k2 of --render, max_merge 64
    T = np.fromfile(inputs / "T.bin", np.float32).reshape(-1, 12)
    B = T.shape[0]
    assert B >= 2 and sorted(p.name for p in inputs.iterdir()) == sorted(["T.bin"] + ["slot%d.%s" % (k, e) for k in range(B) for e in ("depth", "var")])
    ctx = ellc.Context(ellc.default_config(W, H, LEVELS, max_keyframes=B))
    try:
        for k in range(B):
            ctx.keyframe_upload(k, np.ascontiguousarray(frames[0], np.uint8))   # (the grey values do not enter the depth plane)
            ctx.keyframe_set_depth(k, np.fromfile(inputs / ("slot%d.depth" % k), np.float32).reshape(H, W),
                                   np.fromfile(inputs / ("slot%d.var" % k), np.float32).reshape(H, W))
        kw = dict(level=0, agree_k2=1.0, max_var=0.0, min_support=3, support_k2=1.0, stride=1)
        want = ctx.fuse_depth(list(range(B)), T, max_merge=64, **kw)
        want_render = ctx.render_depth(list(range(B)), T, **kw)
    finally:
        ctx.close()
    assert depth.tobytes() == want["depth"].tobytes()
    assert rendered.tobytes() == want_render["depth"].tobytes()
    moved = depth.view(np.uint32) != rendered.view(np.uint32)
    print("requests", B, "targets with a depth in the fused view:", int((depth > 0).sum()), "fused", want["n_fused"], "of which differ from the render's:",
          int(moved.sum()))
    # the driver really fuses: targets move, and only where members were merged
    assert want["n_fused"] > 0 and moved.sum() > 0 and (want["merged"][moved] >= 2).all() and (want["agree"][moved] >= 2).all()
    assert np.array_equal(depth > 0, rendered > 0)
    for name in ("poses_orig.txt", "matchframes_globalopt.txt", "matchframes.txt"):
        assert (plain / name).read_bytes() == (fused / name).read_bytes(), name
    assert (plain / "poses_orig.txt").stat().st_size > 0
    assert sorted(p.name for p in plain.iterdir()) == sorted(p.name for p in fused.iterdir()) and not (plain / "fused.pfm").exists()
