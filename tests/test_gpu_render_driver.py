"""The map render above the C ABI: globalOptimize::renderLocalMap / write_pfm of the facade against the Python binding's render of the
same planes and transforms, and ellc_main --render on a tracked sequence (every other output file byte-identical)."""
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
PLANES = (("depth", np.float32), ("var", np.float32), ("source", np.int32), ("agree", np.int32), ("intensity", np.uint8))


def make_sequence(n_frames):
    rng = np.random.default_rng(42)
    tex = synth.value_noise_texture(W, H, rng)
    idepth = synth.smooth_field(W, H, rng, cell=64, lo=0.7, hi=1.3)
    fx, fy, cx, cy = synth.default_intrinsics(W, H)
    step = np.array([0.0008, -0.0005, 0.0004, 0.004, 0.0015, -0.001])
    return [tex] + [synth.render_current(tex, idepth, synth.se3_exp(step * n), fx, fy, cx, cy) for n in range(1, n_frames)]


RENDER_PROGRAM = r"""
// Three keyframes in the loop-closure ring, each with a world pose of its own, rendered into a fourth pose: the planes, the transforms
// and the ring slots' level-0 depth / variance go to files for the caller to render again through another binding.
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
  const float poses[3][6] = {{0, 0, 0, 0, 0, 0}, {0.02f, -0.01f, 0.03f, 0.1f, -0.2f, 0.05f}, {-0.05f, 0.04f, 0.01f, -0.2f, 0.1f, 0.3f}};
  const float view_pose[6] = {0.01f, 0.02f, -0.01f, 0.05f, 0.05f, -0.1f};
  for (int k = 0; k < 3; k++) {
    std::memcpy(f1.poseWrtWorld, poses[k], 24);
    loop.pushToArray(&f1, &dm);
  }
  if (loop.lastPushedArrayId != 2) return 3;
  ellc_map_filter flt;
  flt.max_var = 0.0f; flt.min_support = 2; flt.support_k2 = 1.0f; flt.stride = 1;
  RenderedView v;
  loop.renderLocalMap(view_pose, 0, flt, 0.75f, NULL, v);
  if (v.ids.size() != 3 || v.ids[0] != 0 || v.ids[1] != 1 || v.ids[2] != 2 || v.T.size() != 36) return 4;
  if (v.cols != W || v.rows != H || v.depth.size() != n || v.intensity.size() != n) return 5;
  std::vector<float> d(n), var(n);
  for (int k = 0; k < 3; k++) {
    if (ellc_keyframe_get_depth_level(loop.ring.ctx, v.slots[k], 0, d.data(), var.data()) != ELLC_OK) return 6;
    if (!dump(dir + "/slot" + std::to_string(k) + ".depth", d.data(), n * 4) || !dump(dir + "/slot" + std::to_string(k) + ".var", var.data(), n * 4)) return 7;
  }
  if (!dump(dir + "/T.bin", v.T.data(), 36 * 4) || !dump(dir + "/view.depth", v.depth.data(), n * 4) || !dump(dir + "/view.var", v.var.data(), n * 4) ||
      !dump(dir + "/view.source", v.source.data(), n * 4) || !dump(dir + "/view.agree", v.agree.data(), n * 4) ||
      !dump(dir + "/view.intensity", v.intensity.data(), n))
    return 8;
  write_pfm(dir + "/view.pfm", v.depth, v.cols, v.rows);
  std::printf("n_valid %d\n", v.n_valid);
  // level 1 goes through as well, with planes of its size
  RenderedView v1;
  loop.renderLocalMap(view_pose, 1, flt, 0.75f, NULL, v1);
  if (v1.cols != W / 2 || v1.rows != H / 2 || v1.depth.size() != n / 4 || v1.n_valid <= 0) return 9;
  // into: the tracking runtime's keyframe receives the rendered planes
  RenderedView v2;
  loop.renderLocalMap(view_pose, 0, flt, 0.75f, &f1, v2);
  if (std::memcmp(v2.depth.data(), v.depth.data(), n * 4) != 0 || v2.n_valid != v.n_valid) return 10;
  if (ellc_keyframe_get_depth_level(rt.ctx, f1.kf_slot, 0, d.data(), var.data()) != ELLC_OK) return 11;
  if (std::memcmp(d.data(), v.depth.data(), n * 4) != 0 || std::memcmp(var.data(), v.var.data(), n * 4) != 0) return 12;
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


def test_render_local_map_equals_the_python_bindings_render(tmp_path, ellc):
    frames = make_sequence(1)
    image = np.ascontiguousarray(frames[0], np.uint8)
    raw = tmp_path / "f.raw"
    raw.write_bytes(image.tobytes())
    src = tmp_path / "render.cpp"
    src.write_text(RENDER_PROGRAM)
    exe = tmp_path / "render"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L", CSRC, "-lellc_hip",
                    "-Wl,-rpath," + CSRC], check=True)
    r = subprocess.run([str(exe), str(raw), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stdout.decode()
    n_valid = int([l for l in r.stdout.decode().split("\n") if l.startswith("n_valid ")][0].split()[1])
    view = {name: np.fromfile(tmp_path / ("view." + name), dt).reshape(H, W) for name, dt in PLANES}
    assert n_valid == int((view["source"] >= 0).sum()) > 0
    # the same planes in a context of the binding's, the same transforms
    ctx = ellc.Context(ellc.default_config(W, H, LEVELS, max_keyframes=3))
    try:
        for k in range(3):
            ctx.keyframe_upload(k, image)
            ctx.keyframe_set_depth(k, np.fromfile(tmp_path / ("slot%d.depth" % k), np.float32).reshape(H, W),
                                   np.fromfile(tmp_path / ("slot%d.var" % k), np.float32).reshape(H, W))
        T = np.fromfile(tmp_path / "T.bin", np.float32).reshape(3, 12)
        got = ctx.render_depth([0, 1, 2], T, level=0, agree_k2=AGREE_K2, **FILTER)
    finally:
        ctx.close()
    assert got["n_valid"] == n_valid
    for name, _ in PLANES:
        assert got[name].tobytes() == view[name].tobytes(), name
    assert len(set((view["source"][view["source"] >= 0] >> 24).tolist())) >= 2   # more than one ring entry is seen
    assert read_pfm(tmp_path / "view.pfm").tobytes() == view["depth"].tobytes()


def test_ellc_main_writes_the_render_and_nothing_else_changes(tmp_path):
    n_frames = 17
    frames = make_sequence(n_frames)
    raw = tmp_path / "frames.raw"
    raw.write_bytes(b"".join(np.ascontiguousarray(f, np.uint8).tobytes() for f in frames))
    exe = os.path.join(CSRC, "ellc_main")
    assert os.path.exists(exe), "ellc_main not built (run __graft_entry__.build())"
    plain, rendered = tmp_path / "plain", tmp_path / "rendered"
    plain.mkdir(); rendered.mkdir()
    pfm = tmp_path / "view.pfm"
    for out, extra in ((plain, []), (rendered, ["--render", str(pfm)])):
        r = subprocess.run([exe, str(raw), str(W), str(H), str(n_frames), str(out), "LC"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode()
    head = pfm.read_bytes().split(b"\n", 3)
    assert head[:3] == [b"Pf", b"%d %d" % (W, H), b"-1.0"] and len(head[3]) == 4 * W * H
    depth = read_pfm(pfm)
    print("targets with a depth in the rendered view:", int((depth > 0).sum()))
    assert depth.shape == (H, W) and np.isfinite(depth).all() and (depth >= 0).all() and (depth > 0).sum() > 0
    for name in ("poses_orig.txt", "matchframes_globalopt.txt", "matchframes.txt"):
        assert (plain / name).read_bytes() == (rendered / name).read_bytes(), name
    assert (plain / "poses_orig.txt").stat().st_size > 0
    assert sorted(p.name for p in plain.iterdir()) == sorted(p.name for p in rendered.iterdir()) and not (plain / "view.pfm").exists()
