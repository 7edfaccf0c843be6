"""The map export above the C ABI: globalOptimize::exportLocalMap / write_ply of the facade against ellc_keyframe_map_points calls a
program makes itself, and ellc_main --map on a tracked sequence (every other output file byte-identical)."""
import os
import subprocess
import numpy as np
import pytest
from egomotion_with_local_loop_closures_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egomotion_with_local_loop_closures_amd", "csrc")
W, H = 160, 120


def make_sequence(n_frames):
    rng = np.random.default_rng(42)
    tex = synth.value_noise_texture(W, H, rng)
    idepth = synth.smooth_field(W, H, rng, cell=64, lo=0.7, hi=1.3)
    fx, fy, cx, cy = synth.default_intrinsics(W, H)
    step = np.array([0.0008, -0.0005, 0.0004, 0.004, 0.0015, -0.001])
    return [tex] + [synth.render_current(tex, idepth, synth.se3_exp(step * n), fx, fy, cx, cy) for n in range(1, n_frames)]


EXPORT_PROGRAM = r"""
// Three keyframes in the loop-closure ring, each with a world pose of its own; exportLocalMap against one ellc_keyframe_map_points call
// per ring slot with transforms computed here.
#include "ellc_facade.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace ellc;
static void world_from_keyframe(const float* pose, float scale, float* T12) {   // exp(pose)^-1 = [R^T | -R^T t], the 3x3 block scaled
  float E[16];
  ellc_se3_exp(pose, E);
  const float t[3] = {E[3], E[7], E[11]};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T12[4 * r + c] = E[4 * c + r] * scale;
    T12[4 * r + 3] = -((E[0 + r] * t[0] + E[4 + r] * t[1]) + E[8 + r] * t[2]);
  }
}
int main(int argc, char** argv) {
  const int W = 160, H = 120;
  std::vector<uint8_t> img((size_t)W * H);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(img.data(), 1, img.size(), f) != img.size()) return 2;
  std::fclose(f);
  ellc_config cfg;
  ellc_default_config(&cfg, W, H, 4);
  Runtime rt(cfg);
  globalOptimize loop(rt, std::string(argv[2]) + "/matchframes_globalopt.txt");
  frame f1(rt, img.data());
  depthMap dm(rt);
  dm.formDepthMap(&f1);
  dm.updateDepthImage();
  const float poses[3][6] = {{0, 0, 0, 0, 0, 0}, {0.02f, -0.01f, 0.03f, 0.1f, -0.2f, 0.05f}, {-0.3f, 0.2f, 0.1f, 1.0f, 0.5f, -2.0f}};
  float scale[globalOptimize::MAX_LOOP_ARRAY_LENGTH_SCALE_AVG];
  for (int i = 0; i < globalOptimize::MAX_LOOP_ARRAY_LENGTH_SCALE_AVG; i++) scale[i] = 1.0f;
  scale[0] = 1.5f; scale[2] = 0.5f;
  for (int k = 0; k < 3; k++) {
    std::memcpy(f1.poseWrtWorld, poses[k], 24);
    loop.pushToArray(&f1, &dm);
  }
  ellc_map_filter flt;
  flt.max_var = 0.0f; flt.min_support = 2; flt.support_k2 = 1.0f; flt.stride = 1;
  for (int level = 0; level < 2; level++) {
    for (int with_scale = 0; with_scale < 2; with_scale++) {
      std::vector<ellc_map_point> cloud;
      const std::vector<int> ids = loop.exportLocalMap(flt, level, cloud, with_scale ? scale : NULL);
      if (ids.size() != 3 || ids[0] != 0 || ids[1] != 1 || ids[2] != 2) return 3;
      std::vector<ellc_map_point> own;
      for (int k = 0; k < 3; k++) {
        float T[12];
        world_from_keyframe(poses[k], with_scale ? scale[k] : 1.0f, T);
        int slot = loop.loopFrameArray[k].kf_slot, n = 0;
        if (ellc_keyframe_map_points(loop.ring.ctx, 1, &slot, T, level, &flt, NULL, 0, NULL, &n) != ELLC_OK) return 4;
        std::vector<ellc_map_point> part((size_t)n + 1);
        if (ellc_keyframe_map_points(loop.ring.ctx, 1, &slot, T, level, &flt, part.data(), n, NULL, &n) != ELLC_OK) return 5;
        for (int i = 0; i < n; i++) { part[i].source = (uint16_t)k; own.push_back(part[i]); }
      }
      if (own.size() != cloud.size() || own.empty()) return 6;
      if (std::memcmp(own.data(), cloud.data(), own.size() * sizeof(ellc_map_point)) != 0) return 7;
      std::printf("level %d scale %d points %zu\n", level, with_scale, cloud.size());
      if (level == 0 && with_scale) write_ply(std::string(argv[2]) + "/ring.ply", cloud);
    }
  }
  return 0;
}
"""


def read_ply(path):
    data = open(path, "rb").read()
    head, sep, payload = data.partition(b"end_header\n")
    assert sep
    lines = head.decode().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int([l for l in lines if l.startswith("element vertex ")][0].split()[2])
    assert [l for l in lines if l.startswith("property ")] == ["property float x", "property float y", "property float z", "property uchar intensity",
                                                               "property float var"]
    assert len(payload) == 17 * n
    return np.frombuffer(payload, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "u1"), ("var", "<f4")]))


def test_export_local_map_equals_the_programs_own_calls(tmp_path):
    frames = make_sequence(1)
    raw = tmp_path / "f.raw"
    raw.write_bytes(np.ascontiguousarray(frames[0], np.uint8).tobytes())
    src = tmp_path / "export.cpp"
    src.write_text(EXPORT_PROGRAM)
    exe = tmp_path / "export"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L", CSRC, "-lellc_hip",
                    "-Wl,-rpath," + CSRC], check=True)
    r = subprocess.run([str(exe), str(raw), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stdout.decode()
    lines = [l for l in r.stdout.decode().strip().split("\n") if l.startswith("level ")]
    assert len(lines) == 4
    cloud = read_ply(tmp_path / "ring.ply")
    assert cloud.size == int(lines[1].split()[-1]) and cloud.size > 0
    assert np.isfinite(cloud["x"]).all() and np.isfinite(cloud["y"]).all() and np.isfinite(cloud["z"]).all() and (cloud["var"] >= 0).all()


def test_ellc_main_writes_the_map_and_nothing_else_changes(tmp_path):
    n_frames = 17
    frames = make_sequence(n_frames)
    raw = tmp_path / "frames.raw"
    raw.write_bytes(b"".join(np.ascontiguousarray(f, np.uint8).tobytes() for f in frames))
    exe = os.path.join(CSRC, "ellc_main")
    assert os.path.exists(exe), "ellc_main not built (run __graft_entry__.build())"
    plain, mapped = tmp_path / "plain", tmp_path / "mapped"
    plain.mkdir(); mapped.mkdir()
    ply = tmp_path / "cloud.ply"
    for out, extra in ((plain, []), (mapped, ["--map", str(ply)])):
        r = subprocess.run([exe, str(raw), str(W), str(H), str(n_frames), str(out), "LC"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode()
    cloud = read_ply(ply)
    print("points in the ring's map:", cloud.size)
    assert cloud.size > 0
    assert np.isfinite(cloud["x"]).all() and np.isfinite(cloud["y"]).all() and np.isfinite(cloud["z"]).all()
    for name in ("poses_orig.txt", "matchframes_globalopt.txt", "matchframes.txt"):
        assert (plain / name).read_bytes() == (mapped / name).read_bytes(), name
    assert (plain / "poses_orig.txt").stat().st_size > 0
    assert not (plain / "cloud.ply").exists()
