"""The absorb call above the C ABI: ellc_main --absorb-matches on a tracked sequence (one well-formed line per push, finite poses, and
nothing changes without the flag), and globalOptimize::absorbMatches of the facade against the Python binding's depth_absorb on the
same slots, state and transforms."""
import os
import subprocess
import numpy as np
import pytest

from test_gpu_fuse_driver import make_sequence, W, H, LEVELS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egomotion_with_local_loop_closures_amd", "csrc")
STATS = ("n_kept", "n_in_view", "n_interior", "n_candidates", "n_visited", "n_created", "n_merged", "n_replaced", "n_occluded", "n_skipped",
         "targets_hit", "targets_touched", "targets_truncated", "n_valid_before", "n_valid_after")
HYP = (("invDepth", np.float32), ("invDepthSmoothed", np.float32), ("variance", np.float32), ("varianceSmoothed", np.float32),
       ("validity", np.int32), ("blacklisted", np.int32), ("valid", np.uint8))


def identity_holds(s):
    return s["n_visited"] == s["n_created"] + s["n_merged"] + s["n_replaced"] + s["n_occluded"] + s["n_skipped"]


def test_ellc_main_absorbs_every_push_and_nothing_changes_without_the_flag(tmp_path):
    n_frames = 17
    frames = make_sequence(n_frames)
    raw = tmp_path / "frames.raw"
    raw.write_bytes(b"".join(np.ascontiguousarray(f, np.uint8).tobytes() for f in frames))
    exe = os.path.join(CSRC, "ellc_main")
    assert os.path.exists(exe), "ellc_main not built (run __graft_entry__.build())"
    plain, again, absorbed = tmp_path / "plain", tmp_path / "again", tmp_path / "absorbed"
    stats_file = tmp_path / "absorb.txt"
    for out, extra in ((plain, []), (again, []), (absorbed, ["--absorb-matches", str(stats_file)])):
        out.mkdir()
        r = subprocess.run([exe, str(raw), str(W), str(H), str(n_frames), str(out), "LC"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout.decode()
    lines = [l.split() for l in stats_file.read_text().splitlines()]
    print(stats_file.read_text())
    # a keyframe is finished, and pushed, at every KEYFRAME_PROPAGATE_INTERVAL-th frame and at the last one: the keyframes the pose file names
    poses = np.array([[float(x) for x in l.split()] for l in (absorbed / "poses_orig.txt").read_text().splitlines()])
    pushed = sorted(set(int(k) for k in poses[:, 1]))
    assert len(lines) == len(pushed) == 3
    ids = []
    for l in lines:
        assert len(l) == 2 + len(STATS)
        v = [int(x) for x in l]
        s = dict(zip(STATS, v[2:]))
        ids.append(v[0])
        assert all(x >= 0 for x in v) and identity_holds(s), l
        assert s["n_candidates"] <= s["n_interior"] <= s["n_in_view"] <= s["n_kept"] and s["targets_touched"] <= s["targets_hit"] <= s["n_candidates"]
        assert s["n_valid_after"] == s["n_valid_before"] + s["n_created"]
        assert (v[1] > 0) or not any(v[2:])   # a push without a match absorbs nothing
    assert ids == pushed
    assert any(int(l[1]) > 0 and int(l[2 + STATS.index("n_visited")]) > 0 for l in lines)   # a condition of the test: a push that folds something
    assert poses.shape[0] == n_frames - 1 and np.isfinite(poses).all()
    # without the flag every output file is what a second run without it writes, byte for byte
    for name in ("poses_orig.txt", "matchframes_globalopt.txt", "matchframes.txt"):
        assert (plain / name).read_bytes() == (again / name).read_bytes(), name
    assert (plain / "poses_orig.txt").stat().st_size > 0
    assert sorted(p.name for p in plain.iterdir()) == sorted(p.name for p in absorbed.iterdir())


ABSORB_PROGRAM = r"""
// Three pushes of one keyframe at three world poses and frame ids with absorbMatches on: the third push's state before the call, the candidates' ring
// slots, their transforms and the stats go to files for the caller to run the same fold through another binding.
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
  {   // too few keyframe slots in the tracking runtime: the push throws
    Runtime small(cfg);
    globalOptimize loop(small, dir + "/unused.txt");
    loop.absorbMatches = true;
    frame f0(small, img.data());
    depthMap dm0(small);
    dm0.formDepthMap(&f0);
    dm0.updateDepthImage();
    bool thrown = false;
    try { loop.pushToArray(&f0, &dm0); } catch (const std::exception&) { thrown = true; }
    if (!thrown) return 3;
  }
  cfg.max_keyframes = 2 + globalOptimize::MAX_LOOP_ARRAY_LENGTH_SCALE_AVG;
  Runtime rt(cfg);
  globalOptimize loop(rt, dir + "/matchframes_globalopt.txt");
  loop.absorbMatches = true;
  loop.absorb_file.open((dir + "/absorb.txt").c_str());
  frame f1(rt, img.data());
  depthMap dm(rt);
  dm.formDepthMap(&f1);
  dm.updateDepthImage();
  const float poses[3][6] = {{0, 0, 0, 0, 0, 0}, {0.002f, -0.001f, 0.003f, 0.01f, -0.02f, 0.005f}, {-0.005f, 0.004f, 0.001f, -0.02f, 0.01f, 0.03f}};
  std::vector<float> a(n), b(n), c(n), d(n);
  std::vector<int32_t> v(n), bl(n);
  std::vector<uint8_t> ok(n);
  for (int k = 0; k < 3; k++) {
    std::memcpy(f1.poseWrtWorld, poses[k], 24);
    f1.frameId = 1 + 20 * k;   // (a candidate must be more than eight frames older than the pushed keyframe)
    if (k == 2) {
      ellc_hypotheses h;
      h.invDepth = a.data(); h.invDepthSmoothed = b.data(); h.variance = c.data(); h.varianceSmoothed = d.data();
      h.validity_counter = v.data(); h.blacklisted = bl.data(); h.isValid = ok.data();
      if (ellc_depth_get_state(rt.ctx, &h) != ELLC_OK) return 4;
      if (!dump(dir + "/state.invDepth", a.data(), n * 4) || !dump(dir + "/state.invDepthSmoothed", b.data(), n * 4) ||
          !dump(dir + "/state.variance", c.data(), n * 4) || !dump(dir + "/state.varianceSmoothed", d.data(), n * 4) ||
          !dump(dir + "/state.validity", v.data(), n * 4) || !dump(dir + "/state.blacklisted", bl.data(), n * 4) || !dump(dir + "/state.valid", ok.data(), n))
        return 5;
    }
    loop.pushToArray(&f1, &dm);
    if (loop.lastAbsorbStats.B != (int)loop.lastMatchSlots.size()) return 6;
  }
  const int B = loop.lastAbsorbStats.B;
  if (B < 1 || (int)loop.lastMatchSim3.size() != B || loop.refineMatchSim3) return 7;
  std::vector<float> T((size_t)B * 12);
  for (int q = 0; q < B; q++) {
    std::memcpy(&T[(size_t)q * 12], loop.lastMatchSim3[(size_t)q].T, 48);
    if (ellc_keyframe_get_depth_level(loop.ring.ctx, loop.lastMatchSlots[(size_t)q], 0, a.data(), b.data()) != ELLC_OK) return 8;
    if (!dump(dir + "/slot" + std::to_string(q) + ".depth", a.data(), n * 4) || !dump(dir + "/slot" + std::to_string(q) + ".var", b.data(), n * 4)) return 9;
  }
  if (!dump(dir + "/T.bin", T.data(), T.size() * 4) || !dump(dir + "/stats.bin", &loop.lastAbsorbStats.stats, sizeof(ellc_absorb_stats))) return 10;
  std::printf("B %d\n", B);
  return 0;
}
"""


def test_absorb_matches_equals_the_python_bindings_absorb(tmp_path, ellc):
    image = np.ascontiguousarray(make_sequence(1)[0], np.uint8)
    raw = tmp_path / "f.raw"
    raw.write_bytes(image.tobytes())
    src = tmp_path / "absorb.cpp"
    src.write_text(ABSORB_PROGRAM)
    exe = tmp_path / "absorb"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L", CSRC, "-lellc_hip",
                    "-Wl,-rpath," + CSRC], check=True)
    r = subprocess.run([str(exe), str(raw), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stdout.decode()
    B = int([l for l in r.stdout.decode().split("\n") if l.startswith("B ")][0].split()[1])
    want = dict(zip(STATS + ("reserved",), np.fromfile(tmp_path / "stats.bin", np.int32).tolist()))
    lines = [l.split() for l in (tmp_path / "absorb.txt").read_text().splitlines()]
    assert len(lines) == 3 and [int(x) for x in lines[2][2:]] == [want[k] for k in STATS] and int(lines[2][1]) == B == 2 and int(lines[0][1]) == 0
    assert identity_holds(want) and want["n_visited"] > 0 and want["reserved"] == 0
    # the same planes, state and transforms in a context of the binding's: slot 0 is the depth map's keyframe, 1.. the candidates
    ctx = ellc.Context(ellc.default_config(W, H, LEVELS, max_keyframes=1 + B))
    try:
        for k in range(1 + B):
            ctx.keyframe_upload(k, image)
        for k in range(B):
            ctx.keyframe_set_depth(1 + k, np.fromfile(tmp_path / ("slot%d.depth" % k), np.float32).reshape(H, W),
                                   np.fromfile(tmp_path / ("slot%d.var" % k), np.float32).reshape(H, W))
        ctx.depth_set_keyframe(0)
        ctx.depth_set_state({name: np.fromfile(tmp_path / ("state." + name), dt).reshape(H, W) for name, dt in HYP})
        T = np.fromfile(tmp_path / "T.bin", np.float32).reshape(B, 12)
        got = ctx.depth_absorb(list(range(1, 1 + B)), T, params=dict(finalise=0), max_var=0.0, min_support=3, support_k2=1.0, stride=1)
    finally:
        ctx.close()
    print("facade", want, "binding", got)
    assert got == want
