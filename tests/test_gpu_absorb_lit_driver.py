"""The v24 light above the C ABI. globalOptimize::absorbMatches with matchAffineLight (a facade program: the fold runs at the lights of
lastMatchSim3, and equals the Python binding's depth_absorb(lights=) on the same slots, state, transforms and lights);
globalOptimize::restoreAffineLight (a facade program: a brightened test frame is scored at (1, 0), the lights are fitted, it is scored
again and the map restarts at the winner's light - each step against the binding); and ellc_main: --absorb-matches with --match-light,
--restore-light with --restore-connection, --restore-light alone refused, and without the new flags every file byte for byte what it was.

The facade programs are those of tests/test_gpu_absorb_driver.py and tests/test_gpu_restore_connection.py with the new switches set and
the lights dumped (ellc_main keeps no state a replay could start from; the facade is what it calls)."""
import os
import subprocess
import numpy as np
import pytest

import absorb_lit_reference as AL
from test_gpu_absorb_driver import ABSORB_PROGRAM, HYP, STATS, identity_holds
from test_gpu_fuse_driver import make_sequence, W, H, LEVELS
from test_gpu_restore_connection import RESTORE_PROGRAM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egomotion_with_local_loop_closures_amd", "csrc")
FILES = ("poses_orig.txt", "matchframes.txt", "matchframes_globalopt.txt")
FLT = dict(max_var=0.0, min_support=3, support_k2=1.0, stride=1)   # the filter of ellc_main --map


def patched(text, pairs):
    for old, new in pairs:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    return text


def compile_program(tmp_path, name, text):
    src = tmp_path / (name + ".cpp")
    src.write_text(text)
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L", CSRC, "-lellc_hip",
                    "-Wl,-rpath," + CSRC], check=True)
    return exe


# the absorb program with the Sim(3) refinement and its light on, and the lights it folded at written out
ABSORB_LIT_PROGRAM = patched(ABSORB_PROGRAM, [
    ("  loop.absorbMatches = true;\n  loop.absorb_file.open(", "  loop.absorbMatches = true;\n  loop.refineMatchSim3 = true;\n  loop.matchAffineLight = true;\n  loop.absorb_file.open("),
    ("(int)loop.lastMatchSim3.size() != B || loop.refineMatchSim3) return 7;", "(int)loop.lastMatchSim3.size() != B || !loop.matchAffineLight) return 7;\n"
     "  std::vector<float> light((size_t)B * 2);\n"
     "  for (int q = 0; q < B; q++) { light[(size_t)q * 2] = loop.lastMatchSim3[(size_t)q].gain; light[(size_t)q * 2 + 1] = loop.lastMatchSim3[(size_t)q].offset; }\n"
     "  if (!dump(dir + \"/light.bin\", light.data(), light.size() * 4)) return 11;"),
])


def test_absorb_matches_with_the_match_light_equals_the_bindings_lit_absorb(tmp_path, ellc):
    image = np.ascontiguousarray(make_sequence(1)[0], np.uint8)
    raw = tmp_path / "f.raw"
    raw.write_bytes(image.tobytes())
    exe = compile_program(tmp_path, "absorb_lit", ABSORB_LIT_PROGRAM)
    r = subprocess.run([str(exe), str(raw), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stdout.decode()
    B = int([l for l in r.stdout.decode().split("\n") if l.startswith("B ")][0].split()[1])
    want = dict(zip(STATS + ("reserved",), np.fromfile(tmp_path / "stats.bin", np.int32).tolist()))
    lines = [l.split() for l in (tmp_path / "absorb.txt").read_text().splitlines()]
    assert len(lines) == 3 and [int(x) for x in lines[2][2:]] == [want[k] for k in STATS] and int(lines[2][1]) == B >= 1
    assert identity_holds(want) and want["n_visited"] > 0
    lights = np.fromfile(tmp_path / "light.bin", np.float32).reshape(B, 2)
    T = np.fromfile(tmp_path / "T.bin", np.float32).reshape(B, 12)
    print("lights", lights)
    assert np.isfinite(lights).all() and (lights[:, 0] > 0.25).all() and (lights[:, 0] < 4).all()
    ctx = ellc.Context(ellc.default_config(W, H, LEVELS, max_keyframes=1 + B))
    try:
        for k in range(1 + B):
            ctx.keyframe_upload(k, image)
        for k in range(B):
            ctx.keyframe_set_depth(1 + k, np.fromfile(tmp_path / ("slot%d.depth" % k), np.float32).reshape(H, W),
                                   np.fromfile(tmp_path / ("slot%d.var" % k), np.float32).reshape(H, W))
        state = {name: np.fromfile(tmp_path / ("state." + name), dt).reshape(H, W) for name, dt in HYP}
        ctx.depth_set_keyframe(0)
        ctx.depth_set_state(state)
        got = ctx.depth_absorb(list(range(1, 1 + B)), T, params=dict(finalise=0), lights=lights, **FLT)
        # a condition of the test: the light reaches the gate - another light gives another fold of the same inputs
        ctx.depth_set_state(state)
        other = ctx.depth_absorb(list(range(1, 1 + B)), T, params=dict(finalise=0), lights=lights * np.float32([1.6, 1.0]) + np.float32([0, -20]), **FLT)
    finally:
        ctx.close()
    print("facade", want, "binding", got)
    assert got == want and other["n_candidates"] != got["n_candidates"]


# the restore program with restoreAffineLight from argv[5], the candidates' lights printed and the winner's written out
RESTORE_LIT_PROGRAM = patched(RESTORE_PROGRAM, [
    ("  if (argc < 5) return 1;", "  if (argc < 6) return 1;"),
    ("  globalOptimizeLoop.restoreConnection = std::atoi(argv[4]) != 0;\n",
     "  globalOptimizeLoop.restoreConnection = std::atoi(argv[4]) != 0;\n  globalOptimizeLoop.restoreAffineLight = std::atoi(argv[5]) != 0;\n"),
    ("  for (size_t q = 0; q < r.tried.size(); q++) std::printf(\"tried %d\\n\", r.tried[q]);\n",
     "  for (size_t q = 0; q < r.tried.size(); q++) std::printf(\"tried %d\\n\", r.tried[q]);\n"
     "  for (size_t q = 0; q < r.ids.size(); q++) std::printf(\"light %d %.9g %.9g\\n\", r.ids[q], r.lights[2 * q], r.lights[2 * q + 1]);\n"),
    ("!dump(dir + \"/test.img\", img.data(), n) ||", "!dump(dir + \"/test.img\", img.data(), n) || !dump(dir + \"/light.bin\", &r.lights[b_chosen * 2], 8) ||"),
])


def test_restore_affine_light_scores_fits_scores_again_and_restarts_at_the_light(tmp_path, ellc):
    n_tracked = 17
    frames = [np.ascontiguousarray(f, np.uint8) for f in make_sequence(n_tracked)]
    frames = frames + [AL.brighten(frames[2])]   # the test frame: a view near the first keyframe, after the exposure has swung
    raw = tmp_path / "frames.raw"
    raw.write_bytes(b"".join(f.tobytes() for f in frames))
    exe = compile_program(tmp_path, "restore_lit", RESTORE_LIT_PROGRAM)
    runs = {}
    for name, lit in (("unlit", "0"), ("lit", "1")):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([str(exe), str(raw), str(n_tracked), str(out), "1", lit], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        print(name, r.stdout.decode())
        assert r.returncode in (0, 5), r.stdout.decode()   # (5: the search chose nobody - possible for the unlit one)
        lines = [l.split() for l in r.stdout.decode().strip().split("\n")]
        runs[name] = dict(code=r.returncode, dir=out, cands={int(l[1]): int(l[5]) for l in lines if l[0] == "cand"},
                          lights={int(l[1]): (float(l[2]), float(l[3])) for l in lines if l[0] == "light"},
                          rec=[dict(zip(l[1::2], l[2::2])) for l in lines if l[0] == "restore"][0])
    unlit, lit = runs["unlit"], runs["lit"]
    assert all(v == (1.0, 0.0) for v in unlit["lights"].values()) and sorted(unlit["cands"]) == sorted(lit["cands"])
    assert lit["code"] == 0 and int(lit["rec"]["chosen"]) in lit["cands"]
    chosen = int(lit["rec"]["chosen"])
    # the winner is the best of the SECOND trial. (What the fitted light is worth is not asserted: the alignment in front of the trial is
    # blind to the exposure change, few pixels land in the interior at its poses, and the fit over them need not resemble (1.6, -20).)
    assert lit["cands"][chosen] == max(lit["cands"].values()) > 0
    assert all(0.25 <= g <= 4.0 and abs(o) <= 255.0 for g, o in lit["lights"].values()), lit["lights"]
    # the same steps through the binding: slot 0 the test frame's image, slot 1 the chosen candidate's planes
    on = lit["dir"]
    want = dict(zip(STATS + ("reserved",), np.fromfile(on / "stats.bin", np.int32).tolist()))
    T = np.fromfile(on / "T.bin", np.float32).reshape(1, 12)
    ctx = ellc.Context(ellc.default_config(W, H, LEVELS, max_keyframes=2))
    try:
        ctx.keyframe_upload(0, np.fromfile(on / "test.img", np.uint8).reshape(H, W))
        ctx.keyframe_upload(1, np.fromfile(on / "cand.img", np.uint8).reshape(H, W))
        ctx.keyframe_set_depth(1, np.fromfile(on / "cand.depth", np.float32).reshape(H, W), np.fromfile(on / "cand.var", np.float32).reshape(H, W))
        first = ctx.trial_propagate_lit([1], [0], T, None, dst_is_keyframe=True, **FLT)
        light, refused = ellc.trial_light_solve(first[0])
        second = ctx.trial_propagate_lit([1], [0], T, [light], dst_is_keyframe=True, **FLT)
        got, factor = ctx.depth_restart(0, [1], T, lights=[light], **FLT)
        state = ctx.depth_get_state()
    finally:
        ctx.close()
    assert not refused and light.tobytes() == np.fromfile(on / "light.bin", np.float32).tobytes(), (light, lit["lights"][chosen])
    assert int(first["n_targets"][0]) == unlit["cands"][chosen] and int(second["n_targets"][0]) == lit["cands"][chosen]
    assert got == want and want["n_created"] == want["targets_hit"] == lit["cands"][chosen]
    assert np.float32(factor) == np.float32(float(lit["rec"]["rescale"]))
    for name, dt in HYP:
        assert state[name].tobytes() == np.fromfile(on / ("state." + name), dt).tobytes(), name


def run_main(raw, n_frames, out, extra):
    exe = os.path.join(CSRC, "ellc_main")
    assert os.path.exists(exe), "ellc_main not built (run __graft_entry__.build())"
    out.mkdir()
    return subprocess.run([exe, str(raw), str(W), str(H), str(n_frames), str(out), "LC"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)


def test_ellc_main_flags(tmp_path):
    """The covered-camera sequence of tests/test_gpu_restore_connection.py, its revisit brightened: frames 23-25 are grey, frames 26..
    revisit the views of frames 9..14 through clip(rint(1.6 I - 20))."""
    steps = [np.ascontiguousarray(f, np.uint8) for f in make_sequence(22)]
    grey = np.full_like(steps[0], 128)
    frames = steps[:22] + [grey] * 3 + [AL.brighten(f) for f in steps[8:14]]
    n_frames = len(frames)
    raw = tmp_path / "frames.raw"
    raw.write_bytes(b"".join(f.tobytes() for f in frames))
    # --restore-light alone is a usage error: nothing runs
    r = run_main(raw, n_frames, tmp_path / "refused", ["--restore-light"])
    assert r.returncode != 0 and b"--restore-light needs --restore-connection" in r.stdout and not any((tmp_path / "refused").iterdir())
    # without the new flags: byte for byte what a second run writes, with and without the old flags the new ones extend
    old = ["--match-sim3", "SIM3", "--match-light", "--restore-connection", "RESTORE"]
    for a, b, flags in (("plain", "again", []), ("old", "old_again", old)):
        for name in (a, b):
            extra = [str(tmp_path / (name + "_" + f.lower() + ".txt")) if f in ("SIM3", "RESTORE") else f for f in flags]
            r = run_main(raw, n_frames, tmp_path / name, extra)
            assert r.returncode == 0, r.stdout.decode()
        for f in FILES:
            assert (tmp_path / a / f).read_bytes() == (tmp_path / b / f).read_bytes(), (a, f)
        for f in ("sim3", "restore"):
            if flags:
                assert (tmp_path / (a + "_" + f + ".txt")).read_bytes() == (tmp_path / (b + "_" + f + ".txt")).read_bytes(), f
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == sorted(FILES)
    unlit_log = [l.split() for l in (tmp_path / "old_restore.txt").read_text().splitlines()]
    assert unlit_log and all(len(l) == 6 for l in unlit_log)
    # the new flags: the absorb with the match light, the recovery with the fitted light
    new = ["--match-sim3", str(tmp_path / "new_sim3.txt"), "--match-light", "--absorb-matches", str(tmp_path / "new_absorb.txt"),
           "--restore-connection", str(tmp_path / "new_restore.txt"), "--restore-light"]
    for name in ("new", "new_again"):
        r = run_main(raw, n_frames, tmp_path / name, [x.replace("new_", name + "_") for x in new])
        assert r.returncode == 0, r.stdout.decode()
    for f in ("sim3", "absorb", "restore"):
        assert (tmp_path / ("new_%s.txt" % f)).read_bytes() == (tmp_path / ("new_again_%s.txt" % f)).read_bytes(), f
    absorb = [[int(x) for x in l.split()] for l in (tmp_path / "new_absorb.txt").read_text().splitlines()]
    assert absorb and all(len(v) == 2 + len(STATS) and identity_holds(dict(zip(STATS, v[2:]))) for v in absorb)
    log = [l.split() for l in (tmp_path / "new_restore.txt").read_text().splitlines()]
    print((tmp_path / "old_restore.txt").read_text(), (tmp_path / "new_restore.txt").read_text())
    assert log and all(len(l) == 8 for l in log)
    assert all(l[6:] == ["1", "0"] for l in log if int(l[2]) < 0)
    found = [l for l in log if int(l[2]) >= 0]
    assert found and int(found[0][0]) > 25 and int(found[0][3]) > 0 and float(found[0][4]) > 0
    assert 0.25 <= float(found[0][6]) <= 4.0 and abs(float(found[0][7])) <= 255.0   # a light ellc_trial_light_solve accepts, or (1, 0)
    poses = np.array([[float(x) for x in l.split()] for l in (tmp_path / "new" / "poses_orig.txt").read_text().splitlines()])
    assert (poses[:, 9] > 0).all()
