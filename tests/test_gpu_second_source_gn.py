"""The Gauss-Newton kernels against the SECOND SOURCE directly (tests/second_source_gn.py, written from the reference's text, not
from the oracle): H, b and the step of one launch of every kernel the schedules run (ellc_debug_schedule_sums, diagnostic library)
against the second source's float64 sums of its own per-pixel terms, at the single-step gates of tests/test_gpu_schedule_sums.py, with
the kernel's name asserted in every case; whole alignments with early exit (resident launch, one launch per iteration, a level-bound
batch): iteration counts per level ==, pose <= 1e-5; the saved and finalised weights of two frames on one keyframe: the same zero /
non-zero pixels, including at early-exited levels (only warped points within 1e-3 px of the tap's bounds are exempt, and counted)."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import second_source_gn as S2                                              # noqa: E402
from egomotion_with_local_loop_closures_amd import synth                  # noqa: E402
from helpers import oracle_problem, gpu_problem                            # noqa: E402
from test_gpu_schedule_sums import GATES, HINV_GATE, check_step, report, _scene_pose, _arith   # noqa: E402

pytestmark = pytest.mark.gpu

POSE_GATE_ALIGN = 1e-5
NEAR_BOUNDS = 1e-3


def levels_of(oracle, W, H, L, pair, max_iter=(4, 7, 9, 12), early_exit=0):
    """the second source's level inputs (images, depth and variance pyramids given by the oracle's Frame / DepthMap)"""
    cfg, kf, cur, dm = oracle_problem(oracle, W, H, L, pair, early_exit=early_exit, max_iter=max_iter)
    return [S2.Level.from_oracle(kf, cur, dm, pair["intrinsics"], l) for l in range(L)], (cfg, kf, cur, dm)


def fca_ref(oracle, lv, pose):
    """float64 sums of the second source's per-pixel terms and the float64 step from them"""
    t = S2.fca_level_step_terms(lv, pose, oracle.se3_exp)
    _, _, Hd, bd = S2.fca_sums(lv, t, f32=False)
    _, new_pose = S2.step_f64(Hd, bd, pose, oracle.concat_relative)
    return dict(Hd=Hd, bd=bd, pose=new_pose)


def run_fca_case(oracle, ellc, W, H, L, pairs, B, levels, arith, kernel, max_iter=(4, 7, 9, 12)):
    lvs = [levels_of(oracle, W, H, L, p, max_iter)[0] for p in pairs]
    n = len(pairs)
    ctx = gpu_problem(ellc, W, H, L, [pairs[b % n] for b in range(B)], max_iter=max_iter, diag=True, arith=_arith(ellc, arith))
    slots = np.arange(B, dtype=np.int32)
    poses = np.stack([_scene_pose(b % n) for b in range(B)])
    worst = {}
    for level in levels:
        got = ctx.debug_schedule_sums(slots, slots, level, poses)
        assert got["kernel"] == kernel, (level, got["kernel"])
        refs = [fca_ref(oracle, lvs[s][level], _scene_pose(s)) for s in range(n)]
        for b in range(B):
            check_step(got["H"][b], got["b"][b], got["pose"][b], refs[b % n], arith, worst,
                       "2nd source %s %s l%d" % (got["kernel"], arith, level))
    ctx.close()
    report(worst)


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_fca_fused_640x480_b32(oracle, ellc, arith):
    W, H, L = 640, 480, 4
    pairs = [synth.make_pair(W, H, seed=900 + i) for i in range(4)]
    kernel = "gn_fca_fused<fast,pipe>" if arith == "fast" else "gn_fca_fused<exact,pipe,divc>"
    run_fca_case(oracle, ellc, W, H, L, pairs, 32, (3, 0), arith, kernel)


@pytest.mark.parametrize("arith,kernel", [("fast", "gn_fca_dense4"), ("exact", "gn_fca_dense_x<divc>")])
def test_fca_dense_1280x960(oracle, ellc, arith, kernel):
    W, H, L = 1280, 960, 5
    mi = (4, 7, 9, 12, 12)
    pairs = [synth.make_pair(W, H, seed=770 + i, dense=True) for i in range(2)]
    run_fca_case(oracle, ellc, W, H, L, pairs, 16, (4, 0), arith, kernel, max_iter=mi)


def test_fca_dense_width_not_a_multiple_of_four(oracle, ellc):
    W, H, L = 642, 480, 4
    pairs = [synth.make_pair(W, H, seed=78, dense=True)]
    run_fca_case(oracle, ellc, W, H, L, pairs, 2, (1, 0), "fast", "gn_fca_dense")


@pytest.mark.parametrize("arith", ["exact", "fast"])
@pytest.mark.parametrize("B", [1, 32])
def test_ica_fused(oracle, ellc, arith, B):
    """gn_ica_fused: b and the step against the second source's float64 b and float64 solve of its float64 H; the kernel's kept H^-1
    against the inverse of that H (scaled by sqrt(diag H))"""
    W, H, L = 640, 480, 4
    n = min(B, 4)
    pairs = [synth.make_pair(W, H, seed=900 + i) for i in range(n)]
    lvs = [levels_of(oracle, W, H, L, p)[0] for p in pairs]
    ctx = gpu_problem(ellc, W, H, L, [pairs[b % n] for b in range(B)], diag=True, arith=_arith(ellc, arith))
    wts = []
    for s in range(n):
        rng = np.random.default_rng(40 + s)
        wts.append([rng.uniform(0.01, 0.0625, size=(H >> l, W >> l)).astype(np.float32) for l in range(L)])
    for b in range(B):
        for l in range(L):
            ctx.keyframe_set_weights(b, l, wts[b % n][l], 1)
    slots = np.arange(B, dtype=np.int32)
    poses = np.stack([_scene_pose(b % n) for b in range(B)])
    worst = {}
    for level in range(L - 1, -1, -1):
        got = ctx.debug_schedule_sums(slots, slots, level, poses, mode=ellc.MODE_ICA)
        assert got["kernel"] == "gn_ica_fused<%s>" % arith, got["kernel"]
        refs = []
        for s in range(n):
            lv = lvs[s][level]
            sd, _, _, Hd = S2.ica_precompute(lv, wts[s][level])
            _, bd, _ = S2.ica_iterate(lv, _scene_pose(s), sd, wts[s][level], oracle.se3_exp)
            _, pose = S2.step_f64(Hd, bd, _scene_pose(s), oracle.concat_relative)
            refs.append(dict(Hd=Hd, bd=bd, pose=pose))
        for b in range(B):
            ref = refs[b % n]
            tag = "2nd source %s B=%d l%d" % (got["kernel"], B, level)
            check_step(None, got["b"][b], got["pose"][b], ref, arith, worst, tag, H_too=False)
            d = np.sqrt(np.diag(ref["Hd"]))
            g_s = got["hinv"][b] * d[:, None] * d[None, :]
            r_s = np.linalg.inv(ref["Hd"]) * d[:, None] * d[None, :]
            err = float(np.abs(g_s - r_s).max() / np.abs(r_s).max())
            prev = worst.get(tag + " hinv", [0.0] * 5)
            worst[tag + " hinv"] = [0.0, max(prev[1], err), 0.0, max(prev[3], err / HINV_GATE[arith]), 0.0]
            assert err < HINV_GATE[arith], (tag, err)
    report(worst)
    ctx.close()


# ---- whole alignments, early exit on ----------------------------------------------------------------------------------------------
CASES = [(21, 0.02, 0.05), (22, 0.03, 0.08), (23, 0.01, 0.03), (24, 0.02, 0.04)]


def _second_source_align(oracle, W, H, L, pair, save=False, cur_image=None):
    lvs, (cfg, kf, cur, dm) = levels_of(oracle, W, H, L, pair, early_exit=1)
    if cur_image is not None:
        cur = oracle.Frame(cfg, cur_image, 5)
        lvs = [S2.Level.from_oracle(kf, cur, dm, pair["intrinsics"], l) for l in range(L)]
    return S2.align(lvs, S2.Givens(oracle), (4, 7, 9, 12), early_exit=True, save_weights=save), lvs


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_align_early_exit_resident_launches_and_batch(oracle, ellc, arith):
    """B = 1 through the resident launch and through one launch per iteration (set_persistent_schedule(0)); then a batch of four
    (the level-bound schedule): per-level iteration counts == the second source's, pose <= 1e-5"""
    W, H, L = 640, 480, 4
    pairs = [synth.make_pair(W, H, seed=s, rot=r, trans=t) for s, r, t in CASES]
    refs = [_second_source_align(oracle, W, H, L, p)[0] for p in pairs]
    assert any((r["iters"] < np.array([4, 7, 9, 12])).any() for r in refs)
    kw = dict(arith=ellc.ARITH_FAST) if arith == "fast" else {}
    for schedule in ("resident", "launches"):
        ctx = gpu_problem(ellc, W, H, L, pairs[:1], early_exit=1, diag=True, **kw)
        if schedule == "launches":
            ctx.set_persistent_schedule(0)
        pose, iters, _ = ctx.align([0], [0])
        ctx.close()
        err = float(np.abs(pose[0] - refs[0]["pose"]).max())
        print("%s B=1 %s: iters %s (2nd source %s), pose err %.2e" % (arith, schedule, list(iters[0]), list(refs[0]["iters"]), err))
        assert list(iters[0]) == list(refs[0]["iters"]), schedule
        assert err <= POSE_GATE_ALIGN, (schedule, err)
    ctx = gpu_problem(ellc, W, H, L, pairs, early_exit=1, **kw)
    idx = np.arange(len(pairs))
    pose, iters, _ = ctx.align(idx, idx)
    ctx.close()
    for i, r in enumerate(refs):
        err = float(np.abs(pose[i] - r["pose"]).max())
        print("%s B=4 alignment %d: iters %s, pose err %.2e" % (arith, i, list(iters[i]), err))
        assert list(iters[i]) == list(r["iters"]), i
        assert err <= POSE_GATE_ALIGN, (i, err)


def _near_bounds(planes, rows, cols):
    x, y = planes["rawX"], planes["rawY"]
    near = np.zeros(x.shape, bool)
    for v, bounds in ((x, (0.0, cols - 1.0, float(cols))), (y, (0.0, rows - 1.0, float(rows)))):
        for b in bounds:
            near |= np.abs(v.astype(np.float64) - b) < NEAR_BOUNDS
    return near


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_saved_and_finalised_weights_two_frames(oracle, ellc, arith):
    """two frames on one keyframe, align(save_weights=True) each, keyframe_finalise_weights: the same zero / non-zero pixels as the
    second source at every level (also where an alignment exited early); values at the saved-weights gate of tests/test_gpu_gn.py
    (exact mode)"""
    W, H, L = 640, 480, 4
    kf_pair = synth.make_pair(W, H, seed=21, rot=0.02, trans=0.05)
    other = synth.make_pair(W, H, seed=21, rot=0.03, trans=0.08)                  # same seed: same texture and depth
    assert np.array_equal(other["kf_image"], kf_pair["kf_image"]) and np.array_equal(other["depth0"], kf_pair["depth0"])
    r0, lvs = _second_source_align(oracle, W, H, L, kf_pair, save=True)
    r1, _ = _second_source_align(oracle, W, H, L, kf_pair, save=True, cur_image=other["cur_image"])
    early = [(r["iters"] < np.array([4, 7, 9, 12])) for r in (r0, r1)]
    assert any(e.any() for e in early), early
    kw_ref = S2.KeyframeWeights(lvs)
    kw_ref.add(r0["saved"]); kw_ref.add(r1["saved"])
    kw_ref.finalise()
    kw = dict(arith=ellc.ARITH_FAST) if arith == "fast" else {}
    ctx = gpu_problem(ellc, W, H, L, [kf_pair, other], early_exit=1, **kw)
    _, it0, _ = ctx.align([0], [0], save_weights=True)
    _, it1, _ = ctx.align([0], [1], save_weights=True)
    assert list(it0[0]) == list(r0["iters"]) and list(it1[0]) == list(r1["iters"]), (it0, it1, r0["iters"], r1["iters"])
    ctx.keyframe_finalise_weights(0)
    exempt_total = 0
    for l in range(L):
        wg, ng = ctx.keyframe_weights(0, l)
        wr = kw_ref.w[l]
        assert ng == kw_ref.n[l] == 2, (l, ng)
        lv = lvs[l]
        exempt = _near_bounds(r0["saved_planes"][l], lv.rows, lv.cols) | _near_bounds(r1["saved_planes"][l], lv.rows, lv.cols)
        differ = (wg == 0) != (wr == 0)
        exempt_total += int((differ & exempt).sum())
        assert not (differ & ~exempt).any(), (l, int((differ & ~exempt).sum()))
        keep = ~exempt
        relmax = float(np.abs(wg[keep] - wr[keep]).max() / np.abs(wr[keep]).max())
        print("%s l%d: early exit %s / %s, zero sets equal, exempt pixels that differ %d, max |diff| / max %.2e"
              % (arith, l, bool(early[0][l]), bool(early[1][l]), int((differ & exempt).sum()), relmax))
        if arith == "exact":
            assert np.allclose(wg[keep], wr[keep], rtol=1e-3, atol=5e-6), (l, np.abs(wg[keep] - wr[keep]).max())
    print("%s: pixels exempt (warped point within %g px of the tap's bounds) that differed: %d" % (arith, NEAR_BOUNDS, exempt_total))
    ctx.close()
