"""The Gauss-Newton side of the oracle against its SECOND SOURCE (tests/second_source_gn.py: a vectorised numpy / f32 restatement
written from PixelWisePyramid.cpp:58-498, 561-954, ImageFunc.cpp:150-292, Frame.cpp:298, 678-695 and UserDefinedFunc.cpp:34-50
directly, not from oracle/ellc_oracle_gn.cpp): the FCA planes (warped x / y with the -1 / -2 markers, residual, weight, J) at every
level at pose 0 (first warp branch) and at a general pose (second branch), H / b of the three row bands, the step and the pose; the
ICA's steepest descent, its b of two bands, H and H^-1; whole alignments with early exit on and off; the saved and finalised weights.
Scenes of 64 x 48, 160 x 120 and 640 x 480, with hand-set depths so that every branch class occurs (the histogram is asserted and
printed). CPU only; parity with the reference stays "partial" by rule — this lowers the risk of ONE reading shared by the oracle and
the kernels."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import second_source_depth as S1                                           # noqa: E402
import second_source_gn as S2                                              # noqa: E402
from egomotion_with_local_loop_closures_amd import synth                  # noqa: E402
from helpers import oracle_problem                                         # noqa: E402

PLANES = ("warpedX", "warpedY", "residual", "weight", "J")
POSE0 = np.zeros(6, np.float32)
# a general pose whose translation points backwards: the hand-set shallow depths land behind the camera
POSE_G = np.array([0.004, -0.003, 0.002, 0.006, -0.005, -0.02], np.float32)
# (w, h, levels, seed, max_iter)
SCENES = ((64, 48, 3, 31, (4, 7, 9)), (160, 120, 3, 32, (4, 7, 9)), (640, 480, 4, 33, (4, 7, 9, 12)))
HIST = S2.new_hist()                                                       # summed over the module, asserted at its end


def plant_rare_depths(oracle, kf, levels, seed):
    """per level: a few depths of 1e-12 (UNZERO clamps the transformed depth at pose 0), a few of 0.005 (behind the camera at
    POSE_G: the negative side of UNZERO) and a few pixels with their depth removed (mask 0)"""
    rng = np.random.default_rng(seed)
    for level in range(levels):
        d = kf.depth(level).copy()
        ys, xs = np.nonzero(d > 0)
        pick = rng.permutation(len(ys))[:12]
        d[ys[pick[:4]], xs[pick[:4]]] = 1e-12
        d[ys[pick[4:8]], xs[pick[4:8]]] = 0.005
        d[ys[pick[8:]], xs[pick[8:]]] = 0.0
        kf.set_depth(level, d)


def scene(oracle, w, h, L, seed, max_iter, rare, early_exit=1, **kw):
    pair = synth.make_pair(w, h, seed=seed, **kw)
    cfg, kf, cur, dm = oracle_problem(oracle, w, h, L, pair, early_exit=early_exit, max_iter=max_iter)
    if rare:
        plant_rare_depths(oracle, kf, L, seed)
    levels = [S2.Level.from_oracle(kf, cur, dm, pair["intrinsics"], l) for l in range(L)]
    return dict(pair=pair, cfg=cfg, kf=kf, cur=cur, dm=dm, levels=levels)


def planes_equal(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in PLANES)


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


# ---------------------------------------------------------------- the given pieces and the vector forms
def test_vector_taps_match_the_scalar_restatement(oracle):
    """tap() against second_source_depth.interp point by point (in bounds, on the last row / column, outside, NaN excluded), the
    -1 sentinel against the oracle's checked tap, and calculateGradient at every level against the oracle's gradient planes"""
    rng = np.random.default_rng(3)
    s = scene(oracle, 64, 48, 3, 31, (4, 7, 9), rare=False)
    for level, lv in enumerate(s["levels"]):
        xs = rng.uniform(-2.0, lv.cols + 1.0, 600).astype(np.float32)
        ys = rng.uniform(-2.0, lv.rows + 1.0, 600).astype(np.float32)
        xs[:40] = rng.integers(0, lv.cols, 40); ys[40:80] = lv.rows - 1 + rng.uniform(0, 1, 40)
        for plane in (lv.cur_img, lv.cur_gx, lv.cur_gy):
            got, _ = S2.tap(plane, xs, ys, lv.rows, lv.cols)
            src = plane[:lv.rows, :lv.cols] if plane.dtype == np.uint8 else plane
            ref = np.array([S1.interp(src, x, y) for x, y in zip(xs, ys)], np.float32)
            assert np.array_equal(got, ref), level
        chk = S2.tap_u8_checked(lv.cur_img, xs, ys, lv.rows, lv.cols)
        assert np.array_equal(chk, oracle.tap_u8(lv.cur_img, xs, ys, check=1, rows=lv.rows, cols=lv.cols)), level
        assert (chk == -1).sum() > 10
        s["cur"].update_level(level, False)
        gx, gy = s["cur"].gradient(level)
        assert np.array_equal(gx, lv.cur_gx) and np.array_equal(gy, lv.cur_gy), level
        assert np.array_equal(oracle.get_intrinsic(s["cfg"], level), np.array([lv.fx, lv.fy, lv.cx, lv.cy], np.float32))


def test_pow_promotions_agree_with_libm(oracle):
    """pow(v, 2) written as the double v * v: identical to libm's pow on every (-c + x) the scenes use. pow(depth, -1) written as
    1.0 / double(depth): glibc's pow is not correctly rounded and sits one double ulp away at a small fraction of the depths (counted
    and printed), so the check is where it matters — every float J term the promotion enters (J3, J4, J5 of the FCA at POSE_G and of
    the ICA precompute), on every pixel of every level of every scene, is the same bits with libm's pow as with the reciprocal."""
    n_z = n_ulp = n_terms = 0
    us = set()
    for (w, h, L, seed, mi) in SCENES:
        s = scene(oracle, w, h, L, seed, mi, rare=True)
        for lv in s["levels"]:
            us.update(np.unique(lv.u).tolist()); us.update(np.unique(lv.v).tolist())
            p_libm = S2.libm_pow_array(lv.z, -1.0)
            n_z += lv.z.size
            n_ulp += int((p_libm != S2.inv_pow(lv.z)).sum())
            t = S2.fca_level_step_terms(lv, POSE_G, oracle.se3_exp)
            for gx, gy in ((t["gradx"], t["grady"]), (lv.kf_gx[lv.ys, lv.xs], lv.kf_gy[lv.ys, lv.xs])):
                a = S2.jacobian(gx, gy, lv.u, lv.v, lv.z, lv.fx, lv.fy)
                b = S2.jacobian(gx, gy, lv.u, lv.v, lv.z, lv.fx, lv.fy, p=p_libm)
                assert np.array_equal(a, b, equal_nan=True), (w, h, lv.level)
                n_terms += 3 * lv.z.size
    assert n_z > 100000
    us = np.array(sorted(us), np.float32).astype(np.float64)
    assert np.array_equal(us * us, S2.libm_pow_array(us, 2.0))
    print("pow(z, -1): libm != 1/z in double at %d of %d depths; float J terms identical: %d" % (n_ulp, n_z, n_terms))


# ---------------------------------------------------------------- FCA: one step
@pytest.mark.parametrize("w,h,L,seed,mi", SCENES)
def test_fca_planes_sums_and_step_bit_exact(oracle, w, h, L, seed, mi):
    """every level, pose 0 (SE3_vec[1] == 0: the first warp branch) and POSE_G (the second): planes ==, the banded f32 H / b ==,
    the f64 sums within 1e-12 of the oracle's Hd / bd, H^-1, delta, weightedPose and the new pose =="""
    s = scene(oracle, w, h, L, seed, mi, rare=True)
    giv = S2.Givens(oracle)
    for pose, branch1 in ((POSE0, True), (POSE_G, False)):
        for level in range(L):
            st = oracle.GNStepper(s["kf"], s["cur"], s["dm"].depth_pyr(), level, pose, sum_mode=0, planes=True)
            ref = st.step(0)
            pl = st.get_planes()
            st.close()
            got = S2.fca_step(s["levels"][level], pose, giv)
            S2.add_hist(HIST, got["hist"])
            assert got["terms"]["branch1"] == branch1
            tag = (w, h, level, branch1)
            for k in PLANES:
                assert np.array_equal(got["planes"][k], pl[k], equal_nan=True), (tag, k)
            assert np.array_equal(got["H"], ref["H"]) and np.array_equal(got["b"], ref["b"]), tag
            assert rel(got["Hd"], ref["Hd"]) <= 1e-12 and rel(got["bd"], ref["bd"]) <= 1e-12, (tag, rel(got["Hd"], ref["Hd"]))
            assert np.array_equal(got["Hinv"], ref["Hinv"]) and np.array_equal(got["delta"], ref["delta"]), tag
            assert got["weighted"] == np.float32(ref["weighted"]), tag
            assert np.array_equal(got["pose"], ref["pose"]), tag


# ---------------------------------------------------------------- ICA: precompute and one iterate
# The ICA Hessian is cv::gemm(weightedSteepestDescent, steepestDescent^T) over N pixels; its summation order over N is OpenCV's and
# not on this machine. The oracle's choice is a float64 sum rounded once to float (the second source does the same and the two agree
# bit for bit on these scenes); the stated tolerance is what any order of a double sum rounded once to float can move: 2 ulp of the
# largest entry for H, and its image through the inverse for H^-1 (scaled by sqrt(diag H), as tests/test_gpu_schedule_sums.py does).
ICA_H_TOL = 2.0 ** -22
ICA_HINV_TOL = 1e-5


@pytest.mark.parametrize("w,h,L,seed,mi", SCENES[:2])
def test_ica_sd_b_exact_and_h_at_tolerance(oracle, w, h, L, seed, mi):
    s = scene(oracle, w, h, L, seed, mi, rare=False)
    rng = np.random.default_rng(seed)
    pose = POSE_G * np.float32(0.5)
    for level in range(L):
        lv = s["levels"][level]
        wts = rng.uniform(0.0, 0.0625, size=(lv.rows, lv.cols)).astype(np.float32)
        s["kf"].set_weights(level, wts, 1)
        st = oracle.GNStepper(s["kf"], s["cur"], s["dm"].depth_pyr(), level, pose, planes=True)
        ref = st.step(1, 0)
        sd, wsd = st.get_sd()
        st.close()
        sd2, wsd2, H2, Hd2 = S2.ica_precompute(lv, wts)
        b2, bd2, hist = S2.ica_iterate(lv, pose, sd2, wts, oracle.se3_exp)
        S2.add_hist(HIST, hist)
        assert np.array_equal(sd, sd2) and np.array_equal(wsd, wsd2), level
        assert np.array_equal(ref["b"], b2), level
        assert rel(bd2, ref["bd"]) <= 1e-12, level
        assert np.abs(ref["H"] - H2).max() <= ICA_H_TOL * np.abs(H2).max(), level
        _, Hinv2 = oracle.lu_inverse(H2)
        dsc = np.sqrt(np.diag(Hd2))
        scale = dsc[:, None] * dsc[None, :]
        assert np.abs((ref["Hinv"] - Hinv2) * scale).max() <= ICA_HINV_TOL * np.abs(Hinv2 * scale).max(), level
        print("ICA l%d: H %s, H^-1 %s" % (level, "==" if np.array_equal(ref["H"], H2) else "within tolerance",
                                          "==" if np.array_equal(ref["Hinv"], Hinv2) else "within tolerance"))


# ---------------------------------------------------------------- whole alignments, saved and finalised weights
def _align_both(oracle, s, mi, early_exit, ica=False, kw=None, save=False, cur=None, levels=None):
    giv = S2.Givens(oracle)
    s["kf"].set_early_exit(early_exit)
    got = S2.align(levels or s["levels"], giv, mi, early_exit=bool(early_exit), ica=ica, kf_weights=kw, save_weights=save)
    pose, iters, wgt = oracle.align(s["kf"], cur or s["cur"], s["dm"].depth_pyr(), loop_closure=ica, save_weights=save)
    assert np.array_equal(got["iters"], iters), (got["iters"], iters)
    assert np.array_equal(got["pose"], pose), (got["pose"], pose)
    assert got["weighted"] == np.float32(wgt)
    S2.add_hist(HIST, got["hist"])
    return got


def test_align_early_exit_on_and_off_fca_ica_and_weights(oracle):
    """160 x 120, 3 levels, max_iter (2, 7, 9) coarsest last: with early exit the coarsest level runs out of iterations and the
    finer ones exit early. Three frames on one keyframe with saved weights (FCA), counts and planes ==, including the early-exited
    levels; finaliseWeights == (n = 3: the scale by 1/n); then ICA on the finalised weights, early exit on and off."""
    w, h, L, mi = 160, 120, 3, (4, 7, 2)
    s = scene(oracle, w, h, L, 40, mi, rare=False, rot=0.01, trans=0.03)
    cfg = s["cfg"]
    kw = S2.KeyframeWeights(s["levels"])
    exits = []
    for k, seed in enumerate((40, 41, 42)):
        if k == 0:
            cur, levels = s["cur"], s["levels"]
        else:
            other = synth.make_pair(w, h, seed=seed, rot=0.006, trans=0.01)
            cur = oracle.Frame(cfg, other["cur_image"], 10 + k)
            levels = [S2.Level.from_oracle(s["kf"], cur, s["dm"], s["pair"]["intrinsics"], l) for l in range(L)]
        got = _align_both(oracle, s, mi, 1, save=True, cur=cur, levels=levels)
        exits.append(got["iters"] < np.array(mi))
        kw.add(got["saved"])
        for level in range(L):
            ow, n = s["kf"].weights(level)
            assert n == kw.n[level] == k + 1 and np.array_equal(ow, kw.w[level]), (k, level)
    exits = np.array(exits)
    assert exits.any() and (~exits).any(), exits                           # early exits and max_iter both occurred
    assert not exits[0][L - 1] and exits[0][:L - 1].any(), exits[0]        # frame 0: max_iter at the coarsest, early exit finer
    s["kf"].finalise_weights()
    kw.finalise()
    for level in range(L):
        assert np.array_equal(s["kf"].weights(level)[0], kw.w[level]), level
    for ee in (1, 0):
        _align_both(oracle, s, mi, ee, ica=True, kw=kw.w)
    # FCA without early exit (the project's option)
    got = _align_both(oracle, s, mi, 0)
    assert list(got["iters"]) == list(mi)


def test_align_640x480_fca(oracle):
    w, h, L, seed, mi = SCENES[2]
    s = scene(oracle, w, h, L, seed, mi, rare=False)
    _align_both(oracle, s, mi, 1)


def test_zz_every_branch_class_occurred():
    """runs last in this module: the histogram over every call above"""
    print("second-source GN branch histogram:", HIST)
    assert all(HIST[k] > 0 for k in S2.BRANCHES), HIST
