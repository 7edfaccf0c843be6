"""The depth map's stencil, rescale and export kernels against the SECOND SOURCE directly (tests/second_source_depth.py, DepthMapStages:
written from DepthPropagation.cpp:1254-1830, not from the oracle): fill, regularise (both modes), the one-launch doRegularization and
regularise + fill + regularise, the export with every level, the rescale given the GPU's own factor, the seeds percentage and the depth
tail of a tracked frame, bit for bit. Each test id names the kernel path its size selects (csrc/ellc_depth_impl.hpp)."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_second_source_depth import (stencil_scene, stages_of, oracle_map, assert_states_equal, same_bits, require,   # noqa: E402
                                      check_fill_classes, REG_CLASSES, REG_CLASSES_OCCL)

pytestmark = pytest.mark.gpu

# The stencil kernels (dm_fill_holes, dm_regularize, dm_fill_reg<false>, dm_reg_fill_reg) work in 32 x 8 tiles with a ring; 202 x 150
# leaves partial tiles on both axes, 480 x 270 on one
STENCIL_SIZES = [(640, 480), (480, 270), (202, 150)]
# the export (ellc_depth_impl.hpp, export_pyramid_steps): dm_export_pyramid produces min(3, L - 1) levels when W and H are multiples
# of 32 (the levels it covers halve exactly); otherwise dm_export_level0 writes level 0 and depth_pyr_level every further level, as it
# does for level 4 of a five-level pyramid (build_depth_pyramid_from(steps + 1))
EXPORT_CASES = [((640, 480, 4), "dm_export_pyramid<false>"),
                ((480, 270, 4), "dm_export_level0+depth_pyr_level"),
                ((202, 150, 4), "dm_export_level0+depth_pyr_level(odd source width)"),
                ((640, 480, 5), "dm_export_pyramid<false>+depth_pyr_level")]
# the rescale inside createKeyFrame (rescale_in_export): merged into dm_export_pyramid<true> from dm_reg_fill_reg's per-tile sums when
# the export is tiled and there are at most DM_MAX_SUM_PARTS = 4 096 tiles of 32 x 8; otherwise dm_sum_stage1 + dm_rescale, then the
# export. 2048 x 1056 has 8 448 tiles and a tiled export; 480 x 270 has none.
RESCALE_CASES = [((640, 480), "dm_export_pyramid<true>(merged)"),
                 ((480, 270), "dm_sum_stage1+dm_rescale+dm_export_level0"),
                 ((2048, 1056), "dm_sum_stage1+dm_rescale+dm_export_pyramid<false>")]
# ellc_depth_make_inv_depth_one is always dm_sum_stage1 + dm_rescale (do_rescale); the export after it is the size's
MAKE_INV_CASES = [((640, 480), "dm_sum_stage1+dm_rescale+dm_export_pyramid<false>"),
                  ((480, 270), "dm_sum_stage1+dm_rescale+dm_export_level0"),
                  ((2048, 1056), "dm_sum_stage1+dm_rescale+dm_export_pyramid<false>")]
# the tracked frame's depth tail (do_fill_regularize_and_update_depth_image): one launch dm_fill_reg<true> with the export fused when
# W is a multiple of 32 and H of 8; otherwise dm_fill_reg<false> and the export on its own
TAIL_CASES = [((320, 240), "dm_fill_reg<true>(fused export)"), ((200, 150), "dm_fill_reg<false>+dm_export_level0")]

case_id = lambda c: "%dx%d-%s" % (c[0][0], c[0][1], c[1]) if len(c[0]) == 2 else "%dx%d_L%d-%s" % (c[0] + (c[1],))


def make_ctx(ellc, pair, W, H, L):
    fx, fy, cx, cy = pair["intrinsics"]
    ctx = ellc.Context(ellc.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, early_exit=1, max_keyframes=2, max_frames=1))
    ctx.keyframe_upload(0, pair["kf_image"])
    ctx.frame_upload(0, pair["cur_image"])
    ctx.keyframe_from_frame(1, 0)
    return ctx


def with_state(ctx, st, slot=0):
    ctx.depth_set_keyframe(slot)
    ctx.depth_set_state(st)
    return ctx


def assert_gpu_export(ctx, slot, s2, L, what):
    """level 0: the Mat (0 where invalid) and the variance array (-1); every further level: the arrays"""
    for l in range(L):
        d, v = ctx.keyframe_depth_level(slot, l)
        assert same_bits(d, s2.depth_mat[l]), "%s: depth level %d (%d pixels differ)" % (what, l, int((d != s2.depth_mat[l]).sum()))
        assert same_bits(v, s2.depthvararr[l]), "%s: variance level %d" % (what, l)


def ulp_distance(a, b):
    a = np.array([a], np.float32).view(np.int32)[0]; b = np.array([b], np.float32).view(np.int32)[0]
    return abs(int(a) - int(b))


@pytest.fixture(scope="module", params=STENCIL_SIZES, ids=lambda s: "%dx%d" % s)
def stencil(request, oracle, ellc):
    W, H = request.param
    L = 4
    cfg, pair, kf, st = stencil_scene(oracle, W, H, L, 800 + W, zero_var=False)
    _, _, _, st0 = stencil_scene(oracle, W, H, L, 800 + W, zero_var=True)
    ctx = make_ctx(ellc, pair, W, H, L)
    yield dict(W=W, H=H, L=L, cfg=cfg, pair=pair, kf=kf, st=st, st_zero_var=st0, ctx=ctx)
    ctx.close()


def test_dm_fill_holes(stencil):
    for key in ("st", "st_zero_var"):
        st = stencil[key]
        s2 = stages_of(stencil["cfg"], stencil["pair"], stencil["kf"], st, stencil["L"])
        s2.fill_depth_holes()
        with_state(stencil["ctx"], st).depth_fill_holes()
        what = "dm_fill_holes %dx%d %s" % (stencil["W"], stencil["H"], key)
        assert_states_equal(stencil["ctx"].depth_get_state(), s2.st, what)
        check_fill_classes(s2.fill_classes, what)


@pytest.mark.parametrize("remove_occlusions", [False, True])
def test_dm_regularize(stencil, remove_occlusions):
    for key in ("st", "st_zero_var"):
        st = stencil[key]
        s2 = stages_of(stencil["cfg"], stencil["pair"], stencil["kf"], st, stencil["L"])
        s2.regularize_depth_map(remove_occlusions)
        with_state(stencil["ctx"], st).depth_regularize(remove_occlusions)
        what = "dm_regularize(%s) %dx%d %s" % (remove_occlusions, stencil["W"], stencil["H"], key)
        assert_states_equal(stencil["ctx"].depth_get_state(), s2.st, what)
        print("%s: %r" % (what, s2.reg_classes))
        require(s2.reg_classes, REG_CLASSES_OCCL if remove_occlusions else REG_CLASSES, what)
        if key == "st_zero_var":
            assert s2.reg_classes["nan_or_inf"] > 0


@pytest.mark.parametrize("remove_occlusions", [False, True])
def test_dm_fill_reg_false_do_regularization(stencil, remove_occlusions):
    s2 = stages_of(stencil["cfg"], stencil["pair"], stencil["kf"], stencil["st"], stencil["L"])
    s2.do_regularization(remove_occlusions)
    with_state(stencil["ctx"], stencil["st"]).depth_do_regularization(remove_occlusions)
    what = "dm_fill_reg<false>(%s) %dx%d" % (remove_occlusions, stencil["W"], stencil["H"])
    assert_states_equal(stencil["ctx"].depth_get_state(), s2.st, what)
    check_fill_classes(s2.fill_classes, what)
    require(s2.reg_classes, REG_CLASSES_OCCL if remove_occlusions else REG_CLASSES, what)


@pytest.mark.parametrize("remove_occlusions", [False, True])
def test_dm_reg_fill_reg(stencil, remove_occlusions):
    s2 = stages_of(stencil["cfg"], stencil["pair"], stencil["kf"], stencil["st"], stencil["L"])
    s2.regularize_depth_map(remove_occlusions)
    first = s2.reg_classes
    s2.do_regularization(False)
    with_state(stencil["ctx"], stencil["st"]).depth_regularize_fill_regularize(remove_occlusions)
    what = "dm_reg_fill_reg(%s) %dx%d" % (remove_occlusions, stencil["W"], stencil["H"])
    assert_states_equal(stencil["ctx"].depth_get_state(), s2.st, what)
    require(first, REG_CLASSES_OCCL if remove_occlusions else REG_CLASSES, what)
    require(s2.fill_classes, ("create", "reject_val_le_30", "negative_val", "fill_rows_3_5"), what)


@pytest.mark.parametrize("case", EXPORT_CASES, ids=case_id)
def test_update_depth_image_and_seeds(oracle, ellc, case):
    (W, H, L), _ = case
    cfg, pair, kf, st = stencil_scene(oracle, W, H, L, 900 + W)
    ctx = with_state(make_ctx(ellc, pair, W, H, L), st)
    s2 = stages_of(cfg, pair, kf, st, L)
    s2.update_depth_image()
    ctx.depth_update_depth_image()
    what = "updateDepthImage %dx%d L%d" % (W, H, L)
    assert_states_equal(ctx.depth_get_state(), s2.st, what)
    assert_gpu_export(ctx, 0, s2, L, what)
    assert ctx.depth_seeds() == s2.calculate_no_of_seeds()
    c = s2.export_classes
    print("%s: %r" % (what, c))
    require(c, ("band_cleared", "exported", "ids_small_negative", "ids_below", "ids_minus_one"), what)
    assert all((n > 0).all() for l, n in c["children"].items() if (W >> l) >= 16), c["children"]
    if W == 202:
        assert c["odd_source_width"] == [2]
    ctx.close()


def check_factor(f_gpu, s2, what):
    """the GPU's factor is f32(count) / f32(the f64 sum of invDepthSmoothed over the valid pixels) — within one f32 ulp
    (the f64 sum's order is the GPU's own) — and within 5e-5 of the reference's serial f32 sum's factor"""
    d = ulp_distance(f_gpu, s2.factor_f64_sum)
    rel = abs(float(f_gpu) / float(s2.factor_serial) - 1)
    print("%s: GPU factor %r, f32(count)/f32(f64 sum) %r (%d ulp), serial f32 %r (%.2e), %r" % (
        what, f_gpu, s2.factor_f64_sum, d, s2.factor_serial, rel, s2.rescale_classes))
    assert d <= 1, (what, f_gpu, s2.factor_f64_sum)
    assert rel < 5e-5, (what, rel)
    require(s2.rescale_classes, ("valid", "valid_in_band"), what)


@pytest.mark.parametrize("case", MAKE_INV_CASES, ids=case_id)
def test_make_inv_depth_one_given_the_gpu_factor(oracle, ellc, case):
    """ellc_depth_make_inv_depth_one (dm_sum_stage1 + dm_rescale) then ellc_depth_update_depth_image"""
    (W, H), _ = case
    L = 4
    cfg, pair, kf, st = stencil_scene(oracle, W, H, L, 1000 + W, plant_export=False)
    ctx = with_state(make_ctx(ellc, pair, W, H, L), st)
    f_gpu = ctx.depth_make_inv_depth_one()
    ctx.depth_update_depth_image()
    s2 = stages_of(cfg, pair, kf, st, L)
    s2.make_inv_depth_one(factor=f_gpu)
    s2.update_depth_image()
    what = "makeInvDepthOne %dx%d" % (W, H)
    check_factor(f_gpu, s2, what)
    assert_states_equal(ctx.depth_get_state(), s2.st, what + " (given the GPU's factor)")
    assert_gpu_export(ctx, 0, s2, L, what)
    ctx.close()


@pytest.mark.parametrize("case", RESCALE_CASES, ids=case_id)
def test_create_keyframe_given_the_gpu_factor(oracle, ellc, case):
    """ellc_depth_create_keyframe: propagate, regularise + fill + regularise, rescale, export. At 2048 x 1056 the second source starts
    from the C++ oracle's propagated map (its scalar propagate is held to the oracle by tests/test_second_source_depth.py)."""
    (W, H), path = case
    L = 4
    cfg, pair, kf, st = stencil_scene(oracle, W, H, L, 1100 + W, plant_export=False)
    ctx = with_state(make_ctx(ellc, pair, W, H, L), st)
    f_gpu = ctx.depth_create_keyframe(1, pair["xi_true"])
    cur = oracle.Frame(cfg, pair["cur_image"], 2)
    cur.set_pose(origin=pair["xi_true"])
    mats = cur.calc_se3(kf)
    mg_new, _ = cur.max_gradient()
    s2 = stages_of(cfg, pair, kf, st, L)
    if W * H > 1 << 20:
        dm = oracle_map(oracle, cfg, kf, st)
        dm.propagate(cur)
        s2.st = dm.get_state()
        s2.switch_keyframe(pair["cur_image"], mg_new)
        s2.new_keyframe_stages(factor=f_gpu)
    else:
        s2.create_keyframe(pair["cur_image"], mg_new, mats, factor=f_gpu)
    what = "createKeyFrame %dx%d %s" % (W, H, path)
    check_factor(f_gpu, s2, what)
    assert_states_equal(ctx.depth_get_state(), s2.st, what + " (given the GPU's factor)")
    assert_gpu_export(ctx, 1, s2, L, what)
    require(s2.export_classes, ("band_cleared", "exported"), what)
    ctx.close()


@pytest.mark.parametrize("case", TAIL_CASES, ids=case_id)
def test_tracked_frame_depth_tail_and_seeds(oracle, ellc, case):
    """ellc_track_frame from a given map: seeds_percent (of the map before the observation) ==, then — from the pose the GPU returned —
    the map and every exported level == the second source's observeDepthRow, doRegularization(), updateDepthImage (main.cpp:500-502)"""
    (W, H), path = case
    L = 4
    cfg, pair, kf, st = stencil_scene(oracle, W, H, L, 1200 + W, plant_export=False)
    ctx = make_ctx(ellc, pair, W, H, L)
    ctx.keyframe_set_depth(0, pair["depth0"], pair["var0"])
    with_state(ctx, st)
    s2 = stages_of(cfg, pair, kf, st, L)
    seeds0 = s2.calculate_no_of_seeds()
    assert ctx.depth_seeds() == seeds0
    pose, iters, _, seeds = ctx.track_frame(0)
    assert seeds == seeds0
    pwo = np.asarray(oracle.concat_relative(np.asarray(pose, np.float32), np.zeros(6, np.float32)), np.float32)
    cur = oracle.Frame(cfg, pair["cur_image"], 2)
    cur.set_pose(origin=pwo, world=pwo)
    s2.set_current(pair["cur_image"], cur.calc_se3(kf))
    s2.observe_depth_row(3, H - 3)
    s2.do_regularization()
    s2.update_depth_image()
    what = "tracked frame %dx%d %s" % (W, H, path)
    print("%s: update returns %r, fill %r, regularise %r" % (what, s2.update_returns, s2.fill_classes, s2.reg_classes))
    assert_states_equal(ctx.depth_get_state(), s2.st, what)
    assert_gpu_export(ctx, 0, s2, L, what)
    assert ctx.depth_seeds() == s2.calculate_no_of_seeds()
    require(s2.fill_classes, ("create", "reject_val_le_30"), what)
    require(s2.reg_classes, ("smoothed", "dropped_blacklist"), what)
    ctx.close()
