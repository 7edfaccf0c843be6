"""ellc_depth_restart_from_keyframes (ABI v18): the live map re-seated on a new keyframe from keyframe slots, starting empty. The call is
held to a twin context driven through the eight existing calls its contract names (state, every level of the new slot's planes, rescale
factor, seeds and the pose bits of a track_frame behind it, all ==), to the numpy restart of tests/trial_propagation_reference.py, and
every refusal to leaving everything as it was."""
import ctypes as C
import numpy as np
import pytest

import absorb_reference as A
import trial_propagation_reference as R
from helpers import gpu_problem

pytestmark = pytest.mark.gpu

FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
BAD_ARG, NOT_READY = -1, -3
SHAPES = {"64x48": (64, 48, 3), "23x17": (23, 17, 2), "131x67": (131, 67, 3)}   # (width, height, levels)
NEW_SLOT, IMAGE_ONLY_SLOT, EMPTY_SLOT, N_SLOTS = 0, 5, 6, 7   # slot 0 becomes the keyframe, 1..4 are the sources, 5 holds an image only, 6 nothing
SOURCES = [1, 2, 3, 4]


def fkw(flt):
    return dict(max_var=flt[0], min_support=flt[1], support_k2=flt[2], stride=flt[3])


def make_ctx(ellc, shape, **kw):
    """absorb_reference.make_scene's five views in keyframe slots 0..4 and frame slots 0..4; NO depth-map keyframe and NO state."""
    w, h, L = SHAPES[shape]
    sc = A.make_scene(w, h)
    ctx = gpu_problem(ellc, w, h, L, sc["views"], max_keyframes=N_SLOTS, **kw)
    ctx.keyframe_upload(IMAGE_ONLY_SLOT, sc["views"][1]["kf_image"])
    return ctx, sc, (w, h, L)


def slot_planes(ctx, slot, L):
    return [ctx.keyframe_depth_level(slot, l) for l in range(L)]


def same_planes(a, b):
    return all(d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes() for (d0, v0), (d1, v1) in zip(a, b))


def twin_restart(ctx, sc, dims, slots, Ts, flt, finalise, **prm):
    """The sequence the contract names, through the existing calls."""
    w, h, L = dims
    ctx.depth_set_keyframe(NEW_SLOT)
    ctx.depth_set_state(R.wiped_state(h, w))
    stats = ctx.depth_absorb(slots, Ts, params=dict(finalise=0, **prm), **fkw(flt))
    factor = 1.0
    if finalise:
        ctx.depth_regularize(True)
        ctx.depth_fill_holes()
        ctx.depth_regularize(False)
        factor = ctx.depth_make_inv_depth_one()
        ctx.depth_update_depth_image()
    return stats, factor


@pytest.mark.parametrize("shape", ["64x48", "23x17"])   # the export's tiled launch with the rescale inside, and its per-level kernels
@pytest.mark.parametrize("B", [4, 1])
def test_finalised_restart_is_the_eight_calls_and_tracking_goes_on(ellc, shape, B):
    (ca, sc, dims), (cb, _, _) = make_ctx(ellc, shape), make_ctx(ellc, shape)
    try:
        slots, Ts = SOURCES[:B], sc["Ts"][:B]
        old = slot_planes(ca, NEW_SLOT, dims[2])
        sa, fa = ca.depth_restart(NEW_SLOT, slots, Ts, **fkw(FILTERS[0]))   # a context that never had a state
        sb, fb = twin_restart(cb, sc, dims, slots, Ts, FILTERS[0], 1)
        print(shape, B, sa, fa)
        assert sa == sb and sa["n_valid_before"] == 0 and sa["n_created"] == sa["targets_hit"] == sa["n_valid_after"] > 0
        assert np.float32(fa).tobytes() == np.float32(fb).tobytes() and np.isfinite(fa) and fa > 0 and fa != 1.0
        ga, gb = ca.depth_get_state(), cb.depth_get_state()
        assert not A.differing(ga, gb), A.differing(ga, gb)
        pa, pb = slot_planes(ca, NEW_SLOT, dims[2]), slot_planes(cb, NEW_SLOT, dims[2])
        assert same_planes(pa, pb) and not same_planes(pa[:1], old[:1])   # the new keyframe's planes are the restarted map's now
        seeds = ca.depth_seeds()
        assert seeds == cb.depth_seeds() and seeds == np.float32(int((ga["valid"] != 0).sum())) / np.float32(dims[0] * dims[1]) * 100 and seeds > 0
        ta, tb = ca.track_frame(0), cb.track_frame(0)   # the depth map's keyframe is the new slot: the alignment runs against its planes
        assert np.isfinite(ta[0]).all() and ta[0].tobytes() == tb[0].tobytes() and ta[1].tobytes() == tb[1].tobytes() and ta[2:] == tb[2:]
        assert ta[3] == seeds
        assert not A.differing(ca.depth_get_state(), cb.depth_get_state())
    finally:
        ca.close(); cb.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_unfinalised_restart_is_the_three_calls_and_the_numpy_restart(ellc, shape):
    (ca, sc, dims), (cb, _, _) = make_ctx(ellc, shape), make_ctx(ellc, shape)
    w, h, L = dims
    try:
        nan = {k: np.full((h, w), np.nan, np.float32) for k in ("invDepth", "invDepthSmoothed", "variance", "varianceSmoothed")}
        nan.update(validity=np.full((h, w), 77, np.int32), blacklisted=np.full((h, w), -5, np.int32), valid=np.ones((h, w), np.uint8))
        reqs = [tuple(ca.keyframe_depth_level(s, 0)) + (ca.image_level(True, s, 0)[0],) for s in SOURCES]
        k_img, k_mg = ca.image_level(True, NEW_SLOT, 0)[0], ca.max_gradient(True, NEW_SLOT)[0]
        before = slot_planes(ca, NEW_SLOT, L)
        for flt in FILTERS:
            for B, prm in ((4, dict()), (1, dict()), (4, dict(photo_gate=0, max_fold=2)), (3, dict(agree_k2=0.25, src_validity=3))):
                # a previous state full of NaN, marked valid everywhere, on another keyframe: it leaves no trace
                ca.depth_set_keyframe(IMAGE_ONLY_SLOT)
                ca.depth_set_state(nan)
                sa, fa = ca.depth_restart(NEW_SLOT, SOURCES[:B], sc["Ts"][:B], params=dict(finalise=0, **prm), **fkw(flt))
                sb, fb = twin_restart(cb, sc, dims, SOURCES[:B], sc["Ts"][:B], flt, 0, **prm)
                ref = R.restart(reqs[:B], sc["intr"], sc["Ts"][:B], flt, k_img, k_mg, **prm)
                print(shape, flt, B, prm, sa)
                ga = ca.depth_get_state()
                assert fa == 1.0 and sa == sb == ref["stats"], (sa, sb, ref["stats"])
                assert not A.differing(ga, cb.depth_get_state()) and not A.differing(ga, ref), A.differing(ga, ref)
                assert sa["n_valid_before"] == 0 and sa["n_valid_after"] == int((ga["valid"] != 0).sum()) > 0
                untouched = ~ref["touched"]
                assert (ga["invDepth"][untouched] == 0).all() and (ga["invDepthSmoothed"] == -1).all() and (ga["blacklisted"] == 0).all()
        assert same_planes(before, slot_planes(ca, NEW_SLOT, L))   # without `finalise` the call writes no slot
        # the map sits on the new keyframe: what regularises and exports it now reaches that slot
        ca.depth_do_regularization(False)
        ca.depth_update_depth_image()
        assert not same_planes(before[:1], slot_planes(ca, NEW_SLOT, L)[:1])
    finally:
        ca.close(); cb.close()


def raw_call(ctx, ellc, new_slot, slots, T, stats, factor, flt=(0.0, 0, 1.0, 1), null=None, B=None, **prm):
    """The status of ellc_depth_restart_from_keyframes, not raised. null: which pointer argument to pass as NULL."""
    kf = np.ascontiguousarray(slots, np.int32).reshape(-1)
    B = kf.size if B is None else B
    Tn = np.ascontiguousarray(np.tile(np.asarray(T, np.float32).reshape(-1)[:12], max(kf.size, 1)))
    f = ellc._lib.EllcMapFilter(flt[0], int(flt[1]), flt[2], int(flt[3]))
    p = ellc._lib.EllcAbsorbParams(prm.get("agree_k2", 1.0), prm.get("max_fold", 64), prm.get("photo_gate", 1), prm.get("src_validity", 20),
                                   prm.get("finalise", 1))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    return ctx._l.ellc_depth_restart_from_keyframes(ctx.h, int(new_slot), B, None if null == "slots" else ptr(kf), None if null == "T" else ptr(Tn),
                                                    None if null == "filter" else C.byref(f), None if null == "params" else C.byref(p),
                                                    None if null == "factor" else C.byref(factor), None if null == "out" else C.byref(stats))


def test_refusals_change_nothing(ellc):
    """The refused calls name slot 5 as the new keyframe while the map lives on slot 0 with the scene's state: afterwards the state, the
    depth map's keyframe (seen through what an export writes) and every slot are what they are in a twin that was never asked."""
    (ctx, sc, dims), (twin, _, _) = make_ctx(ellc, "64x48"), make_ctx(ellc, "64x48")
    fresh, _, _ = make_ctx(ellc, "64x48")
    w, h, L = dims
    T = sc["Ts"][0]
    try:
        for c in (ctx, twin):
            c.depth_set_keyframe(NEW_SLOT)
            c.depth_set_state(sc["state"])
        stats = ellc._lib.EllcAbsorbStats(*range(101, 117))
        factor = C.c_float(-7.0)

        def call(new_slot=IMAGE_ONLY_SLOT, slots=(1,), **kw):
            return raw_call(ctx, ellc, new_slot, list(slots), T, stats, factor, **kw)

        assert call(new_slot=-1) == BAD_ARG and call(new_slot=N_SLOTS) == BAD_ARG
        assert call(new_slot=1) == BAD_ARG and call(new_slot=2, slots=(1, 2)) == BAD_ARG and call(new_slot=2, slots=(2, 1)) == BAD_ARG   # among the sources
        assert call(new_slot=EMPTY_SLOT) == NOT_READY                                             # no image
        assert call(B=0) == BAD_ARG and call(B=-1) == BAD_ARG
        assert call(slots=(1, 2, 3, 4, 1, 2, 3, 4)) == BAD_ARG                                    # B > max_keyframes
        assert call(slots=(-1,)) == BAD_ARG and call(slots=(N_SLOTS,)) == BAD_ARG and call(slots=(1, N_SLOTS)) == BAD_ARG
        assert call(null="slots") == BAD_ARG and call(null="T") == BAD_ARG and call(null="filter") == BAD_ARG and call(null="params") == BAD_ARG
        assert call(flt=(0.0, -1, 1.0, 1)) == BAD_ARG and call(flt=(0.0, 9, 1.0, 1)) == BAD_ARG and call(flt=(0.0, 0, 1.0, 0)) == BAD_ARG
        assert call(flt=(0.0, 0, -1.0, 1)) == BAD_ARG and call(flt=(0.0, 0, np.inf, 1)) == BAD_ARG and call(flt=(np.nan, 0, 1.0, 1)) == BAD_ARG
        assert call(agree_k2=-1.0) == BAD_ARG and call(agree_k2=np.nan) == BAD_ARG
        assert call(max_fold=0) == BAD_ARG and call(max_fold=65) == BAD_ARG
        assert call(src_validity=-1) == BAD_ARG and call(src_validity=256) == BAD_ARG
        assert call(photo_gate=2) == BAD_ARG and call(finalise=2) == BAD_ARG and call(finalise=-1) == BAD_ARG
        assert call(slots=(EMPTY_SLOT,)) == NOT_READY and call(slots=(1, EMPTY_SLOT)) == NOT_READY
        assert call(new_slot=NEW_SLOT, slots=(IMAGE_ONLY_SLOT,)) == NOT_READY                     # a source without depth
        with pytest.raises(ellc.EllcError):
            ctx.depth_restart(1, [1], [T])
        assert [getattr(stats, k) for k in ellc._lib.ABSORB_STATS_FIELDS] == list(range(101, 117)) and factor.value == -7.0
        assert not A.differing(ctx.depth_get_state(), twin.depth_get_state()) and not A.differing(ctx.depth_get_state(), sc["state"])
        # a refused restart of a context without a map leaves it without one
        assert raw_call(fresh, ellc, 1, [1], T, stats, factor) == BAD_ARG
        with pytest.raises(ellc.EllcError):
            fresh.depth_seeds()
        # the depth map's keyframe is still slot 0: an export reaches slot 0 and no other slot, exactly as in the twin
        for c in (ctx, twin):
            c.depth_do_regularization(False)
            c.depth_update_depth_image()
        for s in range(5):
            assert same_planes(slot_planes(ctx, s, L), slot_planes(twin, s, L)), s
        assert not A.differing(ctx.depth_get_state(), twin.depth_get_state())
        # the pointers that may be NULL, and the edges of the accepted range
        assert call(null="out", finalise=0) == 0 and factor.value == 1.0
        # (finalise stays off here: with src_validity 0 the regularisation would drop every hypothesis again)
        assert call(null="factor", agree_k2=0.0, max_fold=1, src_validity=0, photo_gate=0, finalise=0) == 0 and stats.n_valid_before == 0 and stats.n_created > 0
        assert ctx.depth_seeds() == np.float32(stats.n_valid_after) / np.float32(w * h) * 100 > 0
        assert call(src_validity=255) == 0 and factor.value > 0 and ctx.depth_seeds() > 0   # finalised, on slot 5
    finally:
        ctx.close(); twin.close(); fresh.close()
