"""ellc_depth_absorb_keyframes (ABI v17) against tests/absorb_reference.py. The reference is fed the slots' planes as keyframe_depth_level /
image_level / max_gradient read them back and the state as depth_get_state reads it back (all pinned by their own tests), so the new
kernels are the only thing under test; all seven state planes are compared with ==, the floats by their bit patterns, and all stats."""
import ctypes as C
import numpy as np
import pytest

import absorb_reference as A
from helpers import gpu_problem

pytestmark = pytest.mark.gpu

FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
BAD_ARG, NOT_READY = -1, -3
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
SHAPES = {"64x48": (64, 48, 3), "23x17": (23, 17, 2), "131x67": (131, 67, 3)}   # (width, height, levels); 131x67 is five tiles at level 0
K_SLOT, IMAGE_ONLY_SLOT, SPARE_SLOT, N_SLOTS = 0, 5, 6, 7
SOURCES = [1, 2, 3, 4]


def fkw(flt):
    return dict(max_var=flt[0], min_support=flt[1], support_k2=flt[2], stride=flt[3])


def make_world(ellc, shape, n_slots=N_SLOTS, **kw):
    """absorb_reference.make_scene: keyframe slot 0 is the live keyframe K with the (halved) state, slots 1..4 the sources; 5 holds an image
    only, 6 an image (the crafted maps)."""
    w, h, L = SHAPES[shape] if isinstance(shape, str) else shape
    sc = A.make_scene(w, h)
    ctx = gpu_problem(ellc, w, h, L, sc["views"], max_keyframes=n_slots, **kw)
    ctx.keyframe_upload(IMAGE_ONLY_SLOT, sc["views"][1]["kf_image"])
    ctx.keyframe_upload(SPARE_SLOT, sc["views"][0]["kf_image"])
    ctx.depth_set_keyframe(K_SLOT)
    ctx.depth_set_state(sc["state"])
    return dict(ctx=ctx, scene=sc, intr=sc["intr"], Ts=sc["Ts"], state=sc["state"], w=w, h=h, L=L, planes={}, refs={})


def planes_of(world, slot):
    """(depth, var, stored image) of a slot's level 0, read back once."""
    if slot not in world["planes"]:
        d, v = world["ctx"].keyframe_depth_level(slot, 0)
        img, (rows, cols) = world["ctx"].image_level(True, slot, 0)
        assert d.shape == (rows, cols)
        world["planes"][slot] = (d, v, img)
    return world["planes"][slot]


def k_planes(world):
    if "k" not in world["planes"]:
        world["planes"]["k"] = (world["ctx"].image_level(True, K_SLOT, 0)[0], world["ctx"].max_gradient(True, K_SLOT)[0])
    return world["planes"]["k"]


def reference(world, slots, Ts, flt, state, **prm):
    """Computed once per case and shared; never written to."""
    key = (tuple(slots), np.asarray(Ts, np.float32).tobytes(), tuple(flt), b"".join(np.ascontiguousarray(state[k]).tobytes() for k in A.PLANES),
           tuple(sorted(prm.items())))
    if key not in world["refs"]:
        k_img, k_mg = k_planes(world)
        world["refs"][key] = A.absorb([planes_of(world, s) for s in slots], world["intr"], Ts, flt, k_img, k_mg, state, **prm)
    return world["refs"][key]


def run(world, slots, Ts, flt, state, ctx=None, **prm):
    """The state uploaded, read back (what the reference is fed), the fold without `finalise`, and the state read back again."""
    ctx = ctx or world["ctx"]
    ctx.depth_set_state(state)
    before = ctx.depth_get_state()
    stats = ctx.depth_absorb(slots, Ts, params=dict(finalise=0, **prm), **fkw(flt))
    return before, ctx.depth_get_state(), stats


def check(world, slots, Ts, flt, state, **prm):
    before, got, stats = run(world, slots, Ts, flt, state, **prm)
    ref = reference(world, slots, Ts, flt, before, **prm)
    print(world["w"], world["h"], "slots", list(slots), "filter", flt, prm, "stats", stats)
    for name in A.PLANES:
        assert got[name].shape == ref[name].shape and got[name].dtype == ref[name].dtype, name
    assert not A.differing(got, ref), (prm, A.differing(got, ref))
    assert stats == ref["stats"], (stats, ref["stats"])
    assert stats["n_visited"] == stats["n_created"] + stats["n_merged"] + stats["n_replaced"] + stats["n_occluded"] + stats["n_skipped"]
    assert stats["n_valid_after"] == int((got["valid"] != 0).sum()) and stats["reserved"] == 0
    return ref, got, stats


@pytest.fixture(scope="module", params=list(SHAPES))
def world(request, ellc):
    wd = make_world(ellc, request.param)
    wd["shape"] = request.param
    yield wd
    wd["ctx"].close()


@pytest.fixture(scope="module")
def world64(ellc):
    wd = make_world(ellc, "64x48")
    yield wd
    wd["ctx"].close()


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_bit_for_bit_against_the_reference(world, flt):
    for photo_gate in (1, 0):
        for max_fold in (64, 2, 1):
            ref, got, stats = check(world, SOURCES, world["Ts"], flt, world["state"], photo_gate=photo_gate, max_fold=max_fold)
            if flt == FILTERS[0] and world["shape"] != "23x17":   # conditions of the test: the scene keeps reaching every class
                for k in ("n_created", "n_merged", "n_replaced", "n_occluded"):
                    assert stats[k] > 0, (k, stats)
                assert stats["n_interior"] < stats["n_in_view"] and (not photo_gate or stats["n_candidates"] < stats["n_interior"])
                assert (stats["targets_truncated"] > 0) == (max_fold < 64)
            # what nobody touched keeps every byte
            keep = ~ref["touched"]
            for name in A.PLANES:
                assert np.array_equal(got[name][keep].view(np.uint8), world["state"][name][keep].view(np.uint8)), name
            assert (got["invDepthSmoothed"][ref["touched"]] == -1).all() and (got["blacklisted"][ref["touched"]] == 0).all()


def test_the_same_slot_three_times_and_the_keyframe_among_the_sources(world64):
    T = world64["Ts"][0]
    ref, _, stats = check(world64, [1, 1, 1], [T, T, T], FILTERS[0], world64["state"])
    assert stats["n_candidates"] % 3 == 0 and stats["n_merged"] >= 2 * stats["n_created"] > 0   # whatever is created is merged into twice
    # K's own slot at the identity, between two sources: its map lands on itself
    ref, _, stats = check(world64, [1, K_SLOT, 2], [world64["Ts"][0], IDENTITY, world64["Ts"][1]], FILTERS[0], world64["state"])
    assert stats["n_created"] > 0 and stats["n_merged"] > 0


def test_more_candidates_than_one_walk_of_the_segment_selects(ellc):
    """absorb_fold takes eight candidates per walk over a target's segment: twenty requests make segments of twenty and more entries, and
    max_fold stops the fold in front of, at and behind the end of a walk."""
    wd = make_world(ellc, "23x17", n_slots=20)
    try:
        same, T = [1] * 20, np.stack([wd["Ts"][0]] * 20)
        mixed, Tm = [1 + k % 4 for k in range(20)], wd["Ts"][[k % 4 for k in range(20)]]
        for max_fold in (64, 19, 17, 16, 15, 9, 8, 7, 1):
            ref, _, stats = check(wd, same, T, FILTERS[0], wd["state"], max_fold=max_fold)
            assert stats["n_candidates"] % 20 == 0 and stats["n_candidates"] >= 20 * stats["targets_hit"] > 0   # twenty entries per source pixel
            assert (stats["targets_truncated"] == stats["targets_hit"]) if max_fold < 20 else (stats["targets_truncated"] < stats["targets_hit"])
            ref, _, stats = check(wd, mixed, Tm, FILTERS[0], wd["state"], max_fold=max_fold)
            assert stats["n_visited"] <= max_fold * stats["targets_hit"]
    finally:
        wd["ctx"].close()


def test_requests_from_128_up(ellc):
    """The id (b << 24) | i has bit 31 set from request 128 on: such candidates sort behind the others and fold like any other."""
    wd = make_world(ellc, (16, 16, 1), n_slots=160)
    ctx = wd["ctx"]
    try:
        ctx.keyframe_set_depth(SPARE_SLOT, np.zeros((16, 16), np.float32), np.full((16, 16), -1, np.float32))
        slots = [SPARE_SLOT] * 126 + [1, 2] + [SPARE_SLOT] * 4 + [1, 2, 3, 4, 1, 2]
        which = [0, 1] + [0, 1, 2, 3, 0, 1]
        Ts = np.concatenate([np.tile(IDENTITY, (126, 1)), wd["Ts"][which[:2]], np.tile(IDENTITY, (4, 1)), wd["Ts"][which[2:]]])
        for max_fold in (64, 2):
            ref, _, stats = check(wd, slots, Ts, FILTERS[0], wd["state"], photo_gate=0, max_fold=max_fold)
            assert stats["n_candidates"] > 40 and stats["n_merged"] > 0 and stats["n_created"] > 0, stats
    finally:
        ctx.close()


def test_zero_variance(world64):
    """var = nvar = 0 on an agreeing candidate is skipped; a zero on one side goes through IEEE infinities to a variance of 0."""
    ctx, w, h = world64["ctx"], world64["w"], world64["h"]
    depth = np.full((h, w), 2.0, np.float32)
    var = np.full((h, w), 1.0 / 64, np.float32)
    var[:, : w // 2] = 0.0
    ctx.keyframe_set_depth(SPARE_SLOT, depth, var)
    world64["planes"].pop(SPARE_SLOT, None)
    state = {k: np.array(world64["state"][k], copy=True) for k in A.PLANES}
    state["valid"][:] = 1
    state["invDepth"][:] = 0.5
    state["variance"][:] = 1.0 / 64
    state["variance"][: h // 2, :] = 0.0
    ref, got, stats = check(world64, [SPARE_SLOT], [IDENTITY], FILTERS[0], state, photo_gate=0)
    inner = np.zeros((h, w), bool); inner[3:h - 3, 3:w - 3] = True   # u = x > 2.1, u < cols - 3.1
    both_zero = inner & (var == 0) & (state["variance"] == 0)
    assert stats["n_skipped"] == int(both_zero.sum()) > 0 and stats["n_merged"] == int((inner & ~both_zero).sum()) and stats["n_candidates"] == int(inner.sum())
    assert not ref["touched"][both_zero].any() and ref["touched"][inner & ~both_zero].all()
    one_zero = inner & ((var == 0) != (state["variance"] == 0))
    assert (got["variance"][one_zero] == 0).all() and (got["invDepth"][one_zero] == 0.5).all()
    none_zero = inner & (var != 0) & (state["variance"] != 0)
    assert (got["variance"][none_zero] == np.float32(1.0 / 128)).all()


def test_a_second_context_a_second_call_and_a_call_behind_a_batch_give_the_same_bytes(ellc):
    wd = make_world(ellc, "64x48", max_batch=3, max_frames=5)
    other = make_world(ellc, "64x48", arith=ellc.ARITH_FAST, grid_batch=4)
    ctx = wd["ctx"]
    try:
        ref, a, stats = check(wd, SOURCES, wd["Ts"], FILTERS[1], wd["state"])
        _, b, stats_b = run(wd, SOURCES, wd["Ts"], FILTERS[1], wd["state"])
        assert not A.differing(a, b) and stats == stats_b
        _, c, stats_c = run(other, SOURCES, other["Ts"], FILTERS[1], other["state"])
        assert not A.differing(a, c) and stats == stats_c
        ctx.set_grid_batch(2)
        _, d, stats_d = run(wd, SOURCES, wd["Ts"], FILTERS[1], wd["state"])
        assert not A.differing(a, d) and stats == stats_d
        before = [ctx.keyframe_depth_level(s, l) for s in range(5) for l in range(wd["L"])]
        plain = ctx.align([1, 2, 3], [1, 2, 3])
        ctx.depth_set_state(wd["state"])
        ctx.align_enqueue([1, 2, 3], [1, 2, 3])
        stats_e = ctx.depth_absorb(SOURCES, wd["Ts"], params=dict(finalise=0), **fkw(FILTERS[1]))
        fetched = ctx.align_fetch(3)
        for x, y in zip(plain, fetched):
            assert x.tobytes() == y.tobytes()
        assert not A.differing(a, ctx.depth_get_state()) and stats == stats_e
        after = [ctx.keyframe_depth_level(s, l) for s in range(5) for l in range(wd["L"])]   # without `finalise` the call writes no slot
        for (d0, v0), (d1, v1) in zip(before, after):
            assert d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes()
    finally:
        ctx.close(); other["ctx"].close()


@pytest.mark.parametrize("shape", ["64x48", "23x17"])   # the export's tiled launch, and its per-level kernels
def test_finalise_is_regularise_and_export_and_tracking_goes_on(ellc, shape):
    a, b = make_world(ellc, shape), make_world(ellc, shape)
    ca, cb = a["ctx"], b["ctx"]
    try:
        sa = ca.depth_absorb(SOURCES, a["Ts"], params=dict(finalise=1))
        sb = cb.depth_absorb(SOURCES, b["Ts"], params=dict(finalise=0))
        cb.depth_do_regularization(False)
        cb.depth_update_depth_image()
        assert sa == sb and sa["n_created"] > 0
        ga, gb = ca.depth_get_state(), cb.depth_get_state()
        assert not A.differing(ga, gb), A.differing(ga, gb)
        for level in range(a["L"]):
            (da, va), (db, vb) = ca.keyframe_depth_level(K_SLOT, level), cb.keyframe_depth_level(K_SLOT, level)
            assert da.tobytes() == db.tobytes() and va.tobytes() == vb.tobytes(), level
        d0, _ = ca.keyframe_depth_level(K_SLOT, 0)
        assert d0.tobytes() != a["scene"]["views"][0]["depth0"].tobytes()   # K's planes are the absorbed map's now
        seeds = ca.depth_seeds()
        assert seeds == cb.depth_seeds() and seeds == np.float32(int((ga["valid"] != 0).sum())) / np.float32(a["w"] * a["h"]) * 100
        ta, tb = ca.track_frame(0), cb.track_frame(0)
        assert np.isfinite(ta[0]).all() and ta[0].tobytes() == tb[0].tobytes() and ta[1].tobytes() == tb[1].tobytes() and ta[2:] == tb[2:]
        assert ta[3] == seeds   # the seeds figure of the map before the observation
    finally:
        ca.close(); cb.close()


def raw_call(ctx, ellc, slots, T, stats, flt=(0.0, 0, 1.0, 1), null=None, B=None, **prm):
    """The status of ellc_depth_absorb_keyframes, not raised. null: which pointer argument to pass as NULL."""
    kf = np.ascontiguousarray(slots, np.int32).reshape(-1)
    B = kf.size if B is None else B
    Tn = np.ascontiguousarray(np.tile(np.asarray(T, np.float32).reshape(-1)[:12], max(kf.size, 1)))
    f = ellc._lib.EllcMapFilter(flt[0], int(flt[1]), flt[2], int(flt[3]))
    p = ellc._lib.EllcAbsorbParams(prm.get("agree_k2", 1.0), prm.get("max_fold", 64), prm.get("photo_gate", 1), prm.get("src_validity", 20),
                                   prm.get("finalise", 1))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    return ctx._l.ellc_depth_absorb_keyframes(ctx.h, B, None if null == "slots" else ptr(kf), None if null == "T" else ptr(Tn),
                                              None if null == "filter" else C.byref(f), None if null == "params" else C.byref(p),
                                              None if null == "out" else C.byref(stats))


def test_refusals_change_nothing(ellc):
    wd = make_world(ellc, "64x48")
    ctx, T = wd["ctx"], wd["Ts"][0]
    fresh = gpu_problem(ellc, 64, 48, 3, wd["scene"]["views"], max_keyframes=N_SLOTS)   # no depth-map keyframe, no state
    try:
        state = ctx.depth_get_state()
        before = [ctx.keyframe_depth_level(s, l) for s in range(5) for l in range(wd["L"])]
        stats = ellc._lib.EllcAbsorbStats(*range(101, 117))

        def call(slots=(1,), **kw):
            return raw_call(ctx, ellc, list(slots), T, stats, **kw)

        assert call(B=0) == BAD_ARG and call(B=-1) == BAD_ARG                                   # B < 1
        assert call(slots=(1, 2, 3, 4, 1, 2, 3, 4)) == BAD_ARG                                  # B > max_keyframes
        assert call(slots=(-1,)) == BAD_ARG and call(slots=(N_SLOTS,)) == BAD_ARG and call(slots=(1, N_SLOTS)) == BAD_ARG
        assert call(null="slots") == BAD_ARG and call(null="T") == BAD_ARG and call(null="filter") == BAD_ARG and call(null="params") == BAD_ARG
        assert call(flt=(0.0, -1, 1.0, 1)) == BAD_ARG and call(flt=(0.0, 9, 1.0, 1)) == BAD_ARG and call(flt=(0.0, 0, 1.0, 0)) == BAD_ARG
        assert call(flt=(0.0, 0, -1.0, 1)) == BAD_ARG and call(flt=(0.0, 0, np.inf, 1)) == BAD_ARG and call(flt=(0.0, 0, np.nan, 1)) == BAD_ARG
        assert call(flt=(np.nan, 0, 1.0, 1)) == BAD_ARG
        assert call(agree_k2=-1.0) == BAD_ARG and call(agree_k2=np.inf) == BAD_ARG and call(agree_k2=np.nan) == BAD_ARG
        assert call(max_fold=0) == BAD_ARG and call(max_fold=65) == BAD_ARG
        assert call(src_validity=-1) == BAD_ARG and call(src_validity=256) == BAD_ARG
        assert call(photo_gate=2) == BAD_ARG and call(photo_gate=-1) == BAD_ARG and call(finalise=2) == BAD_ARG and call(finalise=-1) == BAD_ARG
        assert call(slots=(IMAGE_ONLY_SLOT,)) == NOT_READY and call(slots=(1, IMAGE_ONLY_SLOT)) == NOT_READY
        assert raw_call(fresh, ellc, [1], T, stats) == NOT_READY
        with pytest.raises(ellc.EllcError):
            ctx.depth_absorb([IMAGE_ONLY_SLOT], [T])
        with pytest.raises(ellc.EllcError):
            ctx.depth_absorb([1], [T], params=dict(max_fold=65))
        # every refused call left the prefilled stats, the state and every slot plane as they were
        assert [getattr(stats, k) for k in ellc._lib.ABSORB_STATS_FIELDS] == list(range(101, 117))
        assert not A.differing(state, ctx.depth_get_state())
        after = [ctx.keyframe_depth_level(s, l) for s in range(5) for l in range(wd["L"])]
        for (d0, v0), (d1, v1) in zip(before, after):
            assert d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes()
        # the edges of the accepted range, and `out` may be NULL
        assert call(agree_k2=0.0, max_fold=1, src_validity=0, photo_gate=0, finalise=0) == 0 and stats.reserved == 0 and stats.n_kept > 0
        ctx.depth_set_state(state)
        assert call(src_validity=255, null="out", finalise=0) == 0
        # and a good call gives what the reference gives
        check(wd, SOURCES, wd["Ts"], FILTERS[0], wd["state"])
    finally:
        ctx.close(); fresh.close()
