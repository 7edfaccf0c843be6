"""ellc_keyframe_render_depth (ABI v13) against tests/render_depth_reference.py. The reference is fed the slots' planes as
keyframe_depth_level / image_level read them back (pinned by their own tests), so the new kernels are the only thing under test; every
plane is compared with ==, the floats by their bit patterns."""
import ctypes as C
import numpy as np
import pytest

import render_depth_reference as R
from helpers import gpu_problem

pytestmark = pytest.mark.gpu

FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
BAD_ARG, NOT_READY = -1, -3
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
# (width, height, levels): 23x17 has 11 columns stored 12 wide at level 1; 131x67 is five tiles at level 0
SHAPES = {"64x48": (64, 48, 3), "23x17": (23, 17, 2), "131x67": (131, 67, 3)}
ZERO_SLOT, IMAGE_ONLY_SLOT, DST_SLOT, N_SLOTS = 3, 4, 5, 6


def fkw(flt):
    return dict(max_var=flt[0], min_support=flt[1], support_k2=flt[2], stride=flt[3])


def make_world(ellc, shape, **kw):
    """Keyframe slots 0, 1, 2 hold scenes 11, 12, 13; 3 an all-zero depth; 4 an image only; 5 an image and no depth (the destination)."""
    w, h, L = SHAPES[shape]
    scenes = [R.make_scene(w, h, seed) for seed in (11, 12, 13)]
    ctx = gpu_problem(ellc, w, h, L, scenes, max_keyframes=N_SLOTS, **kw)
    ctx.keyframe_upload(ZERO_SLOT, scenes[0]["kf_image"])
    ctx.keyframe_set_depth(ZERO_SLOT, np.zeros((h, w), np.float32), np.full((h, w), -1, np.float32))
    ctx.keyframe_upload(IMAGE_ONLY_SLOT, scenes[1]["kf_image"])
    ctx.keyframe_upload(DST_SLOT, scenes[2]["kf_image"])
    m = float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0]))
    return dict(ctx=ctx, scenes=scenes, intrinsics=scenes[0]["intrinsics"], Ts=R.scene_transforms(m), w=w, h=h, L=L, m=m, planes={}, refs={})


def planes_of(world, slot, level):
    """(depth, var, stored image) of a slot's level, read back once."""
    if (slot, level) not in world["planes"]:
        d, v = world["ctx"].keyframe_depth_level(slot, level)
        img, (rows, cols) = world["ctx"].image_level(True, slot, level)
        assert d.shape == (rows, cols)
        world["planes"][(slot, level)] = (d, v, img)
    return world["planes"][(slot, level)]


def reference(world, slots, level, Ts, flt, agree_k2=1.0):
    key = (tuple(slots), level, np.asarray(Ts, np.float32).tobytes(), tuple(flt), agree_k2)
    if key not in world["refs"]:
        world["refs"][key] = R.render([planes_of(world, s, level) for s in slots], R.level_intrinsics(*world["intrinsics"], level), Ts, flt, agree_k2)
    return world["refs"][key]


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
    ctx = world["ctx"]
    if world["shape"] == "23x17":
        img1, (_, cols1) = ctx.image_level(True, 0, 1)
        assert cols1 == 11 and img1.shape[1] == 12
    for level in range(world["L"]):
        ref = reference(world, [0, 1, 2], level, world["Ts"], flt)
        got = ctx.render_depth([0, 1, 2], world["Ts"], level=level, agree_k2=1.0, **fkw(flt))
        st = ref["stats"]
        classes = dict(multi=int((st["hits"] >= 2).sum()), agreeing=int((ref["agree"] >= 2).sum()), disagreeing=int((st["disagree"] > 0).sum()),
                       behind=sum(st["behind"]), outside=sum(st["outside"]), most=int(st["hits"].max()))
        print(world["shape"], "level", level, "filter", flt, "n_valid", got["n_valid"], "reference", ref["n_valid"], classes)
        for name in R.PLANES:
            assert got[name].shape == ref[name].shape and got[name].dtype == ref[name].dtype, name
        assert R.planes_equal(got, ref), (level, flt, [n for n in R.PLANES if got[n].tobytes() != ref[n].tobytes()])
        assert (got["agree"][got["source"] >= 0] >= 1).all() and (got["agree"][got["source"] < 0] == 0).all()
        assert got["n_valid"] == int((got["depth"] > 0).sum()) > 0
        if level == 0:   # a condition of the test: the scenes and transforms must keep exercising collisions and drops
            assert min(classes[k] for k in ("multi", "agreeing", "disagreeing", "behind", "outside")) > 0, classes


@pytest.mark.parametrize("shape", ["64x48", "23x17"])
def test_both_arithmetic_modes_give_the_same_bytes(ellc, shape):
    exact = make_world(ellc, shape, arith=ellc.ARITH_EXACT)
    fast = make_world(ellc, shape, arith=ellc.ARITH_FAST, grid_batch=4)
    try:
        for level in range(exact["L"]):
            a = exact["ctx"].render_depth([0, 1, 2], exact["Ts"], level=level, **fkw(FILTERS[0]))
            b = fast["ctx"].render_depth([0, 1, 2], fast["Ts"], level=level, **fkw(FILTERS[0]))
            assert a["n_valid"] > 0 and R.planes_equal(a, b)
            assert R.planes_equal(b, reference(fast, [0, 1, 2], level, fast["Ts"], FILTERS[0]))
    finally:
        exact["ctx"].close(); fast["ctx"].close()


def test_the_same_slot_twice_goes_to_the_lower_request(world64):
    ctx, T = world64["ctx"], world64["Ts"][1]
    got = ctx.render_depth([1, 1], [T, T], **fkw(FILTERS[0]))
    won = got["source"] >= 0
    assert won.sum() > 100
    assert ((got["source"][won] >> 24) == 0).all() and (got["agree"][won] >= 2).all() and (got["agree"][won] % 2 == 0).all()
    assert R.planes_equal(got, reference(world64, [1, 1], 0, [T, T], FILTERS[0]))
    single = ctx.render_depth([1], [T], **fkw(FILTERS[0]))
    for name in ("depth", "var", "source", "intensity"):
        assert single[name].tobytes() == got[name].tobytes(), name
    assert np.array_equal(2 * single["agree"], got["agree"])


def test_a_batch_equals_itself_on_a_second_call(world64):
    ctx = world64["ctx"]
    slots, Ts = [2, 0, 1, 0], world64["Ts"][[1, 2, 0, 1]]
    a = ctx.render_depth(slots, Ts, **fkw(FILTERS[1]))
    b = ctx.render_depth(slots, Ts, **fkw(FILTERS[1]))
    assert a["n_valid"] > 0 and a["n_valid"] == b["n_valid"]
    for name in R.PLANES:
        assert a[name].tobytes() == b[name].tobytes(), name
    assert R.planes_equal(a, reference(world64, slots, 0, Ts, FILTERS[1]))


def test_everything_behind_the_camera_and_an_empty_slot(world64):
    ctx = world64["ctx"]
    back = IDENTITY.copy(); back[10] = -1.0; back[11] = -0.5   # z' = -Z - 1/2 < 0 for every ok pixel, the 1e30 of the spoilt ones included
    got = ctx.render_depth([0, 1], [back, back], **fkw(FILTERS[0]))
    assert got["n_valid"] == 0 and (got["depth"] == 0).all() and (got["var"] == -1).all() and (got["source"] == -1).all()
    assert (got["agree"] == 0).all() and (got["intensity"] == 0).all()
    # a request on a slot with an all-zero depth contributes nothing
    Ts = world64["Ts"]
    with_empty = ctx.render_depth([0, ZERO_SLOT, 1], [Ts[1], Ts[0], Ts[2]], **fkw(FILTERS[0]))
    assert R.planes_equal(with_empty, reference(world64, [0, ZERO_SLOT, 1], 0, [Ts[1], Ts[0], Ts[2]], FILTERS[0]))
    without = ctx.render_depth([0, 1], [Ts[1], Ts[2]], **fkw(FILTERS[0]))
    assert with_empty["n_valid"] == without["n_valid"] > 0 and not ((with_empty["source"] >> 24) == 1).any()
    for name in ("depth", "var", "agree", "intensity"):
        assert with_empty[name].tobytes() == without[name].tobytes(), name
    assert ctx.render_depth([ZERO_SLOT], [Ts[0]])["n_valid"] == 0


def dense_scenes(w, h):
    """Three scenes whose depth is positive everywhere (smooth, about 2) with a small variance: under the identity every pixel lands on itself."""
    out = []
    yy, xx = np.mgrid[0:h, 0:w]
    for k, s in enumerate(R.make_scene(w, h, seed) for seed in (11, 12, 13)):
        s = dict(s)
        s["depth0"] = (2.0 + 0.25 * np.sin(0.1 * xx + k) * np.cos(0.13 * yy)).astype(np.float32)
        s["var0"] = np.full((h, w), 0.01, np.float32)
        out.append(s)
    return out


@pytest.mark.parametrize("kind", ["semi-dense", "dense"])
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_destination_slot_is_what_set_depth_would_leave(ellc, kind, arith):
    w, h, L = SHAPES["64x48"]
    ar = ellc.ARITH_FAST if arith == "fast" else ellc.ARITH_EXACT
    if kind == "dense":
        scenes = dense_scenes(w, h)
        slots, Ts = [0], np.stack([IDENTITY])
    else:
        scenes = [R.make_scene(w, h, seed) for seed in (11, 12, 13)]
        m = float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0]))
        slots, Ts = [0, 1, 2], R.scene_transforms(m)
    a = gpu_problem(ellc, w, h, L, scenes, max_keyframes=N_SLOTS, arith=ar)
    b = gpu_problem(ellc, w, h, L, scenes, max_keyframes=N_SLOTS, arith=ar)
    try:
        for ctx in (a, b):
            ctx.keyframe_upload(DST_SLOT, scenes[0]["kf_image"])
        got = a.render_depth(slots, Ts, dst_slot=DST_SLOT)
        frac = got["n_valid"] / float(w * h)
        print(kind, arith, "valid fraction %.4f" % frac)
        assert (frac >= 0.9) if kind == "dense" else (0.05 < frac < 0.9)
        plain = a.render_depth(slots, Ts)   # the planes do not depend on the destination
        assert R.planes_equal(got, plain)
        b.keyframe_set_depth(DST_SLOT, got["depth"], got["var"])
        for level in range(L):
            (da, va), (db, vb) = a.keyframe_depth_level(DST_SLOT, level), b.keyframe_depth_level(DST_SLOT, level)
            assert da.tobytes() == db.tobytes() and va.tobytes() == vb.tobytes(), level
        d0, v0 = a.keyframe_depth_level(DST_SLOT, 0)
        assert d0.tobytes() == got["depth"].tobytes() and v0.tobytes() == got["var"].tobytes()
        for mode in (ellc.MODE_FCA, ellc.MODE_ICA):
            ra, rb = a.align([DST_SLOT, 0], [0, 1], mode=mode), b.align([DST_SLOT, 0], [0, 1], mode=mode)
            for x, y in zip(ra, rb):
                assert x.tobytes() == y.tobytes(), mode
        # the destination is a source of the next render like any other slot
        ra, rb = a.render_depth([DST_SLOT, 1], Ts[[0, 0]], level=1), b.render_depth([DST_SLOT, 1], Ts[[0, 0]], level=1)
        assert ra["n_valid"] > 0 and R.planes_equal(ra, rb)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("cache_records", [0, 1])
def test_reads_only(ellc, cache_records):
    wd = make_world(ellc, "64x48", cache_records=cache_records, max_batch=3, max_frames=3)
    ctx, Ts = wd["ctx"], wd["Ts"]
    try:
        before = [ctx.keyframe_depth_level(s, l) for s in range(3) for l in range(wd["L"])]
        first = ctx.align([0, 1, 2], [0, 1, 2])
        ctx.align_enqueue([0, 1, 2], [0, 1, 2])
        plain = ctx.align_fetch(3)
        r0 = ctx.render_depth([0, 1, 2], Ts, **fkw(FILTERS[1]))
        ctx.render_depth([2, 1], Ts[:2], level=1)
        second = ctx.align([0, 1, 2], [0, 1, 2])
        for x, y in zip(first, second):
            assert x.tobytes() == y.tobytes()
        after = [ctx.keyframe_depth_level(s, l) for s in range(3) for l in range(wd["L"])]
        for (d0, v0), (d1, v1) in zip(before, after):
            assert d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes()
        # behind a batch in flight and before its fetch: the batch returns what it returns without the render, and so does the render
        ctx.align_enqueue([0, 1, 2], [0, 1, 2])
        r1 = ctx.render_depth([0, 1, 2], Ts, **fkw(FILTERS[1]))
        fetched = ctx.align_fetch(3)
        for x, y in zip(plain, fetched):
            assert x.tobytes() == y.tobytes()
        assert r0["n_valid"] > 0 and R.planes_equal(r0, r1)
    finally:
        ctx.close()


def raw_call(ctx, ellc, slots, T, level=0, flt=(0.0, 0, 1.0, 1), agree_k2=1.0, dst=-1, null=None, B=None):
    """The status of ellc_keyframe_render_depth, not raised. null: which pointer argument to pass as NULL."""
    kf = np.ascontiguousarray(slots, np.int32).reshape(-1)
    B = kf.size if B is None else B
    Tn = np.ascontiguousarray(np.tile(np.asarray(T, np.float32).reshape(-1)[:12], max(kf.size, 1)))
    f = ellc._lib.EllcMapFilter(flt[0], int(flt[1]), flt[2], int(flt[3]))
    h, w = ctx.cfg.height, ctx.cfg.width
    depth = np.zeros((h, w), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    return ctx._l.ellc_keyframe_render_depth(ctx.h, B, None if null == "slots" else p(kf), None if null == "T" else p(Tn), int(level),
                                             None if null == "filter" else C.byref(f), C.c_float(agree_k2), int(dst), p(depth), None, None, None,
                                             None, None)


def test_bad_arguments_and_unready_slots(world64, ellc):
    ctx, T = world64["ctx"], world64["Ts"][1]

    def call(slots=(0,), **kw):
        return raw_call(ctx, ellc, list(slots), T, **kw)

    assert call() == 0
    assert call(slots=(0,), B=0) == BAD_ARG and call(slots=(0,), B=-1) == BAD_ARG          # B < 1
    assert call(slots=(0, 1, 2, 0, 1, 2, 0)) == BAD_ARG                                    # B > max_keyframes
    assert call(slots=(-1,)) == BAD_ARG and call(slots=(N_SLOTS,)) == BAD_ARG and call(slots=(0, N_SLOTS)) == BAD_ARG
    assert call(level=-1) == BAD_ARG and call(level=world64["L"]) == BAD_ARG
    assert call(null="slots") == BAD_ARG and call(null="T") == BAD_ARG and call(null="filter") == BAD_ARG
    assert call(flt=(0.0, -1, 1.0, 1)) == BAD_ARG and call(flt=(0.0, 9, 1.0, 1)) == BAD_ARG and call(flt=(0.0, 0, 1.0, 0)) == BAD_ARG
    assert call(flt=(0.0, 0, -1.0, 1)) == BAD_ARG and call(flt=(0.0, 0, np.inf, 1)) == BAD_ARG and call(flt=(0.0, 0, np.nan, 1)) == BAD_ARG
    assert call(flt=(np.nan, 0, 1.0, 1)) == BAD_ARG
    assert call(flt=(-1.0, 8, 0.0, 1)) == 0 and call(flt=(np.inf, 0, 1.0, 7)) == 0          # the edges of the accepted range
    assert call(agree_k2=-1.0) == BAD_ARG and call(agree_k2=np.inf) == BAD_ARG and call(agree_k2=np.nan) == BAD_ARG
    assert call(agree_k2=0.0) == 0
    assert call(dst=-2) == BAD_ARG and call(dst=N_SLOTS) == BAD_ARG
    assert call(dst=DST_SLOT, level=1) == BAD_ARG                                          # a destination takes level 0 only
    assert call(slots=(0, 1), dst=1) == BAD_ARG and call(slots=(1,), dst=1) == BAD_ARG     # a destination that is also a source
    # slots without depth (4: an image only) or without anything; the destination's own state does not matter
    assert call(slots=(IMAGE_ONLY_SLOT,)) == NOT_READY and call(slots=(0, IMAGE_ONLY_SLOT)) == NOT_READY
    with pytest.raises(ellc.EllcError):
        ctx.render_depth([IMAGE_ONLY_SLOT], [T])
    # every output pointer may be NULL
    f = ellc._lib.EllcMapFilter(0.0, 0, 1.0, 1)
    kf = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert ctx._l.ellc_keyframe_render_depth(ctx.h, 1, p(kf), p(np.ascontiguousarray(T)), 0, C.byref(f), C.c_float(1.0), -1, None, None, None, None,
                                             None, None) == 0
    # (more than 2^24 pixels on a level cannot be configured: the largest accepted image is 4096 x 4096)


def test_more_than_256_requests_are_refused(ellc):
    w, h, L = 16, 16, 1
    s = R.make_scene(w, h, 11)
    ctx = gpu_problem(ellc, w, h, L, [s], max_keyframes=257)
    try:
        assert raw_call(ctx, ellc, [0] * 257, IDENTITY) == BAD_ARG
        assert raw_call(ctx, ellc, [0] * 256, IDENTITY) == 0
        got = ctx.render_depth([0] * 256, np.tile(IDENTITY, (256, 1)))
        won = got["source"] >= 0
        assert won.sum() > 0 and ((got["source"][won] >> 24) == 0).all() and (got["agree"][won] == 256).all()
    finally:
        ctx.close()


def test_a_refused_call_leaves_the_destination_alone(world64, ellc):
    ctx, Ts = world64["ctx"], world64["Ts"]
    # slot 2 as the destination of refused calls: its planes and an alignment against it stay
    before = [ctx.keyframe_depth_level(2, l) for l in range(world64["L"])]
    pose = ctx.align([2], [2])
    assert raw_call(ctx, ellc, [0, IMAGE_ONLY_SLOT], Ts[0], dst=2) == NOT_READY
    assert raw_call(ctx, ellc, [0, 2], Ts[0], dst=2) == BAD_ARG
    assert raw_call(ctx, ellc, [0], Ts[0], dst=2, agree_k2=-1.0) == BAD_ARG
    assert raw_call(ctx, ellc, [0], Ts[0], dst=2, level=1) == BAD_ARG
    assert raw_call(ctx, ellc, [0], Ts[0], dst=2, flt=(0.0, 0, 1.0, 0)) == BAD_ARG
    after = [ctx.keyframe_depth_level(2, l) for l in range(world64["L"])]
    for (d0, v0), (d1, v1) in zip(before, after):
        assert d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes()
    again = ctx.align([2], [2])
    for x, y in zip(pose, again):
        assert x.tobytes() == y.tobytes()
    assert R.planes_equal(ctx.render_depth([0, 1, 2], Ts), reference(world64, [0, 1, 2], 0, Ts, FILTERS[0]))
