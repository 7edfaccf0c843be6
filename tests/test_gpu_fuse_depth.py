"""ellc_keyframe_fuse_depth (ABI v16) against tests/fuse_depth_reference.py. The reference is fed the slots' planes as
keyframe_depth_level / image_level read them back (pinned by their own tests), so the new kernels are the only thing under test; every
plane is compared with ==, the floats by their bit patterns."""
import ctypes as C
import numpy as np
import pytest

import fuse_depth_reference as FU
import render_depth_reference as R
from helpers import gpu_problem

pytestmark = pytest.mark.gpu

FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
BAD_ARG, NOT_READY = -1, -3
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
# (width, height, levels): 23x17 has 11 columns stored 12 wide at level 1; 131x67 is five tiles at level 0
SHAPES = {"64x48": (64, 48, 3), "23x17": (23, 17, 2), "131x67": (131, 67, 3)}
ZERO_SLOT, IMAGE_ONLY_SLOT, DST_SLOT, SPARE_SLOT, N_SLOTS = 3, 4, 5, 6, 7
# the request sets of the bit-for-bit test: (slots, which of the scene transforms)
REQUESTS = [([0, 1, 2], [0, 1, 2]), ([0, 1, 2, 0], [0, 1, 2, 1])]


def fkw(flt):
    return dict(max_var=flt[0], min_support=flt[1], support_k2=flt[2], stride=flt[3])


def make_world(ellc, shape, **kw):
    """Keyframe slots 0, 1, 2 hold scenes 11, 12, 13; 3 an all-zero depth; 4 an image only; 5 an image and no depth (a destination);
    6 an image (the crafted map of the zero-variance test)."""
    w, h, L = SHAPES[shape]
    scenes = [R.make_scene(w, h, seed) for seed in (11, 12, 13)]
    ctx = gpu_problem(ellc, w, h, L, scenes, max_keyframes=N_SLOTS, **kw)
    ctx.keyframe_upload(ZERO_SLOT, scenes[0]["kf_image"])
    ctx.keyframe_set_depth(ZERO_SLOT, np.zeros((h, w), np.float32), np.full((h, w), -1, np.float32))
    ctx.keyframe_upload(IMAGE_ONLY_SLOT, scenes[1]["kf_image"])
    ctx.keyframe_upload(DST_SLOT, scenes[2]["kf_image"])
    ctx.keyframe_upload(SPARE_SLOT, scenes[0]["kf_image"])
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


def reference(world, slots, level, Ts, flt, agree_k2=1.0, max_merge=64):
    """Computed once per case and shared."""
    key = (tuple(slots), level, np.asarray(Ts, np.float32).tobytes(), tuple(flt), agree_k2, max_merge)
    if key not in world["refs"]:
        world["refs"][key] = FU.fuse([planes_of(world, s, level) for s in slots], R.level_intrinsics(*world["intrinsics"], level), Ts, flt,
                                     agree_k2, max_merge)
    return world["refs"][key]


def same_bytes(a, b, names=FU.PLANES):
    return [n for n in names if a[n].tobytes() != b[n].tobytes()]


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
def test_bit_for_bit_against_the_reference_and_the_render(world, flt):
    ctx = world["ctx"]
    if world["shape"] == "23x17":
        img1, (_, cols1) = ctx.image_level(True, 0, 1)
        assert cols1 == 11 and img1.shape[1] == 12
    for slots, which in REQUESTS:
        Ts = world["Ts"][which]
        for level in range(world["L"]):
            rendered = ctx.render_depth(slots, Ts, level=level, agree_k2=1.0, **fkw(flt))
            for max_merge in (64, 1):
                ref = reference(world, slots, level, Ts, flt, max_merge=max_merge)
                got = ctx.fuse_depth(slots, Ts, level=level, agree_k2=1.0, max_merge=max_merge, **fkw(flt))
                st = ref["stats"]
                winner = st["render"]
                classes = dict(fused=int((ref["merged"] >= 2).sum()), three=int((ref["merged"] >= 3).sum()),
                               moved=int((ref["depth"].view(np.uint32) != winner["depth"].view(np.uint32)).sum()),
                               truncated=int(st["truncated"].sum()), skipped=int(st["skipped"].sum()), longest=int(st["segment"].max()))
                print(world["shape"], "requests", slots, "level", level, "filter", flt, "max_merge", max_merge, "n_valid", got["n_valid"], "n_fused",
                      got["n_fused"], "reference", ref["n_valid"], ref["n_fused"], classes)
                for name in FU.PLANES:
                    assert got[name].shape == ref[name].shape and got[name].dtype == ref[name].dtype, name
                assert FU.planes_equal(got, ref), (slots, level, flt, max_merge, FU.differing(got, ref))
                assert got["n_fused"] == int((got["merged"] >= 2).sum()) and np.array_equal(got["merged"] > 0, got["depth"] > 0)
                # what the render decides is the render's, byte for byte
                assert not same_bytes(got, rendered, ("source", "agree", "intensity")) and got["n_valid"] == rendered["n_valid"]
                one = got["merged"] == 1
                assert np.array_equal(got["depth"][one].view(np.uint32), rendered["depth"][one].view(np.uint32))
                assert np.array_equal(got["var"][one].view(np.uint32), rendered["var"][one].view(np.uint32))
                if level == 0 and flt == FILTERS[0]:   # conditions of the test, from the reference's stats: the scenes must keep exercising the merge
                    assert classes["fused"] > 0 and classes["moved"] > 0, classes
                    if max_merge == 64:
                        assert classes["three"] > 0 and classes["truncated"] == 0, classes
                    else:
                        assert classes["truncated"] > 0 and ref["merged"].max() == 2, classes
            plain = ctx.fuse_depth(slots, Ts, level=level, agree_k2=1.0, max_merge=0, **fkw(flt))
            assert not same_bytes(plain, rendered, R.PLANES) and plain["n_valid"] == rendered["n_valid"] and plain["n_fused"] == 0
            assert np.array_equal(plain["merged"], (rendered["depth"] > 0).astype(np.int32))


def test_the_same_slot_three_times(world64):
    ctx, T = world64["ctx"], world64["Ts"][1]
    ref = reference(world64, [1, 1, 1], 0, [T, T, T], FILTERS[0])
    won = ref["source"] >= 0
    assert won.sum() > 100 and (ref["merged"][won] >= 3).all()   # a condition of the test: every target fuses all three
    got = ctx.fuse_depth([1, 1, 1], [T, T, T], **fkw(FILTERS[0]))
    assert ((got["source"][got["source"] >= 0] >> 24) == 0).all()
    assert FU.planes_equal(got, ref), FU.differing(got, ref)
    assert got["n_fused"] == got["n_valid"] == int(won.sum())


def test_more_members_than_one_walk_of_the_segment_selects(ellc):
    """fuse_merge takes eight members per walk over a target's segment: twenty requests make segments of up to twenty and more entries, and
    max_merge stops the merge in front of, at and behind the end of a walk."""
    w, h, L = SHAPES["23x17"]
    scenes = [R.make_scene(w, h, seed) for seed in (11, 12, 13)]
    ctx = gpu_problem(ellc, w, h, L, scenes, max_keyframes=20)
    wd = dict(ctx=ctx, intrinsics=scenes[0]["intrinsics"], planes={}, refs={})
    Ts = R.scene_transforms(float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0])))
    try:
        same, T = [1] * 20, np.stack([Ts[1]] * 20)
        mixed, Tm = [k % 3 for k in range(20)], Ts[[(k // 3) % 3 for k in range(20)]]
        for max_merge in (64, 19, 18, 17, 16, 15, 9, 8, 7, 1):
            ref = reference(wd, same, 0, T, FILTERS[0], max_merge=max_merge)
            won = ref["source"] >= 0
            # a condition of the test: every target holds twenty entries per source pixel that lands on it (20, 40 or 60), none skipped
            assert won.sum() > 50 and (ref["agree"][won] % 20 == 0).all() and ref["agree"].max() >= 40
            assert (ref["merged"][won] == np.minimum(ref["agree"][won] - 1, max_merge) + 1).all()
            got = ctx.fuse_depth(same, T, max_merge=max_merge, **fkw(FILTERS[0]))
            assert FU.planes_equal(got, ref), (max_merge, FU.differing(got, ref))
            for level in range(L):
                ref = reference(wd, mixed, level, Tm, FILTERS[0], max_merge=max_merge)
                got = ctx.fuse_depth(mixed, Tm, level=level, max_merge=max_merge, **fkw(FILTERS[0]))
                assert FU.planes_equal(got, ref), (max_merge, level, FU.differing(got, ref))
                if level == 0 and max_merge == 64:
                    print("mixed requests: largest segment", int(ref["agree"].max()), "targets with more than eight members", int((ref["agree"] > 9).sum()))
                    assert (ref["agree"] > 9).sum() > 0
    finally:
        ctx.close()


def test_winners_from_request_128_and_up(ellc):
    """source = (b << 24) | i is a negative int32 from request 128 on, and not -1: such targets have a winner, merge and count like any other."""
    w, h, L = 16, 16, 1
    scenes = [R.make_scene(w, h, seed) for seed in (11, 12, 13)]
    ctx = gpu_problem(ellc, w, h, L, scenes, max_keyframes=160)
    empty = 3
    ctx.keyframe_upload(empty, scenes[0]["kf_image"])
    ctx.keyframe_set_depth(empty, np.zeros((h, w), np.float32), np.full((h, w), -1, np.float32))
    wd = dict(ctx=ctx, intrinsics=scenes[0]["intrinsics"], planes={}, refs={})
    Ts3 = R.scene_transforms(float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0])))
    try:
        slots = [empty] * 130 + [1, 1, 1, 1, 0, 1, 2, 0, 1, 2]
        Ts = np.concatenate([np.tile(IDENTITY, (130, 1)), Ts3[[1, 1, 1, 1, 0, 1, 2, 0, 1, 2]]])
        for max_merge in (64, 2, 0):
            ref = reference(wd, slots, 0, Ts, FILTERS[0], max_merge=max_merge)
            won = ref["depth"] > 0
            # conditions of the test: every winner comes from request 130 and up, and targets fuse
            assert won.sum() > 20 and (ref["source"][won] < -1).all() and (((ref["source"][won].astype(np.int64) & 0xffffffff) >> 24) >= 130).all()
            assert ref["n_valid"] == int(won.sum()) and (ref["merged"][won] >= 1).all() and (ref["merged"][~won] == 0).all()
            if max_merge:
                assert ref["n_fused"] > 0 and (ref["merged"] >= 3).sum() > 0
            got = ctx.fuse_depth(slots, Ts, max_merge=max_merge, **fkw(FILTERS[0]))
            assert FU.planes_equal(got, ref), (max_merge, FU.differing(got, ref), got["n_valid"], ref["n_valid"], got["n_fused"], ref["n_fused"])
            assert got["n_valid"] == ctx.render_depth(slots, Ts, **fkw(FILTERS[0]))["n_valid"]
    finally:
        ctx.close()


def test_zero_variance(world64):
    ctx, w, h = world64["ctx"], world64["w"], world64["h"]
    depth = np.full((h, w), 2.0, np.float32)
    var = np.full((h, w), 1.0 / 64, np.float32)
    var[:, : w // 2] = 0.0
    ctx.keyframe_set_depth(SPARE_SLOT, depth, var)
    world64["planes"].pop((SPARE_SLOT, 0), None)
    got = ctx.fuse_depth([SPARE_SLOT, SPARE_SLOT], [IDENTITY, IDENTITY], **fkw(FILTERS[0]))
    ref = reference(world64, [SPARE_SLOT, SPARE_SLOT], 0, [IDENTITY, IDENTITY], FILTERS[0])
    assert FU.planes_equal(got, ref), FU.differing(got, ref)
    assert got["n_valid"] == w * h and (got["agree"] == 2).all() and (got["source"] == np.arange(w * h).reshape(h, w)).all()
    zero = var == 0
    assert (got["merged"][zero] == 1).all() and (got["var"][zero] == 0).all()           # skipped for s == 0, although it agrees
    assert (got["merged"][~zero] == 2).all() and (got["var"][~zero] == np.float32(1.0 / 128)).all()   # 1 / (64 + 64), exactly
    assert (got["depth"] == 2.0).all() and got["n_fused"] == int((~zero).sum())
    assert ref["stats"]["skipped"][zero].all() and not ref["stats"]["skipped"][~zero].any()


def test_a_second_call_and_a_call_behind_a_batch_give_the_same_bytes(ellc):
    wd = make_world(ellc, "64x48", max_batch=3, max_frames=3)
    ctx = wd["ctx"]
    try:
        slots, Ts = [2, 0, 1, 0], wd["Ts"][[1, 2, 0, 1]]
        a = ctx.fuse_depth(slots, Ts, **fkw(FILTERS[1]))
        b = ctx.fuse_depth(slots, Ts, **fkw(FILTERS[1]))
        assert a["n_fused"] > 0 and not same_bytes(a, b) and (a["n_valid"], a["n_fused"]) == (b["n_valid"], b["n_fused"])
        assert FU.planes_equal(a, reference(wd, slots, 0, Ts, FILTERS[1]))
        before = [ctx.keyframe_depth_level(s, l) for s in range(3) for l in range(wd["L"])]
        plain = ctx.align([0, 1, 2], [0, 1, 2])
        ctx.align_enqueue([0, 1, 2], [0, 1, 2])
        c = ctx.fuse_depth(slots, Ts, **fkw(FILTERS[1]))
        fetched = ctx.align_fetch(3)
        for x, y in zip(plain, fetched):
            assert x.tobytes() == y.tobytes()
        assert not same_bytes(a, c) and (a["n_valid"], a["n_fused"]) == (c["n_valid"], c["n_fused"])
        after = [ctx.keyframe_depth_level(s, l) for s in range(3) for l in range(wd["L"])]   # without a destination the call only reads
        for (d0, v0), (d1, v1) in zip(before, after):
            assert d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", ["64x48", "23x17"])
def test_both_arithmetic_modes_give_the_same_bytes(ellc, shape):
    exact = make_world(ellc, shape, arith=ellc.ARITH_EXACT)
    fast = make_world(ellc, shape, arith=ellc.ARITH_FAST, grid_batch=4)
    try:
        for level in range(exact["L"]):
            a = exact["ctx"].fuse_depth([0, 1, 2], exact["Ts"], level=level, **fkw(FILTERS[0]))
            b = fast["ctx"].fuse_depth([0, 1, 2], fast["Ts"], level=level, **fkw(FILTERS[0]))
            assert a["n_valid"] > 0 and FU.planes_equal(a, b)
            assert FU.planes_equal(b, reference(fast, [0, 1, 2], level, fast["Ts"], FILTERS[0]))
    finally:
        exact["ctx"].close(); fast["ctx"].close()


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


def slots_equal(a, b, slot, L, ellc, frame=0):
    """The slot level by level, and one alignment against it in both modes."""
    for level in range(L):
        (da, va), (db, vb) = a.keyframe_depth_level(slot, level), b.keyframe_depth_level(slot, level)
        assert da.tobytes() == db.tobytes() and va.tobytes() == vb.tobytes(), level
    for mode in (ellc.MODE_FCA, ellc.MODE_ICA):
        ra, rb = a.align([slot], [frame], mode=mode), b.align([slot], [frame], mode=mode)
        for x, y in zip(ra, rb):
            assert x.tobytes() == y.tobytes(), mode


@pytest.mark.parametrize("kind", ["semi-dense", "dense"])
def test_destination_slot_is_what_set_depth_would_leave(ellc, kind):
    w, h, L = SHAPES["64x48"]
    if kind == "dense":
        scenes = dense_scenes(w, h)
        Ts = np.stack([IDENTITY] * 3)
    else:
        scenes = [R.make_scene(w, h, seed) for seed in (11, 12, 13)]
        Ts = R.scene_transforms(float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0])))
    assert np.array_equal(Ts[0], IDENTITY)
    a = gpu_problem(ellc, w, h, L, scenes, max_keyframes=N_SLOTS)
    b = gpu_problem(ellc, w, h, L, scenes, max_keyframes=N_SLOTS)
    try:
        for ctx in (a, b):
            ctx.keyframe_upload(DST_SLOT, scenes[0]["kf_image"])
        # (i) into a slot that holds an image only
        plain = a.fuse_depth([0, 1], Ts[:2])
        got = a.fuse_depth([0, 1], Ts[:2], dst_slot=DST_SLOT)
        frac = got["n_valid"] / float(w * h)
        print(kind, "(i) valid fraction %.4f" % frac, "fused", got["n_fused"])
        assert (frac >= 0.9) if kind == "dense" else (0.05 < frac < 0.9)
        assert got["n_fused"] > 0 and FU.planes_equal(got, plain)   # the planes do not depend on the destination
        b.keyframe_set_depth(DST_SLOT, got["depth"], got["var"])
        slots_equal(a, b, DST_SLOT, L, ellc)
        d0, v0 = a.keyframe_depth_level(DST_SLOT, 0)
        assert d0.tobytes() == got["depth"].tobytes() and v0.tobytes() == got["var"].tobytes()
        # (ii) the destination among the sources: slot 0 fused with the others into itself
        plain = a.fuse_depth([0, 1, 2], Ts)
        got = a.fuse_depth([0, 1, 2], Ts, dst_slot=0)
        frac = got["n_valid"] / float(w * h)
        print(kind, "(ii) valid fraction %.4f" % frac, "fused", got["n_fused"])
        assert (frac >= 0.9) if kind == "dense" else (0.05 < frac < 0.9)
        assert got["n_fused"] > 0 and FU.planes_equal(got, plain)   # every kernel read slot 0 before the planes were copied into it
        b.keyframe_set_depth(0, got["depth"], got["var"])
        slots_equal(a, b, 0, L, ellc)
        d0, v0 = a.keyframe_depth_level(0, 0)
        assert d0.tobytes() == got["depth"].tobytes() and v0.tobytes() == got["var"].tobytes()
        # the fused slot is a source of the next call like any other
        ra, rb = a.fuse_depth([0, 1], Ts[[0, 0]], level=1), b.fuse_depth([0, 1], Ts[[0, 0]], level=1)
        assert ra["n_valid"] > 0 and FU.planes_equal(ra, rb)
    finally:
        a.close(); b.close()


def raw_call(ctx, ellc, slots, T, level=0, flt=(0.0, 0, 1.0, 1), agree_k2=1.0, max_merge=64, dst=-1, null=None, B=None):
    """The status of ellc_keyframe_fuse_depth, not raised. null: which pointer argument to pass as NULL."""
    kf = np.ascontiguousarray(slots, np.int32).reshape(-1)
    B = kf.size if B is None else B
    Tn = np.ascontiguousarray(np.tile(np.asarray(T, np.float32).reshape(-1)[:12], max(kf.size, 1)))
    f = ellc._lib.EllcMapFilter(flt[0], int(flt[1]), flt[2], int(flt[3]))
    h, w = ctx.cfg.height, ctx.cfg.width
    depth = np.zeros((h, w), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    return ctx._l.ellc_keyframe_fuse_depth(ctx.h, B, None if null == "slots" else p(kf), None if null == "T" else p(Tn), int(level),
                                           None if null == "filter" else C.byref(f), C.c_float(agree_k2), int(max_merge), int(dst), p(depth),
                                           None, None, None, None, None, None, None)


def test_refusals_change_nothing(world64, ellc):
    ctx, T, Ts = world64["ctx"], world64["Ts"][1], world64["Ts"]
    good = ctx.fuse_depth([0, 1, 2], Ts)
    before = [ctx.keyframe_depth_level(2, l) for l in range(world64["L"])]
    pose = ctx.align([2], [2])

    def call(slots=(0,), **kw):
        return raw_call(ctx, ellc, list(slots), T, dst=kw.pop("dst", 2), **kw)   # slot 2 is the destination of every refused call

    assert raw_call(ctx, ellc, [0], T) == 0
    assert call(B=0) == BAD_ARG and call(B=-1) == BAD_ARG                                     # B < 1
    assert call(slots=(0, 1, 2, 0, 1, 2, 0, 1)) == BAD_ARG                                    # B > max_keyframes
    assert call(slots=(-1,)) == BAD_ARG and call(slots=(N_SLOTS,)) == BAD_ARG and call(slots=(0, N_SLOTS)) == BAD_ARG
    assert call(level=-1, dst=-1) == BAD_ARG and call(level=world64["L"], dst=-1) == BAD_ARG
    assert call(null="slots") == BAD_ARG and call(null="T") == BAD_ARG and call(null="filter") == BAD_ARG
    assert call(flt=(0.0, -1, 1.0, 1)) == BAD_ARG and call(flt=(0.0, 9, 1.0, 1)) == BAD_ARG and call(flt=(0.0, 0, 1.0, 0)) == BAD_ARG
    assert call(flt=(0.0, 0, -1.0, 1)) == BAD_ARG and call(flt=(0.0, 0, np.inf, 1)) == BAD_ARG and call(flt=(0.0, 0, np.nan, 1)) == BAD_ARG
    assert call(flt=(np.nan, 0, 1.0, 1)) == BAD_ARG
    assert call(agree_k2=-1.0) == BAD_ARG and call(agree_k2=np.inf) == BAD_ARG and call(agree_k2=np.nan) == BAD_ARG
    assert call(dst=-2) == BAD_ARG and call(dst=N_SLOTS) == BAD_ARG
    assert call(level=1) == BAD_ARG                                                           # (iii) a destination takes level 0 only
    assert call(max_merge=-1) == BAD_ARG and call(max_merge=65) == BAD_ARG
    assert call(slots=(IMAGE_ONLY_SLOT,)) == NOT_READY and call(slots=(0, IMAGE_ONLY_SLOT)) == NOT_READY
    with pytest.raises(ellc.EllcError):
        ctx.fuse_depth([IMAGE_ONLY_SLOT], [T])
    with pytest.raises(ellc.EllcError):
        ctx.fuse_depth([0], [T], max_merge=65)
    # the edges of the accepted range, without a destination
    assert raw_call(ctx, ellc, [0], T, flt=(-1.0, 8, 0.0, 1)) == 0 and raw_call(ctx, ellc, [0], T, flt=(np.inf, 0, 1.0, 7)) == 0
    assert raw_call(ctx, ellc, [0], T, agree_k2=0.0) == 0 and raw_call(ctx, ellc, [0], T, max_merge=0) == 0
    # every output pointer may be NULL
    f = ellc._lib.EllcMapFilter(0.0, 0, 1.0, 1)
    kf = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert ctx._l.ellc_keyframe_fuse_depth(ctx.h, 1, p(kf), p(np.ascontiguousarray(T)), 0, C.byref(f), C.c_float(1.0), 64, -1, None, None, None, None,
                                           None, None, None, None) == 0
    # the destination of the refused calls is as it was, and a good call gives the bytes it gave before
    after = [ctx.keyframe_depth_level(2, l) for l in range(world64["L"])]
    for (d0, v0), (d1, v1) in zip(before, after):
        assert d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes()
    again = ctx.align([2], [2])
    for x, y in zip(pose, again):
        assert x.tobytes() == y.tobytes()
    now = ctx.fuse_depth([0, 1, 2], Ts)
    assert not same_bytes(good, now) and FU.planes_equal(now, reference(world64, [0, 1, 2], 0, Ts, FILTERS[0]))
