"""ellc_keyframe_trial_propagate (ABI v18) against tests/trial_propagation_reference.py. The reference is fed the slots' planes as
keyframe_depth_level / image_level / max_gradient read them back (all pinned by their own tests), so the new kernels are the only thing
under test: the integer fields are compared with ==, each double sum within n_interior * 2^-52 * sum |term| of math.fsum, and everything
that must not enter a record (the batch, the split into launches, the arithmetic mode, what is in flight) byte for byte."""
import ctypes as C
import numpy as np
import pytest

import absorb_reference as A
import trial_propagation_reference as R
from helpers import gpu_problem

pytestmark = pytest.mark.gpu

FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
BAD_ARG, NOT_READY = -1, -3
SHAPES = {"64x48": (64, 48, 3), "23x17": (23, 17, 2), "131x67": (131, 67, 3)}   # (width, height, levels); 131x67 is five tiles at level 0
DST_KF, IMAGE_ONLY_SLOT, N_SLOTS = 0, 5, 6   # keyframe slot 0 is the destination, 1..4 the sources, 5 holds an image only
DST_FRAME, EMPTY_FRAME, N_FRAMES = 5, 6, 7   # frame slot 5 holds keyframe 0's image, 6 nothing
SOURCES = [1, 2, 3, 4]


def fkw(flt):
    return dict(max_var=flt[0], min_support=flt[1], support_k2=flt[2], stride=flt[3])


def make_world(ellc, shape, **kw):
    w, h, L = SHAPES[shape]
    sc = A.make_scene(w, h)
    ctx = gpu_problem(ellc, w, h, L, sc["views"], max_keyframes=N_SLOTS, max_frames=N_FRAMES, **kw)
    ctx.keyframe_upload(IMAGE_ONLY_SLOT, sc["views"][1]["kf_image"])
    ctx.frame_upload(DST_FRAME, sc["views"][0]["kf_image"])
    return dict(ctx=ctx, scene=sc, intr=sc["intr"], Ts=sc["Ts"], w=w, h=h, L=L, shape=shape, planes={}, refs={})


def planes_of(world, slot):
    """(depth, var, stored image) of a keyframe slot's level 0, read back once."""
    if slot not in world["planes"]:
        d, v = world["ctx"].keyframe_depth_level(slot, 0)
        img, (rows, cols) = world["ctx"].image_level(True, slot, 0)
        assert d.shape == (rows, cols)
        world["planes"][slot] = (d, v, img)
    return world["planes"][slot]


def dst_planes(world):
    if "dst" not in world["planes"]:
        world["planes"]["dst"] = (world["ctx"].image_level(True, DST_KF, 0)[0], world["ctx"].max_gradient(True, DST_KF)[0])
    return world["planes"]["dst"]


def reference(world, slot, T, flt, photo_gate):
    """Computed once per case and shared; never written to."""
    key = (slot, np.asarray(T, np.float32).tobytes(), tuple(flt), photo_gate)
    if key not in world["refs"]:
        d_img, d_mg = dst_planes(world)
        world["refs"][key] = R.trial(planes_of(world, slot), world["intr"], T, flt, d_img, d_mg, photo_gate=photo_gate)
    return world["refs"][key]


def check(world, got, slots, Ts, flt, photo_gate):
    assert got.dtype.itemsize == 48 and got.shape == (len(slots),)
    for b, slot in enumerate(slots):
        ref = reference(world, slot, Ts[b], flt, photo_gate)
        rec = {k: got[k][b].item() for k in R.FIELDS}
        print(world["shape"], "slot", slot, "filter", flt, "gate", photo_gate, rec, "bounds", R.sum_bound(ref, 0), R.sum_bound(ref, 1))
        for k in R.INT_FIELDS:
            assert rec[k] == ref[k], (k, rec, ref)
        assert abs(rec["sum_r2"] - ref["sum_r2"]) <= R.sum_bound(ref, 0), (rec["sum_r2"], ref["sum_r2"], R.sum_bound(ref, 0))
        assert abs(rec["sum_abs_r"] - ref["sum_abs_r"]) <= R.sum_bound(ref, 1), (rec["sum_abs_r"], ref["sum_abs_r"], R.sum_bound(ref, 1))
        assert (got["reserved"][b] == 0).all()


@pytest.fixture(scope="module", params=list(SHAPES))
def world(request, ellc):
    wd = make_world(ellc, request.param, diag=True)
    yield wd
    wd["ctx"].close()


@pytest.fixture(scope="module")
def world64(ellc):
    wd = make_world(ellc, "64x48", diag=True, max_batch=3)
    yield wd
    wd["ctx"].close()


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_records_against_the_reference(world, flt):
    ctx = world["ctx"]
    wrong = world["Ts"][[2, 3, 0, 1]]   # every source at another source's transform as well: the scores a search has to tell apart
    for photo_gate in (1, 0):
        got = ctx.trial_propagate(SOURCES + SOURCES, [DST_KF] * 8, np.concatenate([world["Ts"], wrong]), dst_is_keyframe=True, photo_gate=photo_gate, **fkw(flt))
        check(world, got, SOURCES + SOURCES, np.concatenate([world["Ts"], wrong]), flt, photo_gate)
        if flt == FILTERS[0] and world["shape"] != "23x17":   # conditions of the test: every class of drop and collisions occur
            for b in range(4):
                assert got["n_kept"][b] >= got["n_in_view"][b] > got["n_interior"][b] > 0 and got["n_low_grad"][b] > 0
                assert got["n_candidates"][b] > got["n_targets"][b] > 0
                assert (got["n_candidates"][b] < got["n_interior"][b]) if photo_gate else (got["n_candidates"][b] == got["n_interior"][b])
                assert not photo_gate or got["n_targets"][b] > got["n_targets"][4 + b]   # the pose shows in the score
            assert int(got["n_kept"][:4].sum()) > int(got["n_in_view"][:4].sum())
        # a frame slot that holds the same image gives the same bytes
        fr = ctx.trial_propagate(SOURCES + SOURCES, [DST_FRAME] * 8, np.concatenate([world["Ts"], wrong]), dst_is_keyframe=False, photo_gate=photo_gate, **fkw(flt))
        assert fr.tobytes() == got.tobytes()


def test_frame_slot_planes_are_the_keyframe_slots(world):
    """The condition of the comparison above: the two destinations hold the same image and the same maxAbsGradient plane."""
    ctx = world["ctx"]
    ctx.trial_propagate([1], [DST_FRAME], world["Ts"][:1])   # builds the frame slot's plane where it is not built
    assert ctx.image_level(False, DST_FRAME, 0)[0].tobytes() == ctx.image_level(True, DST_KF, 0)[0].tobytes()
    assert ctx.max_gradient(False, DST_FRAME)[0].tobytes() == ctx.max_gradient(True, DST_KF)[0].tobytes()


def test_alone_reversed_repeated_and_split_give_the_same_bytes(world):
    ctx, Ts = world["ctx"], world["Ts"]
    flt = FILTERS[1]
    whole = ctx.trial_propagate(SOURCES, [DST_KF] * 4, Ts, dst_is_keyframe=True, **fkw(flt))
    check(world, whole, SOURCES, Ts, flt, 1)
    for b in range(4):
        alone = ctx.trial_propagate([SOURCES[b]], [DST_KF], Ts[b:b + 1], dst_is_keyframe=True, **fkw(flt))
        assert alone.tobytes() == whole[b:b + 1].tobytes(), b
    rev = ctx.trial_propagate(SOURCES[::-1], [DST_KF] * 4, Ts[::-1], dst_is_keyframe=True, **fkw(flt))
    assert rev[::-1].tobytes() == whole.tobytes()
    again = ctx.trial_propagate(SOURCES, [DST_KF] * 4, Ts, dst_is_keyframe=True, **fkw(flt))
    assert again.tobytes() == whole.tobytes()
    rep = ctx.trial_propagate(SOURCES * 3, [DST_KF] * 12, np.tile(Ts, (3, 1)), dst_is_keyframe=True, **fkw(flt))
    assert rep.tobytes() == whole.tobytes() * 3
    # the split into launches (the diagnostic hook forces the group size) does not enter a record
    for group in (0, 1, 3):
        hooked, ms = ctx.profile_trial_propagate(SOURCES * 2, [DST_KF] * 8, np.tile(Ts, (2, 1)), dst_is_keyframe=True, max_group_requests=group, **fkw(flt))
        assert hooked.tobytes() == whole.tobytes() * 2 and ms > 0, group


def test_2048_requests(ellc):
    wd = make_world(ellc, "23x17")
    ctx = wd["ctx"]
    try:
        four = ctx.trial_propagate(SOURCES, [DST_KF] * 4, wd["Ts"], dst_is_keyframe=True)
        check(wd, four, SOURCES, wd["Ts"], FILTERS[0], 1)
        big = ctx.trial_propagate(SOURCES * 512, [DST_KF] * 2048, np.tile(wd["Ts"], (512, 1)), dst_is_keyframe=True)
        assert big.shape == (2048,) and big.tobytes() == four.tobytes() * 512
        small = ctx.trial_propagate(SOURCES, [DST_KF] * 4, wd["Ts"], dst_is_keyframe=True)   # the staging has grown: a small call behind it
        assert small.tobytes() == four.tobytes()
    finally:
        ctx.close()


def test_another_arithmetic_mode_and_a_batch_in_flight_give_the_same_bytes_and_slots_stay(world64, ellc):
    ctx, Ts, L = world64["ctx"], world64["Ts"], world64["L"]
    other = make_world(ellc, "64x48", arith=ellc.ARITH_FAST, grid_batch=4)
    try:
        flt = FILTERS[1]
        before = [ctx.keyframe_depth_level(s, l) for s in range(5) for l in range(L)]
        plain = ctx.align([1, 2, 3], [1, 2, 3])
        a = ctx.trial_propagate(SOURCES, [DST_KF] * 4, Ts, dst_is_keyframe=True, **fkw(flt))
        check(world64, a, SOURCES, Ts, flt, 1)
        b = other["ctx"].trial_propagate(SOURCES, [DST_KF] * 4, other["Ts"], dst_is_keyframe=True, **fkw(flt))
        assert a.tobytes() == b.tobytes()
        ctx.align_enqueue([1, 2, 3], [1, 2, 3])
        c = ctx.trial_propagate(SOURCES, [DST_FRAME] * 4, Ts, dst_is_keyframe=False, **fkw(flt))
        fetched = ctx.align_fetch(3)
        assert c.tobytes() == a.tobytes()
        for x, y in zip(plain, fetched):
            assert x.tobytes() == y.tobytes()
        # the call wrote nothing that belongs to a slot: every level of the depth planes and a later alignment are as before
        after = [ctx.keyframe_depth_level(s, l) for s in range(5) for l in range(L)]
        for (d0, v0), (d1, v1) in zip(before, after):
            assert d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes()
        for x, y in zip(plain, ctx.align([1, 2, 3], [1, 2, 3])):
            assert x.tobytes() == y.tobytes()
    finally:
        other["ctx"].close()


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_n_targets_is_what_an_absorb_into_a_wiped_state_creates(world, flt):
    ctx = world["ctx"]
    wiped = R.wiped_state(world["h"], world["w"])
    ctx.depth_set_keyframe(DST_KF)
    for photo_gate in (1, 0):
        got = ctx.trial_propagate(SOURCES, [DST_KF] * 4, world["Ts"], dst_is_keyframe=True, photo_gate=photo_gate, **fkw(flt))
        for b, slot in enumerate(SOURCES):
            ctx.depth_set_state(wiped)
            st = ctx.depth_absorb([slot], world["Ts"][b:b + 1], params=dict(finalise=0, photo_gate=photo_gate), **fkw(flt))
            assert got["n_targets"][b] == st["n_created"] == st["targets_hit"] == st["n_valid_after"], (b, got[b], st)
            assert [got[k][b] for k in ("n_kept", "n_in_view", "n_interior", "n_candidates")] == [st[k] for k in ("n_kept", "n_in_view", "n_interior", "n_candidates")]


def raw_call(ctx, ellc, out, src=(1,), dst=(DST_KF,), dst_is_kf=1, flt=(0.0, 0, 1.0, 1), photo_gate=1, null=None, B=None):
    """The status of ellc_keyframe_trial_propagate, not raised. null: which pointer argument to pass as NULL."""
    s = np.ascontiguousarray(src, np.int32).reshape(-1)
    d = np.ascontiguousarray(dst, np.int32).reshape(-1)
    B = s.size if B is None else B
    Tn = np.ascontiguousarray(np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), max(s.size, 1)))
    f = ellc._lib.EllcMapFilter(flt[0], int(flt[1]), flt[2], int(flt[3]))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    return ctx._l.ellc_keyframe_trial_propagate(ctx.h, B, None if null == "src" else ptr(s), int(dst_is_kf), None if null == "dst" else ptr(d),
                                                None if null == "T" else ptr(Tn), None if null == "filter" else C.byref(f), int(photo_gate),
                                                None if null == "out" else ptr(out))


def test_refusals_leave_out_untouched(world64, ellc):
    ctx = world64["ctx"]
    out = np.zeros(4, np.dtype(ellc._lib.EllcTrialPropagation))
    out.view(np.uint8)[:] = 0xA5
    filled = out.tobytes()

    def call(**kw):
        return raw_call(ctx, ellc, out, **kw)

    assert call(B=0) == BAD_ARG and call(B=-1) == BAD_ARG and call(B=2049) == BAD_ARG
    assert call(src=(-1,)) == BAD_ARG and call(src=(N_SLOTS,)) == BAD_ARG and call(src=(1, N_SLOTS), dst=(0, 0)) == BAD_ARG
    assert call(dst=(-1,)) == BAD_ARG and call(dst=(N_SLOTS,)) == BAD_ARG
    assert call(dst=(N_FRAMES,), dst_is_kf=0) == BAD_ARG and call(dst=(N_SLOTS,), dst_is_kf=0) == NOT_READY   # frame slot 6 exists (empty), keyframe slot 6 does not
    assert call(null="src") == BAD_ARG and call(null="dst") == BAD_ARG and call(null="T") == BAD_ARG and call(null="filter") == BAD_ARG
    assert call(null="out") == BAD_ARG
    assert call(flt=(0.0, -1, 1.0, 1)) == BAD_ARG and call(flt=(0.0, 9, 1.0, 1)) == BAD_ARG and call(flt=(0.0, 0, 1.0, 0)) == BAD_ARG
    assert call(flt=(0.0, 0, -1.0, 1)) == BAD_ARG and call(flt=(0.0, 0, np.inf, 1)) == BAD_ARG and call(flt=(0.0, 0, np.nan, 1)) == BAD_ARG
    assert call(flt=(np.nan, 0, 1.0, 1)) == BAD_ARG
    assert call(photo_gate=2) == BAD_ARG and call(photo_gate=-1) == BAD_ARG and call(dst_is_kf=2) == BAD_ARG and call(dst_is_kf=-1) == BAD_ARG
    assert call(src=(IMAGE_ONLY_SLOT,)) == NOT_READY and call(src=(1, IMAGE_ONLY_SLOT), dst=(0, 0)) == NOT_READY
    assert call(dst=(EMPTY_FRAME,), dst_is_kf=0) == NOT_READY
    with pytest.raises(ellc.EllcError):
        ctx.trial_propagate([IMAGE_ONLY_SLOT], [DST_KF], world64["Ts"][:1], dst_is_keyframe=True)
    assert out.tobytes() == filled
    # a destination needs an image only, and a good call gives what the reference gives
    assert call(src=(1,), dst=(IMAGE_ONLY_SLOT,)) == 0 and out[0]["n_kept"] > 0 and out[1:].tobytes() == filled[48:]
    got = ctx.trial_propagate(SOURCES, [DST_KF] * 4, world64["Ts"], dst_is_keyframe=True)
    check(world64, got, SOURCES, world64["Ts"], FILTERS[0], 1)
