"""ellc_keyframe_cull_depth (ABI v22) against tests/cull_depth_reference.py, on the world and shapes of tests/test_gpu_sim3.py (whose
helpers are used, not copied). The reference is fed the slots' planes as keyframe_depth_level / image_level read them back (pinned by
their own tests), so the new kernel and the host code around it are the only thing under test: the five planes are compared as bytes
and every stat with ==."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cull_depth_reference as Q
import refine_depth_reference as R
import test_gpu_sim3 as G
from egomotion_with_local_loop_closures_amd import synth
from helpers import gpu_problem
from test_gpu_refine_depth import NOWHERE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FILTERS, LIGHTS, SHAPES, fkw = R.FILTERS, R.LIGHTS, G.SHAPES, G.fkw
BAD_ARG, NOT_READY = G.BAD_ARG, G.NOT_READY
K_SLOT = 0
# the image-only slot and the all-zero-depth slot among the views
ODD_VIEWS = [(1, 1), (G.IMAGE_ONLY_SLOT, 2), (G.ZERO_SLOT, 1), (2, 2)]


def call_args(world, vl):
    return [s for s, _ in vl], np.stack([world["Ts"][t] for _, t in vl])


def view_of(world, slot, level, as_kf):
    """(depth, var, stored image) of a view as the call reads it: no depth planes for a frame slot or for the image-only slot."""
    if not as_kf:
        return (None, None, world["ctx"].image_level(False, slot, level)[0])
    if slot == G.IMAGE_ONLY_SLOT:
        return (None, None, world["ctx"].image_level(True, slot, level)[0])
    return G.planes_of(world, slot, level)


def reference(world, level, vl, as_kf, flt, light, params):
    """cull_depth_reference.cull of one call on the planes read back from the slots, computed once per world and left unchanged."""
    key = ("cull", level, tuple(vl), as_kf, tuple(flt), None if light is None else tuple(light), tuple(sorted(params.items())))
    if key not in world["refs"]:
        slots, Ts = call_args(world, vl)
        views = {s: view_of(world, s, level, as_kf) for s in set(slots)}
        world["refs"][key] = Q.cull(G.planes_of(world, K_SLOT, level), [views[s] for s in slots], G.intr_of(world, level), Ts,
                                    None if light is None else [light] * len(vl), flt, params)
    return world["refs"][key]


def check_against(got, ref, what):
    """The five planes as bytes, every stat with ==."""
    for name in Q.PLANES:
        assert got[name].dtype == ref[name].dtype and got[name].shape == ref[name].shape and got[name].tobytes() == ref[name].tobytes(), (what, name)
    for k in Q.INT_FIELDS:
        assert int(got["stats"][k]) == ref[k], (what, k, got["stats"][k], ref[k])
    assert sorted(got["stats"]) == sorted(Q.INT_FIELDS)


def same_result(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in Q.PLANES) and a["stats"] == b["stats"]


def run(world, vl, light=None, level=0, as_kf=True, flt=FILTERS[0], params=None, ctx=None, **kw):
    slots, Ts = call_args(world, vl)
    params = Q.case_params(len(vl)) if params is None else params
    return (ctx or world["ctx"]).cull_depth(K_SLOT, slots, Ts, None if light is None else [light] * len(vl), level=level, views_are_keyframes=as_kf,
                                            params=params, **fkw(flt), **kw)


@pytest.fixture(scope="module", params=list(SHAPES))
def world(request, ellc):
    wd = G.make_world(ellc, request.param)
    yield wd
    wd["ctx"].close()


@pytest.fixture(scope="module")
def world64(ellc):
    wd = G.make_world(ellc, "64x48")
    yield wd
    wd["ctx"].close()


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
@pytest.mark.parametrize("light", LIGHTS, ids=["unit", "dim"])
def test_parity_with_the_reference(world, flt, light):
    """Every level, views as keyframe slots and as frame slots, B of 1, 3 and 64 (slots repeated), the image-only slot and the all-zero
    depth among the views, photo_k 0, a non-default parameter set, a NULL light."""
    seen, culled = np.zeros(6, np.int64), 0
    for level in range(world["L"]):
        for as_kf in (True, False):
            for B in (1, 3, 64):
                vl, params = R.view_list(B), Q.case_params(B)
                got = run(world, vl, light, level, as_kf, flt, params)
                what = "%s level %d filter %s light %s views %s B %d" % (world["shape"], level, flt, light, "kf" if as_kf else "frames", B)
                ref = reference(world, level, vl, as_kf, flt, light, params)
                check_against(got, ref, what)
                seen += np.bincount(ref["status"].reshape(-1), minlength=6)
                culled += ref["n_culled_free_space"] + ref["n_culled_unsupported"] + ref["n_culled_photo"]
        params = Q.case_params(len(ODD_VIEWS))
        check_against(run(world, ODD_VIEWS, light, level, True, flt, params), reference(world, level, ODD_VIEWS, True, flt, light, params),
                      "odd views, level %d" % level)
        for params in (Q.case_params(3, photo_k=0.0), Q.case_params(3, photo_k=-1.0), dict(Q.OTHER_PARAMS)):
            check_against(run(world, R.view_list(3), light, level, True, flt, params), reference(world, level, R.view_list(3), True, flt, light, params),
                          "level %d params %s" % (level, params))
    print(world["shape"], flt, light, "status counts %s, culled %d" % (seen.tolist(), culled))
    assert culled > 0 and seen[Q.KEPT] > 0
    if light == LIGHTS[0]:   # a NULL light is (1, 0)
        params = Q.case_params(3)
        check_against(run(world, R.view_list(3), None, 0, True, flt, params), reference(world, 0, R.view_list(3), True, flt, light, params), "NULL light")


def test_sums_equal_the_pinned_consistency_call(world):
    """B = 1, a keyframe view, photo_k 0: sum_agree / sum_in_front / sum_behind are n_agree / n_in_front / n_behind of
    ellc_keyframe_depth_consistency(K, view, T) under the same filter and agree_k2, n_kept its n_kept; every level of the shape."""
    ctx = world["ctx"]
    judged = 0
    for level in range(world["L"]):
        for flt in FILTERS:
            for agree_k2 in (1.0, 0.25):
                for slot, t in R.BASE_VIEWS:
                    T = world["Ts"][t]
                    got = ctx.cull_depth(K_SLOT, [slot], [T], level=level, params=Q.case_params(1, photo_k=0.0, agree_k2=agree_k2), **fkw(flt))
                    rec = ctx.depth_consistency([K_SLOT], [slot], [T], level=level, agree_k2=agree_k2, **fkw(flt))[0]
                    what = (level, flt, agree_k2, slot, t)
                    assert got["stats"]["n_kept"] == int(rec["n_kept"]), what
                    assert got["stats"]["sum_agree"] == int(rec["n_agree"]), what
                    assert got["stats"]["sum_in_front"] == int(rec["n_in_front"]), what
                    assert got["stats"]["sum_behind"] == int(rec["n_behind"]), what
                    assert got["stats"]["sum_photo"] == 0 and not got["photo"].any()
                    judged += int(rec["n_overlap"])
    assert judged > 0


def test_order_a_blind_view_and_a_second_call_change_no_byte(world):
    ctx = world["ctx"]
    for level in range(world["L"]):
        for as_kf in (True, False):
            # (the two odd slots are keyframe slots: the context has three frame slots)
            slots, Ts = call_args(world, R.view_list(6)[:4] + ODD_VIEWS[1:3] if as_kf else R.view_list(6))
            kw = dict(level=level, views_are_keyframes=as_kf, **fkw(FILTERS[1]))
            first = ctx.cull_depth(K_SLOT, slots, Ts, [LIGHTS[1]] * 6, **kw)
            assert same_result(first, ctx.cull_depth(K_SLOT, slots, Ts, [LIGHTS[1]] * 6, **kw)), (level, as_kf)
            assert same_result(first, ctx.cull_depth(K_SLOT, slots[::-1], Ts[::-1], [LIGHTS[1]] * 6, **kw)), (level, as_kf)
            # a seventh view in which no point of K has a candidate, at the end and in the middle
            blind = ctx.cull_depth(K_SLOT, slots + [1], np.concatenate([Ts, NOWHERE[None]]), [LIGHTS[1]] * 7, **kw)
            assert same_result(first, blind), (level, as_kf)
            mid = ctx.cull_depth(K_SLOT, slots[:1] + [2] + slots[1:], np.concatenate([Ts[:1], NOWHERE[None], Ts[1:]]), [LIGHTS[1]] * 7, **kw)
            assert same_result(first, mid), (level, as_kf)
        assert first["stats"]["n_kept"] > 0


@pytest.mark.parametrize("shape", ["64x48", "131x67"])
def test_another_configuration_gives_the_same_bytes(ellc, shape):
    one = G.make_world(ellc, shape, arith=ellc.ARITH_EXACT)
    two = G.make_world(ellc, shape, arith=ellc.ARITH_FAST, grid_batch=4, max_batch=7)
    try:
        for level in range(one["L"]):
            a = run(one, R.view_list(3), LIGHTS[1], level)
            b = run(two, R.view_list(3), LIGHTS[1], level)
            assert a["stats"]["n_kept"] > 0 and same_result(a, b), level
    finally:
        one["ctx"].close(); two["ctx"].close()


def snapshot(world, slots=range(4)):
    ctx = world["ctx"]
    out = []
    for s in slots:
        for l in range(world["L"]):
            d, v = ctx.keyframe_depth_level(s, l)
            out.append(d.tobytes() + v.tobytes() + ctx.image_level(True, s, l)[0].tobytes())
    return out


def test_destination_slot(ellc):
    """dst == K at level 0: the slot's depth and variance on every level afterwards are what a twin context holds after keyframe_set_depth
    with the returned planes; dst == another slot likewise, K untouched; dst == -1: every plane of every slot untouched. A refine_depth
    behind the call sees the culled map."""
    one, twin = G.make_world(ellc, "64x48"), G.make_world(ellc, "64x48")
    try:
        vl = R.view_list(3)
        slots, Ts = call_args(one, vl)
        before = snapshot(one)
        for dst in (2, K_SLOT):   # a view first, then K itself (the views' maps are inputs: the second call sees the first's store)
            unchanged = snapshot(one)
            res = run(one, vl, LIGHTS[1])
            culled = (res["status"] >= Q.CULLED_FREE_SPACE) & (res["status"] <= Q.CULLED_PHOTO)
            assert culled.any() and (res["status"] == Q.KEPT).any() and snapshot(one) == unchanged
            got = run(one, vl, LIGHTS[1], dst_slot=dst)
            assert same_result(got, res), dst
            twin["ctx"].keyframe_set_depth(dst, res["depth"], res["var"])
            for level in range(one["L"]):
                a, b = one["ctx"].keyframe_depth_level(dst, level), twin["ctx"].keyframe_depth_level(dst, level)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (dst, level)
            assert one["ctx"].keyframe_depth_level(dst, 0)[0].tobytes() == res["depth"].tobytes()
        after = snapshot(one)
        assert after[one["L"]:2 * one["L"]] == before[one["L"]:2 * one["L"]] and after[3 * one["L"]:] == before[3 * one["L"]:]   # slots 1 and 3
        # the refinement behind the call sees the culled map: no culled pixel takes part, and the twin answers alike
        a = one["ctx"].refine_depth(K_SLOT, [1], Ts[:1], params=dict(min_views=1))
        b = twin["ctx"].refine_depth(K_SLOT, [1], Ts[:1], params=dict(min_views=1))
        assert all(a[k].tobytes() == b[k].tobytes() for k in R.PLANES) and a["stats"] == b["stats"]
        assert not a["status"][culled].any() and (a["depth"][culled] == 0).all() and a["stats"]["n_kept"] == res["stats"]["n_kept"] - int(culled.sum())
        src, dstn, T3 = [0, 2], [1, 1], np.stack([one["Ts"][1], one["Ts"][1]])
        assert one["ctx"].sim3_step(src, dstn, T3).tobytes() == twin["ctx"].sim3_step(src, dstn, T3).tobytes()
    finally:
        one["ctx"].close(); twin["ctx"].close()


PATTERN = 0xA5
GOOD = (1.0, 16.0, 3.0, 1, 2, 1, 2)


def raw_call(ctx, ellc, n, kf=K_SLOT, level=0, slots=(1, 2), T=None, light=(1.0, 0.0, 1.0, 0.0), flt=(0.0, 0, 1.0, 1), params=GOOD, dst=-1, as_kf=1,
             B=None, null=None):
    """(status, every output untouched?) of ellc_keyframe_cull_depth, not raised. null: which pointer argument to pass as NULL."""
    s = np.ascontiguousarray(slots, np.int32).reshape(-1)
    B = s.size if B is None else B
    Tn = np.ascontiguousarray(np.tile(np.asarray(G.IDENTITY, F), max(s.size, 1)) if T is None else T, F).reshape(-1)
    li = np.ascontiguousarray(np.resize(np.asarray(light, F), 2 * max(s.size, 1)))
    f = ellc._lib.EllcMapFilter(flt[0], int(flt[1]), flt[2], int(flt[3]))
    prm = ellc._lib.EllcCullParams(*params)
    outs = dict(depth=np.full(4 * n, PATTERN, np.uint8), var=np.full(4 * n, PATTERN, np.uint8), votes=np.full(4 * n, PATTERN, np.uint8),
                photo=np.full(n, PATTERN, np.uint8), status=np.full(n, PATTERN, np.uint8), stats=np.full(64, PATTERN, np.uint8))
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    st = ctx._l.ellc_keyframe_cull_depth(ctx.h, int(kf), int(level), int(B), int(as_kf), None if null == "slots" else p(s), None if null == "T" else p(Tn),
                                         None if null == "light" else p(li), None if null == "filter" else C.byref(f),
                                         None if null == "params" else C.byref(prm), int(dst), p(outs["depth"]), p(outs["var"]), p(outs["votes"]),
                                         p(outs["photo"]), p(outs["status"]), p(outs["stats"]))
    return st, all(bool((a == PATTERN).all()) for a in outs.values())


def test_refused_calls_write_nothing_and_touch_no_slot(world64, ellc):
    ctx = world64["ctx"]
    n = world64["w"] * world64["h"]
    before = snapshot(world64)

    def refused(code, **kw):
        st, untouched = raw_call(ctx, ellc, n, **kw)
        assert st == code and untouched, (st, code, untouched, kw)

    def accepted(**kw):
        st, untouched = raw_call(ctx, ellc, n, **kw)
        assert st == 0 and not untouched, (st, kw)

    accepted(); accepted(null="light"); accepted(as_kf=0)
    for null in ("slots", "T", "filter", "params"):
        refused(BAD_ARG, null=null)
    refused(BAD_ARG, B=0); refused(BAD_ARG, B=-1); refused(BAD_ARG, slots=[1] * 65)                      # B outside 1..64
    accepted(slots=[1] * 64)
    refused(BAD_ARG, as_kf=2); refused(BAD_ARG, as_kf=-1)
    refused(BAD_ARG, level=-1); refused(BAD_ARG, level=world64["L"])
    refused(BAD_ARG, flt=(0.0, -1, 1.0, 1)); refused(BAD_ARG, flt=(0.0, 9, 1.0, 1)); refused(BAD_ARG, flt=(0.0, 0, 1.0, 0))   # the filter errors of map_points
    refused(BAD_ARG, flt=(0.0, 0, -1.0, 1)); refused(BAD_ARG, flt=(0.0, 0, np.inf, 1)); refused(BAD_ARG, flt=(0.0, 0, np.nan, 1))
    refused(BAD_ARG, flt=(np.nan, 0, 1.0, 1))
    for bad in (np.nan, np.inf, -np.inf):   # a value of T or of the light that is not finite, in the first view and in the last
        for k in (0, 3, 12 + 11):
            T = np.tile(np.asarray(G.IDENTITY, F), 2); T[k] = bad
            refused(BAD_ARG, T=T)
        for k in range(4):
            li = np.array([1, 0, 1, 0], F); li[k] = bad
            refused(BAD_ARG, light=li)
    # agree_k2 negative or not finite, sigma_i2 <= 0 or not finite, photo_k not finite (any finite photo_k is accepted)
    for bad in (np.nan, np.inf, -np.inf, -1.0):
        refused(BAD_ARG, params=(bad,) + GOOD[1:])
    for bad in (np.nan, np.inf, -np.inf, -1.0, 0.0):
        refused(BAD_ARG, params=GOOD[:1] + (bad,) + GOOD[2:])
    for bad in (np.nan, np.inf, -np.inf):
        refused(BAD_ARG, params=GOOD[:2] + (bad,) + GOOD[3:])
    accepted(params=(0.0, 1e-3, -5.0, 1, 1, 1, 1)); accepted(params=(1.0, 16.0, 0.0, 2, 2, 2, 2))
    for k in range(3, 7):   # the four counts: 1..B with B = 2
        for bad in (0, 3, -1):
            refused(BAD_ARG, params=GOOD[:k] + (bad,) + GOOD[k + 1:])
    refused(BAD_ARG, params=GOOD[:4] + (2,) + GOOD[5:], slots=(1,))                                      # min_judged 2 with one view
    refused(BAD_ARG, dst=-2); refused(BAD_ARG, dst=G.N_SLOTS); refused(BAD_ARG, dst=0, level=1)          # the destination errors of the fusion
    refused(BAD_ARG, kf=-1); refused(BAD_ARG, kf=G.N_SLOTS)                                              # K out of range
    refused(BAD_ARG, slots=(-1, 1)); refused(BAD_ARG, slots=(1, G.N_SLOTS)); refused(BAD_ARG, slots=(1, G.N_SLOTS), as_kf=0)   # a view out of range
    # the order: what comes first in the header's list is what is reported (the message names it)
    for kw, word in ((dict(null="params", B=0), "null"), (dict(B=0, as_kf=2), "B out"), (dict(as_kf=2, level=-1), "views_are_keyframes"),
                     (dict(level=-1, flt=(0.0, 9, 1.0, 1)), "level"), (dict(flt=(0.0, 9, 1.0, 1), params=(-1.0,) + GOOD[1:]), "filter"),
                     (dict(params=(-1.0,) + GOOD[1:3] + (0, 2, 1, 2)), "parameters"), (dict(params=GOOD[:3] + (0, 2, 1, 2), dst=-2), "count"),
                     (dict(dst=-2, kf=-1), "destination"), (dict(kf=-1, slots=(G.IMAGE_ONLY_SLOT, 1)), "slot index")):
        st, untouched = raw_call(ctx, ellc, n, **kw)
        message = ctx._l.ellc_last_error(ctx.h).decode()
        assert st == BAD_ARG and untouched and word in message, (kw, word, message)
    # K without depth or without anything; a view without an image (slot 4 of the frames was never uploaded)
    refused(NOT_READY, kf=G.IMAGE_ONLY_SLOT)
    accepted(slots=(G.IMAGE_ONLY_SLOT, 1))                                                              # a keyframe view needs no depth
    fresh = gpu_problem(ellc, world64["w"], world64["h"], world64["L"], world64["scenes"][:1], max_keyframes=3, max_frames=3)
    try:
        for kw in (dict(kf=1), dict(slots=(0, 1)), dict(slots=(0, 2), as_kf=0)):
            st, untouched = raw_call(fresh, ellc, n, **kw)
            assert st == NOT_READY and untouched, kw
        with pytest.raises(ellc.EllcError):
            fresh.cull_depth(1, [0, 0], [G.IDENTITY] * 2)
    finally:
        fresh.close()
    # an all-zero depth is a map without hypotheses, not an error
    zero = ctx.cull_depth(G.ZERO_SLOT, [1, 2], [G.IDENTITY] * 2)
    assert zero["stats"]["n_kept"] == 0 and not zero["status"].any() and not zero["depth"].any() and (zero["var"] == -1).all()
    # K among the views at the identity agrees with itself
    own = ctx.cull_depth(K_SLOT, [K_SLOT], [G.IDENTITY], params=Q.case_params(1, photo_k=0.0))
    assert own["stats"]["sum_agree"] == own["stats"]["n_kept"] == own["stats"]["n_retained"] > 0
    # the context still answers as before, and no plane of any slot has changed
    check_against(run(world64, R.view_list(3), LIGHTS[0]), reference(world64, 0, R.view_list(3), True, FILTERS[0], LIGHTS[0], Q.case_params(3)),
                  "after the refusals")
    assert snapshot(world64) == before


def test_profile_twin_gives_the_same_result(ellc):
    wd = G.make_world(ellc, "64x48", diag=True)
    try:
        slots, Ts = call_args(wd, R.view_list(3))
        plain = wd["ctx"].cull_depth(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, **fkw(FILTERS[0]))
        timed, ms = wd["ctx"].profile_cull_depth(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, **fkw(FILTERS[0]))
        assert same_result(plain, timed) and ms > 0 and plain["stats"]["n_kept"] > 0
    finally:
        wd["ctx"].close()


@pytest.mark.parametrize("case", [(64, 48, 3), (131, 67, 3)], ids=["64x48", "131x67"])
def test_recovery_carries_over(ellc, case):
    """The library's planes for the two recovery inputs of tests/test_cull_depth_reference.py equal the reference's byte for byte, so the
    CPU result (at least 75 % of the spoilt hypotheses culled, at most 1 % of the others) carries over; asserted here on the library's
    planes too."""
    w, h, L = case
    scenes, Ts, _ = R.shared_world(w, h, 5, 11, depth_noise=0.02)
    depth, spoilt, clean = Q.spoil(scenes[0]["depth0"], scenes[0]["var0"])
    ctx = gpu_problem(ellc, w, h, L, scenes)
    try:
        ctx.keyframe_set_depth(0, depth, scenes[0]["var0"])
        world = dict(ctx=ctx, planes={}, intrinsics=scenes[0]["intrinsics"])
        views = list(range(1, 5))
        got = ctx.cull_depth(0, views, Ts)
        kf = G.planes_of(world, 0, 0)
        assert kf[0].tobytes() == depth.tobytes()
        ref = Q.cull(kf, [G.planes_of(world, s, 0) for s in views], G.intr_of(world, 0), Ts, None, Q.NO_FILTER)
        check_against(got, ref, "recovery %dx%d" % (w, h))
        n_spoilt, culled_spoilt, n_clean, culled_clean = Q.recovery_figures(got, spoilt, clean)
        print("%dx%d: spoilt %d, culled %d; others %d, culled %d; stats %s" % (w, h, n_spoilt, culled_spoilt, n_clean, culled_clean, got["stats"]))
        assert culled_spoilt >= 0.75 * n_spoilt and culled_clean <= 0.01 * n_clean, (culled_spoilt, n_spoilt, culled_clean, n_clean)
    finally:
        ctx.close()


def test_driver_cull_matches_file(tmp_path):
    """ellc_main --match-sim3 S --match-light --cull-matches C on the 33-frame loop-closure sequence of tests/test_gpu_driver.py: one
    line per push that had candidates, thirteen integer fields that add up. Without the flag (the options the driver had before) no such
    file appears and the run is what it was: the vote touches the ring's copy alone, so the tracking outputs of both runs are
    byte-identical, as are the Sim(3) lines of the first push with candidates, which ran before any vote; and --cull-matches without
    --match-sim3 is a usage error."""
    W, H, n_frames = 160, 120, 33
    rng = np.random.default_rng(7)
    tex = synth.value_noise_texture(W, H, rng)
    idepth = synth.smooth_field(W, H, rng, cell=64, lo=0.7, hi=1.3)
    fx, fy, cx, cy = synth.default_intrinsics(W, H)
    step = np.array([0.0004, -0.0003, 0.0002, 0.0015, 0.0006, -0.0004])
    frames = [tex] + [synth.render_current(tex, idepth, synth.se3_exp(step * n), fx, fy, cx, cy) for n in range(1, n_frames)]
    raw = tmp_path / "frames.raw"
    raw.write_bytes(b"".join(np.ascontiguousarray(f, np.uint8).tobytes() for f in frames))
    exe = os.path.join(ROOT, "egomotion_with_local_loop_closures_amd", "csrc", "ellc_main")
    plain = tmp_path / "plain"; plain.mkdir()
    flagged = tmp_path / "flagged"; flagged.mkdir()
    base = [exe, str(raw), str(W), str(H), str(n_frames)]
    s_plain, s_flagged, cfile = tmp_path / "sim3_plain.txt", tmp_path / "sim3_flagged.txt", tmp_path / "cull.txt"
    r = subprocess.run(base + [str(plain), "LC", "--match-sim3", str(s_plain), "--match-light"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()
    r = subprocess.run(base + [str(flagged), "LC", "--match-sim3", str(s_flagged), "--match-light", "--cull-matches", str(cfile)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()
    assert sorted(p.name for p in plain.iterdir()) == sorted(p.name for p in flagged.iterdir())
    for name in ("poses_orig.txt", "matchframes.txt"):
        assert (plain / name).read_bytes() == (flagged / name).read_bytes(), name
    matches = (flagged / "matchframes_globalopt.txt").read_text().strip().split("\n")
    pushes = []
    for m in matches:
        if not pushes or pushes[-1][0] != m.split(" ")[0]:
            pushes.append([m.split(" ")[0], 0])
        pushes[-1][1] += 1
    lines = cfile.read_text().strip().split("\n")
    assert len(pushes) >= 2 and len(lines) == len(pushes)
    judged = 0
    for (frame_id, n_cand), l in zip(pushes, lines):
        c = l.split(" ")
        print(l)
        assert len(c) == 13 and c[0] == frame_id and int(c[1]) == min(n_cand, 64)
        v = [int(x) for x in c[1:]]
        views, n_kept = v[0], v[1]
        assert 0 < n_kept <= W * H and sum(v[2:7]) == n_kept and all(x >= 0 for x in v)
        assert sum(v[7:10]) <= views * n_kept and v[11] <= v[10] <= views * n_kept
        judged += sum(v[7:10])
    assert judged > 0
    first = pushes[0][1]
    assert s_plain.read_text().split("\n")[:first] == s_flagged.read_text().split("\n")[:first]
    r = subprocess.run(base + [str(plain), "LC", "--cull-matches", str(cfile)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode != 0 and b"--match-sim3" in r.stdout
