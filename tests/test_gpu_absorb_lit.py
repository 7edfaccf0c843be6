"""ellc_depth_absorb_keyframes_lit and ellc_depth_restart_from_keyframes_lit (ABI v24) against tests/absorb_lit_reference.py: the seven
state planes by their bytes and the sixteen counts with ==, at a brightening light, a darkening one and mixed lights per request; NULL and
(1, 0) lights against the unlit entry points on a twin context; everything that must not enter the result; the restart against the calls
its contract names; every refusal; and the demonstration - a destination brightened by clip(rint(1.6 I - 20)) loses nearly half of its
candidates to the unlit gate and keeps them at the light, on the reference first and then on the device.

The demonstration's figures (n_candidates of the four sources, filter (0, 0, 1, 1), gate on; reference == device):
    64x48:  unaltered 3650, altered unlit 1909 (0.52), altered at (1.6, -20) 4014 (1.10)
    131x67: unaltered 10078, altered unlit 3221 (0.32), altered at (1.6, -20) 10280 (1.02)"""
import ctypes as C
import numpy as np
import pytest

import absorb_lit_reference as AL
import absorb_reference as A
import trial_propagation_reference as R
from helpers import gpu_problem
from test_gpu_absorb import FILTERS, IMAGE_ONLY_SLOT, K_SLOT, N_SLOTS, SHAPES, SOURCES, fkw, k_planes, make_world, planes_of

pytestmark = pytest.mark.gpu

BAD_ARG, NOT_READY = -1, -3
F = np.float32
BRIGHT, DARK = np.tile(np.array([1.6, -20.0], F), (4, 1)), np.tile(np.array([0.7, 15.0], F), (4, 1))
MIXED = np.array([[1.6, -20.0], [1.0, 0.0], [0.7, 15.0], [1.25, -7.5]], F)
UNIT = np.tile(np.array([1.0, 0.0], F), (4, 1))
LIGHTS = {"bright": BRIGHT, "dark": DARK, "mixed": MIXED}


def raw_lit(ctx, ellc, slots, Ts, lights, flt=(0.0, 0, 1.0, 1), stats=None, restart_slot=None, factor=None, **prm):
    """The status of the _lit entry points, not raised; lights None goes down as NULL."""
    kf = np.ascontiguousarray(slots, np.int32).reshape(-1)
    T = np.ascontiguousarray(Ts, F).reshape(-1)
    L = None if lights is None else np.ascontiguousarray(lights, F).reshape(-1)
    f = ellc._lib.EllcMapFilter(flt[0], int(flt[1]), flt[2], int(flt[3]))
    p = ellc._lib.EllcAbsorbParams(prm.get("agree_k2", 1.0), prm.get("max_fold", 64), prm.get("photo_gate", 1), prm.get("src_validity", 20),
                                   prm.get("finalise", 0))
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    st = None if stats is None else C.byref(stats)
    if restart_slot is None:
        return ctx._l.ellc_depth_absorb_keyframes_lit(ctx.h, kf.size, ptr(kf), ptr(T), ptr(L), C.byref(f), C.byref(p), st)
    return ctx._l.ellc_depth_restart_from_keyframes_lit(ctx.h, int(restart_slot), kf.size, ptr(kf), ptr(T), ptr(L), C.byref(f), C.byref(p),
                                                        None if factor is None else C.byref(factor), st)


def stats_dict(ellc, st):
    return {k: int(getattr(st, k)) for k in ellc._lib.ABSORB_STATS_FIELDS}


def reference(world, slots, Ts, lights, flt, state, **prm):
    """Computed once per case and shared; never written to."""
    key = (tuple(slots), np.asarray(Ts, F).tobytes(), None if lights is None else np.asarray(lights, F).tobytes(), tuple(flt),
           b"".join(np.ascontiguousarray(state[k]).tobytes() for k in A.PLANES), tuple(sorted(prm.items())))
    if key not in world["refs"]:
        k_img, k_mg = k_planes(world)
        world["refs"][key] = AL.absorb_lit([planes_of(world, s) for s in slots], world["intr"], Ts, lights, flt, k_img, k_mg, state, **prm)
    return world["refs"][key]


def run(world, slots, Ts, lights, flt, state, ctx=None, **prm):
    ctx = ctx or world["ctx"]
    ctx.depth_set_state(state)
    before = ctx.depth_get_state()
    stats = ctx.depth_absorb(slots, Ts, params=dict(finalise=0, **prm), lights=lights, **fkw(flt))
    return before, ctx.depth_get_state(), stats


def check(world, slots, Ts, lights, flt, state, **prm):
    before, got, stats = run(world, slots, Ts, lights, flt, state, **prm)
    ref = reference(world, slots, Ts, lights, flt, before, **prm)
    print(world["w"], world["h"], "filter", flt, prm, "lights", np.asarray(lights).reshape(-1)[:4], "stats", stats)
    assert not A.differing(got, ref), (prm, A.differing(got, ref))
    assert stats == ref["stats"], (stats, ref["stats"])
    assert stats["n_visited"] == stats["n_created"] + stats["n_merged"] + stats["n_replaced"] + stats["n_occluded"] + stats["n_skipped"]
    assert stats["n_valid_after"] == int((got["valid"] != 0).sum()) and stats["reserved"] == 0
    return ref, got, stats


@pytest.fixture(scope="module", params=list(SHAPES))
def world(request, ellc):
    wd = make_world(ellc, request.param)
    wd["shape"] = request.param
    wd["twin"] = make_world(ellc, request.param)
    yield wd
    wd["ctx"].close(); wd["twin"]["ctx"].close()


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
@pytest.mark.parametrize("which", list(LIGHTS))
def test_bit_for_bit_against_the_lit_reference(world, flt, which):
    lights = LIGHTS[which]
    unlit = A.absorb([planes_of(world, s) for s in SOURCES], world["intr"], world["Ts"], flt, *k_planes(world), world["state"])["stats"]
    for max_fold in (64, 1):
        ref, got, stats = check(world, SOURCES, world["Ts"], lights, flt, world["state"], max_fold=max_fold)
        if flt == FILTERS[0] and world["shape"] != "23x17":   # conditions of the test: the light enters, and the scene reaches every class
            # (at (0.7, 15) the scene's grey values move by less than the gate's width: the same candidates pass, as on the reference)
            assert (stats["n_candidates"] != unlit["n_candidates"] or which == "dark") and 0 < stats["n_candidates"] < stats["n_interior"]
            for k in ("n_created", "n_merged", "n_replaced"):
                assert stats[k] > 0, (k, stats)
        keep = ~ref["touched"]
        for name in A.PLANES:
            assert np.array_equal(got[name][keep].view(np.uint8), world["state"][name][keep].view(np.uint8)), name
    # the gate off: the light does not enter, the unlit call's bytes
    _, off, s_off = run(world, SOURCES, world["Ts"], lights, flt, world["state"], photo_gate=0)
    world["twin"]["ctx"].depth_set_state(world["state"])
    s_plain = world["twin"]["ctx"].depth_absorb(SOURCES, world["Ts"], params=dict(finalise=0, photo_gate=0), **fkw(flt))
    assert s_off == s_plain and not A.differing(off, world["twin"]["ctx"].depth_get_state())


@pytest.mark.parametrize("finalise", [0, 1])
def test_null_and_unit_lights_are_the_unlit_entry_point(world, ellc, finalise):
    ctx, twin, L = world["ctx"], world["twin"]["ctx"], world["L"]
    flt = FILTERS[1]
    for lights in (None, UNIT):
        twin.depth_set_state(world["state"])
        want = twin.depth_absorb(SOURCES, world["Ts"], params=dict(finalise=finalise), **fkw(flt))
        ctx.depth_set_state(world["state"])
        st = ellc._lib.EllcAbsorbStats(*range(101, 117))
        assert raw_lit(ctx, ellc, SOURCES, world["Ts"], lights, flt, st, finalise=finalise) == 0
        assert stats_dict(ellc, st) == want and want["n_candidates"] > 0
        assert not A.differing(ctx.depth_get_state(), twin.depth_get_state())
        for level in range(L):
            (da, va), (db, vb) = ctx.keyframe_depth_level(K_SLOT, level), twin.keyframe_depth_level(K_SLOT, level)
            assert da.tobytes() == db.tobytes() and va.tobytes() == vb.tobytes(), level
    # one request at (1, 0) among others: its candidates are the unlit call's
    alone_lit = run(world, [2], world["Ts"][1:2], MIXED[1:2], flt, world["state"])[2]
    twin.depth_set_state(world["state"])
    alone = twin.depth_absorb([2], world["Ts"][1:2], params=dict(finalise=0), **fkw(flt))
    assert alone_lit == alone


def test_a_second_call_another_context_and_the_requests_one_by_one(world, ellc):
    w, h, L = SHAPES[world["shape"]]
    other = make_world(ellc, world["shape"], arith=ellc.ARITH_FAST, grid_batch=4)
    try:
        flt = FILTERS[1]
        ref, a, stats = check(world, SOURCES, world["Ts"], MIXED, flt, world["state"])
        _, b, stats_b = run(world, SOURCES, world["Ts"], MIXED, flt, world["state"])
        assert not A.differing(a, b) and stats == stats_b
        _, c, stats_c = run(other, SOURCES, other["Ts"], MIXED, flt, other["state"])
        assert not A.differing(a, c) and stats == stats_c
        world["ctx"].set_grid_batch(2)
        _, d, stats_d = run(world, SOURCES, world["Ts"], MIXED, flt, world["state"])
        assert not A.differing(a, d) and stats == stats_d
        # a request alone: its candidates at its own light, whatever the batch holds (the four per-pixel counts add up)
        alone = [run(world, [s], world["Ts"][k:k + 1], MIXED[k:k + 1], flt, world["state"])[2] for k, s in enumerate(SOURCES)]
        for k in ("n_kept", "n_in_view", "n_interior", "n_candidates"):
            assert sum(x[k] for x in alone) == stats[k], k
    finally:
        other["ctx"].close()


@pytest.mark.parametrize("shape", ["64x48", "23x17"])   # the export's tiled launch, and its per-level kernels
def test_finalise_is_regularise_and_export(ellc, shape):
    a, b = make_world(ellc, shape), make_world(ellc, shape)
    ca, cb = a["ctx"], b["ctx"]
    try:
        sa = ca.depth_absorb(SOURCES, a["Ts"], params=dict(finalise=1), lights=MIXED)
        sb = cb.depth_absorb(SOURCES, b["Ts"], params=dict(finalise=0), lights=MIXED)
        cb.depth_do_regularization(False)
        cb.depth_update_depth_image()
        assert sa == sb and sa["n_created"] > 0
        assert not A.differing(ca.depth_get_state(), cb.depth_get_state())
        for level in range(a["L"]):
            (da, va), (db, vb) = ca.keyframe_depth_level(K_SLOT, level), cb.keyframe_depth_level(K_SLOT, level)
            assert da.tobytes() == db.tobytes() and va.tobytes() == vb.tobytes(), level
    finally:
        ca.close(); cb.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_restart_lit_is_the_calls_its_contract_names(ellc, shape):
    """set_keyframe + the wiped set_state + absorb_lit + createKeyFrame's tail on a twin, bit for bit, and the numpy restart."""
    a, b = make_world(ellc, shape), make_world(ellc, shape)
    ca, cb = a["ctx"], b["ctx"]
    w, h, L = a["w"], a["h"], a["L"]
    try:
        reqs = [planes_of(a, s) for s in SOURCES]
        k_img, k_mg = k_planes(a)
        for flt, finalise, prm in ((FILTERS[0], 0, dict()), (FILTERS[1], 0, dict(max_fold=1)), (FILTERS[0], 1, dict())):
            ca.depth_set_keyframe(IMAGE_ONLY_SLOT)   # a previous state on another keyframe leaves no trace
            ca.depth_set_state(a["state"])
            sa, fa = ca.depth_restart(K_SLOT, SOURCES, a["Ts"], params=dict(finalise=finalise, **prm), lights=MIXED, **fkw(flt))
            cb.depth_set_keyframe(K_SLOT)
            cb.depth_set_state(R.wiped_state(h, w))
            sb = cb.depth_absorb(SOURCES, b["Ts"], params=dict(finalise=0, **prm), lights=MIXED, **fkw(flt))
            fb = 1.0
            if finalise:
                cb.depth_regularize(True); cb.depth_fill_holes(); cb.depth_regularize(False)
                fb = cb.depth_make_inv_depth_one()
                cb.depth_update_depth_image()
            ga = ca.depth_get_state()
            assert sa == sb and sa["n_valid_before"] == 0 and sa["n_created"] == sa["targets_hit"] > 0
            assert np.float32(fa).tobytes() == np.float32(fb).tobytes()
            assert not A.differing(ga, cb.depth_get_state())
            for level in range(L):
                (da, va), (db, vb) = ca.keyframe_depth_level(K_SLOT, level), cb.keyframe_depth_level(K_SLOT, level)
                assert da.tobytes() == db.tobytes() and va.tobytes() == vb.tobytes(), level
            if not finalise:
                ref = AL.restart_lit(reqs, a["intr"], a["Ts"], MIXED, flt, k_img, k_mg, **prm)
                assert sa == ref["stats"] and not A.differing(ga, ref), (sa, ref["stats"])
                unlit, _ = cb.depth_restart(K_SLOT, SOURCES, b["Ts"], params=dict(finalise=0, **prm), **fkw(flt))
                if flt == FILTERS[0] and shape != "23x17":
                    assert unlit["n_candidates"] != sa["n_candidates"]   # a condition of the test: the lights enter
    finally:
        ca.close(); cb.close()


def test_refusals_change_nothing(ellc):
    wd = make_world(ellc, "64x48")
    ctx, T = wd["ctx"], wd["Ts"][:1]
    fresh = gpu_problem(ellc, 64, 48, 3, wd["scene"]["views"], max_keyframes=N_SLOTS)   # no depth-map keyframe, no state
    try:
        state = ctx.depth_get_state()
        before = [ctx.keyframe_depth_level(s, l) for s in range(5) for l in range(wd["L"])]
        stats = ellc._lib.EllcAbsorbStats(*range(101, 117))
        factor = C.c_float(7.5)
        one = np.array([[1.6, -20.0]], F)

        def both(slots=(1,), lights=one, Ts=None, **kw):
            Ts = np.tile(T, (len(slots), 1)) if Ts is None else Ts
            lights = None if lights is None else np.tile(np.asarray(lights, F).reshape(-1, 2)[:1], (max(len(slots), 1), 1)) if len(lights) == 1 else lights
            return (raw_lit(ctx, ellc, list(slots), Ts, lights, stats=stats, **kw),
                    raw_lit(ctx, ellc, list(slots), Ts, lights, stats=stats, restart_slot=6, factor=factor, **kw))

        for bad in ((np.nan, 0.0), (1.0, np.nan), (np.inf, 0.0), (1.0, -np.inf)):
            assert both(lights=np.array([bad], F)) == (BAD_ARG, BAD_ARG), bad
        assert both(slots=(1, 2), lights=np.array([[1.0, 0.0], [1.0, np.nan]], F)) == (BAD_ARG, BAD_ARG)   # the last value of the last request
        assert both(slots=()) == (BAD_ARG, BAD_ARG) and both(slots=(1, 2, 3, 4, 1, 2, 3, 4)) == (BAD_ARG, BAD_ARG)
        assert both(slots=(-1,)) == (BAD_ARG, BAD_ARG) and both(slots=(N_SLOTS,)) == (BAD_ARG, BAD_ARG)
        assert both(flt=(0.0, 9, 1.0, 1)) == (BAD_ARG, BAD_ARG) and both(flt=(np.nan, 0, 1.0, 1)) == (BAD_ARG, BAD_ARG)
        assert both(agree_k2=-1.0) == (BAD_ARG, BAD_ARG) and both(max_fold=0) == (BAD_ARG, BAD_ARG) and both(max_fold=65) == (BAD_ARG, BAD_ARG)
        assert both(src_validity=256) == (BAD_ARG, BAD_ARG) and both(photo_gate=2) == (BAD_ARG, BAD_ARG) and both(finalise=2) == (BAD_ARG, BAD_ARG)
        assert both(slots=(IMAGE_ONLY_SLOT,), lights=np.array([[np.nan, 0.0]], F)) == (BAD_ARG, BAD_ARG)   # the argument in front of the slot
        assert both(slots=(IMAGE_ONLY_SLOT,)) == (NOT_READY, NOT_READY)
        assert raw_lit(ctx, ellc, [1], T, one, stats=stats, restart_slot=N_SLOTS, factor=factor) == BAD_ARG     # the new slot out of range
        assert raw_lit(ctx, ellc, [1], T, one, stats=stats, restart_slot=1, factor=factor) == BAD_ARG           # ... among the sources
        assert raw_lit(fresh, ellc, [1], T, one, stats=stats) == NOT_READY
        with pytest.raises(ellc.EllcError):
            ctx.depth_absorb([1], T, lights=[[np.nan, 0.0]])
        with pytest.raises(ellc.EllcError):
            ctx.depth_restart(6, [1], T, lights=[[1.0, np.inf]])
        assert [getattr(stats, k) for k in ellc._lib.ABSORB_STATS_FIELDS] == list(range(101, 117)) and factor.value == 7.5
        assert not A.differing(state, ctx.depth_get_state())
        after = [ctx.keyframe_depth_level(s, l) for s in range(5) for l in range(wd["L"])]
        for (d0, v0), (d1, v1) in zip(before, after):
            assert d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes()
        # `out` may be NULL, and a good call gives what the reference gives
        assert raw_lit(ctx, ellc, [1], T, one, photo_gate=1) == 0
        check(wd, SOURCES, wd["Ts"], BRIGHT, FILTERS[0], wd["state"])
    finally:
        ctx.close(); fresh.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_brighter_destination_keeps_its_candidates_at_the_light(ellc, shape):
    """THE test of the feature. K's image is replaced by clip(rint(1.6 I - 20)), uploaded. On the REFERENCE first: the unlit gate keeps at
    most 0.6 of the unaltered scene's candidates, the gate at (1.6, -20) at least 0.95 (64x48 and 131x67; at 23x17 the unlit loss is too
    small for the condition and the device is held to the reference only). Then the device == the reference in both runs. A DARKER
    destination (0.7 I + 15, light (0.7, 15)) is held to the reference only: g < 5 takes its candidates and no light repairs that."""
    plain = make_world(ellc, shape)
    try:
        base = A.absorb([planes_of(plain, s) for s in SOURCES], plain["intr"], plain["Ts"], FILTERS[0], *k_planes(plain), plain["state"])["stats"]
        dev_base = run(plain, SOURCES, plain["Ts"], None, FILTERS[0], plain["state"])[2]
        assert dev_base == base
        k_img = k_planes(plain)[0]
        w, h = plain["w"], plain["h"]
        for gain, offset in ((1.6, -20.0), (0.7, 15.0)):
            wd = make_world(ellc, shape)
            try:
                wd["ctx"].keyframe_upload(K_SLOT, np.ascontiguousarray(AL.brighten(k_img[:h, :w], gain, offset)))
                wd["ctx"].depth_set_keyframe(K_SLOT)
                lights = np.tile(np.array([gain, offset], F), (4, 1))
                reqs = [planes_of(wd, s) for s in SOURCES]
                ref_unlit = A.absorb(reqs, wd["intr"], wd["Ts"], FILTERS[0], *k_planes(wd), wd["state"])
                ref_lit = AL.absorb_lit(reqs, wd["intr"], wd["Ts"], lights, FILTERS[0], *k_planes(wd), wd["state"])
                n0, n1, n2 = base["n_candidates"], ref_unlit["stats"]["n_candidates"], ref_lit["stats"]["n_candidates"]
                print(shape, (gain, offset), "n_candidates: unaltered", n0, "altered unlit", n1, "(%.2f)" % (n1 / n0), "altered lit", n2, "(%.2f)" % (n2 / n0))
                if gain > 1 and shape != "23x17":
                    assert n1 <= 0.6 * n0 and n2 >= 0.95 * n0, (n0, n1, n2)
                _, got_unlit, s_unlit = run(wd, SOURCES, wd["Ts"], None, FILTERS[0], wd["state"])
                assert s_unlit == ref_unlit["stats"] and not A.differing(got_unlit, ref_unlit)
                _, got_lit, s_lit = run(wd, SOURCES, wd["Ts"], lights, FILTERS[0], wd["state"])
                assert s_lit == ref_lit["stats"] and not A.differing(got_lit, ref_lit)
            finally:
                wd["ctx"].close()
    finally:
        plain["ctx"].close()
