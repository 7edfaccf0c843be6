"""ellc_keyframe_joint_step / _apply / _refine and ellc_joint_solve (ABI v23) against tests/joint_reference.py, on the world and shapes of
tests/test_gpu_sim3.py (whose helpers are used, not copied). The reference is fed the slots' planes as keyframe_depth_level / image_level
read them back, so the new kernels and the host code around them are the only thing under test: integers with ==, every double sum
against the exactly rounded sum of the same exactly known terms, the apply's planes as bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import joint_reference as J
import refine_depth_reference as R
import test_gpu_sim3 as G
from egomotion_with_local_loop_closures_amd import synth
from helpers import gpu_problem
from test_joint_reference import assert_recovery, recovery_figures

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FILTERS, LIGHTS, SHAPES, fkw = R.FILTERS, R.LIGHTS, G.SHAPES, G.fkw
BAD_ARG, NOT_READY = G.BAD_ARG, G.NOT_READY
K_SLOT = 0
NOWHERE = np.array([1, 0, 0, 1e6, 0, 1, 0, 0, 0, 0, 1, 0], F)   # a view at this transform sees no point of K inside its image
XI_RECORDED = np.random.default_rng(23).normal(0, 2e-3, (J.MAX_VIEWS, 6))


def call_args(world, B):
    vl = R.view_list(B)
    return [s for s, _ in vl], np.stack([world["Ts"][t] for _, t in vl])


def case_params(B):
    return dict(min_views=min(J.DEFAULT_PARAMS["min_views"], B))


def inputs(world, level, B, as_kf):
    slots, Ts = call_args(world, B)
    imgs = {s: (G.planes_of(world, s, level)[2] if as_kf else world["ctx"].image_level(False, s, level)[0]) for s in set(slots)}
    return G.planes_of(world, K_SLOT, level), [imgs[s] for s in slots], G.intr_of(world, level), Ts


def check_step(got, ref, what):
    """One record against the reference: integers with ==, each double sum within n 2^-52 sum |term| of the exactly rounded sum (a sum
    without a term is exactly 0), entries of views >= B zero. Returns the largest distance / bound."""
    for k in J.STEP_INTS:
        assert int(got[k]) == ref[k], (what, k, int(got[k]), ref[k])
    assert got["n_view_terms"].tolist() == ref["n_view_terms"].tolist(), what
    flat = np.concatenate([np.asarray(got[name], np.float64).reshape(-1) for name in J.SUMS] + [[got["chi2_photo"], got["chi2_prior"]]])
    worst = 0.0
    sums = J.sums_of(ref)
    assert flat.size == len(sums)
    for value, (name, want, bound) in zip(flat, sums):
        dist = abs(value - want)
        assert dist <= bound, (what, name, value, want, dist, bound)
        if bound > 0:
            worst = max(worst, dist / bound)
    return worst


def check_apply(got, ref, what):
    """The five planes as bytes, the counts with ==, T within 2 f32 ulp of max |T| of scipy's exponential (test_the_loop_link_by_link's
    bound; with xi = 0 the bytes)."""
    for name in J.APPLY_PLANES:
        assert got[name].dtype == ref[name].dtype and got[name].tobytes() == ref[name].tobytes(), (what, name)
    for k in J.APPLY_INTS:
        assert int(got["stats"][k]) == ref[k], (what, k, got["stats"][k], ref[k])
    assert np.abs(got["T"].astype(np.float64) - ref["T"].astype(np.float64)).max() <= 2 * G.ulp_of(np.abs(ref["T"]).max()), what


def same_apply(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in J.APPLY_PLANES + ("T",)) and a["stats"] == b["stats"]


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


@pytest.mark.parametrize("B", [1, 3, 8])
def test_step_and_apply_against_the_reference(world, ellc, B):
    """Every level; filter, light and the kind of the views' slots change from level to level and from B to B, so that the three shapes
    see both filters, both lights, keyframe and frame slots with every B. The apply at xi = 0, at a recorded xi and at the library's own
    solve, the last from the inverse depths the second left."""
    ctx = world["ctx"]
    worst, used, stepped, solved = 0.0, 0, 0, 0
    for level in range(world["L"]):
        pick = level + B
        flt, light, as_kf = FILTERS[pick % 2], LIGHTS[(pick // 2) % 2], bool((pick // 4 + level) % 2 == 0)
        kf, views, intr, Ts = inputs(world, level, B, as_kf)
        slots = call_args(world, B)[0]
        prm = case_params(B)
        kw = dict(level=level, views_are_keyframes=as_kf, params=prm, **fkw(flt))
        what = "%s level %d B %d filter %s light %s views %s" % (world["shape"], level, B, flt, light, "kf" if as_kf else "frames")
        got = ctx.joint_step(K_SLOT, slots, Ts, [light] * B, **kw)
        ref = J.step(kf, views, intr, Ts, [light] * B, flt, prm)
        worst = max(worst, check_step(got, ref, what))
        used += ref["n_used"]
        plane = None
        for name, xi in (("zero", np.zeros((B, 6))), ("recorded", XI_RECORDED[:B]), ("solved", None)):
            if xi is None:
                xi, refused = ellc.joint_solve(got, 1e-3)
                assert refused == J.solve(ref, 1e-3)[1], what
                if refused:
                    continue
                solved += 1
            out = ctx.joint_apply(K_SLOT, slots, Ts, xi, [light] * B, inv_depth=plane, **kw)
            want = J.apply(kf, views, intr, Ts, [light] * B, flt, xi, prm, plane)
            check_apply(out, want, what + " xi " + name)
            if name == "zero":
                assert out["T"].tobytes() == Ts.tobytes()
            stepped += want["n_stepped"]
            if name == "recorded":
                plane = out["inv_depth"]
        # the step at given inverse depths, the plane's zeros and a NaN falling back to the slot's own
        if plane is not None:
            plane = plane.copy()
            plane[::5, ::3] = np.nan
            got2 = ctx.joint_step(K_SLOT, slots, Ts, [light] * B, inv_depth=plane, **kw)
            worst = max(worst, check_step(got2, J.step(kf, views, intr, Ts, [light] * B, flt, prm, plane), what + " at a plane"))
        if light == LIGHTS[0]:   # a NULL light is (1, 0)
            assert ctx.joint_step(K_SLOT, slots, Ts, None, **kw).tobytes() == got.tobytes(), what
    print(world["shape"], "B", B, "used %d, stepped %d, solves %d, largest distance / bound of the sums %.3g" % (used, stepped, solved, worst))
    assert used > 0 and stepped > 0 and (solved > 0 or B == 1)


def test_other_parameters_reach_the_kernels(world64):
    ctx = world64["ctx"]
    kf, views, intr, Ts = inputs(world64, 0, 3, True)
    slots = call_args(world64, 3)[0]
    other = dict(sigma_i2=4.0, huber_k=3.0, prior_weight=0.0, max_step_rel=0.02, min_views=1)
    got = ctx.joint_step(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, params=other, **fkw(FILTERS[0]))
    ref = J.step(kf, views, intr, Ts, [LIGHTS[1]] * 3, FILTERS[0], other)
    check_step(got, ref, "other parameters")
    assert ref["chi2_prior"] == 0.0 and got["chi2_prior"] == 0.0
    out = ctx.joint_apply(K_SLOT, slots, Ts, XI_RECORDED[:3], [LIGHTS[1]] * 3, params=other, **fkw(FILTERS[0]))
    want = J.apply(kf, views, intr, Ts, [LIGHTS[1]] * 3, FILTERS[0], XI_RECORDED[:3], other)
    check_apply(out, want, "other parameters")
    assert want["n_bad_step"] > 0 and want["n_stepped"] > 0


@pytest.mark.parametrize("shape", ["64x48", "131x67"])
def test_another_configuration_gives_the_same_bytes(ellc, shape):
    one = G.make_world(ellc, shape, arith=ellc.ARITH_EXACT)
    two = G.make_world(ellc, shape, arith=ellc.ARITH_FAST, grid_batch=4, max_batch=7)
    try:
        slots, Ts = call_args(one, 3)
        for level in range(one["L"]):
            kw = dict(level=level, **fkw(FILTERS[0]))
            a = one["ctx"].joint_step(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, **kw)
            b = two["ctx"].joint_step(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, **kw)
            again = one["ctx"].joint_step(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, **kw)
            assert a["n_used"] > 0 and a.tobytes() == b.tobytes() == again.tobytes(), level
            pa = one["ctx"].joint_apply(K_SLOT, slots, Ts, XI_RECORDED[:3], [LIGHTS[1]] * 3, **kw)
            pb = two["ctx"].joint_apply(K_SLOT, slots, Ts, XI_RECORDED[:3], [LIGHTS[1]] * 3, **kw)
            assert same_apply(pa, pb) and same_apply(pa, one["ctx"].joint_apply(K_SLOT, slots, Ts, XI_RECORDED[:3], [LIGHTS[1]] * 3, **kw)), level
        ra = one["ctx"].joint_refine(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, max_iter=2, **fkw(FILTERS[0]))
        rb = two["ctx"].joint_refine(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, max_iter=2, **fkw(FILTERS[0]))
        assert ra["T"].tobytes() == rb["T"].tobytes() and ra["rec"].tobytes() == rb["rec"].tobytes() and ra["iters"] == rb["iters"]
        assert all(ra[k].tobytes() == rb[k].tobytes() for k in J.APPLY_PLANES)
    finally:
        one["ctx"].close(); two["ctx"].close()


def blocks_of(rec):
    """{(b, c): the 6 x 6 block of S, its unused lower triangle zero on the diagonal blocks}, the views' A, a, s and term counts."""
    B = int(rec["B"])
    N = 6 * B
    out = {}
    for b in range(B):
        for c in range(b, B):
            out[(b, c)] = [[float(rec["S"][J.tri(N, 6 * b + k, 6 * c + l)]) if 6 * b + k <= 6 * c + l else 0.0 for l in range(6)] for k in range(6)]
        out[b] = (rec["A"][b].tobytes(), rec["a"][b].tobytes(), rec["s"][6 * b:6 * b + 6].tobytes(), int(rec["n_view_terms"][b]))
    return out


def test_a_blind_view_changes_no_byte_of_the_other_views_sums(world):
    ctx = world["ctx"]
    slots, Ts = call_args(world, 3)
    for level in range(world["L"]):
        for as_kf in (True, False):
            kw = dict(level=level, views_are_keyframes=as_kf, **fkw(FILTERS[1]))
            first = ctx.joint_step(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, **kw)
            base = blocks_of(first)
            # a fourth view from which no pixel gets four taps, at the end and in the middle
            for where, order in (("end", [0, 1, 2, None]), ("middle", [0, None, 1, 2])):
                s4 = [slots[o] if o is not None else 1 for o in order]
                T4 = np.stack([Ts[o] if o is not None else NOWHERE for o in order])
                blind = ctx.joint_step(K_SLOT, s4, T4, [LIGHTS[1]] * 4, **kw)
                got = blocks_of(blind)
                pos = {o: i for i, o in enumerate(order)}
                for b in range(3):
                    assert got[pos[b]] == base[b], (level, as_kf, where, b)
                    for c in range(b, 3):
                        assert got[(pos[b], pos[c])] == base[(b, c)], (level, as_kf, where, b, c)
                z = pos[None]
                assert got[z] == (bytes(21 * 8), bytes(6 * 8), bytes(6 * 8), 0)
                assert all(not np.any(v) for k, v in got.items() if isinstance(k, tuple) and z in k)
                for k in ("chi2_photo", "chi2_prior", "n_terms", "n_kept", "n_taking_part", "n_used", "n_too_few_views", "n_no_information"):
                    assert blind[k] == first[k], (level, as_kf, where, k)
                xi4 = np.stack([XI_RECORDED[o] if o is not None else XI_RECORDED[7] for o in order])
                pa = ctx.joint_apply(K_SLOT, slots, Ts, XI_RECORDED[:3], [LIGHTS[1]] * 3, **kw)
                pb = ctx.joint_apply(K_SLOT, s4, T4, xi4, [LIGHTS[1]] * 4, **kw)
                assert all(pa[k].tobytes() == pb[k].tobytes() for k in J.APPLY_PLANES) and pa["stats"] == pb["stats"], (level, as_kf, where)
        assert first["n_used"] > 0


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
    with the returned planes; dst == another slot likewise, K untouched; dst == -1: every plane of every slot untouched. The apply and
    the loop alike."""
    one, twin = G.make_world(ellc, "64x48"), G.make_world(ellc, "64x48")
    try:
        slots, Ts = call_args(one, 3)
        before = snapshot(one)
        calls = (lambda dst: one["ctx"].joint_apply(K_SLOT, slots, Ts, XI_RECORDED[:3], [LIGHTS[1]] * 3, dst_slot=dst, **fkw(FILTERS[0])),
                 lambda dst: one["ctx"].joint_refine(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, max_iter=2, dst_slot=dst, **fkw(FILTERS[0])))
        results = [call(-1) for call in calls]
        assert results[0]["stats"]["n_stepped"] > 0 and results[1]["iters"] > 0 and snapshot(one) == before
        L = one["L"]
        for res, call in zip(results, calls):
            for dst in (2, 3):   # a view, then the empty slot: K keeps its planes, so that the second call reads what the first read
                got = call(dst)
                assert all(got[k].tobytes() == res[k].tobytes() for k in J.APPLY_PLANES + ("T",)), dst
                twin["ctx"].keyframe_set_depth(dst, res["depth"], res["var"])
                for level in range(L):
                    a, b = one["ctx"].keyframe_depth_level(dst, level), twin["ctx"].keyframe_depth_level(dst, level)
                    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (dst, level)
                assert one["ctx"].keyframe_depth_level(dst, 0)[0].tobytes() == res["depth"].tobytes()
            after = snapshot(one)
            assert after[:2 * L] == before[:2 * L]   # slots 0 (K) and 1
        # K itself, the main use: read first, stored afterwards
        got = calls[0](K_SLOT)
        assert all(got[k].tobytes() == results[0][k].tobytes() for k in J.APPLY_PLANES)
        twin["ctx"].keyframe_set_depth(K_SLOT, results[0]["depth"], results[0]["var"])
        for level in range(L):
            a, b = one["ctx"].keyframe_depth_level(K_SLOT, level), twin["ctx"].keyframe_depth_level(K_SLOT, level)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), level
        # the stored slot still serves the other ring calls as the twin's does
        src, dstn, T3 = [0, 2], [1, 1], np.stack([one["Ts"][1], one["Ts"][1]])
        assert one["ctx"].sim3_step(src, dstn, T3).tobytes() == twin["ctx"].sim3_step(src, dstn, T3).tobytes()
    finally:
        one["ctx"].close(); twin["ctx"].close()


PATTERN = 0xA5
GOOD = (16.0, 1.345, 1.0, 0.5, 2)


def raw_call(ctx, ellc, n, entry="step", kf=K_SLOT, level=0, slots=(1, 2), T=None, light=(1.0, 0.0, 1.0, 0.0), flt=(0.0, 0, 1.0, 1), params=GOOD, dst=-1,
             as_kf=1, B=None, null=None, xi=None, max_iter=2, eps=0.0, lam=0.0, trace_capacity=None):
    """(status, every output untouched?) of one of the three entry points, not raised. null: which pointer argument to pass as NULL."""
    s = np.ascontiguousarray(slots, np.int32).reshape(-1)
    B = s.size if B is None else B
    Tn = np.ascontiguousarray(np.tile(np.asarray(G.IDENTITY, F), max(s.size, 1)) if T is None else T, F).reshape(-1)
    li = np.ascontiguousarray(np.resize(np.asarray(light, F), 2 * max(s.size, 1)))
    f = ellc._lib.EllcMapFilter(flt[0], int(flt[1]), flt[2], int(flt[3]))
    prm = ellc._lib.EllcJointParams(*params)
    x = np.ascontiguousarray(np.zeros(6 * max(s.size, 1)) if xi is None else xi, np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    pat = lambda nbytes: np.full(nbytes, PATTERN, np.uint8)   # noqa: E731
    head = (ctx.h, int(kf), int(level), int(B), int(as_kf), None if null == "slots" else p(s), None if null == "T" else p(Tn),
            None if null == "light" else p(li), None if null == "filter" else C.byref(f), None if null == "params" else C.byref(prm), None)
    planes = dict(inv=pat(4 * n), depth=pat(4 * n), var=pat(4 * n), views=pat(n), status=pat(n))
    if entry == "step":
        outs = dict(rec=pat(11600))
        st = ctx._l.ellc_keyframe_joint_step(*head, None if null == "out" else p(outs["rec"]))
    elif entry == "apply":
        outs = dict(T=pat(48 * max(s.size, 1)), stats=pat(32), **planes)
        st = ctx._l.ellc_keyframe_joint_apply(*head, None if null == "xi" else p(x), int(dst), None if null == "T_out" else p(outs["T"]), p(outs["inv"]),
                                              p(outs["depth"]), p(outs["var"]), p(outs["views"]), p(outs["status"]), p(outs["stats"]))
    else:
        cap = max_iter + 1 if trace_capacity is None else trace_capacity
        m = max(cap, 1) * max(s.size, 1)
        outs = dict(T=pat(48 * max(s.size, 1)), rec=pat(11600), iters=pat(4), tT=pat(48 * m), tR=pat(11600 * max(cap, 1)), tX=pat(48 * m), tA=pat(4 * max(cap, 1)),
                    **planes)
        st = ctx._l.ellc_keyframe_joint_refine(*head, int(max_iter), C.c_float(eps), C.c_double(lam), int(dst), None if null == "T_out" else p(outs["T"]),
                                               None if null == "out" else p(outs["rec"]), p(outs["iters"]), p(outs["inv"]), p(outs["depth"]),
                                               p(outs["var"]), p(outs["views"]), p(outs["status"]), p(outs["tT"]), p(outs["tR"]), p(outs["tX"]),
                                               p(outs["tA"]), int(cap))
    return st, all(bool((a == PATTERN).all()) for a in outs.values())


def test_refused_calls_write_nothing_and_touch_no_slot(world64, ellc):
    ctx = world64["ctx"]
    n = world64["w"] * world64["h"]
    before = snapshot(world64)

    def refused(code, only=("step", "apply", "refine"), **kw):
        for entry in only:
            st, untouched = raw_call(ctx, ellc, n, entry=entry, **kw)
            assert st == code and untouched, (entry, st, code, untouched, kw)

    def accepted(only=("step", "apply", "refine"), **kw):
        for entry in only:
            st, untouched = raw_call(ctx, ellc, n, entry=entry, **kw)
            assert st == 0 and not untouched, (entry, st, kw)

    accepted(); accepted(null="light"); accepted(as_kf=0)
    refused(BAD_ARG, B=0); refused(BAD_ARG, B=-1); refused(BAD_ARG, slots=[1] * 9)                         # B outside 1..8
    accepted(slots=[1] * 8)
    refused(BAD_ARG, kf=-1); refused(BAD_ARG, kf=G.N_SLOTS)                                                # K out of range
    refused(BAD_ARG, slots=(-1, 1)); refused(BAD_ARG, slots=(1, G.N_SLOTS)); refused(BAD_ARG, slots=(1, G.N_SLOTS), as_kf=0)   # a view out of range
    refused(BAD_ARG, level=-1); refused(BAD_ARG, level=world64["L"])
    refused(BAD_ARG, as_kf=2); refused(BAD_ARG, as_kf=-1)
    for null in ("slots", "T", "filter", "params"):
        refused(BAD_ARG, null=null)
    refused(BAD_ARG, only=("step", "refine"), null="out"); refused(BAD_ARG, only=("apply", "refine"), null="T_out"); refused(BAD_ARG, only=("apply",), null="xi")
    refused(BAD_ARG, flt=(0.0, -1, 1.0, 1)); refused(BAD_ARG, flt=(0.0, 9, 1.0, 1)); refused(BAD_ARG, flt=(0.0, 0, 1.0, 0))   # the filter errors of map_points
    refused(BAD_ARG, flt=(0.0, 0, -1.0, 1)); refused(BAD_ARG, flt=(0.0, 0, np.inf, 1)); refused(BAD_ARG, flt=(0.0, 0, np.nan, 1))
    refused(BAD_ARG, flt=(np.nan, 0, 1.0, 1))
    for bad in (np.nan, np.inf, -np.inf):   # a value of T, of the light or of xi that is not finite, in the first view and in the last
        for k in (0, 3, 12 + 11):
            T = np.tile(np.asarray(G.IDENTITY, F), 2); T[k] = bad
            refused(BAD_ARG, T=T)
        for k in range(4):
            li = np.array([1, 0, 1, 0], F); li[k] = bad
            refused(BAD_ARG, light=li)
        for k in (0, 11):
            xi = np.zeros(12); xi[k] = bad
            refused(BAD_ARG, only=("apply",), xi=xi)
    for k in range(4):   # every float parameter: NaN, inf, negative; all but prior_weight also 0
        for bad in (np.nan, np.inf, -1.0) + ((0.0,) if k != 2 else ()):
            refused(BAD_ARG, params=GOOD[:k] + (bad,) + GOOD[k + 1:])
    accepted(only=("step", "apply"), params=(1e-3, 1e-3, 0.0, 1e-3, 1))
    refused(BAD_ARG, only=("refine",), params=(16.0, 1.345, 0.0, 0.5, 2))                                   # the loop needs the prior
    for min_views in (0, 3, -1):   # 1..B with B = 2
        refused(BAD_ARG, params=GOOD[:4] + (min_views,))
    for max_iter in (0, 17, -1):
        refused(BAD_ARG, only=("refine",), max_iter=max_iter, trace_capacity=32)
    accepted(only=("refine",), max_iter=16); accepted(only=("refine",), max_iter=1)
    refused(BAD_ARG, only=("refine",), eps=-1.0); refused(BAD_ARG, only=("refine",), eps=np.nan); refused(BAD_ARG, only=("refine",), eps=np.inf)
    refused(BAD_ARG, only=("refine",), lam=-1.0); refused(BAD_ARG, only=("refine",), lam=np.nan); refused(BAD_ARG, only=("refine",), lam=np.inf)
    refused(BAD_ARG, only=("refine",), max_iter=4, trace_capacity=4)
    refused(BAD_ARG, only=("apply", "refine"), dst=-2); refused(BAD_ARG, only=("apply", "refine"), dst=G.N_SLOTS)
    refused(BAD_ARG, only=("apply", "refine"), dst=0, level=1)                                              # the destination errors of the fusion
    # K without depth or without anything; a view without an image
    refused(NOT_READY, kf=G.IMAGE_ONLY_SLOT)
    accepted(slots=(G.IMAGE_ONLY_SLOT, 1))                                                                 # a view needs no depth
    fresh = gpu_problem(ellc, world64["w"], world64["h"], world64["L"], world64["scenes"][:1], max_keyframes=3, max_frames=3)
    try:
        for kw in (dict(kf=1), dict(slots=(0, 1)), dict(slots=(0, 2), as_kf=0)):
            for entry in ("step", "apply", "refine"):
                st, untouched = raw_call(fresh, ellc, n, entry=entry, **kw)
                assert st == NOT_READY and untouched, (entry, kw)
        with pytest.raises(ellc.EllcError):
            fresh.joint_step(1, [0, 0], [G.IDENTITY] * 2)
    finally:
        fresh.close()
    # an all-zero depth is a map without hypotheses, not an error: an empty record, a refused solve, a loop that makes no iteration
    zero = ctx.joint_step(G.ZERO_SLOT, [1, 2], [G.IDENTITY] * 2)
    assert zero["n_kept"] == 0 and zero["B"] == 2 and not np.any(zero["S"]) and ellc.joint_solve(zero)[1]
    res = ctx.joint_refine(G.ZERO_SLOT, [1, 2], [G.IDENTITY] * 2)
    assert res["iters"] == 0 and not res["status"].any() and not res["depth"].any() and res["T"].tobytes() == np.tile(G.IDENTITY, 2).tobytes()
    # the context still answers as before, and no plane of any slot has changed
    kf, views, intr, Ts = inputs(world64, 0, 3, True)
    got = ctx.joint_step(K_SLOT, call_args(world64, 3)[0], Ts, [LIGHTS[0]] * 3, **fkw(FILTERS[0]))
    check_step(got, J.step(kf, views, intr, Ts, [LIGHTS[0]] * 3, FILTERS[0]), "after the refusals")
    assert snapshot(world64) == before


def test_the_loop_link_by_link(world, ellc):
    """From the trace: every traced record is joint_step's at the traced T and the state's inverse depths, every xi joint_solve's of its
    record, every trial joint_apply's of the accepted state (the same code: bytes), the acceptance the header's rule, the outputs the last
    accepted trial's; and every moved T is within 2 f32 ulp of max |T| of numpy's solve and scipy's exponential from the same record."""
    ctx = world["ctx"]
    slots, Ts = call_args(world, 3)
    lam, eps, max_iter, accepted = 1e-3, 1e-7, 4, 0
    for level in range(world["L"]):
        kw = dict(level=level, **fkw(FILTERS[0]))
        res = ctx.joint_refine(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, max_iter=max_iter, eps=eps, lam=lam, trace=True, **kw)
        n = len(res["trace_rec"])
        assert 1 <= n <= max_iter + 1 and res["trace_accepted"][0] == 1 and res["trace_T"][0].tobytes() == Ts.tobytes()
        T, plane, rec, iters, last = Ts, None, res["trace_rec"][0], 0, None
        assert rec.tobytes() == ctx.joint_step(K_SLOT, slots, T, [LIGHTS[1]] * 3, **kw).tobytes(), level
        for e in range(1, n):
            xi, refused = ellc.joint_solve(rec, lam)
            assert not refused and res["trace_xi"][e - 1].tobytes() == xi.tobytes() and np.abs(xi).max() >= eps, (level, e)
            trial = ctx.joint_apply(K_SLOT, slots, T, xi, [LIGHTS[1]] * 3, inv_depth=plane, **kw)
            assert res["trace_T"][e].tobytes() == trial["T"].tobytes(), (level, e)
            want_xi, ref_refused = J.solve(rec, lam)
            assert not ref_refused
            assert np.abs(trial["T"].astype(np.float64) - J.move_poses(want_xi, T)).max() <= 2 * G.ulp_of(np.abs(T).max()), (level, e)
            rec_t = ctx.joint_step(K_SLOT, slots, trial["T"], [LIGHTS[1]] * 3, inv_depth=trial["inv_depth"], **kw)
            assert res["trace_rec"][e].tobytes() == rec_t.tobytes(), (level, e)
            c0, c1 = J.cost(rec), J.cost(rec_t)
            ok = c0 is not None and c1 is not None and c1 <= c0
            assert bool(res["trace_accepted"][e]) == ok, (level, e, c0, c1)
            if not ok:
                assert e == n - 1
                break
            T, plane, rec, last = trial["T"], trial["inv_depth"], rec_t, trial
            iters += 1
        if n - 1 == iters and iters < max_iter:   # the loop ended on its own: a refused solve or a step below eps
            xi, refused = ellc.joint_solve(rec, lam)
            assert refused or np.abs(xi).max() < eps, level
        assert res["iters"] == iters and res["T"].tobytes() == T.tobytes() and res["rec"].tobytes() == rec.tobytes(), level
        accepted += iters
        if last is None:   # no accepted trial (the first step of the 23x17 world's level 0 raises the cost): K's own planes, nothing stepped
            d, v, _ = G.planes_of(world, K_SLOT, level)
            assert res["depth"].tobytes() == d.tobytes() and res["var"].tobytes() == v.tobytes(), level
            assert not res["inv_depth"].any() and not res["views"].any() and not res["status"].any(), level
        else:
            for name in J.APPLY_PLANES:
                assert res[name].tobytes() == last[name].tobytes(), (level, name)
        print(world["shape"], "level", level, "steps", n, "accepted", iters, "cost %.4g -> %.4g" % (J.cost(res["trace_rec"][0]), J.cost(rec)))
    assert accepted > 0


@pytest.mark.parametrize("case", J.RECOVERY, ids=["64x48-3views", "131x67-5views"])
def test_recovery_on_the_library(ellc, case):
    """The two recovery inputs of tests/test_joint_reference.py through ellc_keyframe_joint_refine: the CPU test's conditions on the
    library's own output, against ellc_keyframe_refine_depth at the same perturbed transforms."""
    w, h, L, n_kf, seed = case
    scenes, Ts_true, Ts_start, d_true = J.perturbed_world(w, h, n_kf, seed)
    ctx = gpu_problem(ellc, w, h, L, scenes)
    try:
        views = list(range(1, n_kf))
        res = ctx.joint_refine(0, views, Ts_start, max_iter=6)
        only = ctx.refine_depth(0, views, Ts_start)
        part = only["status"] != R.NOT_TAKING_PART
        kf = (scenes[0]["depth0"], scenes[0]["var0"], scenes[0]["kf_image"])
        assert res["iters"] >= 2 and np.array_equal(res["inv_depth"] > 0, part)
        figures = recovery_figures(kf, d_true, Ts_true, Ts_start, res["inv_depth"], res["T"], only["depth"], part)
        assert_recovery((w, h), figures)
        # the planes agree with each other: depth = 1 / inv_depth where the last accepted trial stepped the pixel
        st = res["status"] == J.STEPPED
        assert st.sum() > 0 and (res["depth"][st] == (F(1.0) / res["inv_depth"][st]).astype(F)).all()
    finally:
        ctx.close()


def test_profile_twins_give_the_same_result(ellc):
    wd = G.make_world(ellc, "64x48", diag=True)
    try:
        slots, Ts = call_args(wd, 3)
        plain = wd["ctx"].joint_step(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, **fkw(FILTERS[0]))
        timed, ms = wd["ctx"].profile_joint_step(K_SLOT, slots, Ts, [LIGHTS[1]] * 3, **fkw(FILTERS[0]))
        assert plain.tobytes() == timed.tobytes() and ms > 0
        plain = wd["ctx"].joint_apply(K_SLOT, slots, Ts, XI_RECORDED[:3], [LIGHTS[1]] * 3, **fkw(FILTERS[0]))
        timed, ms = wd["ctx"].profile_joint_apply(K_SLOT, slots, Ts, XI_RECORDED[:3], [LIGHTS[1]] * 3, **fkw(FILTERS[0]))
        assert same_apply(plain, timed) and ms > 0
    finally:
        wd["ctx"].close()


def test_driver_joint_matches_file(tmp_path):
    """ellc_main --match-sim3 S --match-light --joint-matches J on the 33-frame loop-closure sequence of tests/test_gpu_driver.py: one
    line per push that had candidates, finite fields, accepted iterations on at least one push. Without the flag no such file appears
    and the run is what it was: the joint refinement touches the ring's copy alone, so the tracking outputs of both runs are
    byte-identical, as are the Sim(3) lines of the first push with candidates, whose evaluation ran before any joint refinement had
    stored a map (its transforms are printed after the joint step moved them: compared without); and --joint-matches without
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
    again = tmp_path / "again"; again.mkdir()
    flagged = tmp_path / "flagged"; flagged.mkdir()
    base = [exe, str(raw), str(W), str(H), str(n_frames)]
    s_plain, s_again, s_flagged, jfile = tmp_path / "sim3_plain.txt", tmp_path / "sim3_again.txt", tmp_path / "sim3_flagged.txt", tmp_path / "joint.txt"
    for out, sfile, extra in ((plain, s_plain, []), (again, s_again, []), (flagged, s_flagged, ["--joint-matches", str(jfile)])):
        r = subprocess.run(base + [str(out), "LC", "--match-sim3", str(sfile), "--match-light"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=600)
        assert r.returncode == 0, r.stdout.decode()
    names = sorted(p.name for p in plain.iterdir())
    assert names == sorted(p.name for p in flagged.iterdir()) == sorted(p.name for p in again.iterdir())
    for name in names:   # without the flag every output file is byte-identical, run to run
        assert (plain / name).read_bytes() == (again / name).read_bytes(), name
    assert s_plain.read_bytes() == s_again.read_bytes()
    for name in ("poses_orig.txt", "matchframes.txt"):
        assert (plain / name).read_bytes() == (flagged / name).read_bytes(), name
    matches = (flagged / "matchframes_globalopt.txt").read_text().strip().split("\n")
    pushes = []
    for m in matches:
        if not pushes or pushes[-1][0] != m.split(" ")[0]:
            pushes.append([m.split(" ")[0], 0])
        pushes[-1][1] += 1
    lines = jfile.read_text().strip().split("\n")
    assert len(pushes) >= 2 and len(lines) == len(pushes)
    accepted = 0
    for (frame_id, n_cand), l in zip(pushes, lines):
        c = l.split(" ")
        print(l)
        assert len(c) == 11 and c[0] == frame_id and int(c[1]) == min(n_cand, J.MAX_VIEWS)
        values = [float(v) for v in c[1:]]
        assert all(np.isfinite(v) for v in values)
        iters, n_kept, n_part, n_used, n_few, n_noinf, n_terms = (int(v) for v in c[2:9])
        assert 0 <= iters <= 6 and 0 <= n_part <= n_kept <= W * H and n_used + n_few + n_noinf == n_part and n_used <= n_terms <= n_used * int(c[1])
        accepted += iters
    assert accepted > 0
    # the first push's Sim(3) lines but for the transform the joint step moved: scale, counts, sums, iterations and light are the evaluation's
    first = pushes[0][1]
    keep = lambda l: [v for k, v in enumerate(l.split(" ")) if k not in (3, 4, 5, 6, 7, 8)]   # noqa: E731
    assert [keep(l) for l in s_plain.read_text().split("\n")[:first]] == [keep(l) for l in s_flagged.read_text().split("\n")[:first]]
    r = subprocess.run(base + [str(plain), "LC", "--joint-matches", str(jfile)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode != 0 and b"--match-sim3" in r.stdout
