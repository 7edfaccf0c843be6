"""ellc_keyframe_sim3_step / ellc_keyframe_sim3_align (ABI v15) against tests/sim3_reference.py. The reference is fed the slots' planes
as keyframe_depth_level / image_level read them back (pinned by their own tests), so the new kernels and the loop around them are the
only thing under test: integer fields are compared with ==, each of the 37 double sums against the exactly rounded sum of the same
exactly known terms, the loop link by link from its trace, and the recovery of a known similarity against the reference's own loop."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_reference as S
from egomotion_with_local_loop_closures_amd import synth
from helpers import gpu_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
BAD_ARG, NOT_READY = -1, -3
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
# (width, height, levels): 23x17 has 11 columns stored 12 wide at level 1; 131x67 is five tiles at level 0
SHAPES = {"64x48": (64, 48, 3), "23x17": (23, 17, 2), "131x67": (131, 67, 3)}
ZERO_SLOT, IMAGE_ONLY_SLOT, N_SLOTS = 3, 4, 5
# (source slot, destination slot, transform): the v14 batch of five pairs, and one pair at the shift that reaches the tap-less band
# (tests/test_sim3_reference.py: the classes the batch has to reach are checked there on the CPU)
BATCH = [(0, 0, 0), (0, 1, 1), (1, 0, 1), (2, 0, 2), (1, 1, 1), (1, 2, 3)]
EPS, MAX_ITER = 1e-4, 10


def fkw(flt):
    return dict(max_var=flt[0], min_support=flt[1], support_k2=flt[2], stride=flt[3])


def make_world(ellc, shape, **kw):
    """Keyframe slots 0, 1, 2 hold scenes 11, 12, 13 (with their spoilt inf / NaN / negative pixels); 3 an all-zero depth; 4 an image only."""
    w, h, L = SHAPES[shape]
    scenes = [S.make_scene(w, h, seed) for seed in (11, 12, 13)]
    ctx = gpu_problem(ellc, w, h, L, scenes, max_keyframes=N_SLOTS, **kw)
    ctx.keyframe_upload(ZERO_SLOT, scenes[0]["kf_image"])
    ctx.keyframe_set_depth(ZERO_SLOT, np.zeros((h, w), np.float32), np.full((h, w), -1, np.float32))
    ctx.keyframe_upload(IMAGE_ONLY_SLOT, scenes[1]["kf_image"])
    m = float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0]))
    fx = float(S.level_intrinsics(*scenes[0]["intrinsics"], 0)[0])
    shift = np.array([1, 0, 0, 3.3 * m / fx, 0, 1, 0, 0, 0, 0, 1, 0], F)
    return dict(ctx=ctx, scenes=scenes, intrinsics=scenes[0]["intrinsics"], Ts=np.concatenate([S.scene_transforms(m), shift[None]]), w=w, h=h, L=L,
                planes={}, refs={}, shape=shape)


def planes_of(world, slot, level):
    """(depth, var, stored image) of a slot's level, read back once."""
    if (slot, level) not in world["planes"]:
        d, v = world["ctx"].keyframe_depth_level(slot, level)
        img, (rows, cols) = world["ctx"].image_level(True, slot, level)
        assert d.shape == (rows, cols)
        world["planes"][(slot, level)] = (d, v, img)
    return world["planes"][(slot, level)]


def intr_of(world, level):
    return S.level_intrinsics(*world["intrinsics"], level)


def reference(world, src, dst, level, T, flt, params=None):
    key = (src, dst, level, np.asarray(T, np.float32).tobytes(), tuple(flt), tuple(sorted((params or {}).items())))
    if key not in world["refs"]:
        world["refs"][key] = S.step(planes_of(world, src, level), planes_of(world, dst, level), intr_of(world, level), T, flt, params)
    return world["refs"][key]


def batch_args(world, batch=BATCH):
    return [s for s, _, _ in batch], [d for _, d, _ in batch], np.stack([world["Ts"][t] for _, _, t in batch])


def check_against(got, ref, what, quiet=False):
    """One record against the reference: integers with ==, each of the 37 double sums within n 2^-52 sum |term| of the exactly rounded sum."""
    for k in S.INT_FIELDS:
        assert int(got[k]) == ref[k], (what, k, int(got[k]), ref[k])
    values = list(got["H"]) + list(got["b"]) + [got["chi2_photo"], got["chi2_depth"]]
    worst = 0.0
    for v, (name, want, bound) in zip(values, S.sums_of(ref)):
        dist = abs(float(v) - want)
        assert dist <= bound, (what, name, float(v), want, dist, bound)
        if bound > 0:
            worst = max(worst, dist / bound)
    if not quiet:
        print(what, "kept %d in view %d photo %d depth %d: largest distance / bound of the 37 sums %.3g" % (
            ref["n_kept"], ref["n_in_view"], ref["n_photo"], ref["n_depth"], worst))


@pytest.fixture(scope="module", params=list(SHAPES))
def world(request, ellc):
    wd = make_world(ellc, request.param)
    yield wd
    wd["ctx"].close()


@pytest.fixture(scope="module")
def world64(ellc):
    wd = make_world(ellc, "64x48")
    yield wd
    wd["ctx"].close()


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_step_against_the_reference(world, flt):
    ctx = world["ctx"]
    if world["shape"] == "23x17":
        img1, (_, cols1) = ctx.image_level(True, 0, 1)
        assert cols1 == 11 and img1.shape[1] == 12
    src, dst, Ts = batch_args(world)
    for level in range(world["L"]):
        got = ctx.sim3_step(src, dst, Ts, level=level, **fkw(flt))
        refs = [reference(world, s, d, level, world["Ts"][t], flt) for s, d, t in BATCH]
        for b, ref in enumerate(refs):
            check_against(got[b], ref, "%s level %d filter %s pair %d->%d" % (world["shape"], level, flt, src[b], dst[b]))
            assert all(float(got[b]["H"][S.h_index(i, 6)]) == 0 for i in (2, 3, 4))
        assert sum(r["n_photo"] for r in refs) > 0 and sum(r["n_depth"] for r in refs) > 0
    # other parameters reach the kernel: a tight gate, a wide Huber threshold, another weight
    other = dict(sigma_i2=4.0, huber_k=3.0, gate_k2=0.5, depth_weight=2.5)
    got = ctx.sim3_step(src, dst, Ts, level=0, params=other, **fkw(flt))
    for b, (s, d, t) in enumerate(BATCH):
        check_against(got[b], reference(world, s, d, 0, world["Ts"][t], flt, other), "%s other parameters pair %d" % (world["shape"], b), quiet=True)


def test_a_record_is_a_function_of_its_own_inputs(world):
    ctx = world["ctx"]
    src, dst, Ts = batch_args(world)
    n = len(BATCH)
    for level in range(world["L"]):
        whole = ctx.sim3_step(src, dst, Ts, level=level, **fkw(FILTERS[1]))
        assert int(whole["n_photo"].sum()) > 0 and int(whole["n_depth"].sum()) > 0
        for b in range(n):   # each request alone
            one = ctx.sim3_step(src[b:b + 1], dst[b:b + 1], Ts[b:b + 1], level=level, **fkw(FILTERS[1]))
            assert one.tobytes() == whole[b:b + 1].tobytes(), (level, b)
        rev = ctx.sim3_step(src[::-1], dst[::-1], Ts[::-1], level=level, **fkw(FILTERS[1]))
        assert rev[::-1].tobytes() == whole.tobytes(), level
        twice = ctx.sim3_step(src * 2, dst * 2, np.concatenate([Ts, Ts]), level=level, **fkw(FILTERS[1]))
        assert twice[:n].tobytes() == whole.tobytes() and twice[n:].tobytes() == whole.tobytes(), level


@pytest.mark.parametrize("shape", ["64x48", "131x67"])
def test_another_configuration_gives_the_same_bytes(ellc, shape):
    one = make_world(ellc, shape, arith=ellc.ARITH_EXACT)
    two = make_world(ellc, shape, arith=ellc.ARITH_FAST, grid_batch=4, max_batch=7)
    try:
        src, dst, Ts = batch_args(one)
        for level in range(one["L"]):
            a = one["ctx"].sim3_step(src, dst, Ts, level=level, **fkw(FILTERS[0]))
            b = two["ctx"].sim3_step(src, dst, Ts, level=level, **fkw(FILTERS[0]))
            assert int(a["n_photo"].sum()) > 0 and a.tobytes() == b.tobytes(), level
    finally:
        one["ctx"].close(); two["ctx"].close()


def test_2048_requests_in_one_call(world64):
    """B is not bounded by max_keyframes (5 here): the largest batch, all ordered pairs of the three scenes over and over."""
    ctx = world64["ctx"]
    pairs = [(s, d) for s in range(3) for d in range(3)]
    src = [pairs[b % 9][0] for b in range(2048)]
    dst = [pairs[b % 9][1] for b in range(2048)]
    Ts = np.stack([world64["Ts"][b % 3] for b in range(2048)])
    got = ctx.sim3_step(src, dst, Ts, **fkw(FILTERS[0]))
    assert got.shape == (2048,)
    for b in range(9):
        check_against(got[b], reference(world64, src[b], dst[b], 0, Ts[b], FILTERS[0]), "request %d of 2048" % b, quiet=True)
    for b in range(9, 2048):
        assert got[b:b + 1].tobytes() == got[b % 9:b % 9 + 1].tobytes(), b
    small = ctx.sim3_step(src[:9], dst[:9], Ts[:9], **fkw(FILTERS[0]))   # after the staging has grown: the same bytes
    assert small.tobytes() == got[:9].tobytes()


PATTERN = 0xA5


def raw_step(ctx, ellc, src, dst, T, level=0, flt=(0.0, 0, 1.0, 1), params=(16.0, 1.345, 9.0, 1.0), null=None, B=None):
    """(status, out untouched?) of ellc_keyframe_sim3_step, not raised. null: which pointer argument to pass as NULL."""
    s = np.ascontiguousarray(src, np.int32).reshape(-1)
    d = np.ascontiguousarray(dst, np.int32).reshape(-1)
    B = s.size if B is None else B
    Tn = np.ascontiguousarray(np.tile(np.asarray(T, np.float32).reshape(-1)[:12], max(s.size, 1)))
    f = ellc._lib.EllcMapFilter(flt[0], int(flt[1]), flt[2], int(flt[3]))
    prm = ellc._lib.EllcSim3Params(*params)
    out = np.full(320 * max(s.size, abs(B), 1), PATTERN, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    st = ctx._l.ellc_keyframe_sim3_step(ctx.h, B, None if null == "src" else p(s), None if null == "dst" else p(d), None if null == "T" else p(Tn),
                                        int(level), None if null == "filter" else C.byref(f), None if null == "params" else C.byref(prm),
                                        None if null == "out" else p(out))
    return st, bool((out == PATTERN).all())


def raw_align(ctx, ellc, T, level_from=0, level_to=0, max_iter=10, eps=1e-4, params=(16.0, 1.345, 9.0, 1.0), trace_capacity=None, null=None, src=(0,), dst=(1,)):
    """(status, every output untouched?) of ellc_keyframe_sim3_align for one pair, not raised."""
    s = np.ascontiguousarray(src, np.int32); d = np.ascontiguousarray(dst, np.int32)
    Tn = np.ascontiguousarray(T, np.float32).reshape(12)
    f = ellc._lib.EllcMapFilter(0.0, 0, 1.0, 1)
    prm = ellc._lib.EllcSim3Params(*params)
    cap = 64 * 8 + 1
    outs = dict(T=np.full(48, PATTERN, np.uint8), rec=np.full(320, PATTERN, np.uint8), iters=np.full(4 * 8, PATTERN, np.uint8),
                tT=np.full(48 * cap, PATTERN, np.uint8), tR=np.full(320 * cap, PATTERN, np.uint8))
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    st = ctx._l.ellc_keyframe_sim3_align(ctx.h, 1, p(s), p(d), p(Tn), int(level_from), int(level_to), C.byref(f), C.byref(prm), int(max_iter),
                                         C.c_float(eps), None if null == "T_out" else p(outs["T"]), None if null == "out" else p(outs["rec"]),
                                         p(outs["iters"]), p(outs["tT"]), p(outs["tR"]), cap if trace_capacity is None else trace_capacity)
    return st, all(bool((a == PATTERN).all()) for a in outs.values())


def test_refused_calls_write_nothing_and_touch_no_slot(world64, ellc):
    ctx, T = world64["ctx"], world64["Ts"][1]

    def snapshot():
        out = []
        for s in range(4):
            for l in range(world64["L"]):
                d, v = ctx.keyframe_depth_level(s, l)
                out.append(d.tobytes() + v.tobytes() + ctx.image_level(True, s, l)[0].tobytes())
        return out

    before = snapshot()

    def refused(code, src=(0,), dst=(1,), **kw):
        st, untouched = raw_step(ctx, ellc, list(src), list(dst), T, **kw)
        assert st == code and untouched, (st, code, untouched, src, dst, kw)

    def accepted(src=(0,), dst=(1,), **kw):
        st, untouched = raw_step(ctx, ellc, list(src), list(dst), T, **kw)
        assert st == 0 and not untouched, (st, src, dst, kw)

    accepted()
    refused(BAD_ARG, B=0); refused(BAD_ARG, B=-1); refused(BAD_ARG, src=[0] * 2049, dst=[1] * 2049)           # B out of range
    refused(BAD_ARG, src=(-1,)); refused(BAD_ARG, src=(N_SLOTS,)); refused(BAD_ARG, src=(0, N_SLOTS), dst=(1, 1))   # a source slot out of range
    refused(BAD_ARG, dst=(-1,)); refused(BAD_ARG, dst=(N_SLOTS,)); refused(BAD_ARG, src=(0, 0), dst=(1, N_SLOTS))   # a destination slot out of range
    refused(BAD_ARG, level=-1); refused(BAD_ARG, level=world64["L"])
    for null in ("src", "dst", "T", "filter", "params"):
        refused(BAD_ARG, null=null)
    assert raw_step(ctx, ellc, [0], [1], T, null="out")[0] == BAD_ARG
    refused(BAD_ARG, flt=(0.0, -1, 1.0, 1)); refused(BAD_ARG, flt=(0.0, 9, 1.0, 1)); refused(BAD_ARG, flt=(0.0, 0, 1.0, 0))
    refused(BAD_ARG, flt=(0.0, 0, -1.0, 1)); refused(BAD_ARG, flt=(0.0, 0, np.inf, 1)); refused(BAD_ARG, flt=(0.0, 0, np.nan, 1))
    refused(BAD_ARG, flt=(np.nan, 0, 1.0, 1))
    accepted(flt=(-1.0, 8, 0.0, 1)); accepted(flt=(np.inf, 0, 1.0, 7))                                         # the edges of the accepted range
    good = (16.0, 1.345, 9.0, 1.0)
    for k in range(4):   # every parameter: NaN, inf, negative; sigma_i2 and huber_k also 0
        for bad in (np.nan, np.inf, -1.0) + ((0.0,) if k < 2 else ()):
            refused(BAD_ARG, params=good[:k] + (bad,) + good[k + 1:])
    accepted(params=(1e-3, 1e-3, 0.0, 0.0))
    # a slot with an image only, as source and as destination, alone and behind a good request
    refused(NOT_READY, src=(IMAGE_ONLY_SLOT,)); refused(NOT_READY, dst=(IMAGE_ONLY_SLOT,))
    refused(NOT_READY, src=(0, IMAGE_ONLY_SLOT), dst=(1, 1)); refused(NOT_READY, src=(0, 0), dst=(1, IMAGE_ONLY_SLOT))
    with pytest.raises(ellc.EllcError):
        ctx.sim3_step([IMAGE_ONLY_SLOT], [0], [T])
    # the loop's own refusals
    assert raw_align(ctx, ellc, T) == (0, False)
    for kw in (dict(level_from=0, level_to=1), dict(level_from=world64["L"], level_to=0), dict(level_to=-1), dict(max_iter=0), dict(max_iter=65),
               dict(eps=-1.0), dict(eps=np.nan), dict(eps=np.inf), dict(trace_capacity=10), dict(level_from=1, trace_capacity=20),
               dict(params=(0.0, 1.345, 9.0, 1.0)), dict(src=(N_SLOTS,)), dict(null="T_out"), dict(null="out")):
        st, untouched = raw_align(ctx, ellc, T, **kw)
        assert st == BAD_ARG and untouched, (kw, st, untouched)
    st, untouched = raw_align(ctx, ellc, T, dst=(IMAGE_ONLY_SLOT,))
    assert st == NOT_READY and untouched
    assert raw_align(ctx, ellc, T, trace_capacity=11) == (0, False) and raw_align(ctx, ellc, T, level_from=1, trace_capacity=21) == (0, False)
    # an all-zero depth is a map without hypotheses, not an error: as source nothing is kept, as destination the depth term is empty
    as_src = ctx.sim3_step([ZERO_SLOT], [0], [T])
    assert not any(as_src.tobytes())
    as_dst = ctx.sim3_step([0], [ZERO_SLOT], [IDENTITY])[0]
    assert int(as_dst["n_kept"]) == int(as_dst["n_in_view"]) > 0 and int(as_dst["n_photo"]) > 0
    assert int(as_dst["n_depth"]) == int(as_dst["n_depth_gated"]) == 0 and float(as_dst["chi2_depth"]) == 0 and float(as_dst["H"][27]) == 0
    # the context still answers as before, and no plane of any slot has changed
    src, dst, Ts = batch_args(world64)
    got = ctx.sim3_step(src, dst, Ts, **fkw(FILTERS[0]))
    for b, (s, d, t) in enumerate(BATCH):
        check_against(got[b], reference(world64, s, d, 0, world64["Ts"][t], FILTERS[0]), "after the refusals %d" % b, quiet=True)
    assert snapshot() == before


def ulp_of(x):
    return float(np.spacing(np.float32(x)))


def test_the_loop_link_by_link(world, ellc):
    """From the trace: every record is sim3_step's at the trace's T, every next T is sim3_apply(sim3_solve(record), T) bit for bit (the
    same host code) and within 2 f32 ulp of max |T| of numpy's solve and scipy's expm from the same record; iters_out, T_out and out
    agree with the trace; a destination without hypotheses leaves T unchanged with 0 iterations."""
    ctx, L = world["ctx"], world["L"]
    batch = BATCH + [(0, ZERO_SLOT, 1)]
    src, dst, Ts = batch_args(world, batch)
    res = ctx.sim3_align(src, dst, Ts, level_from=L - 1, level_to=0, max_iter=MAX_ITER, eps=EPS, trace=True, **fkw(FILTERS[0]))
    by_level = {l: [] for l in range(L)}   # (pair, entry) of every evaluation, by the level the replay puts it on
    updates = 0
    for b in range(len(batch)):
        tT, tR = res["trace_T"][b], res["trace_rec"][b]
        assert tT[0].tobytes() == Ts[b].tobytes()
        e = 0
        for k, level in enumerate(range(L - 1, -1, -1)):
            made = 0
            while True:
                by_level[level].append((b, e))
                xi, singular = ellc.sim3_solve(tR[e])
                T_next = tT[e] if singular else ellc.sim3_apply(xi, tT[e])
                e += 1
                assert e < len(tT), (b, level)
                assert tT[e].tobytes() == T_next.tobytes(), (b, level, e)
                if singular:
                    break
                made += 1
                updates += 1
                ref_xi, ref_singular = S.solve(tR[e - 1]["H"], tR[e - 1]["b"])
                assert not ref_singular
                T_np = S.apply(ref_xi, tT[e - 1])
                dist, bound = float(np.abs(T_next.astype(np.float64) - T_np.astype(np.float64)).max()), 2 * ulp_of(np.abs(T_np).max())
                assert dist <= bound, (b, level, e, dist, bound, np.linalg.cond(S.mirrored(tR[e - 1]["H"])))
                if np.abs(xi).max() <= EPS or made >= MAX_ITER:
                    break
            assert int(res["iters"][b, k]) == made, (b, level)
        by_level[0].append((b, e))   # the final evaluation
        assert e == len(tT) - 1, (b, e, len(tT))
        assert tT[e].tobytes() == res["T"][b].tobytes() and tR[e].tobytes() == res["rec"][b:b + 1].tobytes(), b
    for level, entries in by_level.items():   # every record of the trace is the step's at that T (one call per level: records do not depend on the batch)
        got = ctx.sim3_step([src[b] for b, _ in entries], [dst[b] for b, _ in entries], np.stack([res["trace_T"][b][e] for b, e in entries]), level=level,
                            **fkw(FILTERS[0]))
        for k, (b, e) in enumerate(entries):
            assert got[k:k + 1].tobytes() == res["trace_rec"][b][e:e + 1].tobytes(), (level, b, e)
    print(world["shape"], "updates checked", updates, "iters", res["iters"].tolist())
    assert updates > 0
    z = len(batch) - 1
    assert res["T"][z].tobytes() == Ts[z].tobytes() and not res["iters"][z].any() and len(res["trace_T"][z]) == L + 1
    # without traces and without iters_out: the same T and records
    plain = ctx.sim3_align(src, dst, Ts, level_from=L - 1, level_to=0, max_iter=MAX_ITER, eps=EPS, **fkw(FILTERS[0]))
    assert plain["T"].tobytes() == res["T"].tobytes() and plain["rec"].tobytes() == res["rec"].tobytes()
    one = ctx.sim3_align(src[1:2], dst[1:2], Ts[1:2], level_from=L - 1, level_to=0, max_iter=MAX_ITER, eps=EPS, **fkw(FILTERS[0]))
    assert one["T"].tobytes() == res["T"][1:2].tobytes() and one["iters"].tolist() == res["iters"][1:2].tolist()


XI_START = np.array([0.01, 0.008, 0.012, 0.01, 0.01, 0.008, 0.0])
RECOVERY_FILTER = (0, 0, 1.0, 1)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_recovery_of_a_known_similarity(ellc, shape):
    """Two keyframes of one scene (make_shared_frame_batch, seed 21, rot 0.02, trans 0.04); the source is keyframe 0 with its depth
    times k and its variance over k^2, the destination keyframe 1, so the true transform is [R / k | t]. The start is the truth
    left-multiplied by exp(+xi) with a log-scale of 0.1 and by exp(-xi) with one of -0.08. A condition on the inputs: the reference's
    own loop (numpy solve, scipy expm, f32 rule) ends within 1 % of the scale. The library's loop differs from it in the order of the
    double sums and by at most an f32 ulp of T per update: its scale, rotation and translation errors may exceed the reference
    loop's by a tenth of those."""
    w, h, L = SHAPES[shape]
    scenes = synth.make_shared_frame_batch(w, h, 2, 21, rot=0.02, trans=0.04)
    ctx = gpu_problem(ellc, w, h, L, scenes, max_keyframes=4)
    try:
        rigid = np.linalg.inv(synth.se3_exp(scenes[1]["xi_true"].astype(np.float64))) @ synth.se3_exp(scenes[0]["xi_true"].astype(np.float64))
        world = dict(ctx=ctx, planes={}, intrinsics=scenes[0]["intrinsics"])
        cases = []
        for slot, k in ((2, 2.0), (3, 0.5)):
            ctx.keyframe_upload(slot, scenes[0]["kf_image"])
            ctx.keyframe_set_depth(slot, scenes[0]["depth0"] * np.float32(k), scenes[0]["var0"] / np.float32(k * k))
            T_true = rigid[:3].copy(); T_true[:, :3] /= k
            for sign, sigma in ((1.0, 0.1), (-1.0, -0.08)):
                xi = sign * XI_START; xi[6] = sigma
                levels = [[0]] + ([[1, 0]] if shape == "64x48" else [])
                for lv in levels:
                    cases.append((slot, k, T_true, S.apply(xi, T_true.astype(F).reshape(12)), lv))
        for lv in ([0], [1, 0]):
            sel = [c for c in cases if c[4] == lv]
            if not sel:
                continue
            res = ctx.sim3_align([c[0] for c in sel], [1] * len(sel), np.stack([c[3] for c in sel]), level_from=lv[0], level_to=0, max_iter=MAX_ITER,
                                 eps=EPS, **fkw(RECOVERY_FILTER))
            for n, (slot, k, T_true, T0, _) in enumerate(sel):
                T_ref, iters_ref, _ = S.align(lambda s, l: planes_of(world, s, l), slot, 1, lambda l: intr_of(world, l), T0, lv, RECOVERY_FILTER,
                                              max_iter=MAX_ITER, eps=EPS)
                e_start, e_ref, e_gpu = S.sim3_errors(T0, T_true), S.sim3_errors(T_ref, T_true), S.sim3_errors(res["T"][n], T_true)
                print("%s k %.1f levels %s: start scale %.3g rot %.3g trans %.3g | reference scale %.3g rot %.3g trans %.3g iters %s | library scale %.3g "
                      "rot %.3g trans %.3g iters %s" % ((shape, k, lv) + e_start + e_ref + (iters_ref,) + e_gpu + (res["iters"][n].tolist(),)))
                assert e_ref[0] <= 0.01, ("the reference's own loop misses the scale", shape, k, lv, e_ref)
                for name, a, b in zip(("scale", "rotation", "translation"), e_gpu, e_ref):
                    assert a <= 1.1 * b, (name, shape, k, lv, a, b)
    finally:
        ctx.close()


def test_driver_match_sim3_file(tmp_path):
    """ellc_main --match-sim3 on the 33-frame loop-closure sequence of tests/test_gpu_driver.py: one line per line of
    matchframes_globalopt.txt, finite fields with n_photo > 0; every other output byte-identical to a run without the flag."""
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
    r = subprocess.run(base + [str(plain), "LC"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()
    sfile = tmp_path / "sim3.txt"
    r = subprocess.run(base + [str(flagged), "LC", "--match-sim3", str(sfile)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()
    assert sorted(p.name for p in plain.iterdir()) == sorted(p.name for p in flagged.iterdir())
    for p in plain.iterdir():
        assert p.read_bytes() == (flagged / p.name).read_bytes(), p.name
    matches = (flagged / "matchframes_globalopt.txt").read_text().strip().split("\n")
    lines = sfile.read_text().strip().split("\n")
    assert len(matches) >= 3 and len(lines) == len(matches)
    for m, l in zip(matches, lines):
        c = l.split(" ")
        print(l)
        assert len(c) == 14 and c[:2] == m.split(" ")[:2]   # frameId kfId scale tx ty tz wx wy wz n_photo n_depth chi2_photo chi2_depth iters
        values = [float(v) for v in c[2:]]
        assert all(np.isfinite(v) for v in values)
        n_photo, n_depth, iters = int(c[9]), int(c[10]), int(c[13])
        assert n_photo > 0 and n_depth >= 0 and 0 <= iters <= 20 and values[0] > 0 and values[9] >= 0 and values[10] >= 0
