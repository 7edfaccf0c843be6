"""CPU checks of tests/sweep_depth_reference.py, the numpy restatement of ellc_keyframe_sweep_depth's rule that the GPU tests hold the
kernel to: scalar against vectorised on the GPU tests' scenes and on the recovery scene, a hand-worked answer on a 5x5 level, every
status reached, ties, the recovery of the inverse depths of a thinned map at true transforms, and what a wrong light does."""
import numpy as np
import pytest

import refine_depth_reference as R
import sim3_reference as S
import sweep_depth_reference as W

F = np.float32
SHAPES = [(64, 48), (23, 17), (131, 67)]
_cache = {}


def cached(key, make):
    """A vectorised result, computed once and left unchanged."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def unrelated_world(w, h):
    """The world of tests/test_gpu_sim3.py on the CPU (level 0): scenes 11, 12, 13 as slots 0, 1, 2; scene_transforms' three transforms
    and the 3.3-pixel shift. K is scene 11's image with NO hypothesis at all (the GPU world's all-zero slot 3) or scene 11 itself."""
    scenes = [S.make_scene(w, h, seed) for seed in (11, 12, 13)]
    m = float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0]))
    intr = S.level_intrinsics(*scenes[0]["intrinsics"], 0)
    shift = np.array([1, 0, 0, 3.3 * m / float(intr[0]), 0, 1, 0, 0, 0, 0, 1, 0], F)
    Ts = np.concatenate([S.scene_transforms(m), shift[None]])
    return scenes, intr, Ts, m


def run_unrelated(world, B, light, empty, fn=W.sweep, **kw):
    scenes, intr, Ts, m = world
    vl = R.view_list(B)
    K = scenes[0]
    kf = (np.zeros_like(K["depth0"]), np.full_like(K["var0"], -1), K["kf_image"]) if empty else (K["depth0"], K["var0"], K["kf_image"])
    params = dict(d_min=0.4 / m, d_max=2.5 / m, n_samples=8, min_grad2=4.0, min_views=min(2, B))
    extra = {k: kw.pop(k) for k in ("every",) if k in kw}
    params.update(kw)
    return fn(kf, [scenes[s]["kf_image"] for s, _ in vl], intr, [Ts[t] for _, t in vl], [light] * B, params, **extra)


def run_thinned(w, h, fn=W.sweep, lights=None, image=None, **kw):
    scenes, Ts, d_true, params = cached(("thinned", w, h), lambda: W.thinned_world(w, h))
    K = scenes[0]
    intr = W.level_intrinsics(*K["intrinsics"], 0)
    extra = {k: kw.pop(k) for k in ("every",) if k in kw}
    p = dict(params)
    p.update(kw)
    img = K["kf_image"] if image is None else image
    return fn((K["depth0"], K["var0"], img), [s["kf_image"] for s in scenes[1:]], intr, Ts, lights, p, **extra), d_true


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_scalar_equals_vectorised(shape):
    """Planes as bytes and integer stats with ==: in full at 23x17, on every 7th swept pixel elsewhere."""
    world = cached(("world", shape), lambda: unrelated_world(*shape))
    every = 1 if shape == (23, 17) else 7
    for B, light, empty in ((3, R.LIGHTS[0], True), (1, R.LIGHTS[1], True), (4, R.LIGHTS[1], False)):
        a = cached((shape, B, light, empty), lambda: run_unrelated(world, B, light, empty))
        b = run_unrelated(world, B, light, empty, fn=W.sweep_scalar, every=every)
        assert W.results_equal(a, b, at=None if every == 1 else b["processed"]), (B, light, empty)
        assert a["n_swept"] == sum(a[k] for k in W.STATUS_NAMES[1:]) and a["n_not_swept"] == shape[0] * shape[1] - a["n_swept"]
        assert a["n_swept"] > 50 and (a["n_ok"] == 0) == empty
        Z0 = (np.zeros_like(world[0][0]["depth0"]) if empty else world[0][0]["depth0"]).astype(F)
        changed = a["depth"].view(np.uint32) != Z0.view(np.uint32)
        assert not (changed & (a["status"] != W.CREATED)).any()   # every pixel that gets no hypothesis keeps K's bits
    a, d_true = cached(("thinned result", shape), lambda: run_thinned(*shape))
    b, _ = run_thinned(*shape, fn=W.sweep_scalar, every=every)
    assert W.results_equal(a, b, at=None if every == 1 else b["processed"]) and a["n_created"] > 0


# 5 columns x 5 rows, fx = fy = 4, cx = cy = 2, one view at T = [I | (1/4, 0, 0)]: a pixel (x, y) at the inverse depth d lands at
# u = x + fx tx d = x + d, v = y. K's image is 16 x + 16 and holds no hypothesis, the view's image is 16 x + 7, so inside a cell
# Iw = 16 u + 7 and rp = 16 d - 9 wherever the taps exist: zero at d* = 9/16. sigma_i2 = 1 (w0 = sp = 1), huber_k = 100 (never reached),
# range [1/4, 3/4], 3 samples: dstep = 1/4, rp = -5, -1, 3, c_j = 25, 1, 9, and with five pattern pixels and one view cost = 125, 5, 45.
# k1 = 1, curv = (125 - 10) + 45 = 160, off = (0.5 * 80) / 160 = 1/4, d = 1/2 + 1/16 = 9/16 = d*: the cost is a parabola in d, so the
# parabola through three samples has its vertex at the exact depth. v = 1 * ((2 / 16) / (1 * 160)) = 1/1280. Z = 1 / 0.75 is not exact
# in f32, so the third cost is 45 up to a few ulp and d is held to 2^-20.
# Taps: a pattern pixel at x = 4 lands at u >= 4.25 and has none, one at y = 4 has v = 4 and has none: pixels with px = 3 or py = 3
# have no valid sample; the four pixels px, py in {1, 2} are created; the border is not swept.
def hand_world(**kw):
    x = np.tile(np.arange(5), (5, 1))
    K = (16 * x + 16).astype(np.uint8)
    V = (16 * x + 7).astype(np.uint8)
    T = np.array([1, 0, 0, 0.25, 0, 1, 0, 0, 0, 0, 1, 0], F)
    params = dict(sigma_i2=1.0, huber_k=100.0, d_min=0.25, d_max=0.75, n_samples=3, min_views=1, min_grad2=100.0)
    params.update(kw)
    kf = (np.zeros((5, 5), F), np.full((5, 5), -1, F), K)
    return kf, [V], (F(4), F(4), F(2), F(2)), [T], None, params


def test_hand_worked_level():
    for fn in (W.sweep, W.sweep_scalar):
        res = fn(*hand_world())
        want = np.zeros((5, 5), np.uint8)
        want[1:4, 1:4] = W.NO_VALID_SAMPLE
        want[1:3, 1:3] = W.CREATED
        assert np.array_equal(res["status"], want)
        assert (res["n_ok"], res["n_swept"], res["n_created"], res["n_no_valid_sample"], res["sum_views"]) == (0, 9, 4, 5, 4)
        made = want == W.CREATED
        assert np.abs(res["d"][made].astype(np.float64) - 9 / 16).max() <= 2.0 ** -20
        assert np.abs(res["depth"][made].astype(np.float64) - 16 / 9).max() <= 2.0 ** -18
        assert np.abs(res["var"][made].astype(np.float64) * 1280 - 1).max() <= 2.0 ** -18
        assert (res["views"][made] == 1).all() and not res["views"][~made].any()
        assert abs(res["sum_cost"] - 20.0) <= 1e-5
        assert (res["depth"][~made] == 0).all() and (res["var"][~made] == -1).all()
    res = W.sweep(*hand_world())
    assert res["costs"][:2, 0].tolist() == [125.0, 5.0] and abs(float(res["costs"][2, 0]) - 45.0) <= 1e-4


def test_every_status_is_reached():
    seen = set()

    def run(**kw):
        a, b = W.sweep(*hand_world(**kw)), W.sweep_scalar(*hand_world(**kw))
        assert W.results_equal(a, b), kw
        seen.update(np.unique(a["status"]).tolist())
        return a

    assert run()["n_created"] == 4                                               # NOT_SWEPT, CREATED, NO_VALID_SAMPLE
    assert run(d_min=0.625, d_max=0.875)["n_at_range_end"] == 4                  # the minimum lies below the range: k1 = 0
    assert run(d_min=0.25, d_max=0.5)["n_at_range_end"] == 4                     # ... above it: k1 = n_samples - 1
    assert run(max_cost=4.0)["n_cost_too_high"] == 4                             # c1 = 5
    assert run(max_cost=5.5)["n_created"] == 4
    # five samples: rp = -5, -3, -1, 1, 3, cost = 125, 45, 5, 5, 45 (up to rounding): c2 = 45 at |k - k1| = 2
    assert run(n_samples=5, distinct_ratio=0.1)["n_not_distinct"] == 4           # 5 <= 4.5 fails
    assert run(n_samples=5, distinct_ratio=0.2)["n_created"] == 4
    assert run(sigma_i2=1e6, var_scale=3e38)["n_flat"] == 4                      # v = 3e38 * 0.125 / 160e-6 overflows
    assert run(min_views=1, min_grad2=2000.0)["n_swept"] == 0                    # gxc * gxc = 1024
    assert seen == set(range(7))
    # the statuses 3..6 on real images too: the unrelated world reaches NOT_DISTINCT and AT_RANGE_END, a cost bound COST_TOO_HIGH
    world = cached(("world", (64, 48)), lambda: unrelated_world(64, 48))
    a = cached(((64, 48), 3, R.LIGHTS[0], True), lambda: run_unrelated(world, 3, R.LIGHTS[0], True))
    assert a["n_not_distinct"] > 0 and a["n_at_range_end"] > 0 and a["n_created"] > 0
    assert run_unrelated(world, 3, R.LIGHTS[0], True, max_cost=1e-3)["n_cost_too_high"] > 0


def test_decision_cases():
    """Rule 4 on constructed costs: ties in k1 go to the lower k, a neighbour that is not valid, c2's window, FLAT by curvature."""
    P = W.Params(dict(n_samples=6, min_views=2, d_min=1.0, d_max=2.0))
    c = lambda *v: [F(x) for x in v]   # noqa: E731
    two = [2] * 6
    st, n1, d, v, c1 = W.decide(c(9, 3, 7, 3, 8, 9), two, P)          # a tie between k = 1 and k = 3: k1 = 1
    assert st == W.NOT_DISTINCT and c1 == 3                            # ... and the other 3 is the c2 that fails the ratio
    st, n1, d, v, c1 = W.decide(c(9, 3, 7, 30, 30, 30), two, P)
    assert st == W.CREATED and float(d) == float(F(P.d(1) + F(F(F(0.5) * F(2.0)) / F(10.0)) * P.dstep))
    assert W.decide(c(9, 7, 7, 3, 3, 9), two, P)[0] == W.CREATED      # the tie's other half is the neighbour, not c2: k1 = 3, cp = 3
    assert float(W.decide(c(9, 7, 7, 3, 3, 9), two, P)[2]) == float(F(P.d(3) + F(F(0.5) * P.dstep)))
    assert W.decide(c(3, 9, 9, 9, 9, 9), two, P)[0] == W.AT_RANGE_END and W.decide(c(9, 9, 9, 9, 9, 3), two, P)[0] == W.AT_RANGE_END
    assert W.decide(c(9, 9, 9, 9, 9, 9), two, P)[0] == W.AT_RANGE_END                     # all equal: k1 = 0
    assert W.decide(c(9, 3, 7, 30, 30, 30), [1, 2, 2, 2, 2, 2], P)[0] == W.AT_RANGE_END   # k1 - 1 not valid
    assert W.decide(c(9, 3, np.nan, 30, 30, 30), two, P)[0] == W.AT_RANGE_END             # k1 + 1 not valid (NaN)
    assert W.decide(c(9, 3, np.inf, 30, 30, 30), two, P)[0] == W.AT_RANGE_END             # ... (inf)
    assert W.decide(c(9, 3, 7, 1, 1, 1), [2, 2, 2, 1, 1, 0], P)[0] == W.CREATED           # samples that are not valid never win and never are c2
    assert W.decide(c(1, 1, 1, 1, 1, 1), [1] * 6, P) == (W.NO_VALID_SAMPLE, 0, None, None, None)
    assert W.decide(c(np.nan, np.inf, np.nan, np.inf, np.nan, np.nan), two, P)[0] == W.NO_VALID_SAMPLE
    assert W.decide(c(9, 3, 7), [2, 2, 2], W.Params(dict(n_samples=3, d_min=1.0, d_max=2.0)))[0] == W.CREATED   # no sample for c2: the test passes
    tiny = np.float32(1e-45)
    with np.errstate(over="ignore"):
        assert W.decide(c(tiny, 0, 0, 9, 9, 9), two, P)[0] == W.FLAT      # curv = 1e-45 > 0, v overflows
        assert W.decide(c(3e38, 1, 3e38, 3e38, 3e38, 3e38), two, P)[0] == W.FLAT   # curv overflows
    # the vectorised decision is the same function: the constructed costs through sweep's own lines, by way of the hand world's shape
    st, n1, d, v, c1 = W.decide(c(9, 3, 7, 30, 30, 30), [2, 3, 2, 2, 2, 2], P)
    assert n1 == 3 and float(v) == float(F(F(1.0) * F(F(F(2.0) * F(P.dstep * P.dstep)) / F(F(3.0) * F(10.0)))))


@pytest.mark.parametrize("shape", [(64, 48), (131, 67)], ids=lambda s: "%dx%d" % s)
def test_recovery_of_a_thinned_map(shape):
    """K's depth0 kept at (x + 2 y) % 3 == 0, four views at their true transforms, the range [0.5 min, 1.5 max] of the true inverse
    depths, 32 samples, ratio 0.7: at least half of the swept pixels are created and at least 0.9 of the created lie within 5 % of the
    true inverse depth. The f32 rule gives 423 of 440 (0.96) created, median relative error 0.0029, 0.983 within 5 % at 64x48, and 1399
    of 1496 (0.94), 0.0019, 0.999 at 131x67."""
    res, d_true = cached(("thinned result", shape), lambda: run_thinned(*shape))
    n_swept, n_made, frac, med, within = W.recovery_figures(res, d_true)
    made = res["status"] == W.CREATED
    ratio = float(np.median(np.abs(res["d"][made].astype(np.float64) - d_true[made]) / np.sqrt(res["var"][made].astype(np.float64))))
    print("%dx%d: swept %d, created %d (%.3f), median relative error %.4f, within 5 %%: %.4f, median |error| / sqrt(var) %.3f" % (
        shape + (n_swept, n_made, frac, med, within, ratio)))
    assert n_swept > 400 and frac >= 0.5 and within >= 0.9
    assert (res["views"][made] >= 2).all()


def test_the_light_is_needed():
    """K's image at 0.8 I (rounded to u8): with the light (1, 0) fewer than a tenth as many pixels are created as with (1 / 0.8, 0)."""
    scenes = cached(("thinned", 64, 48), lambda: W.thinned_world(64, 48))[0]
    dim = np.rint(0.8 * scenes[0]["kf_image"].astype(np.float64)).astype(np.uint8)
    # the swept set is read from K's own image: with the dim image fewer pixels reach min_grad2, in both runs alike
    right, _ = run_thinned(64, 48, lights=[(1 / 0.8, 0.0)] * 4, image=dim)
    wrong, _ = run_thinned(64, 48, lights=[(1.0, 0.0)] * 4, image=dim)
    print("created with the light (1.25, 0): %d of %d; with (1, 0): %d" % (right["n_created"], right["n_swept"], wrong["n_created"]))
    assert right["n_swept"] == wrong["n_swept"] and right["n_created"] > 100 and wrong["n_created"] < 0.1 * right["n_created"]
