"""CPU checks of tests/map_points_reference.py, the numpy restatement of ellc_keyframe_map_points' rule that the GPU tests hold the
kernels to: a hand-written known answer, scalar against vectorised, and the seeded scenes really reaching every branch of the rule."""
import numpy as np
import pytest

import map_points_reference as R

F = np.float32
FILTERS = [(0, 0, 1.0, 1), (0.0125, 0, 1.0, 1), (0, 3, 0.02, 1), (0.0125, 2, 0.02, 2), (0, 0, 1.0, 3)]
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def hand_planes():
    inf, nan = np.inf, np.nan
    depth = np.array([[2, 2, 0, inf, 4],
                      [2, -1, 0, nan, 4],
                      [4, 0, 0, 0, 0],
                      [1, 0, 0, 8, 8]], F)
    var = np.full((4, 5), 0.01, F)
    var[0, 1] = -1.0
    img = (10 * np.arange(4)[:, None] + np.arange(5)[None, :]).astype(np.uint8)
    return depth, var, img


# (x, y, z, px, py, intensity, support) typed out by hand: fx = fy = 2, cx = cy = 1, so X = (px - 1) Z / 2, Y = (py - 1) Z / 2.
# ok pixels: (0,0) (0,4) (1,0) (1,4) (2,0) (3,0) (3,3) (3,4) as (row, col); (0,1) has var -1, (1,1) depth -1, (0,3) inf, (1,3) NaN.
# k2 = 1, every var 0.01: a neighbour supports iff (1/Zn - 1/Zc)^2 <= 0.02.
#   (0,0) Z 2, a corner: of its three neighbours only (1,0) is ok, 1/2 - 1/2 = 0 -> 1
#   (0,4) Z 4, a corner: (0,3) inf, (1,3) NaN, (1,4) Z 4 -> 1
#   (1,0) Z 2, left edge: (0,0) supports; (2,0) Z 4: (1/4 - 1/2)^2 = 0.0625 > 0.02 -> 1
#   (1,4) Z 4, right edge: (0,4) supports -> 1
#   (2,0) Z 4: (1,0) Z 2 fails (0.0625), (3,0) Z 1 fails ((1 - 1/4)^2) -> 0
#   (3,0) Z 1, a corner: (2,0) fails -> 0
#   (3,3) and (3,4), Z 8 both, bottom edge: each other -> 1
HAND = [(-1.0, -1.0, 2.0, 0, 0, 0, 1),
        (6.0, -2.0, 4.0, 4, 0, 4, 1),
        (-1.0, 0.0, 2.0, 0, 1, 10, 1),
        (6.0, 0.0, 4.0, 4, 1, 14, 1),
        (-2.0, 2.0, 4.0, 0, 2, 20, 0),
        (-0.5, 1.0, 1.0, 0, 3, 30, 0),
        (8.0, 8.0, 8.0, 3, 3, 33, 1),
        (12.0, 8.0, 8.0, 4, 3, 34, 1)]


def hand_records(rows, source=0):
    out = np.zeros(len(rows), R.POINT_DTYPE)
    for i, (x, y, z, px, py, inten, sup) in enumerate(rows):
        out[i] = (x, y, z, F(0.01), px, py, inten, sup, source)
    return out


@pytest.mark.parametrize("fn", [R.map_points, R.map_points_scalar])
def test_hand_written_known_answer(fn):
    depth, var, img = hand_planes()
    intr = (F(2), F(2), F(1), F(1))
    assert R.records_equal(fn(depth, var, img, intr, IDENTITY, (0, 0, 1.0, 1)), hand_records(HAND))
    assert R.records_equal(fn(depth, var, img, intr, IDENTITY, (0, 1, 1.0, 1), source=3), hand_records([h for h in HAND if h[6] >= 1], source=3))
    # stride 2 keeps even columns of even rows; the support is still that of the full-resolution neighbourhood
    assert R.records_equal(fn(depth, var, img, intr, IDENTITY, (0, 0, 1.0, 2)), hand_records([HAND[0], HAND[1], HAND[4]]))
    # max_var below every variance: nothing; k2 = 0 with equal depths still supports (0 <= 0)
    assert fn(depth, var, img, intr, IDENTITY, (0.005, 0, 1.0, 1)).size == 0
    assert [int(s) for s in fn(depth, var, img, intr, IDENTITY, (0, 0, 0.0, 1))["support"]] == [1, 1, 1, 1, 0, 0, 1, 1]
    # a transform with a scale and a translation: x = 2 X + 1, y = 3 Y - 1, z = Z + 0.5
    T = [2, 0, 0, 1, 0, 3, 0, -1, 0, 0, 1, 0.5]
    got = fn(depth, var, img, intr, T, (0, 0, 1.0, 1))
    assert [tuple(float(v) for v in (g["x"], g["y"], g["z"])) for g in got] == [(2 * h[0] + 1, 3 * h[1] - 1, h[2] + 0.5) for h in HAND]


@pytest.mark.parametrize("flt", FILTERS)
def test_scalar_and_vectorised_agree_on_the_smallest_shape(flt):
    s = R.make_scene(23, 17, 3)
    intr = R.level_intrinsics(*s["intrinsics"], 0)
    a = R.map_points(s["depth0"], s["var0"], s["kf_image"], intr, R.scaled_transform(), flt, source=2)
    b = R.map_points_scalar(s["depth0"], s["var0"], s["kf_image"], intr, R.scaled_transform(), flt, source=2)
    assert a.size > 0 and R.records_equal(a, b)


@pytest.mark.parametrize("w,h,seed,kept", [(131, 67, 5, 378), (64, 48, 11, 115), (23, 17, 3, 18)])
def test_seeded_scenes_reach_every_branch(w, h, seed, kept):
    s = R.make_scene(w, h, seed)
    d, v = s["depth0"], s["var0"]
    (y0, x0), (y1, x1), (y2, x2), (y3, x3), (y4, x4), (y5, x5) = s["spoilt"]
    assert np.isposinf(d[y0, x0]) and d[y1, x1] == -2 and np.isnan(d[y2, x2]) and d[y3, x3] == F(1e30)
    assert v[y4, x4] == -1 and d[y4, x4] > 0 and np.isnan(v[y5, x5]) and d[y5, x5] > 0
    cl = R.classify(d, v, (0.0125, 2, 0.02, 2))
    ok = cl["ok"]
    with np.errstate(invalid="ignore"):
        classes = dict(depth_inf=np.isposinf(d), depth_neg=d < 0, depth_nan=np.isnan(d), var_neg=(d > 0) & np.isfinite(d) & (v < 0),
                       var_nan=(d > 0) & np.isnan(v))
    for name, m in classes.items():
        assert m.any() and not (m & ok).any(), name
    assert ok[y3, x3]   # 1e30 is a depth like any other
    assert (ok & ~cl["var_pass"]).any() and (ok & ~cl["on_stride"]).any() and (ok & cl["var_pass"] & cl["on_stride"] & ~cl["sup_pass"]).any()
    assert int(cl["kept"].sum()) == kept


def test_every_support_value_and_an_empty_tile_at_131x67():
    s = R.make_scene(131, 67, 5)
    cl = R.classify(s["depth0"], s["var0"], (0, 0, 1.0, 1))
    assert int(cl["kept"].sum()) == 3674
    assert sorted(set(cl["support"][cl["kept"]].tolist())) == list(range(9))
    s = R.make_scene(131, 67, 5, clear_rows=(20, 50))
    k = R.classify(s["depth0"], s["var0"], (0, 0, 1.0, 1))["kept"].reshape(-1)
    assert [int(k[i:i + 2048].sum()) for i in range(0, k.size, 2048)] == [896, 248, 0, 608, 71]


def test_level_intrinsics_are_the_f32_of_the_double_quotient():
    fx = 0.855 * 131
    got = R.level_intrinsics(fx, fx, 65.5, 33.5, 2)
    assert got[0] == F(np.float64(F(fx)) / 4.0) and got[2] == F(65.5 / 4.0) and all(isinstance(g, np.float32) for g in got)
