"""CPU checks of tests/render_depth_reference.py, the numpy restatement of ellc_keyframe_render_depth's rule that the GPU tests hold the
kernels to: a hand-written known answer, scalar against vectorised on the GPU tests' scenes, and an identity transform."""
import numpy as np
import pytest

import render_depth_reference as R

F = np.float32
FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
SHAPES = [(64, 48, 3), (23, 17, 2), (131, 67, 3)]


# 6 columns x 5 rows, fx = fy = 4, cx = cy = 2, filter (0, 0, 1, 1): every ok pixel is kept. All numbers are powers of two: exact.
# Request 0, identity: X = (x - 2) Z / 4, u = (X / Z) 4 + 2 = x: every pixel lands on itself with z' = Z, r = 1, nvar = V.
#   A (1,1) Z 2 V 1/4;  B (2,2) Z 4 V 1/2;  C (3,3) Z 2 V 1/8;  D (4,4) Z 1 V 1/16          (as (x, y))
# Request 1, T = identity with t = (1/2, 0, -1): a pixel with Z = 2 has z' = 1, nid = 1, x' = (x - 2) / 2 + 1/2, u = 4 x' + 2 = 2 x,
# v = 4 (y - 2) / 2 + 2 = 2 y - 2, r = 1 / (1/2) = 2, nvar = 16 V.
#   E (1,2) Z 2 V 1/32  -> target (2,2), z' 1, nvar 1/2: NEARER than B (z' 4) and wins, though its request is the higher one
#   F (2,3) Z 2 V 1/4   -> target (4,4), z' 1, nvar 4: ties with D (z' 1) bit for bit; request 0 wins
#   G (4,2) Z 2         -> target (8,2): outside the image
#   H (0,1) Z 2 V 1e38  -> target (0,0), nvar = 1.6e39 overflows f32: dropped
#   I (5,0) Z 1/2       -> z' = -1/2: behind the camera
# agree_k2 = 1/2: at (2,2) B against E: d = 1/4 - 1 = -3/4, d^2 = 9/16 > (1/2)(1/2 + 1/2): B disagrees -> 1;
# at (4,4) F against D: d = 0 -> 2.
def hand_case():
    d0 = np.zeros((5, 6), F); v0 = np.full((5, 6), -1, F)
    for x, y, Z, V in ((1, 1, 2, 0.25), (2, 2, 4, 0.5), (3, 3, 2, 0.125), (4, 4, 1, 0.0625)):
        d0[y, x] = Z; v0[y, x] = V
    d1 = np.zeros((5, 6), F); v1 = np.full((5, 6), -1, F)
    for x, y, Z, V in ((1, 2, 2, 0.03125), (2, 3, 2, 0.25), (4, 2, 2, 0.125), (0, 1, 2, 1e38), (5, 0, 0.5, 0.125)):
        d1[y, x] = Z; v1[y, x] = V
    img0 = (10 * np.arange(5)[:, None] + np.arange(6)[None, :]).astype(np.uint8)
    img1 = (100 + img0).astype(np.uint8)
    Ts = np.array([IDENTITY, [1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, -1]], F)
    return [(d0, v0, img0), (d1, v1, img1)], (4.0, 4.0, 2.0, 2.0), Ts


def hand_answer():
    depth = np.zeros((5, 6), F); var = np.full((5, 6), -1, F)
    source = np.full((5, 6), -1, np.int32); agree = np.zeros((5, 6), np.int32); inten = np.zeros((5, 6), np.uint8)
    #       x  y  z'   nvar    source            agree intensity
    for x, y, z, nv, src, ag, I in ((1, 1, 2.0, 0.25, 7, 1, 11),
                                    (2, 2, 1.0, 0.5, (1 << 24) | 13, 1, 121),
                                    (3, 3, 2.0, 0.125, 21, 1, 33),
                                    (4, 4, 1.0, 0.0625, 28, 2, 44)):
        depth[y, x] = z; var[y, x] = nv; source[y, x] = src; agree[y, x] = ag; inten[y, x] = I
    return dict(depth=depth, var=var, source=source, agree=agree, intensity=inten, n_valid=4)


@pytest.mark.parametrize("fn", [R.render, R.render_scalar])
def test_hand_written_answer(fn):
    reqs, intr, Ts = hand_case()
    got = fn(reqs, intr, Ts, (0, 0, 1.0, 1), agree_k2=0.5)
    want = hand_answer()
    for name in R.PLANES:
        assert np.array_equal(got[name], want[name]), (name, got[name])
    assert R.planes_equal(got, want)
    if fn is R.render:
        st = got["stats"]
        assert st["behind"] == [0, 1] and st["outside"] == [0, 1] and st["bad_var"] == [0, 1]
        assert st["hits"][2, 2] == 2 and st["hits"][4, 4] == 2 and st["disagree"][2, 2] == 1 and st["disagree"][4, 4] == 0
    # with a generous agree_k2 the loser at (2, 2) agrees as well: 9/16 <= 1 (1/2 + 1/2)
    assert fn(reqs, intr, Ts, (0, 0, 1.0, 1), agree_k2=1.0)["agree"][2, 2] == 2


def scene_requests(w, h, level=0):
    """Scenes 11, 12, 13 of the GPU tests as level-0 requests (the CPU side has no pyramid kernels: level 0 only)."""
    scenes = [R.make_scene(w, h, seed) for seed in (11, 12, 13)]
    m = float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0]))
    reqs = [(s["depth0"], s["var0"], s["kf_image"]) for s in scenes]
    return reqs, R.level_intrinsics(*scenes[0]["intrinsics"], 0), R.scene_transforms(m)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_scalar_equals_vectorised(shape, flt):
    reqs, intr, Ts = scene_requests(*shape[:2])
    a = R.render(reqs, intr, Ts, flt)
    b = R.render_scalar(reqs, intr, Ts, flt)
    assert R.planes_equal(a, b)
    assert a["n_valid"] > 0 and (a["agree"][a["source"] >= 0] >= 1).all() and (a["agree"][a["source"] < 0] == 0).all()


def test_scalar_equals_vectorised_on_five_tiles():
    reqs, intr, Ts = scene_requests(*SHAPES[2][:2])
    assert R.planes_equal(R.render(reqs, intr, Ts, FILTERS[1]), R.render_scalar(reqs, intr, Ts, FILTERS[1]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_scenes_reach_every_case_class(shape):
    reqs, intr, Ts = scene_requests(*shape[:2])
    for flt in FILTERS:
        st = R.render(reqs, intr, Ts, flt)["stats"]
        out = R.render(reqs, intr, Ts, flt)
        assert (st["hits"] >= 2).sum() > 0 and (out["agree"] >= 2).sum() > 0 and (st["disagree"] > 0).sum() > 0
        assert sum(st["behind"]) > 0 and sum(st["outside"]) > 0


def test_identity_puts_every_kept_pixel_on_itself():
    s = R.make_scene(64, 48, 11)
    intr = R.level_intrinsics(*s["intrinsics"], 0)
    for flt in FILTERS:
        out = R.render([(s["depth0"], s["var0"], s["kf_image"])], intr, [IDENTITY], flt)
        kept = R.classify(s["depth0"], s["var0"], flt)["kept"]
        assert kept.sum() > 100 and out["n_valid"] == int(kept.sum())
        assert np.array_equal(out["source"] >= 0, kept)
        ys, xs = np.nonzero(kept)
        assert np.array_equal(out["source"][ys, xs], ys * 64 + xs)
        assert np.array_equal(out["depth"][ys, xs].view(np.uint32), s["depth0"][ys, xs].view(np.uint32))
        assert np.array_equal(out["intensity"][ys, xs], s["kf_image"][ys, xs]) and (out["agree"][ys, xs] == 1).all()
