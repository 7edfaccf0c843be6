"""CPU checks of tests/depth_consistency_reference.py, the numpy restatement of ellc_keyframe_depth_consistency's rule that the GPU tests
hold the kernels to: a hand-written known answer, scalar against vectorised on the GPU tests' scenes, and the identity pair."""
import numpy as np
import pytest

import depth_consistency_reference as D

F = np.float32
FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
PAIRS = [(0, 0, 0), (0, 1, 1), (1, 0, 1), (2, 0, 2), (1, 1, 1)]   # (source, destination, transform) of the GPU tests' batch


# 6 columns x 5 rows, fx = fy = 1, cx = cy = 0, filter (0, 0, 1, 1): every ok pixel is kept. All numbers are powers of two: exact.
# T = identity with t = (0, 0, -1): a source pixel (x, y) with Z = 2 has X = 2 x, Y = 2 y, z' = 1, nid = 1, u = 2 x, v = 2 y,
# r = 1 / (1/2) = 2, nvar = 16 V. agree_k2 = 1/2. Source image 10 y + x, destination image 100 + 2 (10 y + x).
#   A (0,0) Z 2 V 1/16 -> (0,0), nvar 1; there Zt 1 Vt 1: d = 0, s = 2: AGREES; w 1/2, q 0, ss 1/2, st 1/2;        |dI| = |0 - 100|
#   B (1,0) Z 2 V 1/16 -> (2,0), nvar 1; there Zt 4 Vt 0: idt 1/4, d 3/4, d^2 9/16 > (1/2) 1: IN FRONT; w 1, q 9/16, ss 1, st 1/4;  |1 - 104|
#   C (2,0) Z 2 V 1/16 -> (4,0), nvar 1; there Zt 1/4 Vt 1: idt 4, d -3, d^2 9 > (1/2) 2: BEHIND; w 1/2, q 9/2, ss 1/2, st 2;       |2 - 108|
#   D (0,1) Z 2        -> (0,2): nothing there (Zt 0): in view, NO OVERLAP
#   E (3,0) Z 2        -> (6,0): OUTSIDE the image
#   F (1,1) Z 1/2      -> z' = -1/2: BEHIND THE CAMERA
#   G (1,2) Z 2 V 0    -> (2,4), nvar 0; there Zt 1 Vt 0: d = 0, s = 0: agrees (0 <= 0), UNWEIGHTED;                 |21 - 184|
#   (5,4) Z 2 V -1: not a hypothesis, not kept
def hand_case():
    sd = np.zeros((5, 6), F); sv = np.full((5, 6), -1, F)
    for x, y, Z, V in ((0, 0, 2, 0.0625), (1, 0, 2, 0.0625), (2, 0, 2, 0.0625), (0, 1, 2, 0.0625), (3, 0, 2, 0.0625), (1, 1, 0.5, 0.0625),
                       (1, 2, 2, 0.0), (5, 4, 2, -1.0)):
        sd[y, x] = Z; sv[y, x] = V
    dd = np.zeros((5, 6), F); dv = np.full((5, 6), -1, F)
    for x, y, Z, V in ((0, 0, 1, 1), (2, 0, 4, 0), (4, 0, 0.25, 1), (2, 4, 1, 0)):
        dd[y, x] = Z; dv[y, x] = V
    simg = (10 * np.arange(5)[:, None] + np.arange(6)[None, :]).astype(np.uint8)
    dimg = (100 + 2 * simg).astype(np.uint8)
    return (sd, sv, simg), (dd, dv, dimg), (1.0, 1.0, 0.0, 0.0), np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -1], F)


HAND = dict(n_kept=7, n_in_view=5, n_overlap=4, n_agree=2, n_in_front=1, n_behind=1, n_weighted=3,
            sum_abs_di=100 + 103 + 106 + 163, sum_di2=100 * 100 + 103 * 103 + 106 * 106 + 163 * 163,
            sum_chi2=0.0 + 0.5625 + 4.5, sum_w_ss=0.5 + 1.0 + 0.5, sum_w_st=0.5 + 0.25 + 2.0)


@pytest.mark.parametrize("fn", [D.consistency, D.consistency_scalar])
def test_hand_written_answer(fn):
    src, dst, intr, T = hand_case()
    got = fn(src, dst, intr, T, (0, 0, 1.0, 1), agree_k2=0.5)
    for k in D.INT_FIELDS + D.SUM_FIELDS:
        assert got[k] == HAND[k], (k, got[k], HAND[k])
    assert got["n_overlap"] == got["n_agree"] + got["n_in_front"] + got["n_behind"]
    if fn is D.consistency:
        assert (got["behind_camera"], got["outside"], got["bad_var"], got["no_overlap"]) == (1, 1, 0, 1)
    # with a generous agree_k2 the pixel in front agrees as well (9/16 <= 1), the one behind still does not (9 > 2)
    wide = fn(src, dst, intr, T, (0, 0, 1.0, 1), agree_k2=1.0)
    assert (wide["n_agree"], wide["n_in_front"], wide["n_behind"]) == (3, 0, 1) and wide["sum_chi2"] == HAND["sum_chi2"]


def scene_planes(w, h):
    """Scenes 11, 12, 13 of the GPU tests as level-0 planes (the CPU side has no pyramid kernels: level 0 only)."""
    scenes = [D.make_scene(w, h, seed) for seed in (11, 12, 13)]
    m = float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0]))
    return [(s["depth0"], s["var0"], s["kf_image"]) for s in scenes], D.level_intrinsics(*scenes[0]["intrinsics"], 0), D.scene_transforms(m)


@pytest.mark.parametrize("shape", [(64, 48), (23, 17)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_scalar_equals_vectorised(shape, flt):
    planes, intr, Ts = scene_planes(*shape)
    kept = 0
    for s, d, t in PAIRS:
        a = D.consistency(planes[s], planes[d], intr, Ts[t], flt)
        b = D.consistency_scalar(planes[s], planes[d], intr, Ts[t], flt)
        assert D.fields_equal(a, b), (s, d, t, a, b)
        assert a["n_overlap"] == a["n_agree"] + a["n_in_front"] + a["n_behind"] and a["n_weighted"] <= a["n_overlap"] <= a["n_in_view"] <= a["n_kept"]
        assert a["n_kept"] == a["n_in_view"] + a["behind_camera"] + a["outside"] + a["bad_var"]
        kept += a["n_kept"]
    assert kept > 0


@pytest.mark.parametrize("shape", [(64, 48), (131, 67)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_scenes_reach_every_case_class(shape, flt):
    planes, intr, Ts = scene_planes(*shape)
    recs = [D.consistency(planes[s], planes[d], intr, Ts[t], flt) for s, d, t in PAIRS]
    for k in ("n_agree", "n_in_front", "n_behind", "no_overlap", "outside", "behind_camera"):
        assert sum(r[k] for r in recs) > 0, k


def test_the_unfiltered_64x48_batch_counts():
    planes, intr, Ts = scene_planes(64, 48)
    recs = [D.consistency(planes[s], planes[d], intr, Ts[t], FILTERS[0]) for s, d, t in PAIRS]
    assert [(r["n_agree"], r["n_in_front"], r["n_behind"]) for r in recs] == [(1098, 0, 0), (288, 7, 458), (600, 32, 145), (0, 0, 0), (1221, 1, 120)]
    assert recs[3]["behind_camera"] == 927 and recs[3]["outside"] == 318 and recs[3]["n_overlap"] == 0


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_identity_pair(flt):
    s = D.make_scene(64, 48, 11)
    p = (s["depth0"], s["var0"], s["kf_image"])
    r = D.consistency(p, p, D.level_intrinsics(*s["intrinsics"], 0), IDENTITY, flt)
    assert r["n_kept"] > 100 and r["n_kept"] == r["n_in_view"] == r["n_overlap"] == r["n_agree"]
    assert r["sum_chi2"] == 0 and r["sum_abs_di"] == 0 and r["sum_w_st"] == r["sum_w_ss"] > 0
    assert r["n_kept"] == int(D.classify(s["depth0"], s["var0"], flt)["kept"].sum())
