"""CPU checks of tests/cull_depth_reference.py, the numpy restatement of ellc_keyframe_cull_depth's rule that the GPU tests hold the
kernel to: scalar against vectorised on the GPU tests' scenes, a hand-worked answer on a 4x4 level, the decision's order, the statuses
and vote classes the GPU tests' inputs have to reach, the order of the views, and the recovery of spoilt hypotheses at true
transforms."""
import numpy as np
import pytest

import cull_depth_reference as Q
import refine_depth_reference as R
import sim3_reference as S

F = np.float32
SHAPES = [(64, 48), (23, 17), (131, 67)]
ZERO_SLOT, IMAGE_ONLY_SLOT = 3, 4


def unrelated_world(w, h):
    """The world of tests/test_gpu_sim3.py on the CPU (level 0 only: the CPU side has no pyramid kernels): scenes 11, 12, 13 as slots
    0, 1, 2, an all-zero depth under scene 11's image as slot 3, scene 12's image alone as slot 4; K is slot 0; scene_transforms' three
    transforms and the 3.3-pixel shift."""
    scenes = [S.make_scene(w, h, seed) for seed in (11, 12, 13)]
    m = float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0]))
    intr = S.level_intrinsics(*scenes[0]["intrinsics"], 0)
    shift = np.array([1, 0, 0, 3.3 * m / float(intr[0]), 0, 1, 0, 0, 0, 0, 1, 0], F)
    Ts = np.concatenate([S.scene_transforms(m), shift[None]])
    slots = [(s["depth0"], s["var0"], s["kf_image"]) for s in scenes]
    slots.append((np.zeros((h, w), F), np.full((h, w), -1, F), scenes[0]["kf_image"]))
    slots.append((None, None, scenes[1]["kf_image"]))
    return slots, intr, Ts


def run_unrelated(world, view_list, flt, light, cull=Q.cull, as_kf=True, detail=None, **params):
    slots, intr, Ts = world
    B = len(view_list)
    views = [slots[s] if as_kf else (None, None, slots[s][2]) for s, _ in view_list]
    return cull(slots[0], views, intr, [Ts[t] for _, t in view_list], [light] * B, flt, Q.case_params(B, **params), **({} if detail is None else dict(detail=detail)))


# the view lists of the parity cases: refine_depth_reference.view_list and the two odd slots among the views
ODD_VIEWS = [(1, 1), (IMAGE_ONLY_SLOT, 2), (ZERO_SLOT, 1), (2, 2)]
_cache = {}


def cached(key, make):
    """A vectorised result, computed once and left unchanged."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def shared_case(w, h):
    """The recovery input: K of the shared scene with every seventh hypothesis spoilt, its four views at the true transforms."""
    def make():
        scenes, Ts, _ = R.shared_world(w, h, 5, 11, depth_noise=0.02)
        K = scenes[0]
        depth, spoilt, clean = Q.spoil(K["depth0"], K["var0"])
        intr = Q.level_intrinsics(*K["intrinsics"], 0)
        return (depth, K["var0"], K["kf_image"]), [(s["depth0"], s["var0"], s["kf_image"]) for s in scenes[1:]], intr, Ts, spoilt, clean
    return cached(("shared", w, h), make)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", R.FILTERS, ids=["all", "filtered"])
def test_scalar_equals_vectorised(shape, flt):
    world = cached(("world", shape), lambda: unrelated_world(*shape))
    taking_part = 0
    for vl, light, as_kf, over in ((R.view_list(3), R.LIGHTS[0], True, {}), (R.view_list(3), R.LIGHTS[1], False, {}), (R.view_list(1), R.LIGHTS[1], True, {}),
                                   (ODD_VIEWS, R.LIGHTS[0], True, {}), (R.view_list(3), R.LIGHTS[0], True, dict(photo_k=0.0)),
                                   (R.view_list(6), R.LIGHTS[0], True, Q.OTHER_PARAMS)):
        key = (shape, flt, tuple(vl), light, as_kf, tuple(sorted(over.items())))
        a = cached(key, lambda: run_unrelated(world, vl, flt, light, as_kf=as_kf, **over))
        b = run_unrelated(world, vl, flt, light, cull=Q.cull_scalar, as_kf=as_kf, **over)
        assert Q.results_equal(a, b), key
        assert a["n_kept"] == sum(a[k] for k in Q.STATUS_FIELDS[1:]) and a["n_not_taking_part"] == shape[0] * shape[1] - a["n_kept"]
        Z0, V0 = np.asarray(world[0][0][0], F), np.asarray(world[0][0][1], F)
        culled = (a["status"] >= Q.CULLED_FREE_SPACE) & (a["status"] <= Q.CULLED_PHOTO)
        assert (a["depth"].view(np.uint32) == Z0.view(np.uint32))[~culled].all() and (a["var"].view(np.uint32) == V0.view(np.uint32))[~culled].all()
        assert (a["depth"][culled] == 0).all() and (a["var"][culled] == -1).all()
        v = a["votes"]
        assert int(((v & 255) + ((v >> 8) & 255) + ((v >> 16) & 255)).max()) <= len(vl) and int(a["photo"].max()) <= len(vl)
        assert ((v >> 24) <= a["photo"]).all()
        if not as_kf:
            assert not (v & 0xFFFFFF).any() and a["n_culled_free_space"] == a["n_culled_unsupported"] == 0   # frames vote photometrically only
        if over.get("photo_k") == 0.0:
            assert not a["photo"].any() and not (v >> 24).any() and a["n_culled_photo"] == 0
        taking_part += a["n_kept"]
    assert taking_part > 0


def test_scalar_equals_vectorised_on_the_shared_scene():
    kf, views, intr, Ts, _, _ = shared_case(64, 48)
    a = cached(("shared result", 64, 48), lambda: Q.cull(kf, views, intr, Ts, None, Q.NO_FILTER))
    assert Q.results_equal(a, Q.cull_scalar(kf, views, intr, Ts, None, Q.NO_FILTER)) and a["n_kept"] > 0


# 4 columns x 4 rows, fx = fy = 2, cx = cy = 1, filter (0, 0, 1, 1). K holds ONE hypothesis, pixel (1, 1) with Z0 = 2, V0 = 1/4 and the
# grey value 15. A view at T = [I | (1, 0, 0)] whose image is 10 x. All numbers are small multiples of powers of two: exact in f32.
#   X = Y = 0, P' = (1, 0, 2), nid = 1/2, u = (1 * 1/2) * 2 + 1 = 2, v = 1: target (2, 1); nvar = ((1/2) / (1/2))^4 * 1/4 = 1/4.
#   Photometric: x0 = 2, x0 + 1 = 3 < 4: four taps, ax = ay = 0, Iw = 20, rp = 20 - 15 = 5, sp = 1/4, e = 5/4.
#   Geometric, the view's map at (2, 1) being (Zt, Vt):
#     (2, 1/4):  idt = 1/2, d = 0: AGREE.
#     (1, 0):    idt = 1, d = -1/2, s = 1/4, d d = 1/4 <= 1 * 1/4: AGREE (the bound is reached); agree_k2 = 1/2: 1/4 > 1/8, d < 0: BEHIND.
#     (4, 0):    idt = 1/4, d = 1/4, d d = 1/16 <= 1/4: AGREE; agree_k2 = 1/8: 1/16 > 1/32, d > 0: IN_FRONT.
def hand_case(Zt=None, Vt=None):
    Z0 = np.zeros((4, 4), F); V0 = np.full((4, 4), -1, F)
    Z0[1, 1] = 2; V0[1, 1] = 0.25
    kimg = np.zeros((4, 4), np.uint8); kimg[1, 1] = 15
    vimg = (10 * np.arange(4)[None, :] + np.zeros((4, 1))).astype(np.uint8)
    vd = vv = None
    if Zt is not None:
        vd = np.zeros((4, 4), F); vv = np.full((4, 4), -1, F)
        vd[1, 2] = Zt; vv[1, 2] = Vt
    T = np.array([1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0], F)
    return (Z0, V0, kimg), (vd, vv, vimg), (2.0, 2.0, 1.0, 1.0), T


def one(r):
    return int(r["status"][1, 1]), int(r["votes"][1, 1]), int(r["photo"][1, 1]), float(r["depth"][1, 1]), float(r["var"][1, 1])


@pytest.mark.parametrize("cull", [Q.cull, Q.cull_scalar], ids=["vectorised", "scalar"])
def test_hand_worked_level(cull):
    def run(views, lights=None, **p):
        kf, _, intr, T = hand_case()
        B = len(views)
        return cull(kf, [hand_case(*v)[1] for v in views], intr, [T] * B, lights, Q.NO_FILTER, Q.case_params(B, **p))

    A, FR, BH, BAD = 1, 1 << 8, 1 << 16, 1 << 24
    # one view, photo_k 3 (e = 5/4: good), every count 1
    assert one(run([(2, 0.25)])) == (Q.KEPT, A, 1, 2.0, 0.25)
    assert one(run([(1, 0)])) == (Q.KEPT, A, 1, 2.0, 0.25)                                    # the bound is reached: agrees
    assert one(run([(1, 0)], agree_k2=0.5)) == (Q.CULLED_UNSUPPORTED, BH, 0, 0.0, -1.0)      # BEHIND: no photometric vote, 1 judged, 0 agree
    assert one(run([(4, 0)], agree_k2=0.125)) == (Q.CULLED_FREE_SPACE, FR, 1, 0.0, -1.0)     # IN_FRONT votes photometrically too
    assert one(run([(None, None)])) == (Q.KEPT, 0, 1, 2.0, 0.25)                              # no depth planes: photometric only
    assert one(run([(0, -1)])) == (Q.KEPT, 0, 1, 2.0, 0.25)                                   # no hypothesis at the target: not judged
    assert one(run([(None, None)], photo_k=0.0)) == (Q.UNSEEN, 0, 0, 2.0, 0.25)
    assert one(run([(None, None)], photo_k=1.0)) == (Q.CULLED_PHOTO, BAD, 1, 0.0, -1.0)       # e = 5/4 > 1
    assert one(run([(None, None)], photo_k=1.25)) == (Q.KEPT, 0, 1, 2.0, 0.25)                # e <= photo_k
    assert one(run([(None, None)], photo_k=1.0, lights=[(0.5, 12.5)])) == (Q.KEPT, 0, 1, 2.0, 0.25)   # Ip = 20 = Iw
    assert one(run([(None, None)], photo_k=1.0, sigma_i2=64.0)) == (Q.KEPT, 0, 1, 2.0, 0.25)  # sp = 1/8, e = 5/8
    # the decision's order: f = 1, a = 1 fails the first test (f > a) and min_support = 2 culls it by the second
    r = run([(2, 0.25), (4, 0)], agree_k2=0.125)
    assert one(r) == (Q.KEPT, A | FR, 2, 2.0, 0.25)
    assert one(run([(2, 0.25), (4, 0)], agree_k2=0.125, min_support=2)) == (Q.CULLED_UNSUPPORTED, A | FR, 2, 0.0, -1.0)
    assert one(run([(4, 0), (4, 0)], agree_k2=0.125, min_in_front=2)) == (Q.CULLED_FREE_SPACE, 2 * FR, 2, 0.0, -1.0)
    assert one(run([(4, 0), (None, None)], agree_k2=0.125, min_in_front=2)) == (Q.KEPT, FR, 2, 2.0, 0.25)   # one judged < min_judged 2: not unsupported
    # min_photo and the majority: one bad of two is not more than half
    assert one(run([(None, None)] * 2, photo_k=1.0)) == (Q.CULLED_PHOTO, 2 * BAD, 2, 0.0, -1.0)
    assert one(run([(None, None)] * 2, photo_k=1.0, lights=[(1, 0), (0.5, 12.5)])) == (Q.KEPT, BAD, 2, 2.0, 0.25)
    assert one(run([(None, None)], photo_k=1.0, min_photo=1)) == (Q.CULLED_PHOTO, BAD, 1, 0.0, -1.0)
    r = run([(2, 0.25), (1, 0), (4, 0)], agree_k2=0.125)   # d d = 1/4 > 1/32 behind, 1/16 > 1/32 in front
    assert one(r) == (Q.KEPT, A | FR | BH, 2, 2.0, 0.25)
    assert (r["n_kept"], r["n_retained"], r["sum_agree"], r["sum_in_front"], r["sum_behind"], r["sum_photo"], r["sum_photo_bad"]) == (1, 1, 1, 1, 1, 2, 0)
    assert r["n_not_taking_part"] == 15 and not r["status"].reshape(-1)[[k for k in range(16) if k != 5]].any()


def test_every_status_and_vote_class_occurs():
    """A condition on the inputs of tests/test_gpu_cull_depth.py: over its parity cases at level 0 of 64x48, every status 0..5 occurs,
    every vote class, a pixel with photo > 0 and a BEHIND vote from another view, a view without depth planes that votes, and a pixel
    that fails the first test of the decision with f > 0 but is culled by the second."""
    world = cached(("world", (64, 48)), lambda: unrelated_world(64, 48))
    seen = np.zeros(6, np.int64)
    classes = np.zeros(4, np.int64)
    behind_and_photo = fails_first_culled_by_second = depthless_votes = 0
    for flt in R.FILTERS:
        for vl, over in ((R.view_list(1), {}), (R.view_list(3), {}), (R.view_list(64), {}), (ODD_VIEWS, {}), (R.view_list(3), dict(photo_k=0.0)),
                         (R.view_list(6), Q.OTHER_PARAMS)):
            detail = []
            r = run_unrelated(world, vl, flt, R.LIGHTS[0], detail=detail, **over)
            seen += np.bincount(r["status"].reshape(-1), minlength=6)
            for (s, _), d in zip(vl, detail):
                classes += np.bincount(d["cls"], minlength=4)
                if s == IMAGE_ONLY_SLOT:
                    assert not d["cls"].any()
                    depthless_votes += int(d["photo"].sum())
            v = r["votes"]
            a, f, h = v & 255, (v >> 8) & 255, (v >> 16) & 255
            behind_and_photo += int(((h > 0) & (r["photo"] > 0)).sum())
            fails_first_culled_by_second += int(((f > 0) & (r["status"] == Q.CULLED_UNSUPPORTED)).sum())
    print("status counts", seen.tolist(), "vote classes (none, agree, in front, behind)", classes.tolist(), "behind and photo", behind_and_photo,
          "f > 0 and unsupported", fails_first_culled_by_second, "votes of the view without depth", depthless_votes)
    assert (seen > 0).all() and (classes > 0).all(), (seen.tolist(), classes.tolist())
    assert behind_and_photo > 0 and fails_first_culled_by_second > 0 and depthless_votes > 0


@pytest.mark.parametrize("shape", [(64, 48), (23, 17)], ids=lambda s: "%dx%d" % s)
def test_permuting_the_views_changes_no_byte(shape):
    world = cached(("world", shape), lambda: unrelated_world(*shape))
    vl = R.view_list(6)[:4] + ODD_VIEWS[1:3]
    a = run_unrelated(world, vl, R.FILTERS[0], R.LIGHTS[0])
    rng = np.random.default_rng(5)
    for _ in range(3):
        perm = [vl[k] for k in rng.permutation(len(vl))]
        assert Q.results_equal(a, run_unrelated(world, perm, R.FILTERS[0], R.LIGHTS[0]))
    assert Q.results_equal(a, run_unrelated(world, vl[::-1], R.FILTERS[0], R.LIGHTS[0])) and a["n_kept"] > 0


@pytest.mark.parametrize("shape", [(64, 48), (131, 67)], ids=lambda s: "%dx%d" % s)
def test_recovery_of_spoilt_hypotheses(shape):
    """refine_depth_reference.shared_world(w, h, 5, 11, depth_noise=0.02): every seventh OK pixel of K in raster order has its inverse
    depth multiplied by 0.5 and 1.6 alternately; K against its four views at the true transforms, default parameters, the no-op filter.
    At least 75 % of the spoilt hypotheses are culled and at most 1 % of the others. Measured with this f32 reference: 131 of 139
    spoilt (94.2 %) and 0 of 831 others at 64x48, 393 of 454 (86.6 %) and 0 of 2724 at 131x67."""
    w, h = shape
    kf, views, intr, Ts, spoilt, clean = shared_case(w, h)
    res = cached(("shared result", w, h), lambda: Q.cull(kf, views, intr, Ts, None, Q.NO_FILTER))
    n_spoilt, culled_spoilt, n_clean, culled_clean = Q.recovery_figures(res, spoilt, clean)
    print("%dx%d: spoilt %d, culled %d (%.1f %%); others %d, culled %d (%.2f %%); free space %d, unsupported %d, photo %d, unseen %d" % (
        w, h, n_spoilt, culled_spoilt, 100.0 * culled_spoilt / n_spoilt, n_clean, culled_clean, 100.0 * culled_clean / n_clean,
        res["n_culled_free_space"], res["n_culled_unsupported"], res["n_culled_photo"], res["n_unseen"]))
    assert res["n_kept"] == n_spoilt + n_clean
    assert culled_spoilt >= 0.75 * n_spoilt, (culled_spoilt, n_spoilt)
    assert culled_clean <= 0.01 * n_clean, (culled_clean, n_clean)
