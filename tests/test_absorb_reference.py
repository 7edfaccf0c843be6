"""CPU checks of tests/absorb_reference.py, the numpy restatement of ellc_depth_absorb_keyframes' rule that the GPU tests hold the
kernels to: a hand-written known answer, scalar against sorted-array form on the GPU tests' scenes, the case classes those scenes reach,
and what the fold does to the map's error."""
import numpy as np
import pytest

import absorb_reference as A
from egomotion_with_local_loop_closures_amd import synth

F = np.float32
FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
SHAPES = [(64, 48), (23, 17), (131, 67)]


# 12 columns x 10 rows, fx = fy = 4, cx = cy = 2, filter (0, 0, 1, 1): every ok pixel is kept; agree_k2 = 1/2, src_validity 20. All four
# requests have the identity: a pixel (x, y) with Z = 2 lands on itself with u = x, v = y exactly, nid = 1/2, r = 1, nvar = V. The
# interior is 3 <= x <= 8, 3 <= y <= 6. K's image is 10 y + x, its maxAbsGradient 10 except where stated; the sources' images are K's except
# where stated, so the residual is 0 (up to an ulp of u where Z is not 2). Per target, as (x, y):
#   (3,3)  not valid; request 0: Z 2 V 1/4                                           -> CREATED: id 1/2, var 1/4, val 20
#   (4,3)  valid, id 1/2, var 0.3, val 7; request 1: Z 2.5 V 0.1, request 2: Z 2.25 V 0.2, request 3: Z 3 V 0.7 - all agree
#          ((1/2 - 1/3)^2 = 1/36 <= (1/2)(0.7 + var)) and are MERGED in that order, rounded at every step (bit patterns below): val 67;
#          with max_fold 2 only requests 1 and 2: val 47, truncated
#   (5,3)  valid, id 1/2, var 1/64, val 3, blacklisted -1; request 0: Z 4 V 1/64: d = -1/4, d^2 = 1/16 > (1/2)(1/32), behind
#                                                                                    -> OCCLUDED, every byte kept
#   (6,3)  valid, id 1/4, var 1/64, val 3, blacklisted -3; request 0: Z 2 V 1/64: d = +1/4, in front -> REPLACED: id 1/2, var 1/64, val 20;
#          request 1: Z 2 V 1/64: d = 0, s = 1/32, w = 1/2 -> MERGED into the replacement: id 1/2, var 1 / (64 + 64), val 40
#   (7,3)  valid, id 1/2, var 0, val 5; request 0: Z 2 V 0: agrees (0 <= 0), s = 0         -> SKIPPED, every byte kept
#   (2,4) (9,4) (4,2) (4,7)  request 0: Z 2 V 1/4: u = 2, u = 9 > 12 - 3.1, v = 2, v = 7 > 10 - 3.1: in view, outside each of the four bounds
#   (3,5)  request 0: Z 2 V 1/4, its grey value is K's + 50: r^2 = 2500 > 1600 + (0.25 * 10) * 10     -> dropped by the gate (created without it)
#   (4,5)  request 0: Z 2 V 1/4, K's maxAbsGradient is 4 < 5 there                            -> dropped by the gate (created without it)
#   (5,5)  request 0: Z 2 V 1/4, K's maxAbsGradient is exactly 5 there                        -> passes; CREATED
#   (8,6)  valid, id 0.7, var 0.02, val 9, blacklisted -2, smoothed 0.71 / 0.021; nobody lands here -> every byte kept
P3_ALL, P3_TWO = (0x3ED8B9E2, 0x3D4F447A), (0x3EDC50AE, 0x3D5F6B0F)   # (4,3): id and var after three merges / after the first two


def bits(*patterns):
    return tuple(np.array([b], np.uint32).view(F)[0] for b in patterns)


def hand_case():
    d = [np.zeros((10, 12), F) for _ in range(4)]
    v = [np.full((10, 12), -1, F) for _ in range(4)]
    for b, x, y, Z, V in ((0, 3, 3, 2, 0.25),
                          (1, 4, 3, 2.5, 0.1), (2, 4, 3, 2.25, 0.2), (3, 4, 3, 3, 0.7),
                          (0, 5, 3, 4, 1 / 64),
                          (0, 6, 3, 2, 1 / 64), (1, 6, 3, 2, 1 / 64),
                          (0, 7, 3, 2, 0),
                          (0, 2, 4, 2, 0.25), (0, 9, 4, 2, 0.25), (0, 4, 2, 2, 0.25), (0, 4, 7, 2, 0.25),
                          (0, 3, 5, 2, 0.25), (0, 4, 5, 2, 0.25), (0, 5, 5, 2, 0.25)):
        d[b][y, x] = Z; v[b][y, x] = V
    k_img = (10 * np.arange(10)[:, None] + np.arange(12)[None, :]).astype(np.uint8)
    img0 = k_img.copy(); img0[5, 3] += 50
    k_mg = np.full((10, 12), 10, F); k_mg[5, 4] = 4; k_mg[5, 5] = 5
    state = dict(invDepth=np.zeros((10, 12), F), invDepthSmoothed=np.zeros((10, 12), F), variance=np.zeros((10, 12), F),
                 varianceSmoothed=np.zeros((10, 12), F), validity=np.zeros((10, 12), np.int32), blacklisted=np.zeros((10, 12), np.int32),
                 valid=np.zeros((10, 12), np.uint8))
    for x, y, i, var, val, bl, si, sv in ((4, 3, 0.5, 0.3, 7, 0, 0.5, 0.3), (5, 3, 0.5, 1 / 64, 3, -1, 0.51, 0.016), (6, 3, 0.25, 1 / 64, 3, -3, 0.26, 0.017),
                                          (7, 3, 0.5, 0, 5, 0, 0.52, 0.001), (8, 6, 0.7, 0.02, 9, -2, 0.71, 0.021)):
        state["invDepth"][y, x] = i; state["variance"][y, x] = var; state["validity"][y, x] = val; state["blacklisted"][y, x] = bl
        state["invDepthSmoothed"][y, x] = si; state["varianceSmoothed"][y, x] = sv; state["valid"][y, x] = 1
    state["blacklisted"][1, 1] = -2   # a blacklisted pixel without a hypothesis, far from everything
    return list(zip(d, v, [img0, k_img, k_img, k_img])), (4.0, 4.0, 2.0, 2.0), np.array([IDENTITY] * 4, F), k_img, k_mg, state


def hand_answer(max_fold, photo_gate):
    _, _, _, _, _, st = hand_case()
    p3 = bits(*(P3_ALL if max_fold >= 3 else P3_TWO))
    #     x  y  invDepth  variance      validity
    new = [(3, 3, F(0.5), F(0.25), 20), (4, 3, p3[0], p3[1], 67 if max_fold >= 3 else 47), (6, 3, F(0.5), F(1 / 128), 40), (5, 5, F(0.5), F(0.25), 20)]
    if not photo_gate:
        new += [(3, 5, F(0.5), F(0.25), 20), (4, 5, F(0.5), F(0.25), 20)]
    for x, y, i, var, val in new:
        st["invDepth"][y, x] = i; st["variance"][y, x] = var; st["validity"][y, x] = val
        st["valid"][y, x] = 1; st["blacklisted"][y, x] = 0; st["invDepthSmoothed"][y, x] = -1; st["varianceSmoothed"][y, x] = -1
    g = 0 if photo_gate else 2
    three = max_fold >= 3
    st["stats"] = dict(n_kept=15, n_in_view=15, n_interior=11, n_candidates=9 + g, n_visited=(9 if three else 8) + g, n_created=2 + g,
                       n_merged=4 if three else 3, n_replaced=1, n_occluded=1, n_skipped=1, targets_hit=6 + g, targets_touched=4 + g,
                       targets_truncated=0 if three else 1, n_valid_before=5, n_valid_after=7 + g, reserved=0)
    return st


@pytest.mark.parametrize("fn", [A.absorb, A.absorb_scalar])
@pytest.mark.parametrize("max_fold", [64, 2])
@pytest.mark.parametrize("photo_gate", [1, 0])
def test_hand_written_answer(fn, max_fold, photo_gate):
    reqs, intr, Ts, k_img, k_mg, state = hand_case()
    got = fn(reqs, intr, Ts, (0, 0, 1.0, 1), k_img, k_mg, state, agree_k2=0.5, max_fold=max_fold, photo_gate=photo_gate, src_validity=20)
    want = hand_answer(max_fold, photo_gate)
    for name in A.PLANES:
        assert np.array_equal(got[name], want[name]), (name, got[name])
    assert A.states_equal(got, want) and got["stats"] == want["stats"], (got["stats"], want["stats"])
    # the pixel nobody hits, the occluded and the skipped target keep every byte, smoothed values and blacklist marks included
    for x, y in ((8, 6), (5, 3), (7, 3), (1, 1)):
        for name in A.PLANES:
            assert got[name][y, x].tobytes() == state[name][y, x].tobytes(), (name, x, y)
    assert got["blacklisted"][6, 8] == -2 and got["invDepthSmoothed"][6, 8] == F(0.71) and got["blacklisted"][3, 5] == -1
    # the input was not written to
    fresh = hand_case()[5]
    assert A.states_equal(state, fresh)


def test_the_order_shows_in_the_last_bits():
    """A condition of the hand case: merging (4,3)'s candidates in another order gives other bits, so the fixed order is under test. In
    exact arithmetic the information-weighted mean of 1/2, 2/5, 4/9, 1/3 under the variances 0.3, 0.1, 0.2, 0.7 is 8.36508 / 19.76190 =
    0.423293 with variance 0.0506024; of the first three 0.430303 with 0.0545455."""
    cand = {1: (F(2.5), F(0.1)), 2: (F(2.25), F(0.2)), 3: (F(3), F(0.7))}

    def fold(order):
        i_t, v_t = F(0.5), F(0.3)
        for b in order:
            Z, nvar = cand[b]
            nid = F(F(1) / Z)
            s = F(v_t + nvar)
            w = F(nvar / s)
            i_t = F(F(w * i_t) + F(F(F(1) - w) * nid))
            v_t = F(F(1) / F(F(F(1) / v_t) + F(F(1) / nvar)))
        return int(np.asarray(i_t, F).view(np.uint32)), int(np.asarray(v_t, F).view(np.uint32))

    assert fold((1, 2, 3)) == P3_ALL and fold((1, 2)) == P3_TWO
    want = bits(*P3_ALL)
    assert abs(float(want[0]) - 8.3650793651 / 19.7619047619) < 1e-6 and abs(float(want[1]) - 1 / 19.7619047619) < 1e-8
    others = [fold(o) for o in ((3, 2, 1), (2, 1, 3), (1, 3, 2), (3, 1, 2), (2, 3, 1))]
    assert any(o != P3_ALL for o in others)
    assert all(abs(float(bits(o[0])[0]) - float(want[0])) < 1e-6 for o in others)   # ... the last bits only


def scene_inputs(w, h, halve=True):
    sc = A.make_scene(w, h, halve=halve)
    v = sc["views"]
    reqs = [(v[b]["depth0"], v[b]["var0"], v[b]["kf_image"]) for b in range(1, 5)]
    return sc, reqs, v[0]["kf_image"], synth.max_abs_gradient(v[0]["kf_image"]).astype(F)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s)
def scene(request):
    return (request.param,) + scene_inputs(*request.param)


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
@pytest.mark.parametrize("photo_gate", [1, 0])
def test_scalar_equals_sorted_arrays(scene, flt, photo_gate):
    shape, sc, reqs, k_img, k_mg = scene
    for max_fold in (64, 2, 1):
        a = A.absorb(reqs, sc["intr"], sc["Ts"], flt, k_img, k_mg, sc["state"], max_fold=max_fold, photo_gate=photo_gate)
        b = A.absorb_scalar(reqs, sc["intr"], sc["Ts"], flt, k_img, k_mg, sc["state"], max_fold=max_fold, photo_gate=photo_gate)
        assert A.states_equal(a, b), A.differing(a, b)
        assert a["stats"] == b["stats"] and np.array_equal(a["touched"], b["touched"])
        s = a["stats"]
        assert s["n_visited"] == s["n_created"] + s["n_merged"] + s["n_replaced"] + s["n_occluded"] + s["n_skipped"]
        assert s["n_valid_after"] == s["n_valid_before"] + s["n_created"] == int((a["valid"] != 0).sum())
        assert s["targets_touched"] == int(a["touched"].sum()) <= s["targets_hit"] and s["n_visited"] <= s["n_candidates"]
        assert (s["n_visited"] == s["n_candidates"]) == (s["targets_truncated"] == 0)
        keep = ~a["touched"]
        for name in A.PLANES:
            assert a[name][keep].tobytes() == sc["state"][name][keep].tobytes(), name


# the counts of the scene (filter (0, 0, 1, 1), agree_k2 1, gate on, src_validity 20): candidates, created, merged, replaced, occluded at
# max_fold 64, and the targets truncated at max_fold 2
TABLE = {(64, 48): (3650, 337, 3151, 98, 64, 905), (23, 17): (329, 50, 271, 8, 0, 70), (131, 67): (10078, 910, 8712, 276, 180, 2283)}


def test_scenes_reach_every_case_class(scene):
    shape, sc, reqs, k_img, k_mg = scene
    a = A.absorb(reqs, sc["intr"], sc["Ts"], FILTERS[0], k_img, k_mg, sc["state"])
    two = A.absorb(reqs, sc["intr"], sc["Ts"], FILTERS[0], k_img, k_mg, sc["state"], max_fold=2)
    s = a["stats"]
    got = (s["n_candidates"], s["n_created"], s["n_merged"], s["n_replaced"], s["n_occluded"], two["stats"]["targets_truncated"])
    print(shape, got, s)
    assert got == TABLE[shape]
    assert s["n_visited"] == s["n_created"] + s["n_merged"] + s["n_replaced"] + s["n_occluded"] + s["n_skipped"] and s["targets_truncated"] == 0
    if shape != (23, 17):
        gate_dropped, bound_dropped = s["n_interior"] - s["n_candidates"], s["n_in_view"] - s["n_interior"]
        for k in ("n_created", "n_merged", "n_replaced", "n_occluded"):
            assert s[k] > 0, k
        assert two["stats"]["targets_truncated"] > 0 and gate_dropped > 0 and bound_dropped > 0
        if shape == (64, 48):
            assert (gate_dropped, s["n_interior"], bound_dropped, s["n_in_view"]) == (396, 4046, 196, 4242)


def test_the_fold_brings_the_map_closer_to_the_truth():
    """On the unhalved scene with the default parameters: the mean |invDepth - truth| over the pixels valid before and after is smaller
    after than before, and smaller still over the created ones."""
    sc, reqs, k_img, k_mg = scene_inputs(64, 48, halve=False)
    a = A.absorb(reqs, sc["intr"], sc["Ts"], FILTERS[0], k_img, k_mg, sc["state"], **A.DEFAULTS)
    was = sc["state"]["valid"] != 0
    both = was & (a["valid"] != 0)
    created = ~was & (a["valid"] != 0)
    assert both.sum() == was.sum() > 0 and created.sum() == a["stats"]["n_created"] > 0
    before = float(np.abs(sc["state"]["invDepth"][both].astype(np.float64) - sc["truth"][both]).mean())
    after = float(np.abs(a["invDepth"][both].astype(np.float64) - sc["truth"][both]).mean())
    fresh = float(np.abs(a["invDepth"][created].astype(np.float64) - sc["truth"][created]).mean())
    print("mean |invDepth - truth|: before %.4f after %.4f created %.4f" % (before, after, fresh))
    assert after < before and fresh < after
