"""CPU checks of tests/absorb_lit_reference.py and tests/trial_lit_reference.py, the numpy restatements of the v24 rule (the photometric
gate against Ip = gain * Is + offset) that the GPU tests hold the kernels to: a hand-worked answer, the scalar against the vectorised
form on the GPU tests' scenes with mixed lights, and light (1, 0) against the existing references on every field."""
import numpy as np
import pytest

import absorb_lit_reference as AL
import absorb_reference as A
import trial_lit_reference as TL
import trial_propagation_reference as T
from egomotion_with_local_loop_closures_amd import synth

F = np.float32
FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]   # test_gpu_trial_propagate.FILTERS
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
SHAPES = [(64, 48), (23, 17), (131, 67)]
MIXED = np.array([[1.6, -20.0], [1.0, 0.0], [0.7, 15.0], [1.25, -7.5]], F)


# 12 columns x 10 rows, fx = fy = 4, cx = cy = 2, identity, Z = 2, V = 1/4, empty state: a pixel lands on itself with u = x, v = y, so
# Iw is K's grey value 10 y + x there. K's maxAbsGradient is 10: a candidate passes iff r * r <= 1600 + (0.25 * 10) * 10 = 1625, |r| <= 40.
#   (3,4)  Iw 43, Is  0: (1, 0): r = 43, 1849 > 1625 DROPPED;      (1.5, 10): Ip = 10, r = 33, 1089 passes      -> created at the light only
#   (5,4)  Iw 45, Is 80: (1, 0): r = -35, 1225 passes;             (1.5, 10): Ip = 130, r = -85, 7225 DROPPED   -> created at (1, 0) only
#   (7,4)  Iw 47, Is 47: (1, 0): r = 0;                            (1.5, 10): Ip = 80.5, r = -33.5, 1122.25     -> created at both
def hand_case():
    d = np.zeros((10, 12), F); v = np.full((10, 12), -1, F)
    k_img = (10 * np.arange(10)[:, None] + np.arange(12)[None, :]).astype(np.uint8)
    img = k_img.copy()
    for x, Is in ((3, 0), (5, 80), (7, 47)):
        d[4, x] = 2; v[4, x] = 0.25; img[4, x] = Is
    return (d, v, img), (4.0, 4.0, 2.0, 2.0), k_img, np.full((10, 12), 10, F)


@pytest.mark.parametrize("fn", [AL.absorb_lit, AL.absorb_lit_scalar])
def test_hand_worked_answer(fn):
    req, intr, k_img, k_mg = hand_case()
    wiped = T.wiped_state(10, 12)
    for light, created in (((1.0, 0.0), (5, 7)), (None, (5, 7)), ((1.5, 10.0), (3, 7))):
        got = fn([req], intr, [IDENTITY], None if light is None else [light], FILTERS[0], k_img, k_mg, wiped, src_validity=20)
        valid = np.zeros((10, 12), np.uint8)
        valid[4, list(created)] = 1
        assert np.array_equal(got["valid"], valid), (light, got["valid"])
        assert (got["invDepth"][valid != 0] == F(0.5)).all() and (got["variance"][valid != 0] == F(0.25)).all() and (got["validity"][valid != 0] == 20).all()
        s = got["stats"]
        assert (s["n_kept"], s["n_in_view"], s["n_interior"], s["n_candidates"], s["n_created"], s["n_valid_after"]) == (3, 3, 3, 2, 2, 2), s
    # the gate off: the light does not enter
    got = fn([req], intr, [IDENTITY], [(1.5, 10.0)], FILTERS[0], k_img, k_mg, wiped, photo_gate=0)
    assert got["stats"]["n_candidates"] == 3 and int(got["valid"].sum()) == 3
    # the trial records of the same pixels: residuals 43, -35, 0 at (1, 0) and 33, -85, -33.5 at the light; the fit's sums at both
    for tf in (TL.trial_lit, TL.trial_lit_scalar):
        for light, r in ((None, (43.0, -35.0, 0.0)), ((1.5, 10.0), (33.0, -85.0, -33.5))):
            rec = tf(req, intr, IDENTITY, light, FILTERS[0], k_img, k_mg)
            assert rec["sum_r2"] == sum(x * x for x in r) and rec["sum_abs_r"] == sum(abs(x) for x in r)
            assert (rec["n_interior"], rec["n_fit"], rec["n_candidates"], rec["n_targets"], rec["n_low_grad"]) == (3, 3, 2, 2, 0)
            assert (rec["sum_s"], rec["sum_t"], rec["sum_ss"], rec["sum_st"], rec["sum_tt"]) == (127.0, 135.0, 80.0 ** 2 + 47.0 ** 2, 80.0 * 45 + 47.0 * 47,
                                                                                              43.0 ** 2 + 45.0 ** 2 + 47.0 ** 2)


def scene_inputs(w, h):
    sc = A.make_scene(w, h)
    v = sc["views"]
    reqs = [(v[b]["depth0"], v[b]["var0"], v[b]["kf_image"]) for b in range(1, 5)]
    return sc, reqs, v[0]["kf_image"], synth.max_abs_gradient(v[0]["kf_image"]).astype(F)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s)
def scene(request):
    return (request.param,) + scene_inputs(*request.param)


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
@pytest.mark.parametrize("photo_gate", [1, 0])
def test_scalar_equals_vectorised_with_mixed_lights(scene, flt, photo_gate):
    shape, sc, reqs, k_img, k_mg = scene
    a = AL.absorb_lit(reqs, sc["intr"], sc["Ts"], MIXED, flt, k_img, k_mg, sc["state"], photo_gate=photo_gate)
    b = AL.absorb_lit_scalar(reqs, sc["intr"], sc["Ts"], MIXED, flt, k_img, k_mg, sc["state"], photo_gate=photo_gate)
    assert A.states_equal(a, b), A.differing(a, b)
    assert a["stats"] == b["stats"] and np.array_equal(a["touched"], b["touched"])
    plain = A.absorb(reqs, sc["intr"], sc["Ts"], flt, k_img, k_mg, sc["state"], photo_gate=photo_gate)
    if photo_gate and flt == FILTERS[0] and shape != (23, 17):
        assert a["stats"]["n_candidates"] != plain["stats"]["n_candidates"]   # a condition of the test: the lights enter
    if not photo_gate:
        assert A.states_equal(a, plain) and a["stats"] == plain["stats"]
    for b_, light in enumerate(MIXED):
        x = TL.trial_lit(reqs[b_], sc["intr"], sc["Ts"][b_], light, flt, k_img, k_mg, photo_gate=photo_gate)
        y = TL.trial_lit_scalar(reqs[b_], sc["intr"], sc["Ts"][b_], light, flt, k_img, k_mg, photo_gate=photo_gate)
        assert x == y, (b_, x, y)
        assert x["n_fit"] == x["n_interior"]


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
@pytest.mark.parametrize("photo_gate", [1, 0])
def test_light_one_zero_is_the_existing_references(scene, flt, photo_gate):
    shape, sc, reqs, k_img, k_mg = scene
    plain = A.absorb(reqs, sc["intr"], sc["Ts"], flt, k_img, k_mg, sc["state"], photo_gate=photo_gate)
    for lights in (None, np.tile(np.array([1, 0], F), (4, 1))):
        a = AL.absorb_lit(reqs, sc["intr"], sc["Ts"], lights, flt, k_img, k_mg, sc["state"], photo_gate=photo_gate)
        assert A.states_equal(a, plain) and a["stats"] == plain["stats"] and np.array_equal(a["touched"], plain["touched"])
    assert A._candidates is AL._plain_candidates   # absorb_lit leaves absorb_reference as it found it
    for b in range(4):
        want = T.trial(reqs[b], sc["intr"], sc["Ts"][b], flt, k_img, k_mg, photo_gate=photo_gate)
        for light in (None, (1.0, 0.0)):
            got = TL.trial_lit(reqs[b], sc["intr"], sc["Ts"][b], light, flt, k_img, k_mg, photo_gate=photo_gate)
            for k in T.FIELDS:
                assert got[k] == want[k], (k, got[k], want[k])
            assert got["sum_abs_terms"][:2] == want["sum_abs_terms"]
    r = AL.restart_lit(reqs, sc["intr"], sc["Ts"], None, flt, k_img, k_mg, photo_gate=photo_gate)
    assert A.states_equal(r, T.restart(reqs, sc["intr"], sc["Ts"], flt, k_img, k_mg, photo_gate=photo_gate))


def test_the_sums_do_not_depend_on_the_light_or_the_gate(scene):
    shape, sc, reqs, k_img, k_mg = scene
    base = TL.trial_lit(reqs[0], sc["intr"], sc["Ts"][0], None, FILTERS[0], k_img, k_mg)
    for light, gate in (((1.6, -20.0), 1), ((0.7, 15.0), 0)):
        other = TL.trial_lit(reqs[0], sc["intr"], sc["Ts"][0], light, FILTERS[0], k_img, k_mg, photo_gate=gate)
        for k in TL.SUMS[2:] + ("n_fit", "n_interior"):
            assert other[k] == base[k], k


@pytest.mark.parametrize("shape", [(64, 48), (131, 67)], ids=lambda s: "%dx%d" % s)
def test_a_brighter_destination_loses_its_candidates_and_the_light_restores_them(shape):
    """The demonstration on the reference alone, with the image altered before its gradient plane is taken: at most 0.6 of the unaltered
    scene's candidates without the light, at least 0.95 with (1.6, -20); the trial's one-shot fit restores at least 0.95 of its targets."""
    sc, reqs, k_img, k_mg = scene_inputs(*shape)
    bright = AL.brighten(k_img)
    b_mg = synth.max_abs_gradient(bright).astype(F)
    base = A.absorb(reqs, sc["intr"], sc["Ts"], FILTERS[0], k_img, k_mg, sc["state"])["stats"]["n_candidates"]
    unlit = A.absorb(reqs, sc["intr"], sc["Ts"], FILTERS[0], bright, b_mg, sc["state"])["stats"]["n_candidates"]
    lit = AL.absorb_lit(reqs, sc["intr"], sc["Ts"], [(1.6, -20.0)] * 4, FILTERS[0], bright, b_mg, sc["state"])["stats"]["n_candidates"]
    print(shape, "n_candidates: unaltered", base, "altered unlit", unlit, "altered lit", lit)
    assert unlit <= 0.6 * base and lit >= 0.95 * base
    t_base = T.trial(reqs[0], sc["intr"], sc["Ts"][0], FILTERS[0], k_img, k_mg)["n_targets"]
    first = TL.trial_lit(reqs[0], sc["intr"], sc["Ts"][0], None, FILTERS[0], bright, b_mg)
    light, refused = TL.light_solve(first)
    second = TL.trial_lit(reqs[0], sc["intr"], sc["Ts"][0], light, FILTERS[0], bright, b_mg)
    print(shape, "n_targets: unaltered", t_base, "altered unlit", first["n_targets"], "fitted light", light, "altered lit", second["n_targets"])
    assert not refused and first["n_targets"] <= 0.6 * t_base and second["n_targets"] >= 0.95 * t_base
