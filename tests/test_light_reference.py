"""CPU checks of tests/light_reference.py, the numpy restatement of the photometric rule with an affine light that the GPU tests hold
ellc_keyframe_light_step and ellc_keyframe_sim3_step_lit to: scalar against vectorised on the GPU tests' scenes, sim3_reference.step
as the independent anchor at the light (1, 0), a hand-worked answer on the 4x4 level of tests/test_sim3_reference.py, the case classes
the GPU tests' batch has to reach, that the light moves pixels across the Huber threshold, and the exact recovery of a known light."""
import numpy as np
import pytest

import light_reference as LR
import sim3_reference as S
import test_sim3_reference as TS

F = np.float32
FILTERS = TS.FILTERS
PAIRS = TS.PAIRS
LIGHTS = [(1.0, 0.0), (0.8, 25.0), (1.25, -20.0)]

_cache = {}


def batch_records(shape, flt, light):
    """The vectorised reference over PAIRS, computed once per (shape, filter, light) and left unchanged."""
    key = (shape, flt, light)
    if key not in _cache:
        planes, intr, Ts = TS.scene_planes(*shape)
        _cache[key] = [LR.step(planes[s], planes[d], intr, Ts[t], flt, light=light, detail=True) for s, d, t in PAIRS]
    return _cache[key]


@pytest.mark.parametrize("shape", TS.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
@pytest.mark.parametrize("light", LIGHTS, ids=["unit", "dim", "bright"])
def test_scalar_equals_vectorised(shape, flt, light):
    planes, intr, Ts = TS.scene_planes(*shape)
    photo = 0
    for (s, d, t), a in zip(PAIRS, batch_records(shape, flt, light)):
        b = LR.step_scalar(planes[s], planes[d], intr, Ts[t], flt, light=light)
        assert LR.fields_equal(a, b), (s, d, t)
        assert a["n_photo_huber"] <= a["n_photo"] <= a["n_in_view"] <= a["n_kept"]
        for k in LR.LIGHT_SUMS:
            assert a["n_" + k] == a["n_photo"] and (a[k] >= 0) and a["abs_" + k] == a[k], k   # every term of the seven sums is >= 0
        photo += a["n_photo"]
    assert photo > 0


@pytest.mark.parametrize("shape", TS.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_unit_light_is_the_sim3_reference(shape, flt):
    """The independent anchor: at (1, 0) the integer fields, chi2_photo and every Sim(3) sum are sim3_reference.step's with ==."""
    for a, b in zip(batch_records(shape, flt, LIGHTS[0]), TS.batch_records(shape, flt)):
        assert S.fields_equal(a, b)
        for k in ("abs_H", "n_H", "abs_b", "n_b", "abs_chi2_photo", "n_chi2_photo", "no_taps", "behind_camera", "outside"):
            assert a[k] == b[k], k


# The 4 x 4 level of tests/test_sim3_reference.py (hand_case; sigma_i2 = 16: w0 = 1/16, sp = 1/4; huber_k = 1/2). Two photometric
# pixels: P (1, 1) with Iw = 24, Is = 20 and Q (0, 0) with Iw = 0, Is = 0.
#   light (1, 0):     P rp = 4, e = 1: HUBER, wp = 1/32; Q rp = 0, wp = 1/16.
#                     sum_w = 3/32, sum_w_s = 20/32, sum_w_t = 24/32, sum_w_ss = 12.5, sum_w_st = 15, sum_w_tt = 18, chi2 = 16/32.
#   light (1/2, 16):  P Ip = 26, rp = -2, e = 1/2: inside, wp = 1/16; Q Ip = 16, rp = -16, e = 4: HUBER, wp = (1/16)(1/8) = 1/128.
#                     sum_w = 9/128, sum_w_s = 20/16, sum_w_t = 24/16, sum_w_ss = 25, sum_w_st = 30, sum_w_tt = 36,
#                     chi2 = 4/16 + 256/128 = 2.25. The Jacobians do not see the light.
HAND = {
    (1.0, 0.0): dict(sums=[3 / 32, 0.625, 0.75, 12.5, 15.0, 18.0, 0.5], huber=1, terms=[([-40, 32, 8, 8, 16, -24, 0], 1 / 32, 4), ([-16, 8, 0, 8, 16, 0, 0], 1 / 16, 0)]),
    (0.5, 16.0): dict(sums=[9 / 128, 1.25, 1.5, 25.0, 30.0, 36.0, 2.25], huber=1,
                      terms=[([-40, 32, 8, 8, 16, -24, 0], 1 / 16, -2), ([-16, 8, 0, 8, 16, 0, 0], 1 / 128, -16)]),
}
HAND_DEPTH_TERMS = TS.HAND_TERMS[2:]


@pytest.mark.parametrize("fn", [LR.step, LR.step_scalar])
@pytest.mark.parametrize("light", list(HAND), ids=["unit", "half"])
def test_hand_worked_answer(fn, light):
    src, dst, intr, T = TS.hand_case()
    got = fn(src, dst, intr, T, (0, 0, 1.0, 1), TS.HAND_PARAMS, light=light)
    want = HAND[light]
    assert [got[k] for k in S.INT_FIELDS] == [4, 4, 2, want["huber"], 2, 1]
    assert [got[k] for k in LR.LIGHT_SUMS] == want["sums"]
    H = np.zeros((7, 7)); b = np.zeros(7)
    for J, w, r in want["terms"] + HAND_DEPTH_TERMS:   # (small dyadic numbers: every product and sum is exact in double)
        J = np.array(J, np.float64)
        H += w * np.outer(J, J); b += w * J * r
    assert list(got["H"]) == list(H[np.triu_indices(7)]) and list(got["b"]) == list(b) and got["chi2_depth"] == 0.5
    if light == (0.5, 16.0):
        assert got["b"] == [6, -4, -1, -2, -4, 2, -1]
    # the fit of the two pixels: the line through (20, 24) and (0, 0)
    (gain, offset), refused = LR.solve(got, light, dict(min_pixels=2))
    assert not refused and abs(float(gain) - 1.2) < 1e-6 and abs(float(offset)) < 1e-6
    assert LR.solve(got, light, dict(min_pixels=3)) == ((F(light[0]), F(light[1])), True)


@pytest.mark.parametrize("shape", [(64, 48), (131, 67)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
@pytest.mark.parametrize("light", LIGHTS, ids=["unit", "dim", "bright"])
def test_scenes_reach_every_case_class(shape, flt, light):
    """A condition on the inputs of the GPU tests, which the reference alone must satisfy: pixels inside the Huber threshold, beyond
    it, in view without four taps, behind the camera and outside the image."""
    recs = batch_records(shape, flt, light)
    classes = {k: sum(r[k] for r in recs) for k in ("n_photo_huber", "no_taps", "behind_camera", "outside")}
    classes["inside_huber"] = sum(r["n_photo"] - r["n_photo_huber"] for r in recs)
    print(shape, flt, light, classes)
    assert min(classes.values()) > 0, classes


def test_the_light_changes_which_pixels_are_huber_pixels():
    for shape in TS.SHAPES:
        moved = 0
        for a, b in zip(batch_records(shape, FILTERS[0], LIGHTS[0]), batch_records(shape, FILTERS[0], LIGHTS[1])):
            assert np.array_equal(a["photo"]["i"], b["photo"]["i"])   # the same photometric pixels ...
            assert np.array_equal(a["photo"]["Is"], b["photo"]["Is"]) and np.array_equal(a["photo"]["Iw"], b["photo"]["Iw"])
            into = int((a["photo"]["inside"] & ~b["photo"]["inside"]).sum()); out_of = int((~a["photo"]["inside"] & b["photo"]["inside"]).sum())
            moved += min(into, out_of)                                # ... on either side of the threshold, both ways
        assert moved > 0, shape


def test_exact_recovery_of_a_known_light():
    """The power-of-two scene of test_sim3_reference.test_identity_pair (u == x and v == y exactly), the source's grey values forced
    even, the destination's image Is / 2 + 40, the same map, T the identity and a Huber threshold nothing reaches: every weight is
    1/16, every sum a dyadic number below 2^53, so the fit is exact."""
    s = S.make_scene(64, 48, 11)
    with np.errstate(all="ignore"):
        d2 = np.where(s["depth0"] > 0, np.exp2(np.round(np.log2(s["depth0"]))), s["depth0"]).astype(F)
    simg = (np.asarray(s["kf_image"]) & 0xFE).astype(np.uint8)
    dimg = (simg // 2 + 40).astype(np.uint8)
    src, dst, intr, prm = (d2, s["var0"], simg), (d2, s["var0"], dimg), (64.0, 64.0, 32.0, 24.0), dict(huber_k=1e6)
    for flt in FILTERS:
        at_unit = LR.step(src, dst, intr, TS.IDENTITY, flt, prm)
        assert at_unit["n_photo"] > 100 and at_unit["n_photo_huber"] == 0 and at_unit["chi2_photo"] > 0
        (gain, offset), refused = LR.solve(at_unit)
        assert not refused and abs(float(gain) - 0.5) <= 1e-6 and abs(float(offset) - 40.0) <= 1e-4, (gain, offset)
        fitted = LR.step(src, dst, intr, TS.IDENTITY, flt, prm, light=(gain, offset))
        assert fitted["chi2_photo"] == 0 and fitted["b"] == [0.0] * 7 and fitted["abs_b"] == [0.0] * 7
        assert LR.fields_equal(fitted, LR.step_scalar(src, dst, intr, TS.IDENTITY, flt, prm, light=(gain, offset)))


def test_refusals_of_the_reference_solve():
    good = dict(sum_w=2.0, sum_w_s=30.0, sum_w_t=50.0, sum_w_ss=500.0, sum_w_st=775.0, n_photo=100)   # gain 0.5, offset 17.5
    assert LR.solve(good) == ((F(0.5), F(17.5)), False)
    lin = (F(0.9), F(3.0))
    assert LR.solve(dict(good, n_photo=15), lin) == (lin, True)
    assert LR.solve(dict(good, sum_w_ss=450.0), lin) == (lin, True)          # a constant source: det = 0
    assert LR.solve(dict(good, sum_w_st=float("nan")), lin) == (lin, True)
    assert LR.solve(good, lin, dict(gain_min=0.6)) == (lin, True) and LR.solve(good, lin, dict(gain_max=1.0, gain_min=0.5)) == ((F(0.5), F(17.5)), False)
