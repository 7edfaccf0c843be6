"""CPU checks of tests/sim3_reference.py, the numpy restatement of ellc_keyframe_sim3_step's rule that the GPU tests hold the kernels
to: scalar against vectorised on the GPU tests' scenes, a hand-worked answer on a 4x4 level, the identity pair, both Jacobians
against central finite differences in double, and the case classes the GPU tests' batch has to reach."""
import numpy as np
import pytest
from scipy.linalg import expm

import sim3_reference as S

F = np.float32
FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
# (source, destination, transform): the v14 batch, and one pair at the shifted transform (index 3 of transforms()) for the tap-less band
PAIRS = [(0, 0, 0), (0, 1, 1), (1, 0, 1), (2, 0, 2), (1, 1, 1), (1, 2, 3)]
SHAPES = [(64, 48), (23, 17), (131, 67)]


def transforms(m, fx):
    """scene_transforms' three, and a pure shift along x of 3.3 pixels at the median depth m: the scenes keep a border of three pixels
    free of hypotheses, so that points of about that depth land between the last column's centre and the image's edge, where a
    candidate exists (u + 0.5 < cols) and the four taps do not (x0 + 1 == cols)."""
    shift = np.array([1, 0, 0, 3.3 * m / fx, 0, 1, 0, 0, 0, 0, 1, 0], F)
    return np.concatenate([S.scene_transforms(m), shift[None]])


def scene_planes(w, h):
    """Scenes 11, 12, 13 of the GPU tests as level-0 planes (the CPU side has no pyramid kernels: level 0 only)."""
    scenes = [S.make_scene(w, h, seed) for seed in (11, 12, 13)]
    m = float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0]))
    intr = S.level_intrinsics(*scenes[0]["intrinsics"], 0)
    return [(s["depth0"], s["var0"], s["kf_image"]) for s in scenes], intr, transforms(m, float(intr[0]))


_cache = {}


def batch_records(shape, flt):
    """The vectorised reference over PAIRS, computed once per (shape, filter) and left unchanged."""
    key = (shape, flt)
    if key not in _cache:
        planes, intr, Ts = scene_planes(*shape)
        _cache[key] = [S.step(planes[s], planes[d], intr, Ts[t], flt) for s, d, t in PAIRS]
    return _cache[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_scalar_equals_vectorised(shape, flt):
    planes, intr, Ts = scene_planes(*shape)
    kept = 0
    for (s, d, t), a in zip(PAIRS, batch_records(shape, flt)):
        b = S.step_scalar(planes[s], planes[d], intr, Ts[t], flt)
        assert S.fields_equal(a, b), (s, d, t)
        assert a["n_photo_huber"] <= a["n_photo"] <= a["n_in_view"] <= a["n_kept"] and a["n_depth"] + a["n_depth_gated"] <= a["n_in_view"]
        assert a["n_kept"] == a["n_in_view"] + a["behind_camera"] + a["outside"] + a["bad_var"]
        for k in (S.h_index(2, 6), S.h_index(3, 6), S.h_index(4, 6)):   # no term ever reaches them
            assert a["H"][k] == 0 and a["n_H"][k] == 0
        assert a["b"][6] == 0 or a["n_depth"] > 0
        kept += a["n_kept"]
    assert kept > 0


# 4 columns x 4 rows, fx = fy = 1, cx = cy = 0, T = identity, filter (0, 0, 1, 1): every ok pixel is kept. All numbers are small
# multiples of powers of two: exact in f32. sigma_i2 = 16 (w0 = 1/16, sp = 1/4), huber_k = 1/2, gate_k2 = 1, depth_weight = 1.
# The destination's image is 8 x + 16 y: inside a cell dx0 = dx1 = 8, gx = 8, gy = 16. Every source pixel has Z = 1, V = 1/4, so
# P' = (x, y, 1), nid = 1, u = x, v = y, ax = ay = 0, nvar = V, the target is the pixel itself.
#   P (1,1): taps (1,1) 24, 32, 40, 48: Iw = 24; Is = 20: rp = 4. A = 8, Bv = 16, Cq = -((8 + 16) 1) = -24;
#            Jp = [-24 - 16, 8 + 24, 16 - 8, 8, 16, -24] = [-40, 32, 8, 8, 16, -24]; e = 4 / 4 = 1 > 1/2: HUBER, wp = (1/16)(1/2) = 1/32;
#            chi2 16/32 = 1/2. Depth: Zt = 2, Vt = 1/4: s = 1/2, rd = 1 - 1/2 = 1/2, rd^2 = 1/4 <= 1/2: IN; wd = 2, a2 = 1,
#            Jd = [-1, 1, 0, 0, 0, -1, -1]; chi2 (1/4) 2 = 1/2.
#   Q (0,0): taps 0, 8, 16, 24: Iw = 0 = Is: rp = 0. A = 8, Bv = 16, Cq = 0; Jp = [-16, 8, 0, 8, 16, 0]; wp = 1/16. Depth: Zt = 0: no overlap.
#   R (3,1): u = 3: x0 + 1 = 4 = cols: IN VIEW (3.5 < 4), NO TAPS. Depth: Zt = 1/4, Vt = 1/4: s = 1/2, rd = 1 - 4 = -3, 9 > 1/2: GATED.
#   S (1,3): v = 3: y0 + 1 = 4 = rows: in view, no taps. Depth: Zt = 1, Vt = 0: s = 1/4, rd = 0: IN; wd = 4, Jd = [-3, 1, 0, 0, 0, -1, -1], r = 0.
#   (2,2) Z = 1, V = -1: not a hypothesis, not kept.
def hand_case():
    sd = np.zeros((4, 4), F); sv = np.full((4, 4), -1, F)
    for x, y, V in ((1, 1, 0.25), (0, 0, 0.25), (3, 1, 0.25), (1, 3, 0.25), (2, 2, -1.0)):
        sd[y, x] = 1; sv[y, x] = V
    dd = np.zeros((4, 4), F); dv = np.full((4, 4), -1, F)
    for x, y, Z, V in ((1, 1, 2, 0.25), (3, 1, 0.25, 0.25), (1, 3, 1, 0)):
        dd[y, x] = Z; dv[y, x] = V
    dimg = (8 * np.arange(4)[None, :] + 16 * np.arange(4)[:, None]).astype(np.uint8)
    simg = dimg.copy(); simg[1, 1] = 20
    return (sd, sv, simg), (dd, dv, dimg), (1.0, 1.0, 0.0, 0.0), np.array(IDENTITY, F)


HAND_PARAMS = dict(sigma_i2=16.0, huber_k=0.5, gate_k2=1.0, depth_weight=1.0)
HAND_TERMS = [   # (J over the seven parameters, w, r) of every term
    ([-40, 32, 8, 8, 16, -24, 0], 1 / 32, 4), ([-16, 8, 0, 8, 16, 0, 0], 1 / 16, 0),
    ([-1, 1, 0, 0, 0, -1, -1], 2, 0.5), ([-3, 1, 0, 0, 0, -1, -1], 4, 0)]


@pytest.mark.parametrize("fn", [S.step, S.step_scalar])
def test_hand_worked_answer(fn):
    src, dst, intr, T = hand_case()
    got = fn(src, dst, intr, T, (0, 0, 1.0, 1), HAND_PARAMS)
    assert [got[k] for k in S.INT_FIELDS] == [4, 4, 2, 1, 2, 1]
    H = np.zeros((7, 7)); b = np.zeros(7)
    for J, w, r in HAND_TERMS:   # (small dyadic numbers: every product and sum is exact in double)
        J = np.array(J, np.float64)
        H += w * np.outer(J, J); b += w * J * r
    assert list(got["H"]) == list(H[np.triu_indices(7)]) and list(got["b"]) == list(b)
    assert got["b"] == [-6, 5, 1, 1, 2, -4, -1] and got["chi2_photo"] == 0.5 and got["chi2_depth"] == 0.5
    if fn is S.step:
        assert (got["behind_camera"], got["outside"], got["bad_var"], got["no_taps"], got["no_overlap"]) == (0, 0, 0, 2, 1)
    # inside the Huber threshold the first pixel has the full weight
    wide = fn(src, dst, intr, T, (0, 0, 1.0, 1), dict(HAND_PARAMS, huber_k=1.0))
    assert wide["n_photo_huber"] == 0 and wide["chi2_photo"] == 1.0 and wide["b"][3] == 2


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_identity_pair(flt):
    """b = 0 and chi2 = 0 exactly need u == x and v == y exactly: ((x - cx) Z / fx) (1 / Z) fx + cx has four roundings in f32 and
    returns x exactly only where they are exact, i.e. for intrinsics and depths that are powers of two. So the scene of this check is
    scene 11 with fx = fy = 64, cx = 32, cy = 24 and every depth moved to the nearest power of two. (Scene 11 as it is, with
    fx = 54.72: u misses x by a few ulp and the f32 rule gives |b| up to 1.4e-3 and chi2_photo up to 6.1e-10 - bounded below - while the
    depth term, whose target is the pixel itself, is exactly 0 on any scene.)"""
    s = S.make_scene(64, 48, 11)
    with np.errstate(all="ignore"):
        d2 = np.where(s["depth0"] > 0, np.exp2(np.round(np.log2(s["depth0"]))), s["depth0"]).astype(F)
    p = (d2, s["var0"], s["kf_image"])
    r = S.step(p, p, (64.0, 64.0, 32.0, 24.0), IDENTITY, flt)
    assert r["n_kept"] > 100 and r["n_kept"] == r["n_in_view"] == r["n_photo"] == r["n_depth"] and r["n_photo_huber"] == r["n_depth_gated"] == 0
    assert r["b"] == [0.0] * 7 and r["abs_b"] == [0.0] * 7 and r["chi2_photo"] == 0 and r["chi2_depth"] == 0
    assert min(r["H"][S.h_index(i, i)] for i in range(7)) > 0
    assert r["n_kept"] == int(S.classify(d2, s["var0"], flt)["kept"].sum())
    # the scene as it is: the depth term is exactly zero; u is within 4 ulp of 64 of x (four roundings of values below 64), a grey
    # value moves by at most 2 * 255 per pixel of that, so chi2_photo <= n (510 * 2^-19)^2 / 16
    q = (s["depth0"], s["var0"], s["kf_image"])
    g = S.step(q, q, S.level_intrinsics(*s["intrinsics"], 0), IDENTITY, flt)
    print("scene 11 as it is: max |b| %.3g chi2_photo %.3g" % (max(abs(v) for v in g["b"]), g["chi2_photo"]))
    assert g["chi2_depth"] == 0 and g["n_depth"] == g["n_in_view"] == g["n_kept"] > 100
    assert g["chi2_photo"] <= g["n_photo"] * (510 * 2.0 ** -19) ** 2 / 16


def test_jacobians_against_central_differences():
    """Jp against central differences of rp, Jd against those of rd, in double at a generic T (pair 0 -> 1 at transform 1, 64x48).
    The double residuals start from the f32 point P' of the reference and move it by expm(xi^): rp(xi) is the bilinear polynomial of
    the pixel's own cell at (u0 + fx (x'/z' - x'0/z'0), ...), u0 the reference's f32 u - so that at xi = 0 it is the reference's
    residual and crossing a cell border cannot enter. Tolerance per pixel: the f32 entries are made of at most 16 rounded operations
    on magnitudes below M = (|gx| fx + |gy| fy) nid (1 + |x'| + |y'| + |z'|) (1 + nid (|x'| + |y'|)) - 2^-20 M - and the central
    difference with h = 1e-4 is off by h^2 times third derivatives of the order nid^2 M: 1e-6 (1 + nid^2) M is asked, more than both."""
    planes, intr, Ts = scene_planes(64, 48)
    T = Ts[1]
    r = S.step(planes[0], planes[1], intr, T, FILTERS[0], detail=True)
    fx, fy, cx, cy = (float(v) for v in intr)
    dimg = planes[1][2].astype(np.float64)
    h = 1e-4
    rng = np.random.default_rng(0)

    def moved(P0, xi):
        return (expm(S.generator(xi)) @ np.array([P0[0], P0[1], P0[2], 1.0]))[:3]

    ph = r["photo"]
    assert ph["i"].size > 200
    worst = 0.0
    for k in rng.permutation(ph["i"].size)[:60]:
        P0 = np.array([ph["xp"][k], ph["yp"][k], ph["zp"][k]], np.float64)
        x0, y0 = int(ph["x0"][k]), int(ph["y0"][k])
        nid = 1.0 / P0[2]
        u0 = float(F(F(F(ph["xp"][k] * F(nid)) * F(fx)) + F(cx))); v0 = float(F(F(F(ph["yp"][k] * F(nid)) * F(fy)) + F(cy)))
        I00, I01, I10, I11 = dimg[y0, x0], dimg[y0, x0 + 1], dimg[y0 + 1, x0], dimg[y0 + 1, x0 + 1]

        def rp(xi):
            P = moved(P0, xi)
            ax = u0 + fx * (P[0] / P[2] - P0[0] / P0[2]) - x0; ay = v0 + fy * (P[1] / P[2] - P0[1] / P0[2]) - y0
            top = I00 + ax * (I01 - I00); bot = I10 + ax * (I11 - I10)
            return top + ay * (bot - top)
        J = np.array([float(c[k]) for c in ph["J"]] + [0.0])
        gx, gy = abs(J[3]) / (fx * nid), abs(J[4]) / (fy * nid)
        M = (gx * fx + gy * fy) * nid * (1 + np.abs(P0).sum()) * (1 + nid * (abs(P0[0]) + abs(P0[1])))
        for p in range(7):
            e = np.zeros(7); e[p] = h
            fd = (rp(e) - rp(-e)) / (2 * h)
            tol = 1e-6 * (1 + nid * nid) * M + 1e-9
            worst = max(worst, abs(fd - J[p]) / tol)
            assert abs(fd - J[p]) <= tol, (k, p, fd, J[p], tol)
    print("photometric Jacobian: worst |fd - J| / tolerance %.3g" % worst)
    dp = r["depth"]
    assert dp["i"].size > 200
    worst = 0.0
    for k in rng.permutation(dp["i"].size)[:60]:
        P0 = np.array([dp["xp"][k], dp["yp"][k], dp["zp"][k]], np.float64)
        nid = 1.0 / P0[2]
        J = np.zeros(7)
        J[[0, 1, 5, 6]] = [float(c[k]) for c in dp["J"]]
        M = nid * nid * (1 + abs(P0[0]) + abs(P0[1])) + nid
        for p in range(7):
            e = np.zeros(7); e[p] = h
            fd = (1.0 / moved(P0, e)[2] - 1.0 / moved(P0, -e)[2]) / (2 * h)   # (1 / Zt is a constant of the pixel)
            tol = 1e-6 * (1 + nid * nid) * M + 1e-9
            worst = max(worst, abs(fd - J[p]) / tol)
            assert abs(fd - J[p]) <= tol, (k, p, fd, J[p], tol)
    print("depth Jacobian: worst |fd - J| / tolerance %.3g" % worst)


@pytest.mark.parametrize("shape", [(64, 48), (131, 67)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
def test_scenes_reach_every_case_class(shape, flt):
    """A condition on the inputs of the GPU tests, which the reference alone must satisfy."""
    recs = batch_records(shape, flt)
    classes = {k: sum(r[k] for r in recs) for k in ("n_photo", "n_photo_huber", "n_depth", "n_depth_gated", "no_taps", "behind_camera", "outside")}
    print(shape, flt, classes)
    assert min(classes.values()) > 0, classes


def test_solve_and_apply_of_the_reference():
    """The numpy side of the loop: solve follows the library's singularity rule, apply is expm in double rounded once."""
    rng = np.random.default_rng(3)
    A = rng.normal(size=(7, 7)); A = A @ A.T + 7 * np.eye(7)
    b = rng.normal(size=7)
    xi, singular = S.solve(A[np.triu_indices(7)], b)
    assert not singular and np.allclose(A @ xi, -b, rtol=0, atol=1e-12)
    A[6, :] = 0; A[:, 6] = 0
    assert S.solve(A[np.triu_indices(7)], b)[1]
    T = np.array([0.9, 0.1, 0, 1, -0.1, 0.9, 0, 2, 0, 0, 1.1, 3], F)
    assert S.apply(np.zeros(7), T).tobytes() == np.asarray(T, F).tobytes()
    grown = S.apply([0, 0, 0, 0, 0, 0, np.log(2.0)], T)   # a pure log-scale doubles all twelve entries
    assert np.allclose(grown, 2 * np.asarray(T, F), rtol=2e-7, atol=0)
    assert S.sim3_errors(grown, T)[0] == pytest.approx(1.0, abs=1e-6)
