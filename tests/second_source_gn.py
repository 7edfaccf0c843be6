"""SECOND SOURCE of the Gauss-Newton side of the oracle (test infrastructure; r06 verdict, "second-source the GN oracle").

A vectorised numpy float32 restatement of

    GetIntrinsic                                              UserDefinedFunc.cpp:34-50
    PixelWisePyramid::calculatePixelWise (FCA, per pixel)     PixelWisePyramid.cpp:58-413
    PixelWisePyramid::calculatePixelWiseParallel (bands)      PixelWisePyramid.cpp:416-455
    PixelWisePyramid::updatePose (step, weightedPose)         PixelWisePyramid.cpp:460-491
    PixelWisePyramid::saveWeights(true)                       PixelWisePyramid.cpp:500-550
    precomputePixelWiseInvCompositional (ICA SD, weighted SD) PixelWisePyramid.cpp:561-685
    iteratePixelWiseInvCompositional (ICA residual, b)        PixelWisePyramid.cpp:690-917
    calculatePixelWiseParallelInvCompositional (bands, H)     PixelWisePyramid.cpp:920-954
    GetImagePoseEstimate, the level / iteration loop          ImageFunc.cpp:150-292
    frame::calculateNonZeroDepthPts (mask = depth > 0)        Frame.cpp:298
    frame::finaliseWeights                                    Frame.cpp:678-695
    frame::getInterpolatedElement (u8 with the -1 sentinel,   Frame.h:181-394
      and the gradient planes), frame::calculateGradient      Frame.cpp:185-285 (via tests/second_source_depth.py)

written FROM THE REFERENCE'S TEXT, statement by statement, WITHOUT looking at oracle/ellc_oracle_gn.cpp or at the HIP kernels: the C++
oracle and the kernels are one author's reading of those lines, and a shared misreading would be green in every GPU-vs-oracle test.
tests/test_second_source_gn.py runs both on the same scenes and compares them plane by plane, sum by sum and step by step.

Taken as given (third-party arithmetic whose text is not available, pinned elsewhere):
  * Eigen's `exp` of the 4x4 twist matrix (PixelWisePyramid.cpp:148-155, :765-770): `oracle.se3_exp`;
  * frame::concatenateRelativePose (the pose update of updatePose): `oracle.concat_relative`;
  * cv::Mat::inv() with its default DECOMP_LU (`hessian.inv()`): `oracle.lu_inverse`; the float64 path uses numpy.linalg.solve;
  * the u8 image pyramid, the keyframe's depth pyramid and the depth map's variance pyramid of a level: the oracle's Frame and
    DepthMap (they are restated and pinned by tests/test_oracle_*.py and tests/second_source_depth.py);
  * the u8 tap, the gradient tap and calculateGradient: tests/second_source_depth.py (restated from Frame.h:181-394 and
    Frame.cpp:185-285); `tap` below is the vectorised form of its `interp`, cross-checked against it on sampled points;
  * cv::gemm for `(H^-1 * b^T)^T` (PixelWisePyramid.cpp:466): products of floats accumulated in double in index order, one rounding
    to float at the end; cv::gemm for the ICA Hessian `weightedSteepestDescent * steepestDescent^T` (:931) over the N pixels: its
    order over N is not known here, so `ica_precompute` sums in float64 and rounds once (the tests state the tolerance);
  * OpenCV's `Mat / int` of finaliseWeights (Frame.cpp:688) as a scale by the float `1.0 / n` (MatExpr scale, convertTo);
    exact for n = 1, 2, 4.

Promotions, written out in float64 where the reference promotes:
  * `pow((-cy + y), 2)`, `pow((-cx + x), 2)` and `pow(depth, -1)` (:296-320, :637-662) are `pow(float, int)`: C++11 returns double,
    so the J term they enter is formed in double and rounded to float when it is stored. pow(v, 2) is the exact double v * v;
    pow(z, -1) is written 1.0 / double(z), the correctly rounded reciprocal. glibc's pow(z, -1) is NOT always that: it is one
    double ulp away at ~0.1 % of depths; tests/test_second_source_gn.py checks that the float J terms are the same either way on
    every pixel of its scenes (and pow(v, 2) == v * v exactly).
  * UNZERO (ExternVariable.h:232) compares against the double literals +-1e-10 and yields a double, stored as float.
  * GetIntrinsic divides the float focal lengths by the double `pow(2, level)` and stores floats.
  * the warp's second branch (`SE3_vec[1] != 0`, :255-261) casts each float product to float: the same arithmetic as the first.
  * `abs` in updatePose (:479) is std::abs(float) (`using namespace std`, <cmath>): no truncation. `fabs` in the weight is exact.

Sums: `hessian += w * SD^T SD` and `sd_param += SD * (r * w)` (:367-368) accumulate per band in float in raster order (here a
SEQUENTIAL np.add.accumulate, never np.sum, which is pairwise); the FCA's three bands of nRows / 3 rows are added as
(H1 + H2) + H3 (:441-442); the ICA iterate runs in TWO bands, [0, nRows / 3) and [nRows / 3, nRows) (:936-947). The same per-pixel
terms summed in float64 are the high-precision reference (`Hd`, `bd`).

Project option, not in the reference: `early_exit=False` runs `max_iter` iterations per level (the reference always leaves a level
once weightedPose < 1, ImageFunc.cpp:246-252)."""
import ctypes
import ctypes.util
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import second_source_depth as S1                                           # noqa: E402

F = np.float32
D = np.float64

# ExternVariable.h
CAMERA_PIXEL_NOISE_2 = F(4.0) * F(4.0)                                     # :148
HUBER_D = F(3.0)                                                           # :149
HUBER_HALF = HUBER_D / F(2)                                                # util::HUBER_D / 2: float / int
POSE_WEIGHT = np.array([100000.0, 100000.0, 100000.0, 10000.0, 10000.0, 10000.0], np.float32)   # util::weight, :76
NUM_POSE_THREADS = 3                                                       # :224
NUM_CONST_WT_POSE_EST_THREADS = 3                                          # :227
UNZERO_EPS = 1e-10                                                         # :232, a double literal

# branch classes counted per call (`hist`)
BRANCHES = ("mask0", "tap_oob", "unzero_clamped", "z_negative", "z_positive", "warp_branch1", "warp_branch2",
            "huber_inside", "huber_outside", "early_exit", "max_iter")


def new_hist():
    return {k: 0 for k in BRANCHES}


def add_hist(into, h):
    for k, v in h.items():
        into[k] = into.get(k, 0) + v
    return into


# ---------------------------------------------------------------- intrinsics, taps
def get_intrinsic(fx, fy, cx, cy, level):
    """UserDefinedFunc.cpp:34-50: float / double pow(2, level), stored as float"""
    s = D(2.0) ** level
    return tuple(F(D(F(v)) / s) for v in (fx, fy, cx, cy))


def tap(img, x1, y1, rows, cols):
    """Vectorised frame::getInterpolatedElement (Frame.h:181-279 for u8, :283-394 for a float plane): `img` is the level's stored
    plane, `rows` / `cols` its iterated size (currentRows / currentCols). Each of the four taps is tested with its own pair of
    coordinates: floor x / floor y, raw x / floor y, floor x / raw y, raw x / raw y, against [0, cols - 1] x [0, rows - 1]; the
    in-bounds taps read (floor or CEIL of the coordinate). Returns (value, number of taps out of bounds). A NaN coordinate is
    counted out of bounds (the reference would index with it)."""
    x1 = np.asarray(x1, F); y1 = np.asarray(y1, F)
    nC = F(cols - 1); nR = F(rows - 1)
    fx_ = np.floor(x1); fy_ = np.floor(y1)
    wt0 = y1 - fy_
    wt1 = x1 - fx_

    def inb(x, y):
        return (x >= 0) & (x <= nC) & (y >= 0) & (y <= nR)

    def read(ok, yi, xi):
        yi = np.where(ok, yi, 0).astype(np.int64); xi = np.where(ok, xi, 0).astype(np.int64)
        return np.where(ok, img[yi, xi].astype(F), F(0))

    cxr = np.ceil(x1); cyr = np.ceil(y1)
    ok1 = inb(fx_, fy_); ok2 = inb(x1, fy_); ok3 = inb(fx_, y1); ok4 = inb(x1, y1)
    p1 = read(ok1, fy_, fx_); p2 = read(ok2, fy_, cxr)
    top = ((F(1) - wt1) * p1) + (wt1 * p2)
    p3 = read(ok3, cyr, fx_); p4 = read(ok4, cyr, cxr)
    btm = ((F(1) - wt1) * p3) + (wt1 * p4)
    val = ((F(1) - wt0) * top) + (wt0 * btm)
    n_oob = 4 - (ok1.astype(np.int32) + ok2 + ok3 + ok4)
    return val.astype(F), n_oob


def tap_u8_checked(img, x1, y1, rows, cols):
    """getInterpolatedElement(x, y, 1): -1 when all four taps are out of bounds"""
    v, n = tap(img, x1, y1, rows, cols)
    return np.where(n == 4, F(-1), v).astype(F)


def unzero(z):
    """UNZERO(val) with double literals: compared and clamped in double, stored as float. Returns (z, clamped mask)."""
    z64 = z.astype(D)
    r = np.where(z64 < 0, np.where(z64 > -UNZERO_EPS, -UNZERO_EPS, z64), np.where(z64 < UNZERO_EPS, UNZERO_EPS, z64))
    return r.astype(F), r != z64


def inv_pow(z):
    """pow(float z, -1) -> double"""
    return D(1.0) / z.astype(D)


def jacobian(gx, gy, u, v, z, fx, fy, p=None):
    """steepest descent row of PixelWisePyramid.cpp:296-320 (== :637-662): J = jacob_top + jacob_bottom per component. u = -cx + x,
    v = -cy + y (float), z the depth, gx / gy the gradient taps. The pow() terms are double, rounded to float on assignment.
    p: pow(z, -1) in double (default 1.0 / double(z))."""
    fx64, fy64 = D(fx), D(fy)
    p = inv_pow(z) if p is None else p
    u64 = u.astype(D); v64 = v.astype(D)
    bottom0 = (gy.astype(D) * (-(fy64 + (v64 * v64) / fy64))).astype(F)
    top0 = gx * (-(v * u) / fy)
    bottom1 = gy * ((v * u) / fx)
    top1 = (gx.astype(D) * (fx64 + (u64 * u64) / fx64)).astype(F)
    bottom2 = gy * ((fy * u) / fx)
    top2 = gx * (-((fx * v) / fy))
    top3 = (gx.astype(D) * (fx64 * p)).astype(F)
    bottom4 = (gy.astype(D) * (fy64 * p)).astype(F)
    bottom5 = (gy.astype(D) * ((-v).astype(D) * p)).astype(F)
    top5 = (gx.astype(D) * ((-u).astype(D) * p)).astype(F)
    zero = np.zeros_like(top0)
    return np.stack([top0 + bottom0, top1 + bottom1, top2 + bottom2, top3 + zero, zero + bottom4, top5 + bottom5]).astype(F)


# ---------------------------------------------------------------- one level's inputs
class Level:
    """Everything one pyramid level of one keyframe / frame pair reads: the stored u8 images, the iterated size, the keyframe's depth
    and the depth map's variance at the level (given: the oracle's Frame / DepthMap), intrinsics, and the gradient planes of both
    frames (calculateGradient on the iterated size, restated in tests/second_source_depth.py)."""

    def __init__(self, kf_img, cur_img, depth, var, intrinsics, level):
        self.level = level
        self.rows, self.cols = depth.shape
        self.kf_img = np.ascontiguousarray(kf_img, np.uint8)
        self.cur_img = np.ascontiguousarray(cur_img, np.uint8)
        self.depth = np.ascontiguousarray(depth, F)
        self.var = np.ascontiguousarray(var, F)
        self.fx, self.fy, self.cx, self.cy = get_intrinsic(*intrinsics, level)
        self.mask = self.depth > F(0)                                       # Frame.cpp:298
        self.cur_gx, self.cur_gy = S1.calculate_gradient(self.cur_img[:self.rows, :self.cols])
        self.kf_gx, self.kf_gy = S1.calculate_gradient(self.kf_img[:self.rows, :self.cols])
        ys, xs = np.nonzero(self.mask)                                      # raster order
        self.ys, self.xs = ys, xs
        self.z = self.depth[ys, xs]
        self.u = F(-self.cx) + xs.astype(F)                                 # (-resized_cx + x)
        self.v = F(-self.cy) + ys.astype(F)

    @classmethod
    def from_oracle(cls, kf, cur, dm, intrinsics, level):
        rows, cols = kf.level_dims(level)[3], kf.level_dims(level)[2]
        _, var = dm.pyr_level(level)
        return cls(kf.image(level), cur.image(level), kf.depth(level), var[:rows, :cols], intrinsics, level)


def _band_rows(rows, n_bands, ys):
    """band index of each listed pixel: bands [k rows / n, (k + 1) rows / n), the last one to nRows (y_increment = nRows / n)"""
    inc = rows // n_bands
    return np.minimum(ys // inc if inc > 0 else np.full_like(ys, n_bands - 1), n_bands - 1)


def _seq_sum(terms):
    """float32 sum in list order, one rounding per addition (the reference's `+=`); terms: (K, n) -> (K,)"""
    if terms.shape[1] == 0:
        return np.zeros(terms.shape[0], F)
    return np.add.accumulate(terms, axis=1, dtype=F)[:, -1]


def banded_sum(terms, band, n_bands, order):
    """each band summed sequentially in raster order; then the bands added in `order` (FCA: (B1 + B2) + B3; ICA: B1 + B2)"""
    parts = [_seq_sum(terms[:, band == k]) for k in range(n_bands)]
    acc = parts[0]
    for k in order[1:]:
        acc = (acc + parts[k]).astype(F)
    return acc.astype(F)


# ---------------------------------------------------------------- FCA
def warp(lv, T):
    """world point, transformed point, UNZERO, warped point (PixelWisePyramid.cpp:223-263) for the listed pixels"""
    R = T.astype(F)
    wX = (lv.u * lv.z) / lv.fx                                              # (x - cx) * depth / fx, x promoted to float
    wY = (lv.v * lv.z) / lv.fy
    wZ = lv.z
    # both branches: ((r0 X + r1 Y) + r2 Z) + t, each product a float (the second branch's float() casts are no-ops)
    pX = ((R[0, 0] * wX + R[0, 1] * wY) + R[0, 2] * wZ) + R[0, 3]
    pY = ((R[1, 0] * wX + R[1, 1] * wY) + R[1, 2] * wZ) + R[1, 3]
    pZ = ((R[2, 0] * wX + R[2, 1] * wY) + R[2, 2] * wZ) + R[2, 3]
    pZ, clamped = unzero(pZ)
    wx = ((pX / pZ) * lv.fx) + lv.cx
    wy = ((pY / pZ) * lv.fy) + lv.cy
    return pX, pY, pZ, clamped, wx.astype(F), wy.astype(F)


def fca_level_step_terms(lv, pose, se3_exp):
    """calculatePixelWise over the whole level at `pose`: per-pixel planes, per-pixel H / b terms of the listed (mask != 0) pixels
    and the branch histogram. se3_exp: the given exponential (oracle.se3_exp)."""
    pose = np.asarray(pose, F)
    T = np.asarray(se3_exp(pose), F)
    h = new_hist()
    n = lv.ys.size
    h["mask0"] = int(lv.mask.size - n)
    branch1 = bool(T[0, 1] == 0)                                            # first warp form when exp's (0, 1) entry is 0
    h["warp_branch1" if branch1 else "warp_branch2"] = n
    tx, ty, tz = T[0, 3], T[1, 3], T[2, 3]
    pX, pY, pZ, clamped, wx, wy = warp(lv, T)
    h["unzero_clamped"] = int(clamped.sum())
    h["z_negative"] = int((pZ < 0).sum())
    h["z_positive"] = int((pZ > 0).sum())
    intensity = tap_u8_checked(lv.cur_img, wx, wy, lv.rows, lv.cols)
    oob = intensity == F(-1)
    h["tap_oob"] = int(oob.sum())
    gradx, _ = tap(lv.cur_gx, wx, wy, lv.rows, lv.cols)
    grady, _ = tap(lv.cur_gy, wx, wy, lv.rows, lv.cols)
    J = jacobian(gradx, grady, lv.u, lv.v, lv.z, lv.fx, lv.fy)
    prev = lv.kf_img[lv.ys, lv.xs].astype(F)
    residual = np.where(oob, F(0), intensity - prev).astype(F)
    # weight (:341-359), computed for every listed pixel, kept where the tap is in bounds
    with np.errstate(all="ignore"):
        d = F(1) / lv.z
        gxs = lv.fx * gradx
        gys = lv.fy * grady
        s = F(1) * lv.var[lv.ys, lv.xs]
        g0 = (tx * pZ - tz * pX) / ((pZ * pZ) * d)
        g1 = (ty * pZ - tz * pY) / ((pZ * pZ) * d)
        drpdd = gxs * g0 + gys * g1
        w_p = F(1) / (CAMERA_PIXEL_NOISE_2 + (s * drpdd) * drpdd)
        wrp = np.abs(residual * np.sqrt(w_p))
        inside = wrp < HUBER_HALF
        wh = np.abs(np.where(inside, F(1), HUBER_HALF / wrp))
        weight = np.where(oob, F(0), wh * w_p).astype(F)
    h["huber_inside"] = int((inside & ~oob).sum())
    h["huber_outside"] = int((~inside & ~oob).sum())
    # per-pixel terms: H_ij += (sd_i * w) * sd_j (a 6x1 by 1x6 product), b_i += sd_i * (r * w)
    wsd = J * weight
    Ht = (wsd[:, None, :] * J[None, :, :]).reshape(36, n)
    rw = residual * weight
    bt = J * rw
    # planes
    shp = (lv.rows, lv.cols)
    P = dict(residual=np.zeros(shp, F), weight=np.zeros(shp, F), warpedX=np.full(shp, F(-2)), warpedY=np.full(shp, F(-2)),
             J=np.zeros((6,) + shp, F))
    P["residual"][lv.ys, lv.xs] = residual
    P["weight"][lv.ys, lv.xs] = weight
    P["warpedX"][lv.ys, lv.xs] = np.where(oob, F(-1), wx)
    P["warpedY"][lv.ys, lv.xs] = np.where(oob, F(-1), wy)
    P["J"][:, lv.ys, lv.xs] = J
    P["rawX"] = np.full(shp, np.nan, F); P["rawY"] = np.full(shp, np.nan, F)       # the warped point, in or out of bounds
    P["rawX"][lv.ys, lv.xs] = wx
    P["rawY"][lv.ys, lv.xs] = wy
    return dict(planes=P, Ht=Ht, bt=bt, hist=h, oob=oob, wx=wx, wy=wy, branch1=branch1, gradx=gradx, grady=grady)


def fca_sums(lv, terms, f32=True):
    """three row bands, each summed in float in raster order, then (H1 + H2) + H3 (PixelWisePyramid.cpp:416-446); and the same terms
    summed in float64. f32=False: the float64 sums only (H, b are None)."""
    s64 = np.array([row.astype(D).sum() for t in (terms["Ht"], terms["bt"]) for row in t])   # row by row: 1280 x 960 stays small
    if not f32:
        return None, None, s64[:36].reshape(6, 6), s64[36:]
    allt = np.concatenate([terms["Ht"], terms["bt"]], axis=0)
    band = _band_rows(lv.rows, NUM_POSE_THREADS, lv.ys)
    s = banded_sum(allt, band, NUM_POSE_THREADS, (0, 1, 2))
    return s[:36].reshape(6, 6), s[36:], s64[:36].reshape(6, 6), s64[36:]


def gemm_hinv_b(Hinv, b):
    """(H^-1 * b^T)^T: float products accumulated in double in index order, rounded to float once (cv::gemm, given)"""
    Hi = np.asarray(Hinv, F).astype(D); bb = np.asarray(b, F).astype(D)
    out = np.zeros(6, D)
    for k in range(6):
        out = out + Hi[:, k] * bb[k]
    return out.astype(F)


def update_pose(Hinv, b, pose, concat_relative):
    """PixelWisePyramid.cpp:460-491: delta = -(H^-1 b), weightedPose = sum_i |delta_i * weight_i| in float left to right, then
    concatenateRelativePose(delta, pose) (given)"""
    delta = (-gemm_hinv_b(Hinv, b)).astype(F)
    wp = F(0)
    for i in range(6):
        wp = F(wp + np.abs(F(delta[i] * POSE_WEIGHT[i])))
    new_pose = np.asarray(concat_relative(delta, np.asarray(pose, F)), F)
    return delta, wp, new_pose


def fca_step(lv, pose, givens):
    """one calculatePixelWiseParallel: planes, H, b (f32 bands and f64), H^-1, delta, weightedPose, the new pose"""
    t = fca_level_step_terms(lv, pose, givens.se3_exp)
    H, b, Hd, bd = fca_sums(lv, t)
    ok, Hinv = givens.lu_inverse(H)
    delta, wp, new_pose = update_pose(Hinv, b, pose, givens.concat_relative)
    return dict(H=H, b=b, Hd=Hd, bd=bd, Hinv=Hinv, delta=delta, weighted=wp, pose=new_pose, planes=t["planes"], hist=t["hist"],
                terms=t)


def step_f64(Hd, bd, pose, concat_relative):
    """the float64 step of the float64 sums: delta = -solve(Hd, bd), applied with the given concatenation"""
    delta = -np.linalg.solve(Hd, bd)
    return delta, np.asarray(concat_relative(delta.astype(F), np.asarray(pose, F)), F)


# ---------------------------------------------------------------- ICA
def ica_precompute(lv, weights):
    """precomputePixelWiseInvCompositional (:561-685): SD from the keyframe's own gradient planes at the pixel, weighted by the
    keyframe's (finalised) weights; 0 where the mask is 0. H = weightedSD * SD^T summed in float64 and rounded once (given: cv::gemm's
    order over N). Returns SD (6, N), weighted SD (6, N), H (f32), Hd (f64)."""
    n = lv.rows * lv.cols
    gx = lv.kf_gx[lv.ys, lv.xs]; gy = lv.kf_gy[lv.ys, lv.xs]
    J = jacobian(gx, gy, lv.u, lv.v, lv.z, lv.fx, lv.fy)
    w = np.asarray(weights, F)[lv.ys, lv.xs]
    WJ = (J * w).astype(F)
    idx = lv.ys * lv.cols + lv.xs
    sd = np.zeros((6, n), F); wsd = np.zeros((6, n), F)
    sd[:, idx] = J; wsd[:, idx] = WJ
    Hd = WJ.astype(D) @ J.astype(D).T
    return sd, wsd, Hd.astype(F), Hd


def ica_iterate(lv, pose, sd, weights, se3_exp):
    """iteratePixelWiseInvCompositional (:690-917): warp as FCA, residual, b_i += SD_i * (r * w) with the keyframe's weights; two
    row bands [0, nRows/3), [nRows/3, nRows) (:936-947), b = b1 + b2. Returns b (f32), bd (f64), hist."""
    T = np.asarray(se3_exp(np.asarray(pose, F)), F)
    h = new_hist()
    n = lv.ys.size
    h["mask0"] = int(lv.mask.size - n)
    h["warp_branch1" if T[0, 1] == 0 else "warp_branch2"] = n
    pX, pY, pZ, clamped, wx, wy = warp(lv, T)
    h["unzero_clamped"] = int(clamped.sum()); h["z_negative"] = int((pZ < 0).sum()); h["z_positive"] = int((pZ > 0).sum())
    intensity = tap_u8_checked(lv.cur_img, wx, wy, lv.rows, lv.cols)
    oob = intensity == F(-1)
    h["tap_oob"] = int(oob.sum())
    residual = np.where(oob, F(0), intensity - lv.kf_img[lv.ys, lv.xs].astype(F)).astype(F)
    w = np.asarray(weights, F)[lv.ys, lv.xs]
    J = sd[:, lv.ys * lv.cols + lv.xs]
    bt = J * (residual * w)
    inc = lv.rows // NUM_CONST_WT_POSE_EST_THREADS
    band = (lv.ys >= inc).astype(np.int64)
    b = banded_sum(bt, band, 2, (0, 1))
    return b, bt.astype(D).sum(axis=1), h


# ---------------------------------------------------------------- the level loop
class Givens:
    """the third-party pieces taken as given (see the module docstring)"""

    def __init__(self, oracle):
        self.se3_exp = oracle.se3_exp
        self.concat_relative = oracle.concat_relative
        self.lu_inverse = oracle.lu_inverse


def align(levels, givens, max_iter, init_pose=None, early_exit=True, ica=False, kf_weights=None, save_weights=False):
    """GetImagePoseEstimate's loop (ImageFunc.cpp:150-292) over `levels` (a list of Level, index = pyramid level), coarsest first.
    After each step: weightedPose < 1 sets iter_counter = MAX_ITER - 1 (early exit; `early_exit=False` is the project's option of
    always running max_iter); then, FCA only, saveWeights(true) when iter_counter == MAX_ITER - 1 — so also at an early-exited
    iteration: the weight plane of that step is added to the keyframe's. Returns dict(pose, iters per level, weighted (last),
    saved = {level: weight plane}, saved_planes = {level: all planes of that step}, hist)."""
    pose = np.zeros(6, F) if init_pose is None else np.asarray(init_pose, F).copy()
    L = len(levels)
    iters = [0] * L
    saved, saved_planes = {}, {}
    hist = new_hist()
    wp = F(0)
    for level in range(L - 1, -1, -1):
        lv = levels[level]
        mi = int(max_iter[level])
        if ica:
            sd, _, H, _ = ica_precompute(lv, kf_weights[level])
            _, Hinv = givens.lu_inverse(H)
        it = 0
        while it < mi:
            if ica:
                b, _, h = ica_iterate(lv, pose, sd, kf_weights[level], givens.se3_exp)
                _, wp, pose = update_pose(Hinv, b, pose, givens.concat_relative)
            else:
                r = fca_step(lv, pose, givens)
                h, wp, pose = r["hist"], r["weighted"], r["pose"]
            add_hist(hist, h)
            iters[level] += 1
            if early_exit and wp < F(1.0):                                  # ImageFunc.cpp:246-247: jump to the last iteration
                hist["early_exit" if it < mi - 1 else "max_iter"] += 1
                it = mi - 1
            elif it == mi - 1:
                hist["max_iter"] += 1
            if not ica and save_weights and it == mi - 1:
                saved[level] = r["planes"]["weight"].copy()
                saved_planes[level] = r["planes"]
            it += 1
    return dict(pose=pose, iters=np.array(iters, np.int32), weighted=wp, saved=saved, saved_planes=saved_planes, hist=hist)


class KeyframeWeights:
    """weight_pyramid / numWeightsAdded of one keyframe: saveWeights(true) adds (float), finaliseWeights divides (Frame.cpp:678-695)"""

    def __init__(self, levels):
        self.w = [np.zeros((lv.rows, lv.cols), F) for lv in levels]
        self.n = [0] * len(levels)

    def add(self, saved):
        for level, plane in saved.items():
            self.w[level] = (self.w[level] + plane).astype(F)
            self.n[level] += 1

    def finalise(self):
        """`weight_pyramid[level] / numWeightsAdded[level]` where the count is > 0 (else the reference prints and keeps the plane)"""
        for level in range(len(self.w)):
            if self.n[level] > 0:
                self.w[level] = (self.w[level] * F(1.0 / self.n[level])).astype(F)


# ---------------------------------------------------------------- libm, for the promotion check
def libm_pow():
    name = ctypes.util.find_library("m") or "libm.so.6"
    m = ctypes.CDLL(name)
    m.pow.restype = ctypes.c_double
    m.pow.argtypes = (ctypes.c_double, ctypes.c_double)
    return m.pow


def libm_pow_array(x, y):
    """libm's pow(double(x_i), y) element by element"""
    f = libm_pow()
    x = np.asarray(x, D).ravel()
    return np.array([f(float(a), float(y)) for a in x], D)
