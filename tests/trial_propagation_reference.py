"""numpy restatement of ellc_keyframe_trial_propagate's records and of ellc_depth_restart_from_keyframes (include/ellc_abi.h, v18), every
intermediate cast to np.float32.

A trial record is steps 1-4 of ellc_depth_absorb_keyframes with the destination's image and maxAbsGradient plane in K's role: the counts
and the targets come from absorb_reference._candidates (imported, once with the gate off - every interior pixel - and once with the
caller's gate); for every interior pixel r = Iw - Is and g at the target are computed as that function's gate computes them, n_low_grad
counts g < 5, the double sums are math.fsum over the f32 terms r * r and |r|. n_targets is the number of distinct targets among the
candidates. trial is the vectorised form, trial_scalar walks pixel by pixel with numpy f32 scalars; tests/test_trial_propagation_reference.py
holds them to each other and to a hand-written answer, the GPU tests hold the kernels to trial.

restart is the wiped state (valid = blacklisted = validity = 0, invDepth = variance = 0, both smoothed fields -1) + absorb_reference.absorb.
"""
import math

import numpy as np

import absorb_reference as A
from absorb_reference import F, FLT_MAX, PLANES, _candidates
from map_points_reference import classify

FIELDS = ("sum_r2", "sum_abs_r", "n_kept", "n_in_view", "n_interior", "n_low_grad", "n_candidates", "n_targets")
INT_FIELDS = FIELDS[2:]


def _residuals(depth, var, img, intr, T12, ident, d_img, d_maxgrad):
    """r and g of the interior pixels `ident` (raster indices of one request), in _candidates' order of operations."""
    depth = np.asarray(depth, F); var = np.asarray(var, F); img = np.asarray(img); d_img = np.asarray(d_img)
    rows, cols = depth.shape
    fx, fy, cx, cy = (F(v) for v in intr)
    T = np.asarray(T12, F).reshape(12)
    i = ident & 0xffffff
    ys, xs = i // cols, i % cols
    Z = depth[ys, xs]
    with np.errstate(all="ignore"):
        X = ((((xs.astype(F) - cx).astype(F) * Z).astype(F)) / fx).astype(F)
        Y = ((((ys.astype(F) - cy).astype(F) * Z).astype(F)) / fy).astype(F)
        P = []
        for r in range(3):
            t = T[4 * r:4 * r + 4]
            acc = ((t[0] * X).astype(F) + (t[1] * Y).astype(F)).astype(F)
            acc = (acc + (t[2] * Z).astype(F)).astype(F)
            P.append((acc + t[3]).astype(F))
        xp, yp, zp = P
        nid = (F(1.0) / zp).astype(F)
        u = (((xp * nid).astype(F) * fx).astype(F) + cx).astype(F)
        v = (((yp * nid).astype(F) * fy).astype(F) + cy).astype(F)
        ux = (u + F(0.5)).astype(F); vy = (v + F(0.5)).astype(F)
        target = vy.astype(np.int64) * cols + ux.astype(np.int64)
        x0 = u.astype(np.int64); y0 = v.astype(np.int64)
        I00 = d_img[y0, x0].astype(F); I01 = d_img[y0, x0 + 1].astype(F); I10 = d_img[y0 + 1, x0].astype(F); I11 = d_img[y0 + 1, x0 + 1].astype(F)
        ax = (u - x0.astype(F)).astype(F); ay = (v - y0.astype(F)).astype(F)
        dx0 = (I01 - I00).astype(F); dx1 = (I11 - I10).astype(F)
        top = (I00 + (ax * dx0).astype(F)).astype(F); bot = (I10 + (ax * dx1).astype(F)).astype(F)
        Iw = (top + (ay * (bot - top).astype(F)).astype(F)).astype(F)
        res = (Iw - img[ys, xs].astype(F)).astype(F)
    g = np.asarray(d_maxgrad, F).reshape(-1)[target]
    return res, g, target


def trial(src, intr, T12, flt, d_img, d_maxgrad, photo_gate=1):
    """src: (depth, var, img), the level-0 planes of the source slot; d_img, d_maxgrad: the destination's image and maxAbsGradient plane.
    Returns the record as a dict of FIELDS, plus sum_abs_terms = (fsum of |r * r|, fsum of |r|) for the bound on the double sums."""
    depth, var, img = src
    every = _candidates(depth, var, img, intr, T12, flt, 0, d_img, d_maxgrad, 0)
    gated = _candidates(depth, var, img, intr, T12, flt, 0, d_img, d_maxgrad, photo_gate)
    res, g, target = _residuals(depth, var, img, intr, T12, every["ident"], d_img, d_maxgrad)
    assert np.array_equal(target, every["target"])
    with np.errstate(all="ignore"):
        r2 = (res * res).astype(F)
        ar = np.abs(res).astype(F)
    rec = dict(sum_r2=math.fsum(float(t) for t in r2), sum_abs_r=math.fsum(float(t) for t in ar),
               n_kept=every["n_kept"], n_in_view=every["n_in_view"], n_interior=every["n_interior"], n_low_grad=int((g < F(5.0)).sum()),
               n_candidates=gated["n_candidates"], n_targets=int(np.unique(gated["target"]).size))
    assert rec["n_interior"] == res.size
    rec["sum_abs_terms"] = (rec["sum_r2"], rec["sum_abs_r"])   # every term is >= 0
    return rec


def trial_scalar(src, intr, T12, flt, d_img, d_maxgrad, photo_gate=1):
    """The same, pixel by pixel with numpy f32 scalars."""
    depth, var, img = (np.asarray(src[0], F), np.asarray(src[1], F), np.asarray(src[2]))
    rows, cols = depth.shape
    fx, fy, cx, cy = (F(v) for v in intr)
    T = np.asarray(T12, F).reshape(12)
    d_img = np.asarray(d_img); mg = np.asarray(d_maxgrad, F)
    rec = dict.fromkeys(INT_FIELDS, 0)
    r2_terms, ar_terms, targets = [], [], set()
    kept = classify(depth, var, flt)["kept"]
    with np.errstate(all="ignore"):
        for y in range(rows):
            for x in range(cols):
                if not kept[y, x]:
                    continue
                rec["n_kept"] += 1
                Z = depth[y, x]; V = var[y, x]
                X = F(F(F(F(x) - cx) * Z) / fx)
                Y = F(F(F(F(y) - cy) * Z) / fy)
                xp, yp, zp = (F(F(F(F(T[4 * r] * X) + F(T[4 * r + 1] * Y)) + F(T[4 * r + 2] * Z)) + T[4 * r + 3]) for r in range(3))
                if not (zp > 0 and zp <= FLT_MAX):
                    continue
                nid = F(F(1.0) / zp)
                u = F(F(F(xp * nid) * fx) + cx)
                v = F(F(F(yp * nid) * fy) + cy)
                ux = F(u + F(0.5)); vy = F(v + F(0.5))
                if not (ux >= 0 and ux < F(cols) and vy >= 0 and vy < F(rows)):
                    continue
                q = F(nid / F(F(1.0) / Z))
                q = F(q * q)
                q = F(q * q)
                nvar = F(q * V)
                if not (nvar >= 0 and nvar <= FLT_MAX):
                    continue
                rec["n_in_view"] += 1
                if not (u > F(2.1) and v > F(2.1) and u < F(F(cols) - F(3.1)) and v < F(F(rows) - F(3.1))):
                    continue
                rec["n_interior"] += 1
                tx, ty = int(ux), int(vy)
                x0, y0 = int(u), int(v)
                I00, I01, I10, I11 = F(d_img[y0, x0]), F(d_img[y0, x0 + 1]), F(d_img[y0 + 1, x0]), F(d_img[y0 + 1, x0 + 1])
                ax = F(u - F(x0)); ay = F(v - F(y0))
                dx0 = F(I01 - I00); dx1 = F(I11 - I10)
                top = F(I00 + F(ax * dx0)); bot = F(I10 + F(ax * dx1))
                Iw = F(top + F(ay * F(bot - top)))
                res = F(Iw - F(img[y, x]))
                g = mg[ty, tx]
                rec["n_low_grad"] += bool(g < F(5.0))
                r2_terms.append(float(F(res * res)))
                ar_terms.append(float(F(abs(res))))
                if photo_gate and (F(F(res * res) / F(F(1600.0) + F(F(F(0.25) * g) * g))) > F(1.0) or g < F(5.0)):
                    continue
                rec["n_candidates"] += 1
                targets.add(ty * cols + tx)
    rec["n_targets"] = len(targets)
    rec["sum_r2"] = math.fsum(r2_terms)
    rec["sum_abs_r"] = math.fsum(ar_terms)
    rec["sum_abs_terms"] = (rec["sum_r2"], rec["sum_abs_r"])
    return {k: (int(v) if k in INT_FIELDS else v) for k, v in rec.items()}


def sum_bound(rec, k):
    """How far a device sum of the n_interior f32 terms, added in any order in double, can lie from math.fsum of them: n * 2^-52 * sum |term|
    (tests/depth_consistency_reference.py's bound, by the same argument: n - 1 roundings, each within 2^-53 of a partial sum that is at
    most the sum of the |terms|, up to second order)."""
    return rec["n_interior"] * 2.0 ** -52 * rec["sum_abs_terms"][k]


def wiped_state(rows, cols):
    return dict(invDepth=np.zeros((rows, cols), F), invDepthSmoothed=np.full((rows, cols), -1.0, F), variance=np.zeros((rows, cols), F),
                varianceSmoothed=np.full((rows, cols), -1.0, F), validity=np.zeros((rows, cols), np.int32),
                blacklisted=np.zeros((rows, cols), np.int32), valid=np.zeros((rows, cols), np.uint8))


def restart(requests, intr, Ts, flt, k_img, k_maxgrad, **prm):
    """ellc_depth_restart_from_keyframes without `finalise`: the wiped state + absorb_reference.absorb. k_img, k_maxgrad: the new
    keyframe's image and maxAbsGradient plane. Returns what absorb returns."""
    rows, cols = np.asarray(requests[0][0]).shape
    return A.absorb(requests, intr, Ts, flt, k_img, k_maxgrad, wiped_state(rows, cols), **prm)


__all__ = ["FIELDS", "INT_FIELDS", "PLANES", "trial", "trial_scalar", "sum_bound", "wiped_state", "restart"]
