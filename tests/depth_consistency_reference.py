"""numpy restatement of ellc_keyframe_depth_consistency's rule (include/ellc_abi.h), every intermediate cast to np.float32.

A source pixel takes part iff map_points_reference.classify keeps it; its candidate (target, nid, nvar) is render_depth_reference's.
At the target of the destination: Zt, Vt, It; it overlaps iff Zt > 0 && Zt <= FLT_MAX && Vt >= 0. idt = 1 / Zt, d = nid - idt,
s = nvar + Vt; it agrees iff d * d <= agree_k2 * s, is in front iff it does not agree and d > 0, behind otherwise; |Is - It| and its
square are summed as integers; it is weighted iff s > 0 && s <= FLT_MAX: w = 1 / s, q = (d * d) * w, ss = (nid * nid) * w,
st = (nid * idt) * w, and the three double sums are math.fsum over the per-pixel f32 terms (the exactly rounded sum: what any
order of double additions is held against).

consistency walks the planes at once, consistency_scalar the pixels one by one; tests/test_depth_consistency_reference.py holds them
to each other and to a hand-written answer, the GPU tests hold the kernels to consistency.
"""
import math

import numpy as np

from map_points_reference import classify, level_intrinsics, make_scene  # noqa: F401  (re-exported for the tests)
from render_depth_reference import _candidates, scene_transforms  # noqa: F401

F = np.float32
FLT_MAX = np.finfo(np.float32).max
INT_FIELDS = ("n_kept", "n_in_view", "n_overlap", "n_agree", "n_in_front", "n_behind", "n_weighted", "sum_abs_di", "sum_di2")
SUM_FIELDS = ("sum_chi2", "sum_w_ss", "sum_w_st")


def consistency(src, dst, intr, T12, flt, agree_k2=1.0):
    """src, dst: (depth, var, img) of the two slots on one level — depth / variance planes (rows, cols) and the STORED image plane;
    intr: the level's four f32 intrinsics; T12: 12 f32, source camera -> destination camera; flt: (max_var, min_support, support_k2,
    stride). Returns the record's fields as Python numbers, abs_<sum>: the sums of the terms' magnitudes (what the tolerance of a
    double sum is made of), and behind_camera / outside / bad_var / no_overlap: how many kept pixels were dropped where."""
    sd, sv, simg = src
    dd, dv, dimg = dst
    dd = np.asarray(dd, F); dv = np.asarray(dv, F)
    rows, cols = dd.shape
    c = _candidates(sd, sv, intr, T12, flt, 0)
    n_in_view = int(c["i"].size)
    n_kept = n_in_view + c["behind"] + c["outside"] + c["bad_var"]
    ty, tx = np.divmod(c["target"], cols)
    Zt = dd[ty, tx]; Vt = dv[ty, tx]
    with np.errstate(all="ignore"):
        ov = (Zt > 0) & (Zt <= FLT_MAX) & (Vt >= 0)
        nid = c["nid"][ov]; nvar = c["nvar"][ov]; Zt = Zt[ov]; Vt = Vt[ov]
        idt = (F(1.0) / Zt).astype(F)
        d = (nid - idt).astype(F)
        s = (nvar + Vt).astype(F)
        d2 = (d * d).astype(F)
        agree = d2 <= (F(agree_k2) * s).astype(F)
        front = ~agree & (d > 0)
        weighted = (s > 0) & (s <= FLT_MAX)
        w = (F(1.0) / s[weighted]).astype(F)
        q = (d2[weighted] * w).astype(F)
        ss = ((nid[weighted] * nid[weighted]).astype(F) * w).astype(F)
        st = ((nid[weighted] * idt[weighted]).astype(F) * w).astype(F)
    si = c["i"][ov]
    Is = np.asarray(simg)[si // cols, si % cols].astype(np.int64)
    It = np.asarray(dimg)[ty[ov], tx[ov]].astype(np.int64)
    di = np.abs(Is - It)
    out = dict(n_kept=n_kept, n_in_view=n_in_view, n_overlap=int(ov.sum()), n_agree=int(agree.sum()), n_in_front=int(front.sum()),
               n_behind=int((~agree & ~front).sum()), n_weighted=int(weighted.sum()), sum_abs_di=int(di.sum()), sum_di2=int((di * di).sum()),
               behind_camera=c["behind"], outside=c["outside"], bad_var=c["bad_var"], no_overlap=n_in_view - int(ov.sum()))
    for name, terms in (("sum_chi2", q), ("sum_w_ss", ss), ("sum_w_st", st)):
        t64 = terms.astype(np.float64)
        out[name] = math.fsum(t64)
        out["abs_" + name] = math.fsum(np.abs(t64))
    return out


def consistency_scalar(src, dst, intr, T12, flt, agree_k2=1.0):
    """The same, pixel by pixel with numpy f32 scalars (the record's twelve fields only)."""
    sd, sv, simg = src
    dd, dv, dimg = dst
    sd = np.asarray(sd, F); sv = np.asarray(sv, F); dd = np.asarray(dd, F); dv = np.asarray(dv, F)
    rows, cols = sd.shape
    fx, fy, cx, cy = (F(v) for v in intr)
    T = np.asarray(T12, F).reshape(12)
    k2 = F(agree_k2)
    kept = classify(sd, sv, flt)["kept"]
    out = {k: 0 for k in INT_FIELDS}
    terms = {k: [] for k in SUM_FIELDS}
    with np.errstate(all="ignore"):
        for y in range(rows):
            for x in range(cols):
                if not kept[y, x]:
                    continue
                out["n_kept"] += 1
                Z, V = sd[y, x], sv[y, x]
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
                r = F(nid / F(F(1.0) / Z))
                r = F(r * r)
                r = F(r * r)
                nvar = F(r * V)
                if not (nvar >= 0 and nvar <= FLT_MAX):
                    continue
                out["n_in_view"] += 1
                tx, ty = int(ux), int(vy)
                Zt, Vt = dd[ty, tx], dv[ty, tx]
                if not (Zt > 0 and Zt <= FLT_MAX and Vt >= 0):
                    continue
                out["n_overlap"] += 1
                idt = F(F(1.0) / Zt)
                d = F(nid - idt)
                s = F(nvar + Vt)
                d2 = F(d * d)
                if d2 <= F(k2 * s):
                    out["n_agree"] += 1
                elif d > 0:
                    out["n_in_front"] += 1
                else:
                    out["n_behind"] += 1
                di = abs(int(np.asarray(simg)[y, x]) - int(np.asarray(dimg)[ty, tx]))
                out["sum_abs_di"] += di
                out["sum_di2"] += di * di
                if s > 0 and s <= FLT_MAX:
                    w = F(F(1.0) / s)
                    out["n_weighted"] += 1
                    terms["sum_chi2"].append(float(F(d2 * w)))
                    terms["sum_w_ss"].append(float(F(F(nid * nid) * w)))
                    terms["sum_w_st"].append(float(F(F(nid * idt) * w)))
    for k in SUM_FIELDS:
        out[k] = math.fsum(terms[k])
    return out


def fields_equal(a, b):
    """The record's twelve fields with == (the double sums of both forms are exactly rounded: equal when the terms are)."""
    return all(a[k] == b[k] for k in INT_FIELDS + SUM_FIELDS)


def sum_bound(ref, name):
    """How far a double sum of the record's n_weighted exactly known terms, added in any order, may lie from the exactly rounded sum:
    every one of the n - 1 additions rounds by at most 2^-53 of a partial sum that cannot exceed sum |term| (1 + small), so the total
    stays within (n - 1) 2^-53 sum |term| to first order; n 2^-52 sum |term| leaves a factor two."""
    return ref["n_weighted"] * 2.0 ** -52 * ref["abs_" + name]
