"""numpy restatement of the photometric rule with an affine light (include/ellc_abi.h, v19): ellc_keyframe_light_step's record and
ellc_keyframe_sim3_step_lit's, every per-pixel intermediate cast to np.float32.

Which pixels take part is sim3_reference's rule word for word (classify, _candidates, the four-tap test), and so are Iw, its
gradients, the Jacobians and the depth term; they are restated here, not imported, because sim3_reference.step does not hand out Iw
and Is. What is new: Ip = gain * Is + offset (the product rounded, then the sum), rp = Iw - Ip, the Huber weight wp from that rp, and
the six sums of the weighted fit of Iw on Is: wIs = wp * Is and wIw = wp * Iw in f32, then sum_w += wp, sum_w_s += wIs,
sum_w_t += wIw, sum_w_ss += (double)wIs * (double)Is, sum_w_st += (double)wIs * (double)Iw, sum_w_tt += (double)wIw * (double)Iw;
every term is known exactly. As in sim3_reference the double sums are math.fsum over those terms, abs_* the sums of the terms'
magnitudes and n_* the numbers of terms.

step walks the planes at once, step_scalar the pixels one by one; tests/test_light_reference.py holds them to each other, to
sim3_reference.step at the light (1, 0) and to a hand-worked answer. solve restates ellc_light_solve, align the alternating loop.
"""
import math

import numpy as np

import sim3_reference as S
from map_points_reference import classify, level_intrinsics  # noqa: F401  (re-exported for the tests)
from render_depth_reference import _candidates

F = np.float32
FLT_MAX = S.FLT_MAX
LIGHT_SUMS = ("sum_w", "sum_w_s", "sum_w_t", "sum_w_ss", "sum_w_st", "sum_w_tt", "chi2_photo")
LIGHT_INT_FIELDS = ("n_kept", "n_in_view", "n_photo", "n_photo_huber")
DEFAULT_LIGHT_PARAMS = dict(gain_min=0.25, gain_max=4.0, min_pixels=16)
UNIT = (1.0, 0.0)


def _total(t):
    t = np.atleast_1d(np.asarray(t, np.float64))
    return math.fsum(t), math.fsum(np.abs(t)), int(t.size)


def step(src, dst, intr, T12, flt, params=None, light=UNIT, detail=False):
    """Arguments as sim3_reference.step, and light = (gain, offset). Returns sim3_reference.step's fields for the record of
    ellc_keyframe_sim3_step_lit (H, b, chi2_*, the six counts, abs_* / n_*, the class counts) and the sums of
    ellc_keyframe_light_step (LIGHT_SUMS with abs_* / n_*). detail=True adds `photo`: per-pixel Is, Iw, r, w of the photometric term."""
    sd, sv, simg = src
    dd, dv, dimg = dst
    sd = np.asarray(sd, F); sv = np.asarray(sv, F); dd = np.asarray(dd, F); dv = np.asarray(dv, F)
    simg = np.asarray(simg); dimg = np.asarray(dimg)
    rows, cols = dd.shape
    fx, fy, cx, cy = (F(v) for v in intr)
    T = np.asarray(T12, F).reshape(12)
    gain, offset = F(light[0]), F(light[1])
    w0, sp, huber_k, gate_k2, depth_weight = S._params(params)
    c = _candidates(sd, sv, intr, T, flt, 0)
    n_in_view = int(c["i"].size)
    ys, xs = np.divmod(c["i"], cols)
    Z = sd[ys, xs]
    nid = c["nid"]
    sums = S._Sums()
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
        u = (((xp * nid).astype(F) * fx).astype(F) + cx).astype(F)
        v = (((yp * nid).astype(F) * fy).astype(F) + cy).astype(F)
        # ---- the photometric term
        ok = (u >= 0) & (v >= 0)
        x0 = np.where(ok, u, 0).astype(np.int64); y0 = np.where(ok, v, 0).astype(np.int64)
        ph = ok & (x0 + 1 < cols) & (y0 + 1 < rows)
        x0 = x0[ph]; y0 = y0[ph]
        I00 = dimg[y0, x0].astype(F); I01 = dimg[y0, x0 + 1].astype(F); I10 = dimg[y0 + 1, x0].astype(F); I11 = dimg[y0 + 1, x0 + 1].astype(F)
        Is = simg[ys[ph], xs[ph]].astype(F)
        ax = (u[ph] - x0.astype(F)).astype(F); ay = (v[ph] - y0.astype(F)).astype(F)
        dx0 = (I01 - I00).astype(F); dx1 = (I11 - I10).astype(F)
        top = (I00 + (ax * dx0).astype(F)).astype(F); bot = (I10 + (ax * dx1).astype(F)).astype(F)
        gy = (bot - top).astype(F)
        Iw = (top + (ay * gy).astype(F)).astype(F)
        gx = (dx0 + (ay * (dx1 - dx0).astype(F)).astype(F)).astype(F)
        Ip = ((gain * Is).astype(F) + offset).astype(F)
        rp = (Iw - Ip).astype(F)
        pn = nid[ph]; px = xp[ph]; py = yp[ph]; pz = zp[ph]
        A = ((gx * fx).astype(F) * pn).astype(F)
        Bv = ((gy * fy).astype(F) * pn).astype(F)
        Cq = (-((((A * px).astype(F) + (Bv * py).astype(F)).astype(F) * pn).astype(F))).astype(F)
        Jp = [((Cq * py).astype(F) - (Bv * pz).astype(F)).astype(F), ((A * pz).astype(F) - (Cq * px).astype(F)).astype(F),
              ((Bv * px).astype(F) - (A * py).astype(F)).astype(F), A, Bv, Cq]
        e = (np.abs(rp) * sp).astype(F)
        inside = e <= huber_k
        wp = np.where(inside, w0, (w0 * (huber_k / e).astype(F)).astype(F)).astype(F)
        sums.add(S.PHOTO_IDX, Jp, wp, rp)
        chi = ((rp * rp).astype(F) * wp).astype(F).astype(np.float64)
        sums.chi["chi2_photo"].append(chi)
        wIs = (wp * Is).astype(F); wIw = (wp * Iw).astype(F)
        d = np.float64
        light_terms = dict(sum_w=wp.astype(d), sum_w_s=wIs.astype(d), sum_w_t=wIw.astype(d), sum_w_ss=wIs.astype(d) * Is.astype(d),
                           sum_w_st=wIs.astype(d) * Iw.astype(d), sum_w_tt=wIw.astype(d) * Iw.astype(d))
        # ---- the depth term (sim3_reference's, unchanged by the light)
        ty, tx = np.divmod(c["target"], cols)
        Zt = dd[ty, tx]; Vt = dv[ty, tx]
        ov = (Zt > 0) & (Zt <= FLT_MAX) & (Vt >= 0)
        s = (c["nvar"] + Vt).astype(F)
        usable = ov & (s > 0) & (s <= FLT_MAX)
        rd = (nid - (F(1.0) / Zt).astype(F)).astype(F)
        gate = (rd * rd).astype(F) <= (gate_k2 * s).astype(F)
        dp = usable & gate
        wd = (depth_weight * (F(1.0) / s[dp]).astype(F)).astype(F)
        a2 = (nid[dp] * nid[dp]).astype(F)
        Jd = [(-((a2 * yp[dp]).astype(F))).astype(F), (a2 * xp[dp]).astype(F), (-a2).astype(F), (-nid[dp]).astype(F)]
        rdd = rd[dp]
        sums.add(S.DEPTH_IDX, Jd, wd, rdd)
        sums.chi["chi2_depth"].append(((rdd * rdd).astype(F) * wd).astype(F).astype(np.float64))
    out = dict(n_kept=n_in_view + c["behind"] + c["outside"] + c["bad_var"], n_in_view=n_in_view, n_photo=int(ph.sum()),
               n_photo_huber=int((~inside).sum()), n_depth=int(dp.sum()), n_depth_gated=int((usable & ~gate).sum()),
               behind_camera=c["behind"], outside=c["outside"], bad_var=c["bad_var"], no_taps=n_in_view - int(ph.sum()),
               no_overlap=n_in_view - int(ov.sum()))
    for k, t in light_terms.items():
        out[k], out["abs_" + k], out["n_" + k] = _total(t)
    if detail:
        out["photo"] = dict(i=c["i"][ph], Is=Is, Iw=Iw, r=rp, w=wp, inside=inside)
    return sums.finish(out)


def step_scalar(src, dst, intr, T12, flt, params=None, light=UNIT):
    """The same, pixel by pixel with numpy f32 scalars (the two records' fields only)."""
    sd, sv, simg = src
    dd, dv, dimg = dst
    sd = np.asarray(sd, F); sv = np.asarray(sv, F); dd = np.asarray(dd, F); dv = np.asarray(dv, F)
    simg = np.asarray(simg); dimg = np.asarray(dimg)
    rows, cols = sd.shape
    fx, fy, cx, cy = (F(v) for v in intr)
    T = np.asarray(T12, F).reshape(12)
    gain, offset = F(light[0]), F(light[1])
    w0, sp, huber_k, gate_k2, depth_weight = S._params(params)
    kept = classify(sd, sv, flt)["kept"]
    out = {k: 0 for k in S.INT_FIELDS}
    H = [[] for _ in range(28)]
    b = [[] for _ in range(7)]
    terms = {k: [] for k in LIGHT_SUMS + ("chi2_depth",)}

    def add(idx, J, w, r):
        wJ = [F(w * Jk) for Jk in J]
        for p, i in enumerate(idx):
            for q in range(p, len(idx)):
                H[S.h_index(i, idx[q])].append(float(wJ[p]) * float(J[q]))
            b[i].append(float(wJ[p]) * float(r))

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
                r4 = F(nid / F(F(1.0) / Z))
                r4 = F(r4 * r4)
                r4 = F(r4 * r4)
                nvar = F(r4 * V)
                if not (nvar >= 0 and nvar <= FLT_MAX):
                    continue
                out["n_in_view"] += 1
                if u >= 0 and v >= 0:
                    x0, y0 = int(u), int(v)
                    if x0 + 1 < cols and y0 + 1 < rows:
                        out["n_photo"] += 1
                        I00, I01, I10, I11 = F(dimg[y0, x0]), F(dimg[y0, x0 + 1]), F(dimg[y0 + 1, x0]), F(dimg[y0 + 1, x0 + 1])
                        Is = F(simg[y, x])
                        ax = F(u - F(x0)); ay = F(v - F(y0))
                        dx0 = F(I01 - I00); dx1 = F(I11 - I10)
                        top = F(I00 + F(ax * dx0)); bot = F(I10 + F(ax * dx1))
                        gy = F(bot - top)
                        Iw = F(top + F(ay * gy))
                        gx = F(dx0 + F(ay * F(dx1 - dx0)))
                        rp = F(Iw - F(F(gain * Is) + offset))
                        A = F(F(gx * fx) * nid); Bv = F(F(gy * fy) * nid)
                        Cq = F(-F(F(F(A * xp) + F(Bv * yp)) * nid))
                        J = [F(F(Cq * yp) - F(Bv * zp)), F(F(A * zp) - F(Cq * xp)), F(F(Bv * xp) - F(A * yp)), A, Bv, Cq]
                        e = F(abs(rp) * sp)
                        if e <= huber_k:
                            wp = w0
                        else:
                            wp = F(w0 * F(huber_k / e))
                            out["n_photo_huber"] += 1
                        add(S.PHOTO_IDX, J, wp, rp)
                        terms["chi2_photo"].append(float(F(F(rp * rp) * wp)))
                        wIs, wIw = F(wp * Is), F(wp * Iw)
                        terms["sum_w"].append(float(wp)); terms["sum_w_s"].append(float(wIs)); terms["sum_w_t"].append(float(wIw))
                        terms["sum_w_ss"].append(float(wIs) * float(Is)); terms["sum_w_st"].append(float(wIs) * float(Iw))
                        terms["sum_w_tt"].append(float(wIw) * float(Iw))
                tx, ty = int(ux), int(vy)
                Zt, Vt = dd[ty, tx], dv[ty, tx]
                if not (Zt > 0 and Zt <= FLT_MAX and Vt >= 0):
                    continue
                s = F(nvar + Vt)
                if not (s > 0 and s <= FLT_MAX):
                    continue
                rd = F(nid - F(F(1.0) / Zt))
                if not F(rd * rd) <= F(gate_k2 * s):
                    out["n_depth_gated"] += 1
                    continue
                out["n_depth"] += 1
                wd = F(depth_weight * F(F(1.0) / s))
                a2 = F(nid * nid)
                add(S.DEPTH_IDX, [F(-F(a2 * yp)), F(a2 * xp), F(-a2), F(-nid)], wd, rd)
                terms["chi2_depth"].append(float(F(F(rd * rd) * wd)))
    out["H"] = [math.fsum(t) for t in H]
    out["b"] = [math.fsum(t) for t in b]
    for k in terms:
        out[k] = math.fsum(terms[k])
    return out


def fields_equal(a, b):
    """Both records' fields with == (the double sums of both forms are exactly rounded: equal when the terms are)."""
    return S.fields_equal(a, b) and all(a[k] == b[k] for k in LIGHT_SUMS)


def light_sums_of(ref):
    """(name, exactly rounded sum, bound) of the light record's seven double sums in the record's order; the bound is
    sim3_reference.sums_of's, n 2^-52 sum |term|, for the reason given there."""
    return [(k, ref[k], ref["n_" + k] * 2.0 ** -52 * ref["abs_" + k]) for k in LIGHT_SUMS]


def solve(rec, light_in=UNIT, params=None):
    """ellc_light_solve in Python doubles: ((gain, offset) as f32, refused)."""
    p = dict(DEFAULT_LIGHT_PARAMS)
    p.update(params or {})
    sw, ss, st, sss, sst = (float(rec[k]) for k in ("sum_w", "sum_w_s", "sum_w_t", "sum_w_ss", "sum_w_st"))
    with np.errstate(all="ignore"):
        det = np.float64(sw) * sss - np.float64(ss) * ss
        gain = (np.float64(sw) * sst - np.float64(ss) * st) / det
        offset = (st - gain * ss) / np.float64(sw)
    ok = int(rec["n_photo"]) >= p["min_pixels"] and det > 1e-10 * sw * sss and float(F(p["gain_min"])) <= gain <= float(F(p["gain_max"])) and abs(offset) <= 255
    if not ok:
        return (F(light_in[0]), F(light_in[1])), True
    return (F(gain), F(offset)), False


def align(planes_of, src, dst, intr_of, T12, levels, flt, params=None, light_params=None, light=UNIT, max_iter=10, eps=1e-4):
    """The loop of ellc_keyframe_sim3_align_lit for ONE pair on this reference (numpy solve, scipy expm): per evaluation the light
    record at (T, l), l' = solve of it, the Sim(3) record at (T, l'). Returns (T, light, iters per level, share of the photometric
    pixels beyond the Huber threshold at the last evaluation made)."""
    T = np.asarray(T12, F).reshape(12).copy()
    l = (F(light[0]), F(light[1]))
    iters, share = [], 0.0
    for level in levels:
        made = 0
        while True:
            a, b, intr = planes_of(src, level), planes_of(dst, level), intr_of(level)
            l, _ = solve(step(a, b, intr, T, flt, params, l), l, light_params)
            r = step(a, b, intr, T, flt, params, l)
            share = r["n_photo_huber"] / max(r["n_photo"], 1)
            xi, singular = S.solve(r["H"], r["b"])
            if singular:
                break
            T = S.apply(xi, T)
            made += 1
            if np.abs(xi).max() <= eps or made >= max_iter:
                break
        iters.append(made)
    return T, l, iters, share
