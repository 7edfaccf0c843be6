"""numpy restatement of ellc_keyframe_cull_depth's rule (include/ellc_abi.h), every per-pixel intermediate cast to np.float32.

A pixel of K takes part iff map_points_reference.classify keeps it. Per view the candidate is ellc_keyframe_render_depth's for
(px, py, Z0, V0) at the view's T (restated here in the candidate's order, with its three drops): target, nid, u, v, nvar. A view that
has depth planes votes geometrically with steps 3-6 of ellc_keyframe_depth_consistency (Zt, Vt at the target; idt = 1 / Zt,
d = nid - idt, s = nvar + Vt; AGREE iff d d <= agree_k2 s, IN_FRONT iff not and d > 0, BEHIND otherwise); with photo_k > 0 a view whose
geometric vote was not BEHIND and that has four taps (rule 3 of ellc_keyframe_sim3_step) votes photometrically: rp = Iw - (gain Is +
offset), e = |rp| sp, bad iff not e <= photo_k. The decision, the outputs and the stats are the header's rules 3 to 5. Every count is
an integer: nothing depends on an order.

cull walks the pixels at once, cull_scalar one by one; tests/test_cull_depth_reference.py holds them to each other and to a hand-worked
answer, the GPU tests hold the kernel to cull. A view is (depth, var, stored image) with depth and var None where it has no depth
planes (a frame slot, or a keyframe slot that holds an image only).
"""
import numpy as np

from map_points_reference import classify, level_intrinsics  # noqa: F401  (re-exported for the tests)

F = np.float32
FLT_MAX = np.finfo(np.float32).max
NOT_TAKING_PART, KEPT, CULLED_FREE_SPACE, CULLED_UNSUPPORTED, CULLED_PHOTO, UNSEEN = range(6)
STATUS_FIELDS = ("n_not_taking_part", "n_retained", "n_culled_free_space", "n_culled_unsupported", "n_culled_photo", "n_unseen")
SUM_FIELDS = ("sum_agree", "sum_in_front", "sum_behind", "sum_photo", "sum_photo_bad")
INT_FIELDS = ("n_kept",) + STATUS_FIELDS[1:] + SUM_FIELDS
DEFAULT_PARAMS = dict(agree_k2=1.0, sigma_i2=16.0, photo_k=3.0, min_support=1, min_judged=2, min_in_front=1, min_photo=2)
PLANES = ("depth", "var", "votes", "photo", "status")
NO_FILTER = (0, 0, 1.0, 1)


def _params(params):
    p = dict(DEFAULT_PARAMS)
    p.update(params or {})
    sp = F(np.sqrt(F(F(1.0) / F(p["sigma_i2"]))))
    return F(p["agree_k2"]), sp, F(p["photo_k"]), int(p["min_support"]), int(p["min_judged"]), int(p["min_in_front"]), int(p["min_photo"])


def _lights(lights, B):
    return np.tile(np.array([1, 0], F), (B, 1)) if lights is None else np.asarray(lights, F).reshape(B, 2)


def _decide(a, f, h, nph, nbad, photo_k, min_support, min_judged, min_in_front, min_photo):
    """Rule 3 for integer arrays (or scalars): the status."""
    a, f, h, nph, nbad = (np.asarray(v, np.int64) for v in (a, f, h, nph, nbad))
    free = (f >= min_in_front) & (f > a)
    unsup = (a + f + h >= min_judged) & (a < min_support)
    bad = (nph >= min_photo) & (2 * nbad > nph) if photo_k > 0 else np.zeros(a.shape, bool)
    unseen = (a + f + h == 0) & (nph == 0)
    return np.where(free, CULLED_FREE_SPACE, np.where(unsup, CULLED_UNSUPPORTED, np.where(bad, CULLED_PHOTO, np.where(unseen, UNSEEN, KEPT))))


def _finish(Z0, V0, ys, xs, a, f, h, nph, nbad, st, n_kept):
    rows, cols = Z0.shape
    depth = Z0.copy(); var = V0.copy()
    status = np.zeros((rows, cols), np.uint8); votes = np.zeros((rows, cols), np.uint32); photo = np.zeros((rows, cols), np.uint8)
    status[ys, xs] = st
    votes[ys, xs] = (a | (f << 8) | (h << 16) | (nbad << 24)).astype(np.uint32)
    photo[ys, xs] = nph
    culled = (status >= CULLED_FREE_SPACE) & (status <= CULLED_PHOTO)
    depth[culled] = F(0.0); var[culled] = F(-1.0)
    out = dict(depth=depth, var=var, votes=votes, photo=photo, status=status, n_kept=n_kept)
    for k, name in enumerate(STATUS_FIELDS):
        out[name] = int((status == k).sum())
    for name, v in zip(SUM_FIELDS, (a, f, h, nph, nbad)):
        out[name] = int(np.asarray(v, np.int64).sum())
    return out


def cull(kf, views, intr, Ts, lights, flt, params=None, detail=None):
    """kf: (depth, var, img) of K on the level - depth / variance planes (rows, cols) and the STORED image plane; views: per view
    (depth, var, stored image), depth and var None where the view has no depth planes; intr: the level's four f32 intrinsics; Ts:
    [B][12] f32, K's camera -> the view's; lights: [B][2] or None; flt: (max_var, min_support, support_k2, stride); params: dict over
    DEFAULT_PARAMS. Returns the five planes and the stats' fields as Python numbers. detail: a list that receives, per view,
    dict(cand, cls (0 none, 1 agree, 2 in front, 3 behind), photo, bad) over the pixels taking part."""
    Z0, V0, img = kf
    Z0 = np.asarray(Z0, F); V0 = np.asarray(V0, F); img = np.asarray(img)
    rows, cols = Z0.shape
    B = len(views)
    Ts = np.asarray(Ts, F).reshape(B, 12)
    lights = _lights(lights, B)
    fx, fy, cx, cy = (F(v) for v in intr)
    agree_k2, sp, photo_k, min_support, min_judged, min_in_front, min_photo = _params(params)
    kept = classify(Z0, V0, flt)["kept"]
    ys, xs = np.nonzero(kept)
    Z = Z0[ys, xs]; V = V0[ys, xs]
    Is = img[ys, xs].astype(F)
    N = xs.size
    a = np.zeros(N, np.int64); f = np.zeros(N, np.int64); h = np.zeros(N, np.int64); nph = np.zeros(N, np.int64); nbad = np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        X = ((((xs.astype(F) - cx).astype(F) * Z).astype(F)) / fx).astype(F)
        Y = ((((ys.astype(F) - cy).astype(F) * Z).astype(F)) / fy).astype(F)
        for b, (vd, vv, vimg) in enumerate(views):
            vimg = np.asarray(vimg)
            T = Ts[b]
            gain, offset = F(lights[b][0]), F(lights[b][1])
            P = []
            for r in range(3):
                t = T[4 * r:4 * r + 4]
                acc = ((t[0] * X).astype(F) + (t[1] * Y).astype(F)).astype(F)
                acc = (acc + (t[2] * Z).astype(F)).astype(F)
                P.append((acc + t[3]).astype(F))
            xp, yp, zp = P
            ok = (zp > 0) & (zp <= FLT_MAX)
            nid = (F(1.0) / zp).astype(F)
            u = (((xp * nid).astype(F) * fx).astype(F) + cx).astype(F)
            v = (((yp * nid).astype(F) * fy).astype(F) + cy).astype(F)
            ux = (u + F(0.5)).astype(F); vy = (v + F(0.5)).astype(F)
            ok &= (ux >= 0) & (ux < F(cols)) & (vy >= 0) & (vy < F(rows))
            r4 = (nid / (F(1.0) / Z).astype(F)).astype(F)
            r4 = (r4 * r4).astype(F)
            r4 = (r4 * r4).astype(F)
            nvar = (r4 * V).astype(F)
            ok &= (nvar >= 0) & (nvar <= FLT_MAX)
            cls = np.zeros(N, np.int64)
            if vd is not None:
                tx = np.where(ok, ux, 0).astype(np.int64); ty = np.where(ok, vy, 0).astype(np.int64)
                Zt = np.asarray(vd, F)[ty, tx]; Vt = np.asarray(vv, F)[ty, tx]
                judged = ok & (Zt > 0) & (Zt <= FLT_MAX) & (Vt >= 0)
                idt = (F(1.0) / Zt).astype(F)
                d = (nid - idt).astype(F)
                s = (nvar + Vt).astype(F)
                agree = (d * d).astype(F) <= (agree_k2 * s).astype(F)
                cls = np.where(judged, np.where(agree, 1, np.where(d > 0, 2, 3)), 0)
            a += cls == 1; f += cls == 2; h += cls == 3
            ph = np.zeros(N, bool); bad = np.zeros(N, bool)
            if photo_k > 0:
                ph = ok & (cls != 3) & (u >= 0) & (v >= 0)
                x0 = np.where(ph, u, 0).astype(np.int64); y0 = np.where(ph, v, 0).astype(np.int64)
                ph &= (x0 + 1 < cols) & (y0 + 1 < rows)
                x0 = np.where(ph, x0, 0); y0 = np.where(ph, y0, 0)
                I00 = vimg[y0, x0].astype(F); I01 = vimg[y0, x0 + 1].astype(F); I10 = vimg[y0 + 1, x0].astype(F); I11 = vimg[y0 + 1, x0 + 1].astype(F)
                ax = (u - x0.astype(F)).astype(F); ay = (v - y0.astype(F)).astype(F)
                dx0 = (I01 - I00).astype(F); dx1 = (I11 - I10).astype(F)
                top = (I00 + (ax * dx0).astype(F)).astype(F); bot = (I10 + (ax * dx1).astype(F)).astype(F)
                gy = (bot - top).astype(F)
                Iw = (top + (ay * gy).astype(F)).astype(F)
                rp = (Iw - ((gain * Is).astype(F) + offset).astype(F)).astype(F)
                e = (np.abs(rp) * sp).astype(F)
                bad = ph & ~(e <= photo_k)
            nph += ph; nbad += bad
            if detail is not None:
                detail.append(dict(cand=ok, cls=cls, photo=ph, bad=bad))
    st = _decide(a, f, h, nph, nbad, photo_k, min_support, min_judged, min_in_front, min_photo)
    return _finish(Z0, V0, ys, xs, a, f, h, nph, nbad, st, int(kept.sum()))


def cull_scalar(kf, views, intr, Ts, lights, flt, params=None):
    """The same, pixel by pixel with numpy f32 scalars."""
    Z0, V0, img = kf
    Z0 = np.asarray(Z0, F); V0 = np.asarray(V0, F); img = np.asarray(img)
    rows, cols = Z0.shape
    B = len(views)
    Ts = np.asarray(Ts, F).reshape(B, 12)
    lights = _lights(lights, B)
    fx, fy, cx, cy = (F(v) for v in intr)
    agree_k2, sp, photo_k, min_support, min_judged, min_in_front, min_photo = _params(params)
    kept = classify(Z0, V0, flt)["kept"]
    ys, xs = np.nonzero(kept)
    counts = np.zeros((5, xs.size), np.int64)
    st = np.zeros(xs.size, np.int64)
    with np.errstate(all="ignore"):
        for k, (y, x) in enumerate(zip(ys.tolist(), xs.tolist())):
            Z, V = Z0[y, x], V0[y, x]
            Is = F(img[y, x])
            X = F(F(F(F(x) - cx) * Z) / fx)
            Y = F(F(F(F(y) - cy) * Z) / fy)
            a = f = h = nph = nbad = 0
            for b in range(B):
                T = Ts[b]
                vd, vv, vimg = views[b]
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
                behind = False
                if vd is not None:
                    Zt, Vt = F(vd[int(vy), int(ux)]), F(vv[int(vy), int(ux)])
                    if Zt > 0 and Zt <= FLT_MAX and Vt >= 0:
                        idt = F(F(1.0) / Zt)
                        d = F(nid - idt)
                        s = F(nvar + Vt)
                        if F(d * d) <= F(agree_k2 * s):
                            a += 1
                        elif d > 0:
                            f += 1
                        else:
                            h += 1
                            behind = True
                if not (photo_k > 0) or behind:
                    continue
                if not (u >= 0 and v >= 0):
                    continue
                x0, y0 = int(u), int(v)
                if not (x0 + 1 < cols and y0 + 1 < rows):
                    continue
                I00, I01, I10, I11 = F(vimg[y0, x0]), F(vimg[y0, x0 + 1]), F(vimg[y0 + 1, x0]), F(vimg[y0 + 1, x0 + 1])
                ax = F(u - F(x0)); ay = F(v - F(y0))
                dx0 = F(I01 - I00); dx1 = F(I11 - I10)
                top = F(I00 + F(ax * dx0)); bot = F(I10 + F(ax * dx1))
                Iw = F(top + F(ay * F(bot - top)))
                rp = F(Iw - F(F(lights[b][0] * Is) + lights[b][1]))
                e = F(abs(rp) * sp)
                nph += 1
                if not e <= photo_k:
                    nbad += 1
            counts[:, k] = (a, f, h, nph, nbad)
            if f >= min_in_front and f > a:
                st[k] = CULLED_FREE_SPACE
            elif a + f + h >= min_judged and a < min_support:
                st[k] = CULLED_UNSUPPORTED
            elif photo_k > 0 and nph >= min_photo and 2 * nbad > nph:
                st[k] = CULLED_PHOTO
            elif a + f + h == 0 and nph == 0:
                st[k] = UNSEEN
            else:
                st[k] = KEPT
    return _finish(Z0, V0, ys, xs, counts[0], counts[1], counts[2], counts[3], counts[4], st, int(kept.sum()))


def results_equal(a, b):
    """The five planes (floats by their bit patterns) and every count and sum with ==."""
    for name in PLANES:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return False
    return all(a[k] == b[k] for k in INT_FIELDS + ("n_not_taking_part",))


def case_params(B, **over):
    """The default parameters with the four counts lowered to B where B is below the default, then `over`."""
    p = {k: min(DEFAULT_PARAMS[k], B) for k in ("min_support", "min_judged", "min_in_front", "min_photo")}
    p.update(over)
    return p


# a non-default parameter set (B >= 3): a tighter agreement, a wider photometric bound, every count raised
OTHER_PARAMS = dict(agree_k2=0.25, sigma_i2=4.0, photo_k=5.0, min_support=2, min_judged=3, min_in_front=2, min_photo=3)


def spoil(depth, var):
    """The recovery input: every seventh OK pixel of K in raster order gets its INVERSE depth multiplied by 0.5 and 1.6 alternately
    (in double, one rounding to f32). Returns (the spoilt depth plane, the mask of the spoilt pixels, the mask of the other OK pixels)."""
    depth = np.asarray(depth, F)
    ok = (depth > 0) & (depth <= FLT_MAX) & (np.asarray(var, F) >= 0)
    idx = np.flatnonzero(ok.reshape(-1))[::7]
    out = depth.copy().reshape(-1)
    factors = np.where(np.arange(idx.size) % 2 == 0, 0.5, 1.6)
    out[idx] = (out[idx].astype(np.float64) / factors).astype(F)
    spoilt = np.zeros(depth.size, bool)
    spoilt[idx] = True
    spoilt = spoilt.reshape(depth.shape)
    return out.reshape(depth.shape), spoilt, ok & ~spoilt


def recovery_figures(res, spoilt, clean):
    """(spoilt pixels, of them culled, clean pixels, of them culled)."""
    culled = (res["status"] >= CULLED_FREE_SPACE) & (res["status"] <= CULLED_PHOTO)
    return int(spoilt.sum()), int((culled & spoilt).sum()), int(clean.sum()), int((culled & clean).sum())
