"""numpy restatement of ellc_keyframe_sweep_depth's rule (include/ellc_abi.h), every per-pixel intermediate cast to np.float32.

A pixel of K is OK iff Z0 > 0 and Z0 <= FLT_MAX and V0 >= 0; it is swept iff it is not OK, lies one pixel inside the level and the squared
central difference of K's grey values reaches min_grad2. Sample k is the inverse depth d_k = d_min + k dstep, dstep = (d_max - d_min) /
(n_samples - 1) rounded once. Its cost takes the views in ascending b: the five pattern pixels (0,0), (1,0), (-1,0), (0,1), (0,-1) each
get ellc_keyframe_render_depth's candidate for (px + dx, py + dy, 1 / d_k, V = 0) and rule 3 of ellc_keyframe_sim3_step (four taps, Iw,
rp = Iw - (gain Is_j + offset), e, wp), c_j = (rp rp) wp; a view counts iff all five have both, E += ((((c_0 + c_1) + c_2) + c_3) + c_4),
n += 1; cost = E / n, valid iff n >= min_views and cost <= FLT_MAX. The decision, the outputs and the stats are the header's rules 4
and 5. sum_cost is math.fsum over the exactly known terms; abs_sum_cost and n_sum_cost are what the bound of such a sum is made of.

sweep walks the swept pixels at once, one sample after the other, and decides with whole arrays of costs (the candidate and tap lines
are refine_depth_reference.evaluate's, imported); sweep_scalar walks pixel by pixel with numpy f32 scalars, restates those lines itself
and decides with `decide` on a pixel's list of costs. tests/test_sweep_depth_reference.py holds the two to each other and to a
hand-worked answer, the GPU tests hold the kernel to sweep.
"""
import math

import numpy as np

import refine_depth_reference as R
from map_points_reference import level_intrinsics, make_scene  # noqa: F401  (re-exported for the tests)

F = np.float32
FLT_MAX = np.finfo(np.float32).max
NOT_SWEPT, CREATED, NO_VALID_SAMPLE, AT_RANGE_END, COST_TOO_HIGH, NOT_DISTINCT, FLAT = range(7)
STATUS_NAMES = ("n_not_swept", "n_created", "n_no_valid_sample", "n_at_range_end", "n_cost_too_high", "n_not_distinct", "n_flat")
INT_FIELDS = ("n_ok", "n_swept") + STATUS_NAMES[1:] + ("sum_views",)
DEFAULT_PARAMS = dict(sigma_i2=16.0, huber_k=1.345, d_min=0.125, d_max=4.0, min_grad2=100.0, max_cost=0.0, distinct_ratio=0.7, var_scale=1.0,
                      n_samples=64, min_views=2)
PLANES = ("depth", "var", "views", "status")
PATTERN = ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))


class Params:
    def __init__(self, params):
        p = dict(DEFAULT_PARAMS)
        p.update(params or {})
        self.w0 = F(F(1.0) / F(p["sigma_i2"]))
        self.sp = F(np.sqrt(self.w0))
        self.huber_k = F(p["huber_k"])
        self.d_min, self.d_max = F(p["d_min"]), F(p["d_max"])
        self.n_samples, self.min_views = int(p["n_samples"]), int(p["min_views"])
        self.dstep = F(F(self.d_max - self.d_min) / F(self.n_samples - 1))
        self.min_grad2, self.max_cost = F(p["min_grad2"]), F(p["max_cost"])
        self.distinct_ratio, self.var_scale = F(p["distinct_ratio"]), F(p["var_scale"])

    def d(self, k):
        return F(self.d_min + F(F(k) * self.dstep))


def classify(Z0, V0, img, min_grad2):
    """Rule 1: (ok, swept) planes."""
    rows, cols = Z0.shape
    with np.errstate(all="ignore"):
        ok = (Z0 > 0) & (Z0 <= FLT_MAX) & (V0 >= 0)
    I = np.asarray(img)[:rows, :cols].astype(F)
    swept = np.zeros((rows, cols), bool)
    if rows >= 3 and cols >= 3:
        gxc = (I[1:-1, 2:] - I[1:-1, :-2]).astype(F)
        gyc = (I[2:, 1:-1] - I[:-2, 1:-1]).astype(F)
        g2 = ((gxc * gxc).astype(F) + (gyc * gyc).astype(F)).astype(F)
        swept[1:-1, 1:-1] = g2 >= F(min_grad2)
    return ok, swept & ~ok


def _finish(out, Z0, V0, ok, swept, ys, xs, st, n1, d, v, c1):
    """The planes and the stats from the decisions of the processed swept pixels (ys, xs)."""
    rows, cols = Z0.shape
    depth = Z0.copy(); var = V0.copy()
    status = np.zeros((rows, cols), np.uint8); nviews = np.zeros((rows, cols), np.uint8)
    status[ys, xs] = st
    nviews[ys, xs] = n1
    made = st == CREATED
    with np.errstate(all="ignore"):
        depth[ys[made], xs[made]] = (F(1.0) / d[made]).astype(F)
    var[ys[made], xs[made]] = v[made]
    out.update(depth=depth, var=var, views=nviews, status=status, n_ok=int(ok.sum()), n_swept=int(swept.sum()), processed=(ys, xs))
    for k, name in enumerate(STATUS_NAMES):
        out[name] = int((status == k).sum())
    out["sum_views"] = int(n1[made].astype(np.int64).sum())
    t = c1[made].astype(np.float64)
    out["sum_cost"], out["abs_sum_cost"], out["n_sum_cost"] = math.fsum(t), math.fsum(np.abs(t)), int(t.size)
    out["d"] = np.zeros((rows, cols), F)
    out["d"][ys[made], xs[made]] = d[made]
    return out


def sample_costs(xs, ys, img, views, intr, Ts, lights, P, shape):
    """Rule 3 for the pixels (xs, ys), sample after sample: (cost [n_samples, N] f32, n [n_samples, N])."""
    N, B = xs.size, len(views)
    cost = np.zeros((P.n_samples, N), F); ns = np.zeros((P.n_samples, N), np.int64)
    zero = np.zeros(N, F)
    Isj = [np.asarray(img)[ys + dy, xs + dx].astype(F) for dx, dy in PATTERN]
    with np.errstate(all="ignore"):
        for k in range(P.n_samples):
            d = np.full(N, P.d(k), F)
            det = []
            for j, (dx, dy) in enumerate(PATTERN):
                one = []
                R.evaluate(xs + dx, ys + dy, d, zero, Isj[j], views, intr, Ts, lights, P.w0, P.sp, P.huber_k, shape, detail=one)
                det.append(one)
            E = np.zeros(N, F); n = np.zeros(N, np.int64)
            for b in range(B):
                allfive = np.ones(N, bool)
                c = []
                for j in range(5):
                    q = det[j][b]
                    allfive &= q["ok"]
                    c.append(((q["rp"] * q["rp"]).astype(F) * q["wp"]).astype(F))
                s = ((((c[0] + c[1]).astype(F) + c[2]).astype(F) + c[3]).astype(F) + c[4]).astype(F)
                E = np.where(allfive, (E + s).astype(F), E)
                n = n + allfive
            cost[k] = (E / n.astype(F)).astype(F)
            ns[k] = n
    return cost, ns


def sweep(kf, views, intr, Ts, lights=None, params=None):
    """kf: (depth, var, img) of K on the level - depth / variance planes (rows, cols) and the STORED image plane; views: the views' STORED
    image planes; intr: the level's four f32 intrinsics; Ts: [B][12] f32, K's camera -> the view's; lights: [B][2] or None; params: dict
    over DEFAULT_PARAMS. Returns the four planes, the stats' fields as Python numbers, abs_sum_cost / n_sum_cost, `d` (the created
    inverse depths, 0 elsewhere), `costs` / `ns` ([n_samples, N]) and `processed` = (ys, xs) of the swept pixels."""
    Z0, V0, img = kf
    Z0 = np.asarray(Z0, F); V0 = np.asarray(V0, F)
    rows, cols = Z0.shape
    B = len(views)
    Ts = np.asarray(Ts, F).reshape(B, 12)
    lights = R._lights(lights, B)
    P = Params(params)
    ok, swept = classify(Z0, V0, img, P.min_grad2)
    ys, xs = np.nonzero(swept)
    N = xs.size
    cost, ns = sample_costs(xs, ys, img, views, intr, Ts, lights, P, (rows, cols))
    K = P.n_samples
    ar = np.arange(N)
    with np.errstate(all="ignore"):
        valid = (ns >= P.min_views) & (cost <= FLT_MAX)
        masked = np.where(valid, cost, np.inf)
        k1 = np.argmin(masked, axis=0)             # the first of the smallest: the lowest k
        some = valid.any(axis=0)
        c1 = cost[k1, ar]; n1 = np.where(some, ns[k1, ar], 0)
        st = np.zeros(N, np.int64)
        st[~some] = NO_VALID_SAMPLE
        run = some.copy()
        km, kp = np.clip(k1 - 1, 0, K - 1), np.clip(k1 + 1, 0, K - 1)
        end = run & ((k1 == 0) | (k1 == K - 1) | ~valid[km, ar] | ~valid[kp, ar])
        st[end] = AT_RANGE_END
        run &= ~end
        cm, cp = cost[km, ar], cost[kp, ar]
        high = run & bool(P.max_cost > 0) & ~(c1 <= P.max_cost)
        st[high] = COST_TOO_HIGH
        run &= ~high
        far = valid & (np.abs(np.arange(K)[:, None] - k1[None, :]) >= 2)
        c2 = np.where(far, cost, np.inf).min(axis=0).astype(F)
        nd = run & far.any(axis=0) & ~(c1 <= (P.distinct_ratio * c2).astype(F))
        st[nd] = NOT_DISTINCT
        run &= ~nd
        curv = ((cm - (F(2.0) * c1).astype(F)).astype(F) + cp).astype(F)
        off = ((F(0.5) * (cm - cp).astype(F)).astype(F) / curv).astype(F)
        dk1 = (P.d_min + (k1.astype(F) * P.dstep).astype(F)).astype(F)
        d = (dk1 + (off * P.dstep).astype(F)).astype(F)
        v = (P.var_scale * ((F(2.0) * F(P.dstep * P.dstep)) / (n1.astype(F) * curv).astype(F)).astype(F)).astype(F)
        good = (curv > 0) & (curv <= FLT_MAX) & (d > 0) & (d <= FLT_MAX) & (v >= 0) & (v <= FLT_MAX)
        st[run & ~good] = FLAT
        st[run & good] = CREATED
    return _finish(dict(costs=cost, ns=ns), Z0, V0, ok, swept, ys, xs, st, n1, d, v, c1)


def decide(costs, ns, P):
    """Rule 4 for one pixel's samples (lists of f32 costs and of n): (status, n1, d, v, c1); d, v and c1 are None where not reached."""
    K = P.n_samples
    valid = [bool(ns[k] >= P.min_views and costs[k] <= FLT_MAX) for k in range(K)]
    k1 = None
    for k in range(K):
        if valid[k] and (k1 is None or costs[k] < costs[k1]):
            k1 = k
    if k1 is None:
        return NO_VALID_SAMPLE, 0, None, None, None
    c1, n1 = costs[k1], ns[k1]
    if k1 == 0 or k1 == K - 1 or not valid[k1 - 1] or not valid[k1 + 1]:
        return AT_RANGE_END, n1, None, None, c1
    cm, cp = costs[k1 - 1], costs[k1 + 1]
    if P.max_cost > 0 and not c1 <= P.max_cost:
        return COST_TOO_HIGH, n1, None, None, c1
    far = [costs[k] for k in range(K) if valid[k] and abs(k - k1) >= 2]
    if far and not c1 <= F(P.distinct_ratio * min(far)):
        return NOT_DISTINCT, n1, None, None, c1
    curv = F(F(cm - F(F(2.0) * c1)) + cp)
    if not (curv > 0 and curv <= FLT_MAX):
        return FLAT, n1, None, None, c1
    off = F(F(F(0.5) * F(cm - cp)) / curv)
    d = F(P.d(k1) + F(off * P.dstep))
    v = F(P.var_scale * F(F(F(2.0) * F(P.dstep * P.dstep)) / F(F(n1) * curv)))
    if not (d > 0 and d <= FLT_MAX and v >= 0 and v <= FLT_MAX):
        return FLAT, n1, None, None, c1
    return CREATED, n1, d, v, c1


def sweep_scalar(kf, views, intr, Ts, lights=None, params=None, every=1):
    """The same, pixel by pixel with numpy f32 scalars. every > 1: only every `every`-th swept pixel in raster order is processed (the
    others stay NOT_SWEPT in the planes and out of the status counts; n_ok and n_swept are those of the level)."""
    Z0, V0, img = kf
    Z0 = np.asarray(Z0, F); V0 = np.asarray(V0, F); img = np.asarray(img)
    rows, cols = Z0.shape
    B = len(views)
    Ts = np.asarray(Ts, F).reshape(B, 12)
    lights = R._lights(lights, B)
    fx, fy, cx, cy = (F(v) for v in intr)
    P = Params(params)

    def term(b, x, y, Z):
        """c_j of pattern pixel (x, y) at the depth Z in view b, or None."""
        T = Ts[b]
        X = F(F(F(F(x) - cx) * Z) / fx)
        Y = F(F(F(F(y) - cy) * Z) / fy)
        xp, yp, zp = (F(F(F(F(T[4 * r] * X) + F(T[4 * r + 1] * Y)) + F(T[4 * r + 2] * Z)) + T[4 * r + 3]) for r in range(3))
        if not (zp > 0 and zp <= FLT_MAX):
            return None
        nid = F(F(1.0) / zp)
        u = F(F(F(xp * nid) * fx) + cx)
        v = F(F(F(yp * nid) * fy) + cy)
        ux = F(u + F(0.5)); vy = F(v + F(0.5))
        if not (ux >= 0 and ux < F(cols) and vy >= 0 and vy < F(rows)):
            return None
        r4 = F(nid / F(F(1.0) / Z))
        r4 = F(r4 * r4)
        r4 = F(r4 * r4)
        nvar = F(r4 * F(0.0))
        if not (nvar >= 0 and nvar <= FLT_MAX):
            return None
        if not (u >= 0 and v >= 0):
            return None
        x0, y0 = int(u), int(v)
        if not (x0 + 1 < cols and y0 + 1 < rows):
            return None
        im = views[b]
        I00, I01, I10, I11 = F(im[y0, x0]), F(im[y0, x0 + 1]), F(im[y0 + 1, x0]), F(im[y0 + 1, x0 + 1])
        ax = F(u - F(x0)); ay = F(v - F(y0))
        dx0 = F(I01 - I00); dx1 = F(I11 - I10)
        top = F(I00 + F(ax * dx0)); bot = F(I10 + F(ax * dx1))
        Iw = F(top + F(ay * F(bot - top)))
        rp = F(Iw - F(F(lights[b][0] * F(img[y, x])) + lights[b][1]))
        e = F(abs(rp) * P.sp)
        wp = P.w0 if e <= P.huber_k else F(P.w0 * F(P.huber_k / e))
        return F(F(rp * rp) * wp)

    ok, swept = classify(Z0, V0, img, P.min_grad2)
    ys, xs = np.nonzero(swept)
    ys, xs = ys[::every], xs[::every]
    N = xs.size
    st = np.zeros(N, np.int64); n1 = np.zeros(N, np.int64)
    d = np.zeros(N, F); v = np.zeros(N, F); c1 = np.zeros(N, F)
    with np.errstate(all="ignore"):
        for i in range(N):
            x, y = int(xs[i]), int(ys[i])
            costs, ns = [], []
            for k in range(P.n_samples):
                Z = F(F(1.0) / P.d(k))
                E = F(0); n = 0
                for b in range(B):
                    c = []
                    for dx, dy in PATTERN:
                        t = term(b, x + dx, y + dy, Z)
                        if t is None:
                            break
                        c.append(t)
                    if len(c) == 5:
                        E = F(E + F(F(F(F(c[0] + c[1]) + c[2]) + c[3]) + c[4]))
                        n += 1
                costs.append(F(E / F(n)))
                ns.append(n)
            s, nn, dd, vv, cc = decide(costs, ns, P)
            st[i], n1[i] = s, nn
            if s == CREATED:
                d[i], v[i] = dd, vv
            if cc is not None:
                c1[i] = cc
    return _finish(dict(), Z0, V0, ok, swept, ys, xs, st, n1, d, v, c1)


def results_equal(a, b, at=None):
    """The four planes (floats by their bit patterns) and every count and the sum with ==. at = (ys, xs): the planes at those pixels
    only, and no counts (a scalar run over a subset of the swept pixels)."""
    for name in PLANES:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        if at is not None:
            x, y = x[at], y[at]
        if not np.array_equal(x, y):
            return False
    if at is not None:
        return a["n_ok"] == b["n_ok"] and a["n_swept"] == b["n_swept"]
    return all(a[k] == b[k] for k in INT_FIELDS + ("n_not_swept", "sum_cost"))


def sum_bound(ref):
    """n 2^-52 sum |term|: what a double sum of n exactly known terms, added in any order, may differ by from the exactly rounded sum."""
    return ref["n_sum_cost"] * 2.0 ** -52 * ref["abs_sum_cost"]


# ---- the recovery scene of the tests (tests/test_sweep_depth_reference.py on the CPU, tests/test_gpu_sweep_depth.py on the device)
RECOVERY_SHAPES = [(64, 48), (131, 67), (23, 17)]


def thinned_world(w, h, n_kf=5, seed=11):
    """refine_depth_reference.shared_world(w, h, n_kf, seed, depth_noise=0.02) with K's depth0 kept at the pixels with (x + 2 y) % 3 == 0 only
    (0 elsewhere): (scenes, Ts of the n_kf - 1 views, K's true inverse depths, the sweep parameters of the recovery: the range
    [0.5 min, 1.5 max] of the true inverse depths, 32 samples, ratio 0.7, min_views 2)."""
    scenes, Ts, d_true = R.shared_world(w, h, n_kf, seed, depth_noise=0.02)
    yy, xx = np.mgrid[0:h, 0:w]
    keep = (xx + 2 * yy) % 3 == 0
    scenes[0] = dict(scenes[0])
    scenes[0]["depth0"] = np.where(keep, scenes[0]["depth0"], 0).astype(F)
    params = dict(d_min=float(F(0.5 * float(d_true.min()))), d_max=float(F(1.5 * float(d_true.max()))), n_samples=32, distinct_ratio=0.7, min_views=2)
    return scenes, Ts, d_true, params


def recovery_figures(res, d_true):
    """(swept, created, created / swept, median relative error of the created inverse depths, fraction of them within 5 % of the truth)."""
    made = res["status"] == CREATED
    with np.errstate(all="ignore"):
        d = 1.0 / res["depth"].astype(np.float64)[made]
    t = np.asarray(d_true, np.float64)[made]
    rel = np.abs(d - t) / t
    n_swept, n_made = res["n_swept"], int(made.sum())
    return n_swept, n_made, n_made / max(n_swept, 1), float(np.median(rel)) if n_made else float("nan"), float((rel <= 0.05).mean()) if n_made else 0.0
