"""numpy restatement of ellc_keyframe_sim3_step's rule (include/ellc_abi.h), every per-pixel intermediate cast to np.float32.

A source pixel takes part iff map_points_reference.classify keeps it; which pixels have a candidate, and its target, nid and nvar,
are render_depth_reference._candidates'. The point (x', y', z') and the projection (u, v) are restated here in the candidate's order.
Photometric term: u >= 0, v >= 0, x0 = (int)u, y0 = (int)v, x0 + 1 < cols, y0 + 1 < rows; the four taps of the destination's stored
image; ax = u - x0, ay = v - y0, dx0 = I01 - I00, dx1 = I11 - I10, top = I00 + ax dx0, bot = I10 + ax dx1, gy = bot - top,
Iw = top + ay gy, gx = dx0 + ay (dx1 - dx0), rp = Iw - Is; A = (gx fx) nid, Bv = (gy fy) nid, Cq = -(((A x') + (Bv y')) nid);
Jp = [Cq y' - Bv z', A z' - Cq x', Bv x' - A y', A, Bv, Cq, 0]; w0 = 1 / sigma_i2, sp = sqrt(w0) (f32); e = |rp| sp; wp = w0 if
e <= huber_k else w0 (huber_k / e). Depth term: the destination's target holds a hypothesis, s = nvar + Vt with 0 < s <= FLT_MAX,
rd = nid - 1 / Zt, rd rd <= gate_k2 s; wd = depth_weight (1 / s), a2 = nid nid, Jd = [-(a2 y'), a2 x', 0, 0, 0, -a2, -nid].
Sums: wJ_i = w J_i in f32; H_ij gets (double)wJ_i (double)J_j, b_i gets (double)wJ_i (double)r, both exact in double; structurally
zero Jacobian entries give no term. The double sums here are math.fsum over those exactly known terms: the exactly rounded sum, what
any order of double additions is held against; abs_* are the sums of the terms' magnitudes and n_* the numbers of terms, what the
bound of such a sum is made of.

step walks the planes at once, step_scalar the pixels one by one; tests/test_sim3_reference.py holds them to each other and to a
hand-worked answer, the GPU tests hold the kernels to step. solve / apply / align restate the host side in numpy and scipy.
"""
import math

import numpy as np

from map_points_reference import classify, level_intrinsics, make_scene  # noqa: F401  (re-exported for the tests)
from render_depth_reference import _candidates, scene_transforms  # noqa: F401

F = np.float32
FLT_MAX = np.finfo(np.float32).max
INT_FIELDS = ("n_kept", "n_in_view", "n_photo", "n_photo_huber", "n_depth", "n_depth_gated")
DEFAULT_PARAMS = dict(sigma_i2=16.0, huber_k=1.345, gate_k2=9.0, depth_weight=1.0)
PHOTO_IDX = (0, 1, 2, 3, 4, 5)     # the entries of the seven parameters the photometric Jacobian has
DEPTH_IDX = (0, 1, 5, 6)           # ... and the depth Jacobian


def h_index(i, j):
    """H[i][j], i <= j, in the row-major upper triangle of the 7 x 7."""
    return i * 7 - (i * (i - 1)) // 2 + (j - i)


def _params(params):
    p = dict(DEFAULT_PARAMS)
    p.update(params or {})
    w0 = F(F(1.0) / F(p["sigma_i2"]))
    return w0, F(np.sqrt(w0)), F(p["huber_k"]), F(p["gate_k2"]), F(p["depth_weight"])


class _Sums:
    """The 37 sums as lists of exactly known double terms."""

    def __init__(self):
        self.H = [[] for _ in range(28)]
        self.b = [[] for _ in range(7)]
        self.chi = {"chi2_photo": [], "chi2_depth": []}

    def add(self, idx, J, w, r):
        """One term's contribution, vectorised over its pixels: J[k] belongs to parameter idx[k]; w, r, J[k] are f32 arrays."""
        with np.errstate(all="ignore"):
            wJ = [(w * Jk).astype(F) for Jk in J]
        for p, i in enumerate(idx):
            for q in range(p, len(idx)):
                self.H[h_index(i, idx[q])].append(wJ[p].astype(np.float64) * J[q].astype(np.float64))
            self.b[i].append(wJ[p].astype(np.float64) * r.astype(np.float64))

    def finish(self, out):
        def total(parts):
            t = np.concatenate([np.atleast_1d(np.asarray(p, np.float64)) for p in parts]) if parts else np.zeros(0)
            return math.fsum(t), math.fsum(np.abs(t)), int(t.size)
        H = [total(p) for p in self.H]
        b = [total(p) for p in self.b]
        out["H"] = [v[0] for v in H]; out["abs_H"] = [v[1] for v in H]; out["n_H"] = [v[2] for v in H]
        out["b"] = [v[0] for v in b]; out["abs_b"] = [v[1] for v in b]; out["n_b"] = [v[2] for v in b]
        for k, parts in self.chi.items():
            out[k], out["abs_" + k], out["n_" + k] = total(parts)
        return out


def step(src, dst, intr, T12, flt, params=None, detail=False):
    """src, dst: (depth, var, img) of the two slots on one level - depth / variance planes (rows, cols) and the STORED image plane;
    intr: the level's four f32 intrinsics; T12: 12 f32, source camera -> destination camera; flt: (max_var, min_support, support_k2,
    stride); params: dict over DEFAULT_PARAMS. Returns the record's fields as Python numbers (H: 28, b: 7), abs_* / n_* per sum, and
    behind_camera / outside / bad_var / no_taps / no_overlap: how many kept pixels went where. detail=True adds `photo` and `depth`:
    per-pixel dicts (i, x', y', z', target, J [k][pixel], r, w) of the two terms."""
    sd, sv, simg = src
    dd, dv, dimg = dst
    sd = np.asarray(sd, F); sv = np.asarray(sv, F); dd = np.asarray(dd, F); dv = np.asarray(dv, F)
    simg = np.asarray(simg); dimg = np.asarray(dimg)
    rows, cols = dd.shape
    fx, fy, cx, cy = (F(v) for v in intr)
    T = np.asarray(T12, F).reshape(12)
    w0, sp, huber_k, gate_k2, depth_weight = _params(params)
    c = _candidates(sd, sv, intr, T, flt, 0)
    n_in_view = int(c["i"].size)
    ys, xs = np.divmod(c["i"], cols)
    Z = sd[ys, xs]
    nid = c["nid"]
    sums = _Sums()
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
        assert np.array_equal(zp.view(np.uint32), c["z"].view(np.uint32))   # the candidate's own z'
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
        rp = (Iw - Is).astype(F)
        pn = nid[ph]; px = xp[ph]; py = yp[ph]; pz = zp[ph]
        A = ((gx * fx).astype(F) * pn).astype(F)
        Bv = ((gy * fy).astype(F) * pn).astype(F)
        Cq = (-((((A * px).astype(F) + (Bv * py).astype(F)).astype(F) * pn).astype(F))).astype(F)
        Jp = [((Cq * py).astype(F) - (Bv * pz).astype(F)).astype(F), ((A * pz).astype(F) - (Cq * px).astype(F)).astype(F),
              ((Bv * px).astype(F) - (A * py).astype(F)).astype(F), A, Bv, Cq]
        e = (np.abs(rp) * sp).astype(F)
        inside = e <= huber_k
        wp = np.where(inside, w0, (w0 * (huber_k / e).astype(F)).astype(F)).astype(F)
        sums.add(PHOTO_IDX, Jp, wp, rp)
        sums.chi["chi2_photo"].append(((rp * rp).astype(F) * wp).astype(F).astype(np.float64))
        # ---- the depth term
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
        sums.add(DEPTH_IDX, Jd, wd, rdd)
        sums.chi["chi2_depth"].append(((rdd * rdd).astype(F) * wd).astype(F).astype(np.float64))
    out = dict(n_kept=n_in_view + c["behind"] + c["outside"] + c["bad_var"], n_in_view=n_in_view, n_photo=int(ph.sum()),
               n_photo_huber=int((~inside).sum()), n_depth=int(dp.sum()), n_depth_gated=int((usable & ~gate).sum()),
               behind_camera=c["behind"], outside=c["outside"], bad_var=c["bad_var"], no_taps=n_in_view - int(ph.sum()),
               no_overlap=n_in_view - int(ov.sum()))
    if detail:
        out["photo"] = dict(i=c["i"][ph], xp=px, yp=py, zp=pz, x0=x0, y0=y0, J=Jp, r=rp, w=wp)
        out["depth"] = dict(i=c["i"][dp], xp=xp[dp], yp=yp[dp], zp=zp[dp], target=c["target"][dp], J=Jd, r=rdd, w=wd)
    return sums.finish(out)


def step_scalar(src, dst, intr, T12, flt, params=None):
    """The same, pixel by pixel with numpy f32 scalars (the record's fields only)."""
    sd, sv, simg = src
    dd, dv, dimg = dst
    sd = np.asarray(sd, F); sv = np.asarray(sv, F); dd = np.asarray(dd, F); dv = np.asarray(dv, F)
    simg = np.asarray(simg); dimg = np.asarray(dimg)
    rows, cols = sd.shape
    fx, fy, cx, cy = (F(v) for v in intr)
    T = np.asarray(T12, F).reshape(12)
    w0, sp, huber_k, gate_k2, depth_weight = _params(params)
    kept = classify(sd, sv, flt)["kept"]
    out = {k: 0 for k in INT_FIELDS}
    H = [[] for _ in range(28)]
    b = [[] for _ in range(7)]
    chi = {"chi2_photo": [], "chi2_depth": []}

    def add(idx, J, w, r):
        wJ = [F(w * Jk) for Jk in J]
        for p, i in enumerate(idx):
            for q in range(p, len(idx)):
                H[h_index(i, idx[q])].append(float(wJ[p]) * float(J[q]))
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
                        rp = F(Iw - Is)
                        A = F(F(gx * fx) * nid); Bv = F(F(gy * fy) * nid)
                        Cq = F(-F(F(F(A * xp) + F(Bv * yp)) * nid))
                        J = [F(F(Cq * yp) - F(Bv * zp)), F(F(A * zp) - F(Cq * xp)), F(F(Bv * xp) - F(A * yp)), A, Bv, Cq]
                        e = F(abs(rp) * sp)
                        if e <= huber_k:
                            wp = w0
                        else:
                            wp = F(w0 * F(huber_k / e))
                            out["n_photo_huber"] += 1
                        add(PHOTO_IDX, J, wp, rp)
                        chi["chi2_photo"].append(float(F(F(rp * rp) * wp)))
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
                add(DEPTH_IDX, [F(-F(a2 * yp)), F(a2 * xp), F(-a2), F(-nid)], wd, rd)
                chi["chi2_depth"].append(float(F(F(rd * rd) * wd)))
    out["H"] = [math.fsum(t) for t in H]
    out["b"] = [math.fsum(t) for t in b]
    for k in chi:
        out[k] = math.fsum(chi[k])
    return out


def fields_equal(a, b):
    """The record's fields with == (the double sums of both forms are exactly rounded: equal when the terms are)."""
    return all(a[k] == b[k] for k in INT_FIELDS + ("chi2_photo", "chi2_depth")) and list(a["H"]) == list(b["H"]) and list(a["b"]) == list(b["b"])


def sums_of(ref):
    """(name, exactly rounded sum, bound) of the record's 37 double sums in the record's order. The bound generalises
    depth_consistency_reference.sum_bound: a double sum of n exactly known terms, added in any order (a fused multiply-add of an exact
    product rounds once, like the addition), has n - 1 roundings of at most 2^-53 of a partial sum that cannot exceed sum |term|
    (1 + small); n 2^-52 sum |term| leaves a factor two."""
    out = []
    for k in range(28):
        out.append(("H[%d]" % k, ref["H"][k], ref["n_H"][k] * 2.0 ** -52 * ref["abs_H"][k]))
    for k in range(7):
        out.append(("b[%d]" % k, ref["b"][k], ref["n_b"][k] * 2.0 ** -52 * ref["abs_b"][k]))
    for k in ("chi2_photo", "chi2_depth"):
        out.append((k, ref[k], ref["n_" + k] * 2.0 ** -52 * ref["abs_" + k]))
    return out


def mirrored(H28):
    """The 7 x 7 symmetric matrix of the record's upper triangle."""
    M = np.zeros((7, 7))
    iu = np.triu_indices(7)
    M[iu] = np.asarray(H28, np.float64)
    return M + np.triu(M, 1).T


def generator(xi7):
    w = np.asarray(xi7, np.float64)
    return np.array([[w[6], -w[2], w[1], w[3]], [w[2], w[6], -w[0], w[4]], [-w[1], w[0], w[6], w[5]], [0, 0, 0, 0]], np.float64)


def apply(xi7, T12):
    """float(expm(xi^) T), the exponential by scipy in double."""
    from scipy.linalg import expm
    T = np.vstack([np.asarray(T12, F).reshape(3, 4).astype(np.float64), [0, 0, 0, 1]])
    return (expm(generator(xi7)) @ T)[:3].astype(F).reshape(12)


def solve(H28, b7):
    """(xi, singular): numpy's solve of H xi = -b on the mirrored matrix; singular by the library's rule on the pivots of L D L^T
    without pivoting (a pivot that fails d_i > 1e-10 max_j H_jj)."""
    A = mirrored(H28)
    thr = 1e-10 * A.diagonal().max()
    L = np.eye(7); d = np.zeros(7)
    for j in range(7):
        d[j] = A[j, j] - (L[j, :j] ** 2 * d[:j]).sum()
        if not d[j] > thr:
            return np.zeros(7), True
        for i in range(j + 1, 7):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * d[:j]).sum()) / d[j]
    return np.linalg.solve(A, -np.asarray(b7, np.float64)), False


def align(planes_of, src, dst, intr_of, T12, levels, flt, params=None, max_iter=10, eps=1e-4):
    """The loop of ellc_keyframe_sim3_align for ONE pair on this reference: planes_of(slot, level) -> (depth, var, img),
    intr_of(level) -> intrinsics, levels: the visited levels in order. Returns (T, iters per level, the T of every evaluation)."""
    T = np.asarray(T12, F).reshape(12).copy()
    iters, visited = [], []
    for level in levels:
        made = 0
        while True:
            visited.append(T.copy())
            r = step(planes_of(src, level), planes_of(dst, level), intr_of(level), T, flt, params)
            xi, singular = solve(r["H"], r["b"])
            if singular:
                break
            T = apply(xi, T)
            made += 1
            if np.abs(xi).max() <= eps or made >= max_iter:
                break
        iters.append(made)
    visited.append(T.copy())
    return T, iters, visited


def sim3_errors(T12, T_true):
    """(scale, rotation, translation) errors of a 3x4 similarity against the true one: |s / s_true - 1|, the Frobenius distance of the
    two rotations, and the distance of the translations relative to max(|t_true|, 1e-12)."""
    A = np.asarray(T12, np.float64).reshape(3, 4); Bt = np.asarray(T_true, np.float64).reshape(3, 4)
    sa = np.cbrt(np.linalg.det(A[:, :3])); sb = np.cbrt(np.linalg.det(Bt[:, :3]))
    return (abs(sa / sb - 1.0), float(np.linalg.norm(A[:, :3] / sa - Bt[:, :3] / sb)),
            float(np.linalg.norm(A[:, 3] - Bt[:, 3]) / max(np.linalg.norm(Bt[:, 3]), 1e-12)))
