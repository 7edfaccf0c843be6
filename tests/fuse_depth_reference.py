"""numpy restatement of ellc_keyframe_fuse_depth's rule (include/ellc_abi.h, v16), every intermediate cast to np.float32.

Candidates, winner, source, agree, intensity and n_valid are render_depth_reference.render's. The MEMBERS of a target are its candidates
other than the winner with (nid - nid_w)^2 <= agree_k2 * (nvar + nvar_w), against the winner's own values, in ascending id
(b << 24) | i; the first max_merge of them are visited. State id_t = nid_w, var_t = nvar_w, m = 1; per visited member s = var_t + nvar,
skipped unless s > 0 && s <= FLT_MAX, else w = nvar / s, id_t = (w * id_t) + ((1 - w) * nid), var_t = 1 / ((1 / var_t) + (1 / nvar)),
m += 1. Where m >= 2: depth = 1 / id_t, var = var_t; merged = m (0 without a winner); n_fused counts merged >= 2. A target has a winner iff
the render's depth is > 0 (its source is negative from request 128 on, and -1 is not the only negative value).

fuse walks arrays sorted by (target, id), one rank of every target's members per step; fuse_scalar walks the targets one by one with
numpy f32 scalars. tests/test_fuse_depth_reference.py holds them to each other and to a hand-written answer, the GPU tests hold the
kernels to fuse.
"""
import numpy as np

import render_depth_reference as R
from render_depth_reference import level_intrinsics, make_scene, scene_transforms  # noqa: F401  (re-exported for the tests)

F = np.float32
FLT_MAX = R.FLT_MAX
PLANES = ("depth", "var", "source", "agree", "merged", "intensity")


def _members(requests, intr, Ts, flt, agree_k2, base):
    """Every candidate that agrees with its target's winner and is not the winner: target, id, nid, nvar, sorted by (target, id)."""
    rows, cols = np.asarray(requests[0][0]).shape
    Ts = np.asarray(Ts, F).reshape(len(requests), 12)
    per = [R._candidates(d, v, intr, Ts[b], flt, b) for b, (d, v, _) in enumerate(requests)]
    target = np.concatenate([c["target"] for c in per]).astype(np.int64)
    ident = np.concatenate([(np.int64(b) << 24) | c["i"] for b, c in enumerate(per)]).astype(np.int64)
    nid = np.concatenate([c["nid"] for c in per]).astype(F)
    nvar = np.concatenate([c["nvar"] for c in per]).astype(F)
    src = base["source"].reshape(-1).astype(np.int64)
    with np.errstate(all="ignore"):
        nid_w = (F(1.0) / base["depth"].reshape(-1)).astype(F)   # 1 / z' of the winner: the division its candidate made
        nvar_w = base["var"].reshape(-1)
        d = (nid - nid_w[target]).astype(F)
        ok = (d * d).astype(F) <= (F(agree_k2) * (nvar + nvar_w[target]).astype(F)).astype(F)
    keep = ok & (ident != (src[target] & 0xffffffff))
    order = np.lexsort((ident[keep], target[keep]))
    return target[keep][order], ident[keep][order], nid[keep][order], nvar[keep][order]


def _finish(base, id_t, var_t, m, visited, skipped, max_merge):
    out = {k: base[k].copy() for k in R.PLANES}
    shape = base["depth"].shape
    with np.errstate(all="ignore"):
        fused = m >= 2
        out["depth"].reshape(-1)[fused] = (F(1.0) / id_t[fused]).astype(F)
        out["var"].reshape(-1)[fused] = var_t[fused]
    out["merged"] = m.astype(np.int32).reshape(shape)
    out["n_valid"] = int((base["depth"] > 0).sum())   # (a winner's z' is > 0; its source has bit 31 set from request 128 on: no sign to go by)
    out["n_fused"] = int(fused.sum())
    members = np.maximum(base["agree"].reshape(-1).astype(np.int64) - 1, 0)
    out["stats"] = dict(segment=base["agree"].copy(), visited=visited.reshape(shape), skipped=skipped.reshape(shape),
                        truncated=(members > max_merge).reshape(shape), render=base)
    return out


def fuse(requests, intr, Ts, flt, agree_k2=1.0, max_merge=64):
    """requests, intr, Ts, flt as render_depth_reference.render. Returns the six planes, n_valid, n_fused and stats: per target the
    segment size (agree), the members visited and skipped, whether members were left unvisited (truncated), and the render itself."""
    base = R.render(requests, intr, Ts, flt, agree_k2)
    n = base["depth"].size
    target, _, nid, nvar = _members(requests, intr, Ts, flt, agree_k2, base)
    won = base["depth"].reshape(-1) > 0
    with np.errstate(all="ignore"):
        id_t = np.where(won, (F(1.0) / base["depth"].reshape(-1)).astype(F), F(0)).astype(F)
    var_t = base["var"].reshape(-1).copy()
    m = won.astype(np.int64)
    visited = np.zeros(n, np.int64); skipped = np.zeros(n, np.int64)
    first = np.ones(target.size, bool); first[1:] = target[1:] != target[:-1]
    start = np.flatnonzero(first)
    rank = np.arange(target.size) - np.repeat(start, np.diff(np.append(start, target.size)))
    for r in range(max_merge):
        sel = rank == r
        if not sel.any():
            break
        t = target[sel]
        with np.errstate(all="ignore"):
            s = (var_t[t] + nvar[sel]).astype(F)
            use = (s > 0) & (s <= FLT_MAX)
            w = (nvar[sel] / s).astype(F)
            new_id = ((w * id_t[t]).astype(F) + ((F(1.0) - w).astype(F) * nid[sel]).astype(F)).astype(F)
            new_var = (F(1.0) / ((F(1.0) / var_t[t]).astype(F) + (F(1.0) / nvar[sel]).astype(F)).astype(F)).astype(F)
        visited[t] += 1
        skipped[t[~use]] += 1
        id_t[t[use]] = new_id[use]
        var_t[t[use]] = new_var[use]
        m[t[use]] += 1
    return _finish(base, id_t, var_t, m, visited, skipped, max_merge)


def fuse_scalar(requests, intr, Ts, flt, agree_k2=1.0, max_merge=64):
    """The same, target by target with numpy f32 scalars."""
    base = R.render(requests, intr, Ts, flt, agree_k2)
    n = base["depth"].size
    target, ident, nid, nvar = _members(requests, intr, Ts, flt, agree_k2, base)
    segs = {}
    for k in range(target.size):
        segs.setdefault(int(target[k]), []).append((int(ident[k]), F(nid[k]), F(nvar[k])))
    id_t = np.zeros(n, F); var_t = base["var"].reshape(-1).copy()
    m = np.zeros(n, np.int64); visited = np.zeros(n, np.int64); skipped = np.zeros(n, np.int64)
    depth = base["depth"].reshape(-1)
    with np.errstate(all="ignore"):
        for t in range(n):
            if not depth[t] > 0:
                continue
            i_t = F(F(1.0) / depth[t]); v_t = F(var_t[t]); count = 1
            for _, i_m, v_m in sorted(segs.get(t, []))[:max_merge]:
                visited[t] += 1
                s = F(v_t + v_m)
                if not (s > 0 and s <= FLT_MAX):
                    skipped[t] += 1
                    continue
                w = F(v_m / s)
                i_t = F(F(w * i_t) + F(F(F(1.0) - w) * i_m))
                v_t = F(F(1.0) / F(F(F(1.0) / v_t) + F(F(1.0) / v_m)))
                count += 1
            id_t[t] = i_t; var_t[t] = v_t; m[t] = count
    return _finish(base, id_t, var_t, m, visited, skipped, max_merge)


def planes_equal(a, b):
    """Plane by plane with ==; the floats by their bit patterns; n_valid and n_fused."""
    for name in PLANES:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        if not np.array_equal(x, y):
            return False
    return a["n_valid"] == b["n_valid"] and a["n_fused"] == b["n_fused"]


def differing(a, b):
    return [n for n in PLANES if np.ascontiguousarray(a[n]).tobytes() != np.ascontiguousarray(b[n]).tobytes()]
