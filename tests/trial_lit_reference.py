"""numpy restatement of ellc_keyframe_trial_propagate_lit's records and of ellc_trial_light_solve (include/ellc_abi.h, v24).

A record is ellc_keyframe_trial_propagate's with step 4's residual taken against Ip = gain * Is + offset (absorb_lit_reference.gate:
r = Iw - Ip), and five sums over the interior pixels - Is, Iw, Is * Is, Is * Iw, Iw * Iw, each term exact in double - that depend on
neither the light nor the gate. The interior pixels, their Iw, Is and g come from absorb_lit_reference.interior (which imports them);
only what the light changes is written here. Every sum is math.fsum of its exact terms; sum_abs_terms holds the sums of their magnitudes
in FIELDS' order of the seven doubles, for trial_propagation_reference.sum_bound (n_fit == n_interior).
trial_lit is the vectorised form, trial_lit_scalar takes step 4 pixel by pixel with numpy f32 scalars and adds the terms one by one.
"""
import math

import numpy as np

from absorb_lit_reference import F, gate, gate_scalar, interior
from trial_propagation_reference import INT_FIELDS, sum_bound  # noqa: F401  (sum_bound re-exported for the tests)

SUMS = ("sum_r2", "sum_abs_r", "sum_s", "sum_t", "sum_ss", "sum_st", "sum_tt")
FIELDS = SUMS[:2] + INT_FIELDS + SUMS[2:] + ("n_fit",)


def trial_lit(src, intr, T12, light, flt, d_img, d_maxgrad, photo_gate=1, gate_fn=gate):
    """src: (depth, var, img) of the source slot at level 0; light: (gain, offset) or None; d_img, d_maxgrad: the destination's image and
    maxAbsGradient plane. Returns the record as a dict of FIELDS plus sum_abs_terms."""
    depth, var, img = src
    gain, offset = (1.0, 0.0) if light is None else light
    every, Iw, Is, g = interior(depth, var, img, intr, T12, flt, 0, d_img, d_maxgrad)
    res, ok = gate_fn(Iw, Is, g, gain, offset)
    keep = ok if photo_gate else np.ones(res.size, bool)
    with np.errstate(all="ignore"):
        r2 = (res * res).astype(F)
        ar = np.abs(res).astype(F)
    s = Is.astype(np.float64); t = Iw.astype(np.float64)   # (the products of two f32 values are exact in double)
    terms = dict(sum_r2=r2.astype(np.float64), sum_abs_r=ar.astype(np.float64), sum_s=s, sum_t=t, sum_ss=s * s, sum_st=s * t, sum_tt=t * t)
    rec = {k: math.fsum(terms[k].tolist()) for k in SUMS}
    rec.update(n_kept=every["n_kept"], n_in_view=every["n_in_view"], n_interior=every["n_interior"], n_low_grad=int((g < F(5.0)).sum()),
               n_candidates=int(keep.sum()), n_targets=int(np.unique(every["target"][keep]).size), n_fit=int(res.size))
    assert rec["n_interior"] == res.size
    rec["sum_abs_terms"] = tuple(math.fsum(np.abs(terms[k]).tolist()) for k in SUMS)
    return rec


def trial_lit_scalar(src, intr, T12, light, flt, d_img, d_maxgrad, photo_gate=1):
    """The same with step 4 and the terms taken pixel by pixel."""
    depth, var, img = src
    gain, offset = (1.0, 0.0) if light is None else light
    every, Iw, Is, g = interior(depth, var, img, intr, T12, flt, 0, d_img, d_maxgrad)
    res, ok = gate_scalar(Iw, Is, g, gain, offset)
    rec = dict.fromkeys(INT_FIELDS + ("n_fit",), 0)
    rec.update(n_kept=every["n_kept"], n_in_view=every["n_in_view"])
    terms = {k: [] for k in SUMS}
    targets = set()
    with np.errstate(all="ignore"):
        for k in range(len(res)):
            rec["n_interior"] += 1
            rec["n_fit"] += 1
            rec["n_low_grad"] += bool(F(g[k]) < F(5.0))
            r = F(res[k])
            s, t = float(Is[k]), float(Iw[k])
            for name, v in zip(SUMS, (float(F(r * r)), float(F(abs(r))), s, t, s * s, s * t, t * t)):
                terms[name].append(v)
            if photo_gate and not ok[k]:
                continue
            rec["n_candidates"] += 1
            targets.add(int(every["target"][k]))
    rec["n_targets"] = len(targets)
    for name in SUMS:
        rec[name] = math.fsum(terms[name])
    rec["sum_abs_terms"] = tuple(math.fsum(abs(v) for v in terms[name]) for name in SUMS)
    return rec


def light_solve(rec, light_in=None, gain_min=0.25, gain_max=4.0, min_pixels=16):
    """ellc_trial_light_solve: ellc_light_solve's rule with weight 1 over the record's interior pixels, in double: (light f32 [2], refused)."""
    keep = np.asarray((1.0, 0.0) if light_in is None else light_in, F)
    n, s, t, ss, st = float(rec["n_fit"]), rec["sum_s"], rec["sum_t"], rec["sum_ss"], rec["sum_st"]
    with np.errstate(all="ignore"):
        det = np.float64(n) * ss - np.float64(s) * s
        gain = (np.float64(n) * st - np.float64(s) * t) / det
        offset = (t - gain * s) / np.float64(n)
    ok = bool(rec["n_fit"] >= min_pixels and det > 1e-10 * n * ss and gain >= float(F(gain_min)) and gain <= float(F(gain_max)) and abs(offset) <= 255.0)
    return (np.asarray((gain, offset), np.float64).astype(F), False) if ok else (keep, True)
