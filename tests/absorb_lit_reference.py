"""numpy restatement of step 4 of ellc_depth_absorb_keyframes_lit (include/ellc_abi.h, v24): the photometric gate with the source's grey
value sent through the request's light, every intermediate cast to np.float32.

    Ip = gain * Is + offset   (the product rounded, then the sum)      r = Iw - Ip
    dropped iff (r * r) / (1600 + (0.25 * g) * g) > 1 || g < 5         (g and the constants in the destination's units)

Everything else is imported: the candidates of steps 1-3 are absorb_reference._candidates with the gate off, Iw and g of an interior
pixel are trial_propagation_reference._residuals (against an all-zero source image its residual Iw - 0 is Iw itself), the fold is
absorb_reference.absorb, which is handed the survivors of the gate here in the place of its own. gate is the vectorised form of step 4,
gate_scalar walks the pixels one by one with numpy f32 scalars; tests/test_absorb_lit_reference.py holds them to each other, to
absorb_reference at (1, 0) and to a hand-worked answer, the GPU tests hold the kernels to absorb_lit.
"""
import numpy as np

import absorb_reference as A
from absorb_reference import F, PLANES, STATS, differing, level_intrinsics, make_scene, states_equal  # noqa: F401  (re-exported for the tests)
from trial_propagation_reference import _residuals, wiped_state

_plain_candidates = A._candidates


def gate(Iw, Is, g, gain, offset):
    """Step 4, vectorised: (r, pass) of interior pixels with warped value Iw, source grey value Is and gradient g at the target."""
    with np.errstate(all="ignore"):
        Ip = ((F(gain) * Is).astype(F) + F(offset)).astype(F)
        r = (Iw - Ip).astype(F)
        ratio = ((r * r).astype(F) / (F(1600.0) + ((F(0.25) * g).astype(F) * g).astype(F)).astype(F)).astype(F)
    return r, ~((ratio > F(1.0)) | (g < F(5.0)))


def gate_scalar(Iw, Is, g, gain, offset):
    """Step 4, pixel by pixel with numpy f32 scalars."""
    r = np.zeros(len(Iw), F)
    ok = np.zeros(len(Iw), bool)
    with np.errstate(all="ignore"):
        for k in range(len(Iw)):
            Ip = F(F(F(gain) * F(Is[k])) + F(offset))
            res = F(F(Iw[k]) - Ip)
            gk = F(g[k])
            r[k] = res
            ok[k] = not (F(F(res * res) / F(F(1600.0) + F(F(F(0.25) * gk) * gk))) > F(1.0) or gk < F(5.0))
    return r, ok


def interior(depth, var, img, intr, T12, flt, b, k_img, k_maxgrad):
    """The interior pixels of one request (steps 1-3) with what step 4 reads: the gate-off candidates of absorb_reference, Iw, Is, g."""
    every = _plain_candidates(depth, var, img, intr, T12, flt, b, k_img, k_maxgrad, 0)
    img = np.asarray(img)
    Iw, g, target = _residuals(depth, var, np.zeros_like(img), intr, T12, every["ident"], k_img, k_maxgrad)
    assert np.array_equal(target, every["target"])
    i = every["ident"] & 0xffffff
    cols = np.asarray(depth).shape[1]
    return every, Iw, img[i // cols, i % cols].astype(F), g


def candidates_lit(depth, var, img, intr, T12, flt, b, k_img, k_maxgrad, photo_gate, light, gate_fn=gate):
    """absorb_reference._candidates with step 4 taken at `light` = (gain, offset)."""
    every, Iw, Is, g = interior(depth, var, img, intr, T12, flt, b, k_img, k_maxgrad)
    if not photo_gate:
        return every
    _, keep = gate_fn(Iw, Is, g, light[0], light[1])
    out = {k: every[k][keep] for k in ("ident", "target", "nid", "nvar")}
    out.update(n_kept=every["n_kept"], n_in_view=every["n_in_view"], n_interior=every["n_interior"], n_candidates=int(keep.sum()))
    return out


def absorb_lit(requests, intr, Ts, lights, flt, k_img, k_maxgrad, state, gate_fn=gate, **prm):
    """absorb_reference.absorb with request b's candidates gated at lights[b] (None: (1, 0) each). Returns what absorb returns."""
    L = np.tile(np.asarray([1.0, 0.0], F), (len(requests), 1)) if lights is None else np.asarray(lights, F).reshape(len(requests), 2)

    def per_request(depth, var, img, intr_, T12, flt_, b, k_img_, k_maxgrad_, photo_gate):
        return candidates_lit(depth, var, img, intr_, T12, flt_, b, k_img_, k_maxgrad_, photo_gate, L[b], gate_fn)

    # (absorb_reference has no parameter for its gate and may not be restated: its per-request step is replaced for the length of this
    # call and put back whatever happens; one call at a time)
    assert A._candidates is _plain_candidates, "absorb_lit is not re-entrant"
    A._candidates = per_request
    try:
        return A.absorb(requests, intr, Ts, flt, k_img, k_maxgrad, state, **prm)
    finally:
        A._candidates = _plain_candidates


def absorb_lit_scalar(requests, intr, Ts, lights, flt, k_img, k_maxgrad, state, **prm):
    return absorb_lit(requests, intr, Ts, lights, flt, k_img, k_maxgrad, state, gate_fn=gate_scalar, **prm)


def restart_lit(requests, intr, Ts, lights, flt, k_img, k_maxgrad, **prm):
    """ellc_depth_restart_from_keyframes_lit without `finalise`: the wiped state + absorb_lit."""
    rows, cols = np.asarray(requests[0][0]).shape
    return absorb_lit(requests, intr, Ts, lights, flt, k_img, k_maxgrad, wiped_state(rows, cols), **prm)


def brighten(img, gain=1.6, offset=-20.0):
    """The altered destination of the demonstration: clip(rint(gain * I + offset)) as u8."""
    return np.clip(np.rint(gain * np.asarray(img, np.float64) + offset), 0, 255).astype(np.uint8)
