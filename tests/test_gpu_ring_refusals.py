"""What the calls over the keyframe ring's maps refuse, entry point by entry point: the status, and that the C-side text of
ellc_last_error begins with the name of the entry point that was called (the validators are shared and take the name as a parameter).
One context at 23x17 with 2 levels and 4 keyframe slots: 0..2 hold an image and a map, 3 an image only. Ten rows: the nine exported
calls, ellc_keyframe_trial_propagate once per kind of destination (it validates a frame slot and a keyframe slot differently).
After all refusals a valid call of every row returns the bytes it returned before them."""
import numpy as np
import pytest

import absorb_reference as A
from helpers import gpu_problem

pytestmark = pytest.mark.gpu

BAD_ARG, NOT_READY = -1, -3
W, H, L, N_SLOTS, NO_DEPTH = 23, 17, 2, 4, 3
GOOD = dict(max_var=0.0, min_support=0, support_k2=1.0, stride=1)


def blob(x):
    """Every array and number of a call's result, as bytes."""
    if isinstance(x, dict):
        return b"".join(blob(x[k]) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return b"".join(blob(v) for v in x)
    return np.asarray(x).tobytes()


@pytest.fixture(scope="module")
def world(ellc):
    sc = A.make_scene(W, H, n_views=3)
    ctx = gpu_problem(ellc, W, H, L, sc["views"], max_keyframes=N_SLOTS)
    ctx.keyframe_upload(NO_DEPTH, sc["views"][1]["kf_image"])
    yield dict(ctx=ctx, Ts=sc["Ts"], state=sc["state"])
    ctx.close()


def rows(world):
    """name -> (takes a level, call(slots, level, flt)): `slots` are the sources of the call, a pair call's destination is slot 0."""
    ctx, Ts = world["ctx"], world["Ts"]

    def T(slots):
        return np.resize(Ts, (len(slots), 12))

    def zeros(slots):
        return [0] * len(slots)

    def absorb(slots, level, flt):
        ctx.depth_set_keyframe(0)
        ctx.depth_set_state(world["state"])
        return ctx.depth_absorb(slots, T(slots), params=dict(finalise=0), **flt)

    return {
        "ellc_keyframe_map_points": (True, lambda s, l, f: ctx.map_points(s, T(s), level=l, **f)),
        "ellc_keyframe_render_depth": (True, lambda s, l, f: ctx.render_depth(s, T(s), level=l, **f)),
        "ellc_keyframe_fuse_depth": (True, lambda s, l, f: ctx.fuse_depth(s, T(s), level=l, **f)),
        "ellc_keyframe_depth_consistency": (True, lambda s, l, f: ctx.depth_consistency(s, zeros(s), T(s), level=l, **f)),
        "ellc_keyframe_sim3_step": (True, lambda s, l, f: ctx.sim3_step(s, zeros(s), T(s), level=l, **f)),
        "ellc_keyframe_sim3_align": (True, lambda s, l, f: ctx.sim3_align(s, zeros(s), T(s), level_from=l, level_to=l, max_iter=2, **f)),
        "ellc_keyframe_trial_propagate/frame": (False, lambda s, l, f: ctx.trial_propagate(s, zeros(s), T(s), dst_is_keyframe=False, **f)),
        "ellc_keyframe_trial_propagate/keyframe": (False, lambda s, l, f: ctx.trial_propagate(s, zeros(s), T(s), dst_is_keyframe=True, **f)),
        "ellc_depth_absorb_keyframes": (False, absorb),
        # (the new keyframe is slot 3 where the sources are good ones, slot 0 where slot 3 is the source under test)
        "ellc_depth_restart_from_keyframes": (False, lambda s, l, f: ctx.depth_restart(0 if NO_DEPTH in s else NO_DEPTH, s, T(s), params=dict(finalise=0), **f)),
    }


def malformed(takes_level):
    """(what, slots, level, filter, expected status)"""
    good = [1, 2]
    cases = [("B = 0", [], 0, GOOD, BAD_ARG)]
    if takes_level:
        cases.append(("level = L", good, L, GOOD, BAD_ARG))
    for k, v in (("min_support", 9), ("stride", 0), ("support_k2", -1.0), ("support_k2", np.inf), ("max_var", np.nan)):
        cases.append(("%s = %s" % (k, v), good, 0, dict(GOOD, **{k: v}), BAD_ARG))
    cases.append(("slot -1", [1, -1], 0, GOOD, BAD_ARG))
    cases.append(("slot max_keyframes", [1, N_SLOTS], 0, GOOD, BAD_ARG))
    cases.append(("slot without depth", [1, NO_DEPTH], 0, GOOD, NOT_READY))
    return cases


def test_every_entry_point_refuses_under_its_own_name(world, ellc):
    ctx = world["ctx"]
    table = rows(world)
    assert len(table) == 10
    before = {name: blob(call([1, 2], 0, GOOD)) for name, (_, call) in table.items()}
    for name, (takes_level, call) in table.items():
        entry = name.split("/")[0]
        for what, slots, level, flt, status in malformed(takes_level):
            with pytest.raises(ellc.EllcError) as e:
                call(slots, level, flt)
            text = ctx._l.ellc_last_error(ctx.h).decode()
            print(name, "|", what, "|", e.value)
            assert str(e.value).startswith("%s -> %d: " % (entry, status)), (name, what, str(e.value))
            assert text.startswith(entry + ": "), (name, what, text)
    for name, (_, call) in table.items():
        assert blob(call([1, 2], 0, GOOD)) == before[name], name
