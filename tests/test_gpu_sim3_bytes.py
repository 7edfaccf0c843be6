"""The bytes of ellc_keyframe_sim3_step and ellc_keyframe_sim3_align pinned from outside: tests/golden/sim3_bytes.npz holds the planes of
tests/test_gpu_sim3.py's world at 23x17 (2 levels) and 64x48 (3 levels) and what the library of ABI v19, where the plain and the lit
call still had a kernel and a loop each, returned for them (tests/golden/make_sim3_bytes.py; the file's `note` names the commit).
Since the two calls share one kernel and one loop, a lit call at the light (1, 0) against the plain call compares a path with itself;
here both are compared with the stored bytes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3_bytes.npz"))
SHAPES = {"23x17": (23, 17, 2), "64x48": (64, 48, 3)}


def fkw(flt):
    return dict(max_var=float(flt[0]), min_support=int(flt[1]), support_k2=float(flt[2]), stride=int(flt[3]))


@pytest.fixture(scope="module", params=list(SHAPES))
def world(request, ellc):
    shape = request.param
    w, h, L = SHAPES[shape]
    z = {k.split("/", 1)[1]: GOLDEN[k] for k in GOLDEN.files if k.startswith(shape + "/")}
    fx, fy, cx, cy = (float(v) for v in z["intrinsics"])
    ctx = ellc.Context(ellc.default_config(w, h, L, fx=fx, fy=fy, cx=cx, cy=cy, max_keyframes=3))
    for slot in range(3):
        ctx.keyframe_upload(slot, z["img"][slot])
        ctx.keyframe_set_depth(slot, z["depth"][slot], z["var"][slot])
    batch = GOLDEN["batch"].tolist()
    yield dict(ctx=ctx, L=L, z=z, src=[s for s, _, _ in batch], dst=[d for _, d, _ in batch], Ts=np.stack([z["Ts"][t] for _, _, t in batch]))
    ctx.close()


def test_the_steps_give_the_stored_bytes(world):
    """sim3_step, and sim3_step_lit without a light and at an explicit (1, 0): the six pairs, every level, both filters."""
    ctx, src, dst, Ts = world["ctx"], world["src"], world["dst"], world["Ts"]
    unit = np.tile(np.asarray((1.0, 0.0), F), (len(src), 1))
    for f, flt in enumerate(GOLDEN["filters"]):
        for level in range(world["L"]):
            want = world["z"]["step"][f, level].tobytes()
            assert any(want)
            assert ctx.sim3_step(src, dst, Ts, level=level, **fkw(flt)).tobytes() == want, (f, level)
            assert ctx.sim3_step_lit(src, dst, Ts, None, level=level, **fkw(flt)).tobytes() == want, (f, level)
            assert ctx.sim3_step_lit(src, dst, Ts, unit, level=level, **fkw(flt)).tobytes() == want, (f, level)


def test_the_loops_give_the_stored_bytes(world):
    """sim3_align, and sim3_align_lit with every fit refused (min_pixels = 2^30): T, records, iteration counts and both traces."""
    ctx, z, L = world["ctx"], world["z"], world["L"]
    kw = dict(level_from=L - 1, level_to=0, max_iter=int(GOLDEN["max_iter"]), eps=float(GOLDEN["eps"]), trace=True, **fkw(GOLDEN["filters"][0]))
    assert int(z["align_iters"].sum()) > 0 and int(z["trace_n"].sum()) == len(z["trace_T"])
    for name, got in (("sim3_align", ctx.sim3_align(world["src"], world["dst"], world["Ts"], **kw)),
                      ("sim3_align_lit", ctx.sim3_align_lit(world["src"], world["dst"], world["Ts"], None, light_params=dict(min_pixels=1 << 30), **kw))):
        assert got["T"].tobytes() == z["align_T"].tobytes(), name
        assert got["rec"].tobytes() == z["align_rec"].tobytes(), name
        assert got["iters"].tobytes() == z["align_iters"].tobytes(), name
        assert [len(t) for t in got["trace_T"]] == z["trace_n"].tolist(), name
        assert np.concatenate(got["trace_T"]).tobytes() == z["trace_T"].tobytes(), name
        assert b"".join(t.tobytes() for t in got["trace_rec"]) == z["trace_rec"].tobytes(), name
