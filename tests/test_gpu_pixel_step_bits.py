"""The tolerance mode's pixel step (tap_request_f / tap_finish_f, fcaf_stage_a / _b: gn_fca_fused, gn_fca_adaptive, gn_fca_persist,
gn_fca_dense and the single-pixel step of gn_fca_dense4) keeps its bits across changes to how it is written.

tests/golden/pixel_step_bits.npz holds H, b and the stepped pose of one launch of the schedule's kernel at every level
(ellc_debug_schedule_sums, diagnostic library), recorded by tests/golden/make_pixel_step_bits.py from the build of the commit before
r11's rewrite of the step for the packed vector instructions (register pairs with one home per sample, the interior test as two
ballots, the 0.5 of the depth derivative folded into block constants). Not one floating-point operation changed there, so every field
is compared as bytes. The case list is the generator's own (imported from it):

  shapes   72 x 52 with 3 levels, 64 x 32 with 2 levels
  maps     synth's semi-dense map; all pixels valid; none (V = 0); the last pixel only (V = 1); a level-0 count that makes every
           block's chunk exactly 256 records (one full step of the loop), and that count + 1 (a last step with one live thread)
  taps     the packed load, and the diagnostic library's row loads (ellc_debug_set_packed_taps(0))
  poses    zero; a small twist; a shift of about 3 pixels (lanes on the border); a shift that sends about a third of the points out
           of the image — four alignments of one launch

The generator asserts from a numpy warp of these poses that interior-only waves, waves with a border lane and lanes without a tap
in bounds all occur, so the cases cannot all stay on one path. The kernel name and the grid of every launch are part of the fixture:
a case that stopped running the kernel it was recorded with fails rather than passes on other code."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_pixel_step_bits", os.path.join(GOLDEN, "make_pixel_step_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    return gen.load_fixture()


@pytest.mark.parametrize("w,h,L", gen.SHAPES)
def test_schedule_sums_keep_the_parent_builds_bits(ellc, golden, w, h, L):
    seen, bad = [], []

    def emit(k, v):
        seen.append(k)
        want = golden[k]
        if isinstance(v, str):
            same = str(want) == v
        else:
            same = want.dtype == v.dtype and want.shape == v.shape and want.tobytes() == np.ascontiguousarray(v).tobytes()
        if not same:
            bad.append(k)

    gen.run_cases(ellc, w, h, L, emit)
    # every case of the shape ran: maps x taps x levels x (H, b, pose, kernel, grid)
    assert len(seen) == len(gen.MAPS) * len(gen.TAPS) * L * 5
    assert sorted(seen) == sorted(k for k in golden if k.startswith("w%d/" % w))
    assert not bad, bad
    # the fixture is not degenerate: the maps with pixels have sums, and the row loads agree with the packed taps in it
    for name in gen.MAPS:
        for l in range(L):
            H = golden[gen.key(w, name, 1, l, "H")]
            if name != "last_pixel":   # (one corner pixel: whether it contributes is the border path's business)
                assert (np.abs(H).sum() > 0) == (name != "none"), (name, l)
            for f in ("H", "b", "pose"):
                assert golden[gen.key(w, name, 1, l, f)].tobytes() == golden[gen.key(w, name, 0, l, f)].tobytes(), (name, l, f)
