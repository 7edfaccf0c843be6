"""The image planes of a slot at all eight pyramid depths, held to the plain numpy reference (tests/image_reference.py) bit for bit.

Shapes (tests/image_shapes.py): the smallest ones that reach every split of the pyramid into chains of up to three pyrDown steps
(build_image_pyramid, L = 1 .. 8: none, 1, 2, 3, 3+1, 3+2, 3+3, 3+3+1), levels 4 or 5 pixels wide where REFLECT_101 folds back into the
level and the last 4-wide tile of pyr_down_chain_u8 holds one column, 128 x 4 levels (the halo larger than the level), levels odd at
every depth, and the partial tiles of maxgrad_fused (32k + 1, 8k + 1), hist256_u8 and ingest_copy_u8 (391 pixels) and pack_tap_rows.
Both arithmetic modes; contexts of the tolerance mode live in the diagnostic library, which exports the row-packed planes. No alignment
is run: everything here is a function of the uploaded image (or depth plane) alone, integer or exact f32 arithmetic, so every
comparison is an equality, and always against the reference, never against another GPU result alone."""
import os
import re
import numpy as np
import pytest
from egomotion_with_local_loop_closures_amd import synth
from helpers import bits_equal
import image_shapes as S

pytestmark = pytest.mark.gpu
ARITH = ("exact", "fast")


RING_SLOTS = 8   # slots per kind in test_staging_ring: comfortably more than the ring has staging buffers (checked against the header)


def upload_ring():
    """ellc_ctx::UPLOAD_RING, the number of pinned staging buffers an upload cycles through. Not part of the ABI: read from the
    declaration in csrc/ellc_context.hpp, so this depends on that line's wording (`constexpr int UPLOAD_RING = N;`) and on the sources
    lying beside the package; the test's slot count is fixed and only checked against it."""
    import egomotion_with_local_loop_closures_amd as pkg
    with open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "ellc_context.hpp")) as f:
        m = re.search(r"constexpr\s+int\s+UPLOAD_RING\s*=\s*(\d+)\s*;", f.read())
    assert m, "ellc_ctx::UPLOAD_RING not found"
    return int(m.group(1))


def make_ctx(ellc, w, h, L, arith, **kw):
    fx, fy, cx, cy = synth.default_intrinsics(w, h)
    fast = arith == "fast"
    cfg = ellc.default_config(w, h, L, fx=fx, fy=fy, cx=cx, cy=cy, arith=ellc.ARITH_FAST if fast else ellc.ARITH_EXACT, **kw)
    return ellc.Context(cfg, diag=fast)


def check_image_planes(ctx, is_kf, slot, ref, what, levels=None):
    """stored planes, their shapes and iterated sizes, of the given levels (default: all)"""
    for l in (range(ctx.levels) if levels is None else levels):
        (sw, sh), (cols, rows) = ref["dims"][l]
        got, it = ctx.image_level(is_kf, slot, l)
        assert got.shape == (sh, sw), (what, l)
        assert it == (rows, cols), (what, l)
        assert np.array_equal(got, ref["levels"][l]), (what, "pyramid level", l)


def check_packed(ctx, slot, ref, what, levels=None):
    if not ctx.diag:        # contexts of the exact mode keep no row-packed planes
        return
    for l in (range(ctx.levels) if levels is None else levels):
        got = ctx.debug_get_packed_level(slot, l)
        assert got.dtype == np.uint32 and got.shape == ref["packed"][l].shape, (what, l)
        assert np.array_equal(got, ref["packed"][l]), (what, "packed level", l)   # (the zero bytes of rows -1, rows, rows + 1 included)


def check_slot(ctx, is_kf, slot, ref, what):
    """everything a slot shows of its image"""
    check_image_planes(ctx, is_kf, slot, ref, what)
    for l in range(ctx.levels):
        gx, gy = ctx.gradient(is_kf, slot, l)
        assert gx.shape == ref["grad"][l][0].shape, (what, l)
        assert bits_equal(gx, ref["grad"][l][0]) and bits_equal(gy, ref["grad"][l][1]), (what, "gradient level", l)
    mg, n = ctx.max_gradient(is_kf, slot)
    assert bits_equal(mg, ref["maxgrad"][0]), (what, "max gradient")
    assert n == ref["maxgrad"][1], (what, "max gradient count")
    assert np.array_equal(ctx.histogram(is_kf, slot), ref["hist"]), (what, "histogram")
    if not is_kf:
        check_packed(ctx, slot, ref, what)


def check_depth(ctx, slot, dref, what):
    d, v = ctx.keyframe_depth_level(slot, 0)
    assert bits_equal(d, dref[0][0]) and bits_equal(v, dref[0][1]), (what, "level 0 is the upload")
    for l in range(1, ctx.levels):
        d, v = ctx.keyframe_depth_level(slot, l)
        assert d.shape == dref[l][0].shape, (what, l)
        assert bits_equal(d, dref[l][0]), (what, "depth level", l)
        assert bits_equal(v, dref[l][1]), (what, "variance level", l)


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("w,h,L", S.SHAPES, ids=S.SHAPE_IDS)
def test_upload_planes(ellc, w, h, L, arith):
    """keyframe_upload and frame_upload: every plane of both slot kinds; each following image goes into the SAME slots, so a plane (or
    part of one) left over from the image before shows as a difference"""
    ctx = make_ctx(ellc, w, h, L, arith)
    for kind, seed in [(k, 0) for k in S.IMAGE_KINDS] + [("checkerboard", 1), ("random_blocks", 1)]:
        img, ref = S.image(w, h, kind, seed), S.reference(w, h, L, kind, seed)
        ctx.keyframe_upload(0, img)
        ctx.frame_upload(0, img)
        check_slot(ctx, 1, 0, ref, (kind, seed, "keyframe slot"))
        check_slot(ctx, 0, 0, ref, (kind, seed, "frame slot"))
    ctx.close()


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("w,h,L", S.SHAPES, ids=S.SHAPE_IDS)
def test_staging_ring(ellc, w, h, L, arith):
    """more uploads back to back than the ring has staging buffers, nothing read in between: every slot holds its own image. What this
    holds is the ring's cursor and the wiring of buffer to slot over more than one turn of the ring. The wait for a buffer's earlier
    copy (upload_done[k]) is taken on every reuse, but a missing wait would show only if the host overtook the device, which at these
    sizes it almost certainly does not: that synchronisation is not deterministically exercised here."""
    n = RING_SLOTS
    assert n >= upload_ring() + 2
    ctx = make_ctx(ellc, w, h, L, arith, max_frames=n, max_keyframes=n)
    jobs = [(("random_blocks", "texture")[i % 2], 10 + i) for i in range(2 * n)]
    assert len({S.image(w, h, k, s).tobytes() for k, s in jobs}) == 2 * n      # all different
    for i in range(n):
        ctx.frame_upload(i, S.image(w, h, *jobs[i]))
    for i in range(n):
        ctx.keyframe_upload(i, S.image(w, h, *jobs[n + i]))
    for i in range(n):
        for is_kf, job in ((0, jobs[i]), (1, jobs[n + i])):
            ref = S.reference(w, h, L, *job)
            check_image_planes(ctx, is_kf, i, ref, ("ring", is_kf, i), levels=sorted({0, L - 1}))
            if not is_kf:
                check_packed(ctx, i, ref, ("ring", i), levels=sorted({0, L - 1}))
    ctx.close()


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("w,h,L", S.SHAPES, ids=S.SHAPE_IDS)
def test_copied_slots(ellc, w, h, L, arith):
    """keyframe_from_frame and copy_slot in every direction: the destination against the reference of the SOURCE IMAGE"""
    ctx = make_ctx(ellc, w, h, L, arith, max_keyframes=4, max_frames=3)
    a, b = ("random_blocks", 2), ("texture", 2)
    ra, rb = S.reference(w, h, L, *a), S.reference(w, h, L, *b)
    dense = S.depth_planes(w, h, "dense")
    ctx.keyframe_upload(0, S.image(w, h, *a))
    ctx.keyframe_set_depth(0, *dense)
    ctx.frame_upload(1, S.image(w, h, *b))
    for s in (0, 2):                                   # the destinations hold another image first
        ctx.frame_upload(s, S.image(w, h, "checkerboard", 2))
    for s in (1, 2, 3):
        ctx.keyframe_upload(s, S.image(w, h, "checkerboard", 3))
    ctx.copy_slot(1, 2, 1, 0)                          # keyframe -> keyframe (the ring's deep copy: depth planes travel along)
    check_slot(ctx, 1, 2, ra, "copy_slot keyframe -> keyframe")
    check_depth(ctx, 2, S.depth_reference(w, h, L, "dense"), "copy_slot keyframe -> keyframe")
    ctx.copy_slot(0, 0, 1, 0)                          # keyframe -> frame
    check_slot(ctx, 0, 0, ra, "copy_slot keyframe -> frame")
    ctx.copy_slot(0, 2, 0, 1)                          # frame -> frame
    check_slot(ctx, 0, 2, rb, "copy_slot frame -> frame")
    ctx.copy_slot(1, 3, 0, 1)                          # frame -> keyframe
    check_slot(ctx, 1, 3, rb, "copy_slot frame -> keyframe")
    ctx.keyframe_upload(3, S.image(w, h, "checkerboard", 3))
    ctx.keyframe_from_frame(3, 1)                      # (distinct indices: frame slot 1 into keyframe slot 3)
    check_slot(ctx, 1, 3, rb, "keyframe_from_frame")
    check_slot(ctx, 1, 1, S.reference(w, h, L, "checkerboard", 3), "keyframe slot 1, which keyframe_from_frame(3, 1) must not touch")
    check_slot(ctx, 1, 0, ra, "the source keyframe slot afterwards")
    check_slot(ctx, 0, 1, rb, "the source frame slot afterwards")
    ctx.close()


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("w,h,L", S.SHAPES, ids=S.SHAPE_IDS)
def test_uploaded_depth_pyramid(ellc, w, h, L, arith):
    """keyframe_set_depth: depth_pyr_level at every level >= 1 (source stride 2 * destination width: rows drift below an odd level),
    cells with 0 .. 4 valid children (tests/test_image_reference.py asserts the inputs hold them). The dense case also takes the path
    that writes the slot's reciprocal planes behind the pyramid; one case after the other goes into the same slot."""
    ctx = make_ctx(ellc, w, h, L, arith, max_keyframes=2)
    for s in (0, 1):
        ctx.keyframe_upload(s, S.image(w, h, "texture"))
    for case in ("dense", "semi_dense", "full_interior", "dense"):
        ctx.keyframe_set_depth(0, *S.depth_planes(w, h, case))
        check_depth(ctx, 0, S.depth_reference(w, h, L, case), case)
    ctx.keyframe_set_depth(1, *S.depth_planes(w, h, "semi_dense", 1))
    check_depth(ctx, 1, S.depth_reference(w, h, L, "semi_dense", 1), "slot 1")
    check_depth(ctx, 0, S.depth_reference(w, h, L, "dense"), "slot 0 after slot 1 was written")
    ctx.close()
