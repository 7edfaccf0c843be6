"""The tolerance mode's interior taps come as one 16-byte load from the frame slot's row-packed plane (FrLevelDev::img4).

Word (y, x) of the plane holds column x of rows y - 1 .. y + 2 of the level image, so the 4 x 4 neighbourhood of a warped point is four
adjacent words. The plane is a function of the image alone and is written by every writer of a frame slot's image planes; the twelve
bytes the taps use reach the same conversions and the same arithmetic as through the four row loads the diagnostic library keeps
(ellc_debug_set_packed_taps(0)), so between the two not a bit may differ.

Shapes: 101 x 75 with 3 levels (odd sizes, stored pitch != width below level 0) and 160 x 120 with 4 levels (down to 20 x 15)."""
import numpy as np
import pytest
from egomotion_with_local_loop_closures_amd import synth
from image_reference import packed_rows as transposed   # the numpy statement of the plane's layout

pytestmark = pytest.mark.gpu
SHAPES = [(101, 75, 3), (160, 120, 4)]
MAX_ITER = (3, 4, 5, 6)
# a start pose far enough off that waves of the coarsest level reach over the image border (the per-tap path), see test_both_tap_paths_run
START = np.array([0.01, -0.008, 0.006, 0.05, -0.04, 0.03], np.float32)
NOWHERE = np.array([0, 0, 0, 50.0, 0, 0], np.float32)   # every point leaves the image: neither tap path returns an intensity


def pairs_of(w, h, n, dense=False, seed=900):
    return [synth.make_pair(w, h, seed=seed + i, dense=dense, rot=0.004, trans=0.012, border=1 if dense else 3) for i in range(n)]


def context(ellc, w, h, L, pairs, frames=True, **kw):
    """pairs[i] in keyframe slot i and (frames) frame slot i"""
    fx, fy, cx, cy = pairs[0]["intrinsics"]
    kw = dict(dict(max_iter=MAX_ITER[:L], max_keyframes=4, max_frames=4, max_batch=3, arith=ellc.ARITH_FAST), **kw)
    ctx = ellc.Context(ellc.default_config(w, h, L, fx=fx, fy=fy, cx=cx, cy=cy, **kw), diag=True)
    for i, p in enumerate(pairs):
        ctx.keyframe_upload(i, p["kf_image"])
        ctx.keyframe_set_depth(i, p["depth0"], p["var0"])
        if frames:
            ctx.frame_upload(i, p["cur_image"])
    return ctx


def check_plane(ctx, slot, L, what):
    for l in range(L):
        img, (rows, cols) = ctx.image_level(0, slot, l)
        got = ctx.debug_get_packed_level(slot, l)
        assert got.shape == img.shape, (what, l)
        assert np.array_equal(got, transposed(img, rows)), (what, l)
        assert not (got[0] & 0xff).any(), (what, l, "row -1")
        assert not (got[rows - 2] >> 24).any() and not (got[rows - 1] >> 16).any(), (what, l, "rows `rows`, `rows` + 1")
        assert (got[1:rows - 2] != 0).any(), (what, l, "the plane is empty")


@pytest.mark.parametrize("w,h,L", SHAPES)
def test_packed_plane_after_every_writer(ellc, w, h, L):
    pairs = pairs_of(w, h, 2)
    ctx = context(ellc, w, h, L, pairs)
    check_plane(ctx, 0, L, "upload")
    check_plane(ctx, 1, L, "upload")
    ctx.frame_upload(0, pairs[1]["cur_image"])
    check_plane(ctx, 0, L, "second upload")
    assert np.array_equal(ctx.debug_get_packed_level(0, 0), ctx.debug_get_packed_level(1, 0))
    ctx.copy_slot(0, 2, 0, 1)   # frame -> frame
    check_plane(ctx, 2, L, "copy_slot from a frame slot")
    ctx.copy_slot(0, 3, 1, 0)   # keyframe -> frame
    check_plane(ctx, 3, L, "copy_slot from a keyframe slot")
    assert np.array_equal(ctx.image_level(0, 3, 0)[0], ctx.image_level(1, 0, 0)[0])
    fx, fy, cx, cy = pairs[0]["intrinsics"]
    ctx.ingest_configure(4 * w, 4 * h, 4 * fx, 4 * fy, 4 * cx, 4 * cy, None, False)
    bgr = np.random.default_rng(3).integers(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8)
    ctx.frame_ingest_bgr(1, bgr)
    check_plane(ctx, 1, L, "ingest")
    ctx.close()


def both(ellc, w, h, L, pairs, **kw):
    on, off = context(ellc, w, h, L, pairs, **kw), context(ellc, w, h, L, pairs, **kw)
    off.debug_set_packed_taps(False)
    return on, off


class RowLoads:
    """Evidence that the two sides of a comparison ran different tap paths: the calls inside the block make the `off` context build
    kernel argument records with the row loads selected (ellc_debug_row_tap_launches rises), the `on` context none."""

    def __init__(self, on, off):
        self.on, self.off = on, off

    def __enter__(self):
        self.n0 = self.off.debug_row_tap_launches()
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            assert self.off.debug_row_tap_launches() > self.n0, "the reference side built no launch with the row loads"
            assert self.on.debug_row_tap_launches() == 0, "the packed side selected the row loads"
        return False


def same(ra, rb):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(ra, rb))


def same_weights(a, b, slot, L):
    for l in range(L):
        wa, na = a.keyframe_weights(slot, l)
        wb, nb = b.keyframe_weights(slot, l)
        if na != nb or not np.array_equal(wa, wb):
            return False
    return True


def same_steps(a, b, kf, fr, L, mode=0):
    """per-iteration H, b and step of the schedule's kernel at every level, from the far start pose"""
    for l in range(L):
        sa, sb = a.debug_schedule_sums(kf, fr, l, START, mode=mode), b.debug_schedule_sums(kf, fr, l, START, mode=mode)
        assert sa["kernel"] == sb["kernel"]
        for k in ("H", "b", "pose", "hinv"):
            assert np.array_equal(sa[k], sb[k]), (l, k, sa["kernel"])
    return True


@pytest.mark.parametrize("w,h,L", SHAPES)
def test_list_path_batch_of_three(ellc, w, h, L):
    pairs = pairs_of(w, h, 3)
    on, off = both(ellc, w, h, L, pairs, early_exit=0)
    start = np.tile(START, (3, 1))
    for sw in (False, True):
        with RowLoads(on, off):
            assert same(on.align([0, 1, 2], [0, 1, 2], init_pose=start, save_weights=sw), off.align([0, 1, 2], [0, 1, 2], init_pose=start, save_weights=sw))
    assert same(on.align([2, 0, 1], [0, 0, 0]), off.align([2, 0, 1], [0, 0, 0]))
    for s in range(3):
        assert same_weights(on, off, s, L)
    with RowLoads(on, off):
        assert same_steps(on, off, [0, 1, 2], [0, 1, 2], L)
    # the single-step API (gn_fca_accumulate) and its debug planes
    with RowLoads(on, off):
        ga, gb = on.gn_iterate(0, 0, L - 1, START, planes=True), off.gn_iterate(0, 0, L - 1, START, planes=True)
    for k in ("H", "b", "delta", "pose", "residual", "weight", "J"):
        assert np.array_equal(ga[k], gb[k]), k
    on.close(); off.close()


@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("w,h,L", SHAPES)
def test_tracking_call(ellc, w, h, L, persist):
    pairs = pairs_of(w, h, 2)
    on, off = both(ellc, w, h, L, pairs, early_exit=1)
    st = synth.make_depth_state(w, h, 7, pairs[1]["kf_image"], pairs[1]["idepth_true"])
    for c in (on, off):
        c.set_persistent_schedule(persist)
    for sw in (False, True):   # one alignment with early exit on: the state-driven schedule, resident or one launch per iteration
        with RowLoads(on, off):
            assert same(on.align([0], [0], init_pose=START, save_weights=sw), off.align([0], [0], init_pose=START, save_weights=sw))
    with RowLoads(on, off):
        assert same(on.align([0, 1], [1, 0]), off.align([0, 1], [1, 0]))
    assert same_weights(on, off, 0, L)
    for c in (on, off):
        c.depth_set_keyframe(1); c.depth_set_state(st); c.depth_regularize(False)
    with RowLoads(on, off):
        assert same(on.track_frame(1, save_weights=True), off.track_frame(1, save_weights=True))
    with RowLoads(on, off):
        assert same(on.track_frame(0, init_pose=START), off.track_frame(0, init_pose=START))
    assert same_weights(on, off, 1, L)
    on.close(); off.close()


@pytest.mark.parametrize("w,h,L", SHAPES)
def test_dense_map(ellc, w, h, L):
    """a map at least nine tenths full: the list-free schedule; 101 and 25 columns are no multiple of four (gn_fca_dense); at the other
    shape gn_fca_dense4 runs, whose quads that its row windows do not serve take the single-pixel step"""
    pairs = pairs_of(w, h, 3, dense=True)
    on, off = both(ellc, w, h, L, pairs, early_exit=0)
    start = np.tile(START, (3, 1))
    with RowLoads(on, off):
        assert same(on.align([0, 1, 2], [0, 1, 2], init_pose=start), off.align([0, 1, 2], [0, 1, 2], init_pose=start))
    kernels = set()
    for l in range(L):
        n0 = off.debug_row_tap_launches()
        sa, sb = on.debug_schedule_sums([0, 1, 2], [0, 1, 2], l, START), off.debug_schedule_sums([0, 1, 2], [0, 1, 2], l, START)
        assert off.debug_row_tap_launches() > n0 and on.debug_row_tap_launches() == 0
        kernels.add(sa["kernel"])
        for k in ("H", "b", "pose"):
            assert np.array_equal(sa[k], sb[k]), (l, k, sa["kernel"])
    # 101, 50 and 25 columns: level 0 and 2 run gn_fca_dense; 160, 80, 40, 20: gn_fca_dense4 (its single-pixel step is the shared one)
    assert ("gn_fca_dense" if w % 4 else "gn_fca_dense4") in kernels, kernels
    on.close(); off.close()


@pytest.mark.parametrize("early_exit", [0, 1])
@pytest.mark.parametrize("w,h,L", SHAPES)
def test_constant_weight_path(ellc, w, h, L, early_exit):
    """ICA, tolerance mode: columns x0, x0 + 1 as one 8-byte load of the packed plane"""
    pairs = pairs_of(w, h, 3)
    on, off = both(ellc, w, h, L, pairs, early_exit=early_exit)
    for c in (on, off):
        for s in range(3):
            for l in range(L):
                c.keyframe_set_weights(s, l, np.full((h >> l, w >> l), 0.03, np.float32), 1)
    start = np.tile(START, (3, 1))
    with RowLoads(on, off):
        assert same(on.align([0, 1, 2], [0, 1, 2], init_pose=start, mode=1), off.align([0, 1, 2], [0, 1, 2], init_pose=start, mode=1))
    with RowLoads(on, off):
        assert same(on.align([1], [1], init_pose=START, mode=1), off.align([1], [1], init_pose=START, mode=1))
    if not early_exit:
        with RowLoads(on, off):
            assert same_steps(on, off, [0, 1, 2], [0, 1, 2], L, mode=1)
    on.close(); off.close()


@pytest.mark.parametrize("w,h,L", SHAPES)
def test_quality_pass_and_both_tap_paths_run(ellc, w, h, L):
    pairs = pairs_of(w, h, 2)
    on, off = both(ellc, w, h, L, pairs, early_exit=0)
    poses = np.stack([START, np.zeros(6, np.float32)])
    for l in range(L):
        n0 = off.debug_row_tap_launches()
        qa, qb = on.align_quality([0, 1], [0, 1], poses, level=l), off.align_quality([0, 1], [0, 1], poses, level=l)
        assert off.debug_row_tap_launches() == n0 + 1 and on.debug_row_tap_launches() == 0
        for k in qa:
            assert np.array_equal(qa[k], qb[k], equal_nan=True), (l, k)
    # Both tap paths ran at the coarsest level from START: most points got an intensity (waves wholly inside: the interior path, the
    # packed load), some did not (they left the image: their waves took the per-tap path). Set against a pose where neither path
    # returns anything, which gives other sums.
    q = on.align_quality([0], [0], START, level=L - 1)
    assert 0 < q["n_used"][0] < q["n_depth"][0], (q["n_used"], q["n_depth"])
    assert q["n_used"][0] * 2 > q["n_depth"][0]
    z = on.align_quality([0], [0], NOWHERE, level=L - 1)
    assert z["n_used"][0] == 0 and z["sum_w"][0] == 0.0 and q["sum_w"][0] > 0.0
    zo = off.align_quality([0], [0], NOWHERE, level=L - 1)
    assert all(np.array_equal(z[k], zo[k], equal_nan=True) for k in z)
    on.close(); off.close()


@pytest.mark.parametrize("w,h,L", SHAPES)
def test_no_stale_plane(ellc, w, h, L):
    """Align against frame slot 0, put another image into slot 0 through each writer, align again: `==` to a context whose slot 0 only
    ever received the second image (its contexts are created without any frame upload; for copy_slot the second image goes into slot 1
    and is copied into the never-written slot 0). START keeps most waves of every level on the interior path, which reads the packed
    plane alone: a plane left over from the first image would give another pose."""
    pairs = pairs_of(w, h, 2)
    second = pairs[1]["cur_image"]
    fx, fy, cx, cy = pairs[0]["intrinsics"]
    bgr = np.random.default_rng(5).integers(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8)
    start = np.tile(START, (3, 1))
    writers = {
        "upload": lambda c: c.frame_upload(0, second),
        "copy_slot": lambda c: (c.frame_upload(1, second), c.copy_slot(0, 0, 0, 1)),
        "ingest": lambda c: (c.ingest_configure(4 * w, 4 * h, 4 * fx, 4 * fy, 4 * cx, 4 * cy, None, False), c.frame_ingest_bgr(0, bgr)),
    }
    for name, wr in writers.items():
        c = context(ellc, w, h, L, pairs[:1], early_exit=0)   # slot 0 holds the first image
        first = c.align([0, 0, 0], [0, 0, 0], init_pose=start)
        wr(c)
        again = c.align([0, 0, 0], [0, 0, 0], init_pose=start)
        planes = [c.debug_get_packed_level(0, l) for l in range(L)]
        c.close()
        ref = context(ellc, w, h, L, pairs[:1], frames=False, early_exit=0)   # no frame slot written yet
        wr(ref)
        want = ref.align([0, 0, 0], [0, 0, 0], init_pose=start)
        for l in range(L):
            assert np.array_equal(planes[l], ref.debug_get_packed_level(0, l)), (name, l)
        ref.close()
        assert same(again, want), name
        assert not same(again, first), (name, "the second image changed nothing")
