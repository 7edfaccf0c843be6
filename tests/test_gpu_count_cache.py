"""The compaction's count launch is left out while the tile counts a slot holds are current (ellc_ctx::kf_counts_ok).

prep_count reads every level's depth plane of every keyframe a group rebuilds and leaves one integer per tile of 2048 pixels; those
integers depend on the depth planes alone. A group whose rebuilt slots have all been counted since their depth planes were last
written launches prep_scatter alone, which reads the kept counts exactly as it reads fresh ones. Against a context that counts in
every call (ellc_debug_set_count_cache(0), the behaviour up to r06) not a bit may differ, and the two counters of
ellc_debug_count_cache_counters say which groups counted."""
import numpy as np
import pytest
from egomotion_with_local_loop_closures_amd import synth

pytestmark = pytest.mark.gpu
W, H, L = 160, 120, 3


def same(ra, rb):
    return all(np.array_equal(x, y) for x, y in zip(ra, rb))


def problem(ellc, pairs, **kw):
    """pairs[i] resident in keyframe slot i / frame slot i (helpers.gpu_problem, but with max_batch as given: gpu_problem raises it
    to the number of pairs, and a batch smaller than max_batch never shares a launch group)"""
    fx, fy, cx, cy = pairs[0]["intrinsics"]
    ctx = ellc.Context(ellc.default_config(W, H, L, fx=fx, fy=fy, cx=cx, cy=cy, **kw), diag=True)
    for i, p in enumerate(pairs):
        ctx.keyframe_upload(i, p["kf_image"])
        ctx.keyframe_set_depth(i, p["depth0"], p["var0"])
        ctx.frame_upload(i, p["cur_image"])
    return ctx


def contexts(ellc, pairs, arith, **kw):
    """a keeps the counts, b counts in every call; same uploads, same weights"""
    kw = dict(dict(max_iter=(3, 4, 5), max_keyframes=4, max_frames=4), **kw)
    if arith == "fast":
        kw["arith"] = ellc.ARITH_FAST
    a = problem(ellc, pairs, **kw)
    b = problem(ellc, pairs, **kw)
    b.debug_set_count_cache(False)
    for ctx in (a, b):
        for s in range(len(pairs)):
            for l in range(L):
                ctx.keyframe_set_weights(s, l, np.full((H >> l, W >> l), 0.03, np.float32), 1)
    return a, b


# FCA in both arithmetic modes, ICA in the tolerance mode (its compaction is prep_scatter<20> / <16>); early exit on makes calls of
# one or two alignments tracking-shaped: launched kernel by kernel, compacted in the count-free form (PrepArgs::lb_tag), which
# stores tagged words where the counts were — and makes the context a tracking context, whose export builds eager lists
@pytest.mark.parametrize("early_exit", [0, 1])
@pytest.mark.parametrize("mode,arith", [(0, "fast"), (0, "exact"), (1, "fast")])
def test_count_cache_changes_no_bit_and_every_writer_invalidates_it(ellc, mode, arith, early_exit):
    pairs = [synth.make_pair(W, H, seed=500 + i, rot=0.004, trans=0.012) for i in range(3)]
    a, b = contexts(ellc, pairs, arith, early_exit=early_exit, max_batch=3)
    src, _ = contexts(ellc, pairs, arith, early_exit=early_exit, max_batch=3)   # the other context of copy_slot_across
    _.close()
    st = synth.make_depth_state(W, H, 7, pairs[1]["kf_image"], pairs[1]["idepth_true"])
    rng = np.random.default_rng(4)
    planes = [rng.uniform(0.01, 0.06, size=(H >> l, W >> l)).astype(np.float32) for l in range(L)]
    batch = [0, 1, 2]   # three alignments: never the state-driven schedule, always a captured launch group

    def check(what, must_count):
        """must_count: the first call's group holds a slot whose counts are stale or overwritten (the others are current: a mixed
        group); it has to launch a count. The repeated calls on unchanged slots launch none."""
        for rep in range(3):
            c0 = a.debug_count_cache_counters()
            ra = a.align(batch, batch, mode=mode)
            rb = b.align(batch, batch, mode=mode)
            c1 = a.debug_count_cache_counters()
            assert same(ra, rb), (what, rep)
            assert c1[0] + c1[1] == c0[0] + c0[1] + 1, (what, rep, c0, c1)   # one group, in one of the two counters
            if rep == 0 and must_count:
                assert c1[0] == c0[0] + 1, (what, "the first call after the writer launched no count", c0, c1)
            if rep > 0:
                assert c1[1] == c0[1] + 1, (what, rep, "a repeated call on unchanged slots launched a count", c0, c1)
        ra, rb = a.align([2, 0, 1], [0, 1, 2], mode=mode), b.align([2, 0, 1], [0, 1, 2], mode=mode)   # another order and pairing, current slots
        assert same(ra, rb), (what, "another pairing")

    check("initial", True)

    def tracked(c):
        c.depth_set_keyframe(1); c.depth_set_state(st); c.depth_regularize(False)
        c.track_frame(1, save_weights=True)

    # In a tracking context the export builds the FCA lists of its keyframe behind itself (eager lists, count-free form: tagged words
    # in the slot's tile counts). An FCA group then reads those lists and does not rebuild the slot at all - its other slots are
    # current, it needs no count; an ICA group rebuilds the slot and has to count.
    after_export = not (early_exit and mode == 0)
    # (name, the first group afterwards has to launch a count, call). Every writer of the two lists this file is modelled on
    # (test_record_cache_is_invalidated_by_every_writer, test_hinv_cache_changes_no_bit), the copy across contexts, and the
    # tracking-shaped calls
    writers = [
        ("keyframe_set_depth", True, lambda c: c.keyframe_set_depth(0, pairs[2]["depth0"], pairs[2]["var0"])),
        ("keyframe_set_depth_level", True, lambda c: c.keyframe_set_depth_level(1, 1, *[x.copy() for x in c.keyframe_depth_level(0, 1)])),
        ("keyframe_set_weights", False, lambda c: [c.keyframe_set_weights(0, l, planes[l], 2) for l in range(L)]),
        ("keyframe_finalise_weights", False, lambda c: c.keyframe_finalise_weights(0)),
        ("keyframe_upload + depth", True, lambda c: (c.keyframe_upload(1, pairs[2]["kf_image"]), c.keyframe_set_depth(1, pairs[2]["depth0"], pairs[2]["var0"]),
                                                    [c.keyframe_set_weights(1, l, planes[l], 1) for l in range(L)])),
        ("copy_slot", True, lambda c: c.copy_slot(1, 0, 1, 2)),
        ("copy_slot_across", True, lambda c: ellc.copy_slot_across(c, 1, 2, src, 1, 0)),
        ("keyframe_from_frame + depth", True, lambda c: (c.keyframe_from_frame(1, 2), c.keyframe_set_depth(1, pairs[0]["depth0"], pairs[0]["var0"]),
                                                        [c.keyframe_set_weights(1, l, planes[l], 1) for l in range(L)])),
        ("depth map -> update_depth_image", after_export, lambda c: (c.depth_set_keyframe(1), c.depth_set_state(st), c.depth_regularize(False),
                                                            c.depth_update_depth_image())),
        ("saved weights (FCA)", False, lambda c: c.align([0, 1], [1, 0], mode=0, save_weights=True)),
        ("single-step API", False, lambda c: c.gn_iterate(0, 1, 1, np.zeros(6, np.float32))),
        # at most two alignments: with early exit on, the count-free form stores tagged words over the slot's counts
        ("tracking-shaped call, one alignment", bool(early_exit), lambda c: c.align([0], [0], mode=0)),
        ("tracking-shaped call, two alignments", bool(early_exit), lambda c: c.align([2, 2], [0, 1], mode=0)),
        ("tracking-shaped call, two keyframes", bool(early_exit), lambda c: c.align([0, 1], [0, 1], mode=0)),
        ("update_depth_image again (eager lists in a tracking context)", after_export, lambda c: c.depth_update_depth_image()),
    ]
    if early_exit:   # a tracking context: the tracked frame's alignment (count-free form) and the fused export behind it
        writers.insert(-1, ("tracked frame (alignment + the export behind it)", after_export, tracked))
    for name, must_count, fn in writers:
        fn(a); fn(b)
        check(name, must_count)
    assert b.debug_count_cache_counters()[1] == 0   # the context that was told to count always did
    a.close(); b.close(); src.close()


@pytest.mark.parametrize("mode,arith", [(0, "fast"), (0, "exact"), (1, "fast")])
def test_count_cache_with_groups_in_flight(ellc, mode, arith):
    """Coalesced groups in flight over disjoint and over shared keyframe slots, with writers between the rounds: the pipelined context
    keeps the counts, the reference context counts in every call and runs every batch synchronously."""
    pairs = [synth.make_pair(W, H, seed=400 + i, rot=0.004, trans=0.012) for i in range(4)]
    a, b = contexts(ellc, pairs, arith, early_exit=0, max_batch=2, concurrent_batches=8, coalesce=2)
    disjoint = [np.array(x, np.int32) for x in ([0, 1], [2, 3], [0, 1], [2, 3], [2, 3], [0, 1], [0, 1], [2, 3])]
    shared = [np.array(x, np.int32) for x in ([0, 1], [1, 2], [2, 3], [3, 0], [1, 2], [0, 1], [3, 0], [2, 3])]

    def round_(what, batches):
        c0 = a.debug_count_cache_counters()
        for q in batches:
            a.align_enqueue(q, q, mode=mode)
        for i, q in enumerate(batches):
            got = a.align_fetch(2)
            assert same(got, b.align(q, q, mode=mode)), (what, i)
        c1 = a.debug_count_cache_counters()
        assert c1[0] + c1[1] == c0[0] + c0[1] + len(batches) // 2, (what, c0, c1)   # groups of two batches side by side
        return c1[0] - c0[0], c1[1] - c0[1]

    assert round_("disjoint, first", disjoint) == (1, 3)   # the first group holds all four slots and counts them; the others find them counted
    assert round_("disjoint, repeated", disjoint) == (0, 4)
    assert round_("shared, repeated", shared) == (0, 4)
    for ctx in (a, b):
        ctx.keyframe_set_depth(2, pairs[0]["depth0"], pairs[0]["var0"])
    assert round_("shared, after a depth writer", shared) == (1, 3)   # the first group holds slot 2 and counts; the later ones find it counted
    assert round_("shared, repeated again", shared) == (0, 4)
    for ctx in (a, b):
        ctx.keyframe_set_depth_level(3, 0, *[x.copy() for x in ctx.keyframe_depth_level(1, 0)])
    # a partial batch between full ones: a group of its own, one slot stale (3) in the last group only
    for q in (shared[0], shared[1][:1], shared[2]):
        a.align_enqueue(q, q, mode=mode)
    for q in (shared[0], shared[1][:1], shared[2]):
        assert same(a.align_fetch(len(q)), b.align(q, q, mode=mode)), "partial batch between full ones"
    assert round_("disjoint, at the end", disjoint) == (0, 4)
    assert b.debug_count_cache_counters()[1] == 0
    a.close(); b.close()
