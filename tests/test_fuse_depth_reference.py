"""CPU checks of tests/fuse_depth_reference.py, the numpy restatement of ellc_keyframe_fuse_depth's rule that the GPU tests hold the
kernels to: a hand-written known answer, scalar against sorted-array form on the GPU tests' scenes, max_merge 0 against the render, and
the conditions the GPU tests rely on."""
import numpy as np
import pytest

import fuse_depth_reference as FU
import render_depth_reference as R

F = np.float32
FILTERS = [(0, 0, 1.0, 1), (0.0125, 2, 0.02, 1)]
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
SHAPES = [(64, 48, 3), (23, 17, 2), (131, 67, 3)]


# 6 columns x 5 rows, fx = fy = 4, cx = cy = 2, filter (0, 0, 1, 1): every ok pixel is kept; agree_k2 = 1/2.
# Requests 0..3 have the identity: a pixel lands on itself with z' = Z, nid = 1 / Z, r = 1, nvar = V; among them the smallest Z wins a
# target, ties go to the lower request. Request 4 has t = (1/2, 0, -1) (tests/test_render_depth_reference.py): its pixel E (1,2), Z 2,
# V 1/32 lands on (2,2) with z' 1, nvar 1/2. Per target, as (x, y):
#   (1,1)  request 0: Z 2 V 1/4 alone                                                            -> merged 1
#   (2,2)  request 0: Z 4 V 1/2; E is NEARER and wins; d = 1/4 - 1, d^2 = 9/16 > (1/2)(1/2 + 1/2): the loser disagrees and is not
#          merged                                                                                 -> agree 1, merged 1
#   (3,1)  winner request 0: Z 2 V 0.3; members request 1: Z 2.5 V 0.1; request 2: Z 2.25 V 0.2; request 3: Z 3 V 0.7 — all agree
#          ((1/2 - 1/3)^2 = 1/36 <= (1/2)(0.7 + 0.3)); merged in THAT order, rounded at every step (bit patterns in hand_answer): agree 4,
#          merged 4; with max_merge 2 only requests 1 and 2: merged 3, truncated
#   (4,1)  winner request 0: Z 2 V 0; request 1: Z 2 V 0 ties, loses to the lower request, agrees (0 <= 0) and is SKIPPED: s = 0;
#          request 2: Z 2 V 1/2: s = 1/2, w = 1, id_t = 1 * 1/2 + 0 * 1/2, var_t = 1 / (inf + 2) = 0 (a zero variance on the state's side)
#                                                                                                 -> agree 3, merged 2, depth 2, var 0
#   (4,3)  winner request 0: Z 2 V 1/2; request 1: Z 4 V 0 (a zero variance on the member's side): d^2 = 1/16 <= (1/2)(1/2); s = 1/2,
#          w = 0, id_t = 0 * 1/2 + 1 * 1/4, var_t = 1 / (2 + inf) = 0                                -> agree 2, merged 2, depth 4, var 0
#   (3,3)  winner request 0: Z 2 V 1/4; request 1: Z 4 V 1/4: s = 1/2, w = 1/2, id_t = 1/4 + 1/8 = 3/8, var_t = 1 / (4 + 4)
#                                                                                                 -> agree 2, merged 2, depth 1 / (3/8), var 1/8
def hand_case():
    d = [np.zeros((5, 6), F) for _ in range(5)]
    v = [np.full((5, 6), -1, F) for _ in range(5)]
    for b, x, y, Z, V in ((0, 1, 1, 2, 0.25), (0, 2, 2, 4, 0.5), (4, 1, 2, 2, 0.03125),
                          (0, 3, 1, 2, 0.3), (1, 3, 1, 2.5, 0.1), (2, 3, 1, 2.25, 0.2), (3, 3, 1, 3, 0.7),
                          (0, 4, 1, 2, 0), (1, 4, 1, 2, 0), (2, 4, 1, 2, 0.5),
                          (0, 4, 3, 2, 0.5), (1, 4, 3, 4, 0),
                          (0, 3, 3, 2, 0.25), (1, 3, 3, 4, 0.25)):
        d[b][y, x] = Z; v[b][y, x] = V
    img0 = (10 * np.arange(5)[:, None] + np.arange(6)[None, :]).astype(np.uint8)
    imgs = [img0, img0, img0, img0, (100 + img0).astype(np.uint8)]
    Ts = np.array([IDENTITY] * 4 + [[1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, -1]], F)
    return list(zip(d, v, imgs)), (4.0, 4.0, 2.0, 2.0), Ts


def hand_p3(order):
    """Target (3,1) step by step: the winner (Z 2, V 0.3), then the members in `order`; returns (depth, var) as the rule rounds them."""
    members = {1: (F(2.5), F(0.1)), 2: (F(2.25), F(0.2)), 3: (F(3), F(0.7))}
    id_t = F(F(1) / F(2)); var_t = F(0.3)
    for b in order:
        Z, nvar = members[b]
        nid = F(F(1) / Z)
        s = F(var_t + nvar)
        w = F(nvar / s)
        id_t = F(F(w * id_t) + F(F(F(1) - w) * nid))
        var_t = F(F(1) / F(F(F(1) / var_t) + F(F(1) / nvar)))
    return F(F(1) / id_t), var_t


def hand_answer(max_merge):
    depth = np.zeros((5, 6), F); var = np.full((5, 6), -1, F)
    source = np.full((5, 6), -1, np.int32); agree = np.zeros((5, 6), np.int32); merged = np.zeros((5, 6), np.int32)
    inten = np.zeros((5, 6), np.uint8)
    # (3,1) as bit patterns, written down once: in exact arithmetic the information-weighted mean of the inverse depths 1/2, 2/5, 4/9,
    # 1/3 under the variances 0.3, 0.1, 0.2, 0.7 is 8.36508 / 19.76190 = 0.423293 (depth 2.362429, variance 1 / 19.76190 = 0.0506024);
    # of the first three 7.88889 / 18.33333 = 0.430303 (depth 2.323944, variance 0.0545455). The last bits are the rule's roundings.
    p3_bits = (0x40173209, 0x3D4F447A) if max_merge >= 3 else (0x4014BB7E, 0x3D5F6B0F)
    p3 = tuple(np.array([b], np.uint32).view(F)[0] for b in p3_bits)
    #       x  y  depth          var      source           agree merged                      intensity
    for x, y, z, nv, src, ag, mg, I in ((1, 1, F(2), F(0.25), 7, 1, 1, 11),
                                        (2, 2, F(1), F(0.5), (4 << 24) | 13, 1, 1, 121),
                                        (3, 1, p3[0], p3[1], 9, 4, 4 if max_merge >= 3 else 3, 13),
                                        (4, 1, F(2), F(0), 10, 3, 2, 14),
                                        (4, 3, F(4), F(0), 22, 2, 2, 34),
                                        (3, 3, F(F(1) / F(0.375)), F(0.125), 21, 2, 2, 33)):
        depth[y, x] = z; var[y, x] = nv; source[y, x] = src; agree[y, x] = ag; merged[y, x] = mg; inten[y, x] = I
    return dict(depth=depth, var=var, source=source, agree=agree, merged=merged, intensity=inten, n_valid=6, n_fused=4)


@pytest.mark.parametrize("fn", [FU.fuse, FU.fuse_scalar])
@pytest.mark.parametrize("max_merge", [64, 2])
def test_hand_written_answer(fn, max_merge):
    reqs, intr, Ts = hand_case()
    got = fn(reqs, intr, Ts, (0, 0, 1.0, 1), agree_k2=0.5, max_merge=max_merge)
    want = hand_answer(max_merge)
    for name in FU.PLANES:
        assert np.array_equal(got[name], want[name]), (name, got[name])
    assert FU.planes_equal(got, want)
    st = got["stats"]
    assert st["skipped"][1, 4] == 1 and st["skipped"].sum() == 1 and st["visited"][1, 4] == 2
    assert st["visited"][1, 3] == min(3, max_merge) and bool(st["truncated"][1, 3]) == (max_merge < 3) and st["truncated"].sum() == (max_merge < 3)
    assert st["segment"][2, 2] == 1 and st["render"]["stats"]["disagree"][2, 2] == 1
    # the fused depth differs from the winner's where the members pull it
    assert got["depth"][3, 3] != st["render"]["depth"][3, 3] and got["depth"][3, 4] == F(4) and got["depth"][1, 3] > F(2)


def test_the_order_shows_in_the_last_bits():
    """A condition of the hand case: merging (3,1)'s members in another order gives other bits, so the fixed order is under test. (hand_p3
    spells the steps for the permutations only; the expected answer of the case is the bit patterns in hand_answer.)"""
    want = hand_p3((1, 2, 3))
    assert (int(np.asarray(want[0], F).view(np.uint32)), int(np.asarray(want[1], F).view(np.uint32))) == (0x40173209, 0x3D4F447A)
    assert abs(float(want[0]) - 19.7619047619 / 8.3650793651) < 1e-6 and abs(float(want[1]) - 1 / 19.7619047619) < 1e-8
    others = [hand_p3(o) for o in ((3, 2, 1), (2, 1, 3), (1, 3, 2), (3, 1, 2), (2, 3, 1))]
    bits = lambda p: (int(np.asarray(p[0], F).view(np.uint32)), int(np.asarray(p[1], F).view(np.uint32)))   # noqa: E731
    assert any(bits(o) != bits(want) for o in others)
    assert all(abs(float(o[0]) - float(want[0])) < 1e-5 for o in others)   # ... the last bits only


def test_a_winner_from_request_128_and_up_is_a_winner():
    """source = (b << 24) | i as int32 is negative from request 128 on: such a target has a winner and merges like any other."""
    reqs, intr, _ = hand_case()
    empty = (np.zeros((5, 6), F), np.full((5, 6), -1, F), reqs[0][2])
    many = [empty] * 130 + reqs[:4]                    # the hand case's identity requests as requests 130 .. 133
    Ts = np.array([IDENTITY] * 134, F)
    for fn in (FU.fuse, FU.fuse_scalar):
        got = fn(many, intr, Ts, (0, 0, 1.0, 1), agree_k2=0.5)
        want = hand_answer(64)
        won = got["depth"] > 0
        assert won.sum() == 6 and got["n_valid"] == 6 and (got["source"][won] < 0).all() and (got["source"][won] != -1).all()
        assert np.array_equal((got["source"][won].astype(np.int64) & 0xffffffff) >> 24, np.full(6, 130))
        assert got["merged"][1, 3] == 4 and got["merged"][3, 3] == 2 and got["merged"][2, 2] == 1 and got["n_fused"] == 4
        for name in ("depth", "var", "merged"):        # (2,2) is won by request 0 here (E is not among the requests): not compared
            keep = np.ones((5, 6), bool); keep[2, 2] = False
            assert np.array_equal(got[name][keep].view(np.uint32), want[name][keep].view(np.uint32)), name


def scene_requests(w, h, pick=(0, 1, 2), T_of=(0, 1, 2)):
    """Scenes 11, 12, 13 of the GPU tests as level-0 requests (the CPU side has no pyramid kernels: level 0 only)."""
    scenes = [R.make_scene(w, h, seed) for seed in (11, 12, 13)]
    m = float(np.median(scenes[0]["depth0"][scenes[0]["depth0"] > 0]))
    reqs = [(scenes[k]["depth0"], scenes[k]["var0"], scenes[k]["kf_image"]) for k in pick]
    return reqs, R.level_intrinsics(*scenes[0]["intrinsics"], 0), R.scene_transforms(m)[list(T_of)]


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("flt", FILTERS, ids=["all", "filtered"])
@pytest.mark.parametrize("max_merge", [64, 1])
def test_scalar_equals_sorted_arrays(shape, flt, max_merge):
    for pick, T_of in (((0, 1, 2), (0, 1, 2)), ((0, 1, 2, 0), (0, 1, 2, 1))):
        reqs, intr, Ts = scene_requests(*shape[:2], pick=pick, T_of=T_of)
        a = FU.fuse(reqs, intr, Ts, flt, max_merge=max_merge)
        b = FU.fuse_scalar(reqs, intr, Ts, flt, max_merge=max_merge)
        assert FU.planes_equal(a, b), FU.differing(a, b)
        for k in ("visited", "skipped", "truncated"):
            assert np.array_equal(a["stats"][k], b["stats"][k]), k
        assert a["n_fused"] == int((a["merged"] >= 2).sum()) and np.array_equal(a["merged"] > 0, a["depth"] > 0)
        assert not np.isnan(a["depth"]).any() and not np.isnan(a["var"]).any()


def test_scalar_equals_sorted_arrays_on_five_tiles():
    reqs, intr, Ts = scene_requests(*SHAPES[2][:2])
    assert FU.planes_equal(FU.fuse(reqs, intr, Ts, FILTERS[0]), FU.fuse_scalar(reqs, intr, Ts, FILTERS[0]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_max_merge_zero_is_the_render(shape):
    reqs, intr, Ts = scene_requests(*shape[:2])
    for flt in FILTERS:
        a = FU.fuse(reqs, intr, Ts, flt, max_merge=0)
        r = R.render(reqs, intr, Ts, flt)
        assert R.planes_equal(a, r) and a["n_fused"] == 0 and np.array_equal(a["merged"], (r["source"] >= 0).astype(np.int32))
        # and whatever max_merge is, what the render decides stays the render's
        b = FU.fuse(reqs, intr, Ts, flt, max_merge=64)
        for name in ("source", "agree", "intensity"):
            assert np.array_equal(b[name], r[name]), name
        one = b["merged"] == 1
        assert np.array_equal(b["depth"][one].view(np.uint32), r["depth"][one].view(np.uint32))
        assert np.array_equal(b["var"][one].view(np.uint32), r["var"][one].view(np.uint32))


# the conditions tests/test_gpu_fuse_depth.py asserts at level 0, unfiltered: (merged >= 2, merged >= 3, truncated at max_merge 1) for
# requests [0, 1, 2], and (merged >= 2, merged >= 3) for [0, 1, 2, 0] with the transforms [0, 1, 2, 1]
CONDITIONS = {(64, 48): ((620, 102, 102), (985, 469)), (131, 67): ((738, 108, 108), (1731, 414)), (23, 17): ((8, 1, 1), (56, 6))}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_scenes_reach_every_case_class(shape):
    three, four = CONDITIONS[shape[:2]]
    reqs, intr, Ts = scene_requests(*shape[:2])
    a = FU.fuse(reqs, intr, Ts, FILTERS[0], max_merge=64)
    one = FU.fuse(reqs, intr, Ts, FILTERS[0], max_merge=1)
    got = (int((a["merged"] >= 2).sum()), int((a["merged"] >= 3).sum()), int(one["stats"]["truncated"].sum()))
    print(shape, "requests [0, 1, 2]:", got)
    assert got == three
    assert (a["depth"].view(np.uint32) != a["stats"]["render"]["depth"].view(np.uint32)).sum() > 0
    assert one["merged"].max() == 2
    reqs, intr, Ts = scene_requests(*shape[:2], pick=(0, 1, 2, 0), T_of=(0, 1, 2, 1))
    b = FU.fuse(reqs, intr, Ts, FILTERS[0], max_merge=64)
    got = (int((b["merged"] >= 2).sum()), int((b["merged"] >= 3).sum()))
    print(shape, "requests [0, 1, 2, 0]:", got)
    assert got == four


def test_the_same_map_three_times_merges_everywhere():
    reqs, intr, Ts = scene_requests(64, 48, pick=(1, 1, 1), T_of=(1, 1, 1))
    a = FU.fuse(reqs, intr, Ts, FILTERS[0])
    won = a["source"] >= 0
    assert won.sum() > 100 and ((a["source"][won] >> 24) == 0).all() and (a["merged"][won] >= 3).all()
