"""Shapes and seeded inputs of the image-side tests (tests/test_image_reference.py on the CPU, tests/test_gpu_image_shapes.py on the
GPU): the smallest shapes that reach every split of the pyramid into chains of up to three pyrDown steps (L = 1 .. 8), thin levels,
levels that are odd at every depth, and the partial tiles of the max-gradient, histogram, upload-copy and row-packing kernels."""
import functools
import numpy as np
from egomotion_with_local_loop_closures_amd import synth
import image_reference as R

# (w, h, L): stored sizes follow the ceil rule; the coarsest iterated level is 4 in at least one axis everywhere except L = 1, 2
SHAPES = [
    (16, 16, 1),     # the smallest context; no pyramid launch; one partial 32 x 8 max-gradient tile column
    (23, 17, 1),     # 391 pixels: 391 mod 256, 391 mod 16 != 0 (histogram, upload copy); height 8k + 1
    (19, 16, 2),     # 1-step chain; stored 10 x 8, iterated 9 x 8
    (18, 17, 3),     # 2-step chain, every level odd, coarsest stored 5 x 5 / iterated 4 x 4
    (512, 16, 3),    # coarsest 128 x 4: one row of blocks, the halo taller than the level
    (16, 512, 3),    # the same, transposed
    (33, 32, 4),     # width 32k + 1; 3-step chain, coarsest 5 x 4
    (35, 33, 4),     # 3-step chain, every level odd in both axes (35 18 9 5, 33 17 9 5)
    (67, 64, 5),     # 3 + 1: a second chain of one step whose source is level 3 (9 x 8 -> 5 x 4)
    (131, 128, 6),   # 3 + 2
    (260, 257, 7),   # 3 + 3
    (517, 515, 8),   # 3 + 3 + 1, all eight levels, odd sources at most levels, coarsest stored 5 x 5
    (512, 512, 8),   # 3 + 3 + 1 with exact halving; stored = iterated at every level; coarsest 4 x 4
]
SHAPE_IDS = ["%dx%d-L%d" % s for s in SHAPES]
IMAGE_KINDS = ("random_blocks", "texture", "checkerboard")
DEPTH_CASES = ("semi_dense", "full_interior", "dense")
BAND = 3   # the depth map's empty outer band (util::XMIN .. YMAX)


def make_image(w, h, kind, seed):
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    if kind == "random_blocks":      # uniform bytes, a block of 255 in a corner (saturation meets REFLECT_101) and a block of 0
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        bh, bw = max(2, h // 3), max(2, w // 3)
        img[:bh, :bw] = 255
        img[h - 1 - bh:h - 1, w - 1 - bw:w - 1] = 0
        return img
    if kind == "texture":            # the image of tests/test_gpu_image.py: value noise with isolated 255 / 0 pixels
        img = synth.value_noise_texture(w, h, rng)
        img[::17, ::13] = 255
        img[5::19, 3::11] = 0
        return img
    if kind == "checkerboard":       # period 1: the worst case for the rounding and for REFLECT_101's parity; seed picks the phase
        yy, xx = np.mgrid[0:h, 0:w]
        return (((xx + yy + seed) & 1) * 255).astype(np.uint8)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def image(w, h, kind, seed=0):
    img = make_image(w, h, kind, seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(w, h, levels, kind, seed=0):
    """everything tests compare of one image, computed once: dict(levels=[stored planes], dims=[((sw, sh), (cols, rows))],
    grad=[(gx, gy)], maxgrad=(map, count), hist, packed=[planes])"""
    img = image(w, h, kind, seed)
    pyr = R.pyramid(img, levels)
    dims = [R.level_dims(w, h, l) for l in range(levels)]
    out = dict(levels=pyr, dims=dims,
               grad=[R.gradient(pyr[l], dims[l][1][1], dims[l][1][0]) for l in range(levels)],
               maxgrad=R.max_gradient(img), hist=R.histogram(img),
               packed=[R.packed_rows(pyr[l], dims[l][1][1]) for l in range(levels)])
    for v in pyr + out["packed"] + [a for g in out["grad"] for a in g] + [out["maxgrad"][0], out["hist"]]:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def depth_planes(w, h, case, seed=0):
    """Level-0 depth / variance planes in the upload's convention (depth 0 / variance -1 = none): depth in [0.5, 2], variance in
    [0.005, 0.02]. semi_dense: about a third of the pixels inside the empty three-pixel band; full_interior: at least nine tenths of
    them; dense: no band, at least nine tenths of the WHOLE plane (the upload then also writes the dense slots' reciprocal planes).
    Five level-1 cells are then given 0, 1, 2, 3 and 4 valid children on purpose (chosen among the cells whose four children, in the
    reference's flat addressing with stride 2 * (w >> 1), all lie inside the band)."""
    rng = np.random.default_rng(77 + 1000 * seed + 13 * w + h + 100000 * DEPTH_CASES.index(case))
    depth = rng.uniform(0.5, 2.0, (h, w)).astype(np.float32)
    var = rng.uniform(0.005, 0.02, (h, w)).astype(np.float32)
    inside = np.ones((h, w), bool)
    if case != "dense":
        inside[:BAND] = inside[-BAND:] = False
        inside[:, :BAND] = inside[:, -BAND:] = False
    # (the five cells below take up to ten pixels out: random holes only as far as nine tenths stay valid with a margin)
    holes = 0.65 if case == "semi_dense" else min(0.04, 0.5 * max(0.0, 0.1 - 10.0 / inside.sum()))
    valid = (rng.random((h, w)) >= holes) & inside
    w1, h1 = w >> 1, h >> 1
    yy, xx = np.mgrid[0:h1, 0:w1]
    base = 2 * (xx + yy * 2 * w1)
    kids = np.stack([base, base + 1, base + 2 * w1, base + 2 * w1 + 1], -1).reshape(-1, 4)     # flat indices into the level-0 plane
    cand = kids[inside.ravel()[kids].all(axis=1)]
    pick = cand[rng.choice(len(cand), 5, replace=False)]
    flat = valid.ravel().copy()
    for n, cell in enumerate(pick):
        flat[cell] = False
        flat[cell[rng.permutation(4)[:n]]] = True
    valid = flat.reshape(h, w)
    d0 = np.where(valid, depth, np.float32(0.0)).astype(np.float32)
    v0 = np.where(valid, var, np.float32(-1.0)).astype(np.float32)
    d0.setflags(write=False); v0.setflags(write=False)
    return d0, v0


@functools.lru_cache(maxsize=None)
def depth_reference(w, h, levels, case, seed=0):
    d0, v0 = depth_planes(w, h, case, seed)
    return R.depth_pyramid(d0, v0, w, h, levels)
