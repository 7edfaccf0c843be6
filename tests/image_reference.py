"""PLAIN REFERENCE of the image side (test infrastructure): what a slot holds after an upload, as a function of the image alone.

A numpy / scipy restatement, int64 and float32, of

    frame::constructImagePyramids (cv::pyrDown, CV_8UC1)   Frame.cpp:170-182
    frame::calculateGradient                               Frame.cpp:185-285
    frame::buildMaxGradients                               Frame.cpp:618-674
    globalOptimize::calculateImageHistogram (cv::calcHist) GlobalOptimize.cpp:68
    depthMap::buildInvVarDepth / mapDepthArr2Mat           DepthPropagation.cpp:1637-1746

and of the row-packed plane of a frame slot (FrLevelDev::img4, the project's own layout: no reference text), written FROM THE
OPERATIONS' DEFINITIONS AND THE REFERENCE'S TEXT, WITHOUT looking at oracle/ellc_oracle_core.cpp or at the HIP kernels: the C++ oracle
and the kernels are one author's reading of those lines. tests/test_image_reference.py pins this module by known answers and holds the
oracle to it; tests/test_gpu_image_shapes.py holds the kernels to it. Every result is integer or exact f32 arithmetic, so every
comparison against it is bit for bit.

cv::pyrDown on CV_8UC1 is documented as: convolve with the separable kernel [1 4 6 4 1] / 16 per axis under BORDER_REFLECT_101
(gfedcb|abcdefgh|gfedcba), keep the even rows and columns, destination ((w + 1) / 2, (h + 1) / 2); its 8-bit path accumulates integers
and rounds once, (sum + 128) >> 8. The reference has four levels (MAX_PYRAMID_LEVEL); for other level counts the same step continues.

Taken as given: the level-0 depth / variance planes a caller uploads, the intrinsics, and everything behind the planes (taps,
compaction, Gauss-Newton sums: tests/second_source_gn.py; the depth map's stages: tests/second_source_depth.py)."""
import numpy as np
from scipy import ndimage

from second_source_depth import calculate_gradient, inv_var_depth_level

F = np.float32
PYR_KERNEL = np.array([1, 4, 6, 4, 1], np.int64)
MIN_ABS_GRAD_DECREASE = F(5.0)             # ExternVariable.h


def pyr_down(img):
    """cv::pyrDown on CV_8UC1. scipy's mode="mirror" is BORDER_REFLECT_101: (d c b | a b c d | c b a), the edge sample not repeated."""
    a = np.asarray(img, np.uint8).astype(np.int64)
    hs = ndimage.correlate1d(a, PYR_KERNEL, axis=1, mode="mirror")
    vs = ndimage.correlate1d(hs, PYR_KERNEL, axis=0, mode="mirror")
    return ((vs[::2, ::2] + 128) >> 8).astype(np.uint8)


def pyr_down_padded(img):
    """The same operation through np.pad(mode="reflect") and shifted sums (the formulation of tests/test_oracle_image_gn.py): a second
    way to the same numbers, kept to hold pyr_down to it."""
    a = np.asarray(img, np.uint8).astype(np.int64)
    h, w = a.shape
    pad = np.pad(a, 2, mode="reflect")
    hs = sum(PYR_KERNEL[i] * pad[:, i:i + w] for i in range(5))
    vs = sum(PYR_KERNEL[i] * hs[i:i + h, :] for i in range(5))
    return ((vs[::2, ::2] + 128) >> 8).astype(np.uint8)


def level_dims(w, h, l):
    """((stored w, stored h), (iterated w, iterated h)) of level l: a stored plane follows pyrDown's ceil rule step by step, the loops
    over a level run over ORIG >> l (truncation)."""
    sw, sh = w, h
    for _ in range(l):
        sw, sh = (sw + 1) // 2, (sh + 1) // 2
    return (sw, sh), (w >> l, h >> l)


def pyramid(img, levels):
    """the stored planes of levels 0 .. levels - 1"""
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(1, levels):
        out.append(pyr_down(out[-1]))
    return out


def gradient(level_img, rows, cols):
    """frame::calculateGradient over the iterated region (currentRows x currentCols) of a stored level plane"""
    return calculate_gradient(np.asarray(level_img, np.uint8)[:rows, :cols])


def max_gradient(img):
    """frame::buildMaxGradients at level 0: (map, number of interior pixels >= MIN_ABS_GRAD_DECREASE). Magnitude sqrt(gx*gx + gy*gy)
    in f32 (multiply, multiply, add, sqrt: each rounded), vertical 3-maximum of rows 1 .. h - 2 into a zeroed buffer, horizontal
    3-maximum of that buffer for the interior; border pixels keep the raw magnitude."""
    gx, gy = calculate_gradient(np.asarray(img, np.uint8))
    mag = np.sqrt((gx * gx + gy * gy).astype(np.float32)).astype(np.float32)
    tmp = np.zeros_like(mag)
    tmp[1:-1, :] = np.maximum(np.maximum(mag[1:-1, :], mag[:-2, :]), mag[2:, :])
    out = mag.copy()
    out[1:-1, 1:-1] = np.maximum(np.maximum(tmp[1:-1, :-2], tmp[1:-1, 1:-1]), tmp[1:-1, 2:])
    return out, int((out[1:-1, 1:-1] >= MIN_ABS_GRAD_DECREASE).sum())


def histogram(img):
    """256 uniform bins over [0, 256), divided by their sum as an f32 (the sum itself is exact)"""
    c = np.bincount(np.asarray(img, np.uint8).ravel(), minlength=256).astype(np.float32)
    return c / np.float32(c.sum(dtype=np.float64))


def packed_rows(level_img, rows):
    """word (y, x) = I(y-1,x) | I(y,x) << 8 | I(y+1,x) << 16 | I(y+2,x) << 24 of the stored level image, rows outside
    [0, rows) contributing a zero byte"""
    sh, sw = level_img.shape
    pad = np.zeros((sh + 3, sw), np.uint32)
    pad[1:1 + rows] = level_img[:rows]
    return pad[0:sh] | (pad[1:sh + 1] << 8) | (pad[2:sh + 2] << 16) | (pad[3:sh + 3] << 24)


def depth_pyramid(depth0, var0, w, h, levels):
    """buildInvVarDepth + mapDepthArr2Mat from level-0 planes in the upload's convention (depth 0 = none, variance -1 = none). Returns a
    list over the levels of (depth, variance, valid children per cell); level 0 is the input (children: None). A pixel counts by its
    variance alone (> 0), so level 0's "no depth" value is never read."""
    out = [(np.asarray(depth0, np.float32).reshape(h, w), np.asarray(var0, np.float32).reshape(h, w), None)]
    for l in range(1, levels):
        out.append(inv_var_depth_level(out[-1][0], out[-1][1], w >> l, h >> l))
    return out
