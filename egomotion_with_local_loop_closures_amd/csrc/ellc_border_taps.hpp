// Where a 4 x 4 neighbourhood with CLAMPED indices lies in the row-packed frame plane (FrLevelDev::img4: word (y, x) holds column x
// of rows y - 1 .. y + 2 in bytes 0 .. 3): the index rule of the tolerance mode's border taps (tap_request_f / tap_finish_f).
// The samples the general taps read for a floor position (x0, y0) are img[clamp(y0 + i, 0, rows - 1)][clamp(x0 + j, 0, cols - 1)],
// i, j = -1 .. 2. With the window origin clamped into the image, xw = clamp(x0, 1, cols - 3) and yw = clamp(y0, 1, rows - 3), the
// 16-byte load of words (yw, xw - 1 .. xw + 2) holds columns xw - 1 .. xw + 2 of rows yw - 1 .. yw + 2, all inside the image, and
// sample (i, j) is byte clamp(y0 + i, 0, rows - 1) - (yw - 1) of word clamp(x0 + j, 0, cols - 1) - (xw - 1). Along one axis of n
// >= 4 positions, with d = v0 - clamp(v0, 1, n - 3): that index is clamp(d + k + 1, 0, 3) for k = -1 .. 2 (d = 0: the identity 0 1
// 2 3; d < 0: the low border, index 0 repeated; d > 0: the high border, index 3 repeated), and it stops changing at |d| = 3, so v0
// is limited to [-2, n] first (for the clamped indices, and for the border tests "v <= 0 or v >= n - 1" of the gradient scales, the
// same as the general taps' [-4, n + 3]).
// Usable from host and device code; tests/test_host_border_taps.py checks it exhaustively on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ELLC_BT_HD __host__ __device__ __forceinline__
#else
#define ELLC_BT_HD inline
#endif

namespace ellc {

ELLC_BT_HD int border_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The floor position along an axis of n positions, limited to where its clamped neighbourhood stops changing
ELLC_BT_HD int border_limit(int v0, int n) { return border_clampi(v0, -2, n); }
// The window origin along that axis (n >= 4)
ELLC_BT_HD int border_origin(int v0, int n) { return border_clampi(v0, 1, n - 3); }

// The four indices clamp(d + k + 1, 0, 3), k = -1 .. 2, in bytes 0 .. 3, for d = border_limit(v0, n) - border_origin(v0, n) in
// [-3, 3]: four bytes out of the twelve 0 0 0 0 | 0 1 2 3 | 3 3 3 3, starting at byte 4 + d. As a selector of v_perm_b32 it puts
// the clamped rows y0 - 1 .. y0 + 2 of a loaded word into its bytes 0 .. 3.
ELLC_BT_HD uint32_t border_select(int d) {
  const uint32_t hi = d < 0 ? 0x03020100u : 0x03030303u, lo = d < 0 ? 0u : 0x03020100u;
  const uint32_t sh = (uint32_t)d & 3u;   // d < 0: 4 + d
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * sh));
#endif
}
ELLC_BT_HD uint32_t border_select_of(int v0, int n) { return border_select(border_limit(v0, n) - border_origin(v0, n)); }

// Bytes sel[0] .. sel[3] of w in bytes 0 .. 3 (v_perm_b32 with both sources w)
ELLC_BT_HD uint32_t border_pick_rows(uint32_t w, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(w, w, sel);
#else
  uint32_t o = 0;
  for (int k = 0; k < 4; k++) o |= ((w >> (8u * ((sel >> (8 * k)) & 3u))) & 0xffu) << (8 * k);
  return o;
#endif
}

// The word of column offset J (-1 .. 2) among the four loaded ones (wk: column xw - 1 + k): w[clamp(d + J + 1, 0, 3)], as selects
template <int J>
ELLC_BT_HD uint32_t border_pick_column(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int d) {
  return d >= 2 - J ? w3 : (d >= 1 - J ? w2 : (d >= -J ? w1 : w0));
}

// The 2 x 2 neighbourhood of the intensity tap alone (the constant-weight path), clamped: rows clamp(y0), clamp(y0 + 1) of columns
// clamp(x0), clamp(x0 + 1). It lies in the two words (yw, xw), (yw, xw + 1) at yw = clamp(y0, 0, rows - 1), xw = clamp(x0, 0, cols - 2)
// (cols >= 2): row clamp(y0) = yw is byte 1 of a word; row clamp(y0 + 1) is byte 2 where y0 is in [0, rows - 2] and byte 1 (the same
// row) otherwise, so the zero byte of a row outside the image is never taken; column clamp(x0) is the first word but for
// x0 >= cols - 1, column clamp(x0 + 1) the second but for x0 < 0.
ELLC_BT_HD int pair_origin_col(int x0, int cols) { return border_clampi(x0, 0, cols - 2); }
ELLC_BT_HD int pair_origin_row(int y0, int rows) { return border_clampi(y0, 0, rows - 1); }
ELLC_BT_HD uint32_t pair_pick_left(uint32_t w0, uint32_t w1, int x0, int cols) { return x0 >= cols - 1 ? w1 : w0; }
ELLC_BT_HD uint32_t pair_pick_right(uint32_t w0, uint32_t w1, int x0) { return x0 < 0 ? w0 : w1; }
ELLC_BT_HD bool pair_two_rows(int y0, int rows) { return (y0 >= 0) & (y0 <= rows - 2); }

}  // namespace ellc
