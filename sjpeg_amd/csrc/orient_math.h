// orient_math.h -- the eight EXIF orientations (tag 0x0112, values 1..8) of the oriented ragged calls
// (sjpeg_hip_orient_ragged_src, resize.hip), stated once for the kernel, the planner and the host.  R is the picture
// as it is stored, w x h; U the upright one, w x h for o in 1..4 and h x w for o in 5..8, with U(x, y) = R(sx, sy):
//     o  meaning                              sx         sy
//     1  as stored                            x          y
//     2  mirrored left-right                  w - 1 - x  y
//     3  rotated 180                          w - 1 - x  h - 1 - y
//     4  mirrored top-bottom                  x          h - 1 - y
//     5  transposed                           y          x
//     6  rotated 90 clockwise to show         y          h - 1 - x
//     7  transverse                           w - 1 - y  h - 1 - x
//     8  rotated 90 counter-clockwise         w - 1 - y  x
// Plain C++ (a host compiler reads it as it is: tests/cxx/orient_math_test.cc).
#ifndef SJPEG_AMD_ORIENT_MATH_H_
#define SJPEG_AMD_ORIENT_MATH_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define SJPEG_ORIENT_HD __host__ __device__
#else
#define SJPEG_ORIENT_HD
#endif

namespace sjpeg_internal {

// a destination row of U is a column of R
SJPEG_ORIENT_HD inline bool orient_transposes(int o) { return o >= 5; }

// the size of U for a stored picture of w x h
SJPEG_ORIENT_HD inline void oriented_size(uint32_t w, uint32_t h, int o, uint32_t* ow, uint32_t* oh) {
  *ow = orient_transposes(o) ? h : w;
  *oh = orient_transposes(o) ? w : h;
}

// the stored position (sx, sy) of the upright sample (x, y); w x h is the STORED picture's size
SJPEG_ORIENT_HD inline void orient_source(uint32_t x, uint32_t y, uint32_t w, uint32_t h, int o, uint32_t* sx, uint32_t* sy) {
  switch (o) {
    default: *sx = x; *sy = y; break;
    case 2: *sx = w - 1u - x; *sy = y; break;
    case 3: *sx = w - 1u - x; *sy = h - 1u - y; break;
    case 4: *sx = x; *sy = h - 1u - y; break;
    case 5: *sx = y; *sy = x; break;
    case 6: *sx = y; *sy = h - 1u - x; break;
    case 7: *sx = w - 1u - y; *sy = h - 1u - x; break;
    case 8: *sx = w - 1u - y; *sy = x; break;
  }
}

// ... and its inverse: the upright position (x, y) of the stored sample (sx, sy)
SJPEG_ORIENT_HD inline void orient_upright(uint32_t sx, uint32_t sy, uint32_t w, uint32_t h, int o, uint32_t* x, uint32_t* y) {
  switch (o) {
    default: *x = sx; *y = sy; break;
    case 2: *x = w - 1u - sx; *y = sy; break;
    case 3: *x = w - 1u - sx; *y = h - 1u - sy; break;
    case 4: *x = sx; *y = h - 1u - sy; break;
    case 5: *x = sy; *y = sx; break;
    case 6: *x = h - 1u - sy; *y = sx; break;
    case 7: *x = h - 1u - sy; *y = w - 1u - sx; break;
    case 8: *x = sy; *y = w - 1u - sx; break;
  }
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_ORIENT_MATH_H_
