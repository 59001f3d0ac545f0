// pf_ray.hpp -- the ray-distance factor of planar-depth tiles (pf_set_tile_depth), host side: the
// per-tile column / row tables and the --tile-depth / PF_TILE_DEPTH value parser.  No HIP include:
// the library's host units, the facade, panofuse_main and tests/cpp/ray_check.cpp all use it.
//
// A perspective depth network predicts depth along the optical axis; the panorama holds distance
// from the camera centre.  On SetWindow's plane at unit distance (Depth.cpp:120-155) tile pixel
// (x, y) in [0,1]^2 sits at pos = corner0 + x hedge + y vedge, and the two depths differ by
//   k = |pos| = sqrt(1 + (tx (1 - 2x))^2 + (ty (2y - 1))^2),  tx = tan(daz / 2), ty = tan(dzen / 2).
// The tables hold the two squared terms per pixel column i (x = i / (w-1), the inverse of Value()'s
// truncating index, Depth.cpp:111-118) and row j, in fp64 from the fp32 window.  The factor has one
// definition everywhere: kf(i, j) = (float)sqrt(1.0 + cu[i] + rv[j]), fp64 adds and sqrt (correctly
// rounded on host and device alike), rounded once to fp32.
#pragma once
#include <cmath>
#include <cstring>

namespace pf {

// cu[w], rv[h] of one tile with viewing window (az_left, az_right, zen_top, zen_down).  An axis of
// one pixel has no extent: its term is 0.
inline void ray_tables(float az_left, float az_right, float zen_top, float zen_down, int w, int h,
                       double* cu, double* rv)
{
    const double tx = tan((double)fabsf(az_right - az_left) / 2);
    const double ty = tan((double)fabsf(zen_top - zen_down) / 2);
    for (int i = 0; i < w; i++) {
        const double u = w > 1 ? tx * (1 - 2 * (double)i / (double)(w - 1)) : 0.0;
        cu[i] = u * u;
    }
    for (int j = 0; j < h; j++) {
        const double v = h > 1 ? ty * (2 * (double)j / (double)(h - 1) - 1) : 0.0;
        rv[j] = v * v;
    }
}

inline float ray_factor(double cu, double rv) { return (float)sqrt(1.0 + cu + rv); }

// "ray" -> 0 (PF_TILE_DEPTH_RAY), "planar" -> 1 (PF_TILE_DEPTH_PLANAR), anything else
// (NULL included) -> -1.
inline int parse_tile_depth(const char* s)
{
    if (!s) return -1;
    if (!strcmp(s, "ray")) return 0;
    if (!strcmp(s, "planar")) return 1;
    return -1;
}

}  // namespace pf
