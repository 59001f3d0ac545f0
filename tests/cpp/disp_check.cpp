// disp_check.cpp -- a caller of the facade's disparity-tile entry points (include/pf_depth.h),
// for tests/test_gpu_disp_cli.py: per tile SolveDisparityToDepth with that one map active, then
// PerspectiveMap::D2DTransform with the coefficients it returned (MergeDepthMaps' loop,
// Depth.cpp:794-805, with the disparity pair), then one SolveDisparityToDepth call with two
// active maps, which must be refused.
//
//   disp_check IN OUT
//
// IN (flat little-endian, written by the test): ntiles, tile w, tile h (int32); per tile fov[4],
// range[4] (float32); baseline w, h (int32) and pixels (float32); every tile's pixels (float32);
// zenith range (2 float32).  stdout: one "abcd <tile> %a %a %a %a" line per tile and
// "two_active <0|1>"; OUT: the transformed tiles (float32).
#include "../../include/pf_depth.h"

#include <cstdio>
#include <string>
#include <vector>

using namespace DepthNamespace;

namespace {
template <class T>
bool get(FILE* f, T* p, size_t n)
{
    return fread(p, sizeof(T), n, f) == n;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 1;
    }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 1;
    int hdr[3];
    if (!get(fi, hdr, 3)) return 1;
    const int n = hdr[0], tw = hdr[1], th = hdr[2];
    std::vector<PerspectiveMap> pmaps(n);
    for (auto& p : pmaps) {
        float fov[4], rng[4];
        if (!get(fi, fov, 4) || !get(fi, rng, 4)) return 1;
        p.width = tw;
        p.height = th;
        p.channels = 1;
        p.SetWindow(fov[0], fov[1], fov[2], fov[3]);
        p.ranges = Vec4f(rng[0], rng[1], rng[2], rng[3]);
    }
    int ed[2];
    if (!get(fi, ed, 2)) return 1;
    EquirectangularMap emap;
    emap.width = ed[0];
    emap.height = ed[1];
    emap.channels = 1;
    emap.data = new float[(size_t)ed[0] * ed[1]];
    if (!get(fi, emap.data, (size_t)ed[0] * ed[1])) return 1;
    for (auto& p : pmaps) {
        p.data = new float[(size_t)tw * th];
        if (!get(fi, p.data, (size_t)tw * th)) return 1;
    }
    Vec2f zr;
    if (!get(fi, &zr.x, 1) || !get(fi, &zr.y, 1)) return 1;
    fclose(fi);

    for (int p = 0; p < n; p++) {
        std::vector<bool> actives(n, false);
        actives[p] = true;
        Vec4f abcd;
        if (!SolveDisparityToDepth(emap, pmaps, actives, zr, abcd)) return 2;
        printf("abcd %d %a %a %a %a\n", p, abcd.x, abcd.y, abcd.z, abcd.w);
        pmaps[p].D2DTransform(abcd);
    }
    for (auto& p : pmaps) fwrite(p.data, sizeof(float), (size_t)tw * th, fo);
    fclose(fo);
    bool two = false;
    if (n >= 2) {
        std::vector<bool> actives(n, false);
        actives[0] = actives[1] = true;
        Vec4f abcd(7.0f, 7.0f, 7.0f, 7.0f);
        two = SolveDisparityToDepth(emap, pmaps, actives, zr, abcd);
    }
    printf("two_active %d\n", two ? 1 : 0);
    return 0;
}
