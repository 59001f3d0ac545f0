// A caller of include/pf_depth.h for tests/test_global_link.py: links against
// libpanofuse_depth.so and uses the post-fusion calibration entry points.
//   global_link            (needs no GPU)
//     DepthNamespace::MedianScaling (Depth.h:337) on a map without any valid pixel: must return
//     false after "MedianScaling: zero val0_median ??", before any GPU call, with the map and the
//     median outputs untouched.  Prints "RET <0|1>" and "UNTOUCHED <0|1>".
//   global_link gpu        (tests/test_gpu_global_cli.py)
//     SolveDepthToDepth2, TransformResult, MedianScaling and CopyInvalidPixels on small
//     hand-filled maps; prints "ABCD a b c d" at %.9g, "BAND <checksum>", "MED ret m0 m1",
//     "MASK <copied pixels>".
#include "../../include/pf_depth.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

using DepthNamespace::EquirectangularMap;

static void fill(EquirectangularMap& m, int w, int h, float scale, float bias)
{
    m.width = w;
    m.height = h;
    m.channels = 1;
    m.data = new float[(size_t)w * h];
    for (int i = 0; i < w * h; ++i)
        m.data[i] = bias + scale * (float)((i * 37) % 101) / 101.0f;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        EquirectangularMap dead, live;
        fill(dead, 8, 4, 0.0f, 0.0f);  // all zero: no valid pixel
        dead.data[3] = 1.0f;
        dead.data[5] = 5e-5f;
        fill(live, 8, 4, 0.5f, 0.2f);
        float before[32], m0 = -1.0f, m1 = -2.0f;
        std::memcpy(before, dead.data, sizeof(before));
        const bool ret = DepthNamespace::MedianScaling(dead, live, &m0, &m1);
        std::cout << "RET " << (ret ? 1 : 0) << std::endl;
        const bool same = std::memcmp(before, dead.data, sizeof(before)) == 0 && m0 == -1.0f &&
                          m1 == -2.0f;
        std::cout << "UNTOUCHED " << (same ? 1 : 0) << std::endl;
        const bool ret2 = DepthNamespace::MedianScaling(live, dead, &m0, &m1);
        std::cout << "RET " << (ret2 ? 1 : 0) << std::endl;
        return 0;
    }
    if (std::string(argv[1]) != "gpu") return 2;
    const int W = 64, H = 32;
    EquirectangularMap emap;
    fill(emap, 16, 8, 0.6f, 0.2f);
    unsigned short data[W * H];
    for (int i = 0; i < W * H; ++i) data[i] = (unsigned short)(4000 + (i * 131) % 50000);
    Vec4f abcd(0, 0, 0, 0);
    if (!DepthNamespace::SolveDepthToDepth2(emap, data, W, H, g_zenith_range, abcd)) return 1;
    std::printf("ABCD %.9g %.9g %.9g %.9g\n", abcd[0], abcd[1], abcd[2], abcd[3]);
    if (!DepthNamespace::TransformResult(data, W, H, g_zenith_range, abcd)) return 1;
    unsigned long long sum = 0;
    for (int i = 0; i < W * H; ++i) sum = sum * 1315423911ull + data[i];
    std::printf("BAND %llu\n", sum);
    EquirectangularMap a, b;
    fill(a, 20, 10, 0.9f, 0.0f);
    fill(b, 16, 8, 0.4f, 0.1f);
    b.data[7] = 0.0f;
    b.data[9] = 1.0f;
    float m0 = 0, m1 = 0;
    const bool ret = DepthNamespace::MedianScaling(a, b, &m0, &m1);
    std::printf("MED %d %.9g %.9g\n", ret ? 1 : 0, m0, m1);
    int copied = 0;
    EquirectangularMap before;
    fill(before, 20, 10, 0.0f, 0.0f);
    std::memcpy(before.data, a.data, sizeof(float) * 200);
    a.CopyInvalidPixels(b);
    for (int i = 0; i < 200; ++i) copied += a.data[i] != before.data[i];
    std::printf("MASK %d\n", copied);
    return 0;
}
