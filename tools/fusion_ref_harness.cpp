// Calls the reference's own DepthNamespace::SolveDepthToDepth (real Ceres 1.13),
// PerspectiveMap::SetWindow / Depth2DepthTransform, SolveDepthAll, SolveDepthBySmoothing and
// ErrorData on maps built in memory.  Nothing of Depth.cpp is restated here: the only lines taken
// from MergeDepthMaps are the range cap (Depth.cpp:783-786) and its call order (one tile active
// per SolveDepthToDepth, then that tile's Depth2DepthTransform: Depth.cpp:794-805).  Compiled by
// tools/make_fusion_golden.py together with the unmodified reference Depth.cpp and the vendored
// Ceres (never committed); Basic.h comes first, as in the reference's Main.cpp.
//   fusion_ref_harness merge|fuse|smooth|joint <case.bin> <out.bin>
// case.bin, 32-bit little-endian words: ntiles tile_w tile_h ew eh ec W H gw gh (int), zr0 zr1
// (float bits), active[ntiles] (int), per tile the window's az_left az_right zen_top zen_down and
// the range's four values, uncapped (float), tiles [ntiles][tile_h][tile_w], baseline
// [eh][ew][ec], ground truth [gh][gw] (absent when gw == 0).
// out.bin, raw bits in this order:
//   merge   abcd [ntiles][4] f32, the transformed tiles f32, the result [H][W] u16 and, with a
//           ground truth, per (align_way 0..2) x (cap_depth 0, 1) eight f32: mse mae mre mselog
//           delta1 delta2 delta3 median_shift_factor (the last preset to a NaN with payload
//           0x7fc0beef: ErrorData writes it under align_way 1 only)
//   fuse    the result [H][W] u16 of SolveDepthAll on the tiles as given
//   smooth  the result [H][W] u16 of SolveDepthBySmoothing
//   joint   abcd [4] f32 of one SolveDepthToDepth over the active tiles
// The reference's own "[SolveDepthAll] oops!" lines go to stdout; the tool counts them.
#include "Basic.h"
#include "ILMBase.h"
#include "Depth.h"
#define STB_IMAGE_IMPLEMENTATION
#include "stb_image.h"
#define STB_IMAGE_WRITE_IMPLEMENTATION
#include "stb_image_write.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static FILE* in_file;
static FILE* out_file;

template <class T>
static T* read_n(size_t n)
{
    T* p = new T[n ? n : 1];
    if (std::fread(p, sizeof(T), n, in_file) != n) {
        std::fprintf(stderr, "case file too short\n");
        std::exit(4);
    }
    return p;
}

template <class T>
static void write_n(const T* p, size_t n)
{
    if (std::fwrite(p, sizeof(T), n, out_file) != n) std::exit(5);
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const std::string mode(argv[1]);
    in_file = std::fopen(argv[2], "rb");
    out_file = std::fopen(argv[3], "wb");
    if (!in_file || !out_file) return 4;
    const int* hd = read_n<int>(10);
    const int ntiles = hd[0], tw = hd[1], th = hd[2], ew = hd[3], eh = hd[4], ec = hd[5];
    int W = hd[6], H = hd[7];
    const int gw = hd[8], gh = hd[9];
    const float* zrv = read_n<float>(2);
    Vec2f zr(zrv[0], zrv[1]);
    const int* active = read_n<int>(ntiles);
    const float* win = read_n<float>((size_t)ntiles * 8);
    const size_t tn = (size_t)tw * th;

    std::vector<DepthNamespace::PerspectiveMap> pmaps(ntiles);
    for (int i = 0; i < ntiles; i++) {
        DepthNamespace::PerspectiveMap& pmap = pmaps[i];
        pmap.width = tw;
        pmap.height = th;
        pmap.channels = 1;
        pmap.data = read_n<float>(tn);
        const float* w = win + i * 8;
        pmap.SetWindow(w[0], w[1], w[2], w[3]);
        pmap.ranges[0] = MIN2(w[4], D2R(359.9));  // Depth.cpp:783-786
        pmap.ranges[1] = MIN2(w[5], D2R(359.9));
        pmap.ranges[2] = w[6];
        pmap.ranges[3] = w[7];
    }
    DepthNamespace::EquirectangularMap emap, gt;
    emap.width = ew;
    emap.height = eh;
    emap.channels = ec;
    emap.data = read_n<float>((size_t)ew * eh * ec);
    if (gw > 0) {
        gt.width = gw;
        gt.height = gh;
        gt.channels = 1;
        gt.data = read_n<float>((size_t)gw * gh);
    }
    unsigned short* data = new unsigned short[(size_t)W * H];
    std::memset(data, 0, sizeof(unsigned short) * W * H);  // Depth.cpp:814

    if (mode == "merge") {
        for (int p = 0; p < ntiles; p++) {  // Depth.cpp:794-805
            std::vector<bool> actives(ntiles, false);
            actives[p] = true;
            Vec4f abcd;
            if (DepthNamespace::SolveDepthToDepth(emap, pmaps, actives, zr, abcd))
                pmaps[p].Depth2DepthTransform(abcd);
            write_n(&abcd[0], 4);
        }
        for (int p = 0; p < ntiles; p++) write_n(pmaps[p].data, tn);
        DepthNamespace::SolveDepthAll(emap, pmaps, data, W, H, zr);
        std::cout.flush();
        write_n(data, (size_t)W * H);
        if (gw > 0)
            for (int align_way = 0; align_way < 3; align_way++)
                for (int cap = 0; cap < 2; cap++) {
                    float m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    const unsigned unset = 0x7fc0beefu;
                    std::memcpy(&m[7], &unset, 4);
                    DepthNamespace::ErrorData(gt, data, W, H, m[0], m[1], m[2], m[3], m[4], m[5],
                                              m[6], align_way, cap != 0, NULL, &m[7]);
                    write_n(m, 8);
                }
    } else if (mode == "fuse") {
        DepthNamespace::SolveDepthAll(emap, pmaps, data, W, H, zr);
        write_n(data, (size_t)W * H);
    } else if (mode == "smooth") {
        DepthNamespace::SolveDepthBySmoothing(pmaps, data, W, H, zr);
        write_n(data, (size_t)W * H);
    } else if (mode == "joint") {
        std::vector<bool> actives(ntiles, false);
        for (int p = 0; p < ntiles; p++) actives[p] = active[p] != 0;
        Vec4f abcd;
        if (!DepthNamespace::SolveDepthToDepth(emap, pmaps, actives, zr, abcd)) return 1;
        write_n(&abcd[0], 4);
    } else {
        return 2;
    }
    std::cout.flush();
    std::fclose(out_file);
    return 0;
}
