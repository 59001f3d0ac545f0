// Calls the reference's own DepthNamespace::ErrorCompare on two image files, prints its seven
// float outputs at %.9g, then reloads the shifted PNG it wrote and dumps the pixels as hex.
// Compiled by tools/make_compare_golden.py together with the unmodified reference Depth.cpp
// (never committed); Basic.h comes first, as in the reference's Main.cpp.
//   compare_ref_harness <gt> <given> <disp 0|1> <align_way> <cap 0|1> <shifted.png>
#include "Basic.h"
#include "ILMBase.h"
#include "Depth.h"
#define STB_IMAGE_IMPLEMENTATION
#include "stb_image.h"
#define STB_IMAGE_WRITE_IMPLEMENTATION
#include "stb_image_write.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    std::string gt(argv[1]), given(argv[2]);
    const bool disp = std::atoi(argv[3]) != 0, cap = std::atoi(argv[5]) != 0;
    const int align_way = std::atoi(argv[4]);
    float v[7];
    if (!DepthNamespace::ErrorCompare(gt, given, disp, v[0], v[1], v[2], v[3], v[4], v[5], v[6],
                                      align_way, cap, argv[6]))
        return 1;
    std::printf("CMP %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", v[0], v[1], v[2], v[3], v[4], v[5],
                v[6]);
    int w = 0, h = 0, c = 0;
    unsigned char* px = stbi_load(argv[6], &w, &h, &c, 0);
    if (!px) return 3;
    std::printf("PIX %d %d %d ", w, h, c);
    for (int i = 0; i < w * h * c; ++i) std::printf("%02x", px[i]);
    std::printf("\n");
    stbi_image_free(px);
    return 0;
}
