// Runs MergeDepthMaps' direct-stitch block (Depth.cpp:822-857, `if (false)` in the reference, so
// the loop is restated here) over the reference's own PerspectiveMap::SetWindow, SphericalTo2D,
// Value and Depth2DepthTransform, on tiles built in memory.  Compiled by
// tools/make_stitch_golden.py together with the unmodified reference Depth.cpp (never
// committed); Basic.h comes first, as in the reference's Main.cpp.
//   stitch_ref_harness <windows.f32> ntiles tile_w tile_h <tiles.f32> <abcd.f32> W H <out.u16>
// windows.f32: per tile the window's az_left az_right zen_top zen_down, then the range's four
// values (uncapped; capped here as Depth.cpp:783-786 caps them).  abcd.f32: per tile the cubic
// Depth2DepthTransform applies first.  Prints "STITCH covered <n> double <n>" and writes the u16
// plane.  Exits with status 3 if any Value index leaves its tile (the reference would read out
// of bounds there).
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

static float* read_floats(const char* fn, size_t n)
{
    float* p = new float[n];
    FILE* f = std::fopen(fn, "rb");
    if (!f || std::fread(p, sizeof(float), n, f) != n) {
        std::fprintf(stderr, "cannot read %zu floats of %s\n", n, fn);
        std::exit(4);
    }
    std::fclose(f);
    return p;
}

int main(int argc, char** argv)
{
    if (argc != 10) return 2;
    const int ntiles = std::atoi(argv[2]), tw = std::atoi(argv[3]), th = std::atoi(argv[4]);
    const int out_width = std::atoi(argv[7]), out_height = std::atoi(argv[8]);
    float* win = read_floats(argv[1], (size_t)ntiles * 8);
    float* tiles = read_floats(argv[5], (size_t)ntiles * tw * th);
    float* abcds = read_floats(argv[6], (size_t)ntiles * 4);
    std::vector<DepthNamespace::PerspectiveMap> pmaps(ntiles);
    for (int i = 0; i < ntiles; i++) {
        DepthNamespace::PerspectiveMap& pmap = pmaps[i];
        pmap.width = tw;
        pmap.height = th;
        pmap.channels = 1;
        pmap.data = new float[(size_t)tw * th];
        std::memcpy(pmap.data, tiles + (size_t)i * tw * th, sizeof(float) * tw * th);
        const float* w = win + i * 8;
        pmap.SetWindow(w[0], w[1], w[2], w[3]);
        pmap.ranges[0] = MIN2(w[4], D2R(359.9));  // Depth.cpp:783-786
        pmap.ranges[1] = MIN2(w[5], D2R(359.9));
        pmap.ranges[2] = w[6];
        pmap.ranges[3] = w[7];
        Vec4f abcd(abcds[i * 4], abcds[i * 4 + 1], abcds[i * 4 + 2], abcds[i * 4 + 3]);
        pmap.Depth2DepthTransform(abcd);
    }
    unsigned short* data = new unsigned short[(size_t)out_width * out_height];
    std::memset(data, 0, sizeof(unsigned short) * out_width * out_height);
    long covered = 0, twice = 0;
    for (int x = 0; x < out_width; x++) {
        for (int y = 0; y < out_height; y++) {
            Vec2f coord((float)x / (float)(out_width - 1) * 2 * MYPI,
                        (float)y / (float)(out_height - 1) * MYPI);
            int hits = 0;
            for (int p = 0; p < (int)pmaps.size(); p++) {
                DepthNamespace::PerspectiveMap& pmap = pmaps[p];
                int x0 = round((pmap.ranges[0] / (2 * MYPI)) * (out_width - 1));
                int x1 = round((pmap.ranges[1] / (2 * MYPI)) * (out_width - 1));
                int y0 = round((pmap.ranges[2] / MYPI) * (out_height - 1));
                int y1 = round((pmap.ranges[3] / MYPI) * (out_height - 1));
                if (x >= MIN2(x0, x1) && x <= MAX2(x0, x1) && y >= y0 && y <= y1) {
                    if (hits++) continue;  // the reference breaks here; the rest only counts
                    Vec2f xy = pmap.SphericalTo2D(coord.x, coord.y);
                    int X = xy[0] * (float)(pmap.width - 1);  // Value's index (Depth.cpp:114-115)
                    int Y = xy[1] * (float)(pmap.height - 1);
                    if (X < 0 || X >= pmap.width || Y < 0 || Y >= pmap.height) {
                        std::fprintf(stderr, "pixel (%d, %d): tile %d index (%d, %d) outside\n", x,
                                     y, p, X, Y);
                        return 3;
                    }
                    float val = pmap.Value(xy[0], xy[1]);
                    data[y * out_width + x] = (unsigned short)(val * 65535.0f);
                }
            }
            covered += hits > 0;
            twice += hits > 1;
        }
    }
    std::printf("STITCH covered %ld double %ld\n", covered, twice);
    FILE* f = std::fopen(argv[9], "wb");
    if (!f) return 5;
    std::fwrite(data, sizeof(unsigned short), (size_t)out_width * out_height, f);
    std::fclose(f);
    return 0;
}
