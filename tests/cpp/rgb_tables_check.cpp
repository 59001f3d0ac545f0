// The staged RGB warp's host tables of one tile, checked without a GPU (tests/test_tile_shapes.py).
//
//   pf_rgb_tables W H PW PH AZ_LEFT AZ_RIGHT ZEN_TOP ZEN_DOWN     (angles in radians)
//
// Builds the taps (pf_probe_rgb_taps) and the patches, unit table and LDS locations
// (rgb_patches_host, csrc/pf_warp.hip) of a W x H tile on a PW x PH panorama, then does on the
// host what k_warp_rgb_box does per staged patch: LDS = the patch's 16-B units of a panorama
// whose bytes are a hash of their offset; a pixel's top and bottom corner pairs are the 6 bytes
// at its two LDS locations and must be the panorama's texels at its taps.  Also checked: every
// unit lies inside the panorama, unit counts are in [1, kRgbUnits], the patches tile the tile.
// Prints one line; exit status 0 when everything holds.
#include "pf_internal.hpp"  // -Icsrc (the package Makefile)

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pf;

static uint8_t pano_byte(long long o) { return (uint8_t)(((uint32_t)o * 2654435761u) >> 13); }

int main(int argc, char** argv)
{
    if (argc != 9) return 2;
    const int w = atoi(argv[1]), h = atoi(argv[2]), pw = atoi(argv[3]), ph = atoi(argv[4]);
    const pf_window fov{(float)atof(argv[5]), (float)atof(argv[6]), (float)atof(argv[7]),
                        (float)atof(argv[8])};
    if (w < 1 || h < 1 || w % 4 || pw % 16) return 2;  // the staged kernel's conditions
    std::vector<RgbTap> taps((size_t)w * h);
    if (pf_probe_rgb_taps(&fov, w, h, pw, ph, reinterpret_cast<uint32_t*>(taps.data()))) return 2;
    TileGeom g{};
    g.w = w;
    g.h = h;
    g.c = 1;
    std::vector<RgbPatch> patches;
    std::vector<uint32_t> units, loc((size_t)w * h);
    std::vector<float> wts(2 * (size_t)w * h);
    rgb_patches_host(g, 0, taps.data(), pw, ph, patches, units, loc.data(), wts.data());

    long long bad = 0, staged = 0, covered = 0;
    int wide = 0;
    if (units.size() != patches.size() * (size_t)kRgbUnits) bad++;
    std::vector<uint8_t> lds(16 * kRgbUnits + 16);
    for (size_t q = 0; q < patches.size() && !bad; q++) {
        const RgbPatch& P = patches[q];
        const int X1 = std::min(w, P.X0 + kRgbPW);
        if (P.nrow < 1 || P.nrow > kRgbPH || P.Y0 + P.nrow > h) { bad++; break; }
        covered += (long long)P.nrow * (X1 - P.X0);
        if (P.wide) { wide++; continue; }
        if (P.units < 1 || P.units > kRgbUnits) { bad++; break; }
        std::fill(lds.begin(), lds.end(), (uint8_t)0);
        for (int u = 0; u < P.units; u++) {
            const long long o = units[q * kRgbUnits + u];
            if (o % 16 || o + 16 > 3LL * pw * ph) { bad++; break; }
            for (int j = 0; j < 16; j++) lds[16 * u + j] = pano_byte(o + j);
        }
        for (int Y = P.Y0; Y < P.Y0 + P.nrow; Y++)
            for (int X = P.X0; X < X1; X++) {
                const long long i = (long long)Y * w + X;
                const RgbTap& t = taps[i];
                const long long x0 = t.x0y0 & 0xFFFFu, y0 = t.x0y0 >> 16;
                const long long x1 = t.x1y1 & 0xFFFFu, y1 = t.x1y1 >> 16;
                const uint32_t lt = loc[i] & 0xFFFFu, lb = loc[i] >> 16;
                if (lt + 6 > 16u * P.units || lb + 6 > 16u * P.units) { bad++; continue; }
                for (int ch = 0; ch < 3; ch++) {
                    bad += lds[lt + ch] != pano_byte((y0 * pw + x0) * 3 + ch);
                    bad += lds[lt + 3 + ch] != pano_byte((y0 * pw + x1) * 3 + ch);
                    bad += lds[lb + ch] != pano_byte((y1 * pw + x0) * 3 + ch);
                    bad += lds[lb + 3 + ch] != pano_byte((y1 * pw + x1) * 3 + ch);
                }
                staged++;
            }
    }
    if (covered != (long long)w * h) bad++;
    printf("%dx%d on %dx%d: patches %zu wide %d staged_pixels %lld bad %lld\n", w, h, pw, ph,
           patches.size(), wide, staged, bad);
    return bad ? 1 : 0;
}
