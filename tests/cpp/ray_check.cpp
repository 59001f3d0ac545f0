// ray_check -- the host-only part of the planar-depth tiles (csrc/pf_ray.hpp: the ray-factor table
// builder of pf_set_tiles and the parser of PF_TILE_DEPTH / --tile-depth) under a host sanitizer:
// tests/test_ray_sanitized.py builds this file with -fsanitize=address,undefined
// -fno-sanitize-recover=all and runs it as a child process.
//
//   ray_check <file>
// <file> holds one case per line:
//   tile <az_left> <az_right> <zen_top> <zen_down> <w> <h>   (the floats as %a hex floats)
//   parse <text>        (the text taken to the end of the line as it is; it may be empty)
// All tile lines form one layout: as pf_set_tiles does, their tables are built one after the
// other into one buffer of exactly sum (w + h) doubles, so a write past a table's end is the
// sanitizer's to find.  Per tile it prints "tile <w> <h> <kf(0,0) bits>" and then the w + h table
// values as 16 hex digits each on one line; per parse case "parse <result>".  It ends with
// "ray_check ok" (status 0) or "ray_check FAILED" (status 1).
#include "pf_ray.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

struct TileCase {
    float win[4];
    int w, h;
};

static unsigned long long bits64(double d)
{
    unsigned long long u;
    std::memcpy(&u, &d, 8);
    return u;
}

static unsigned bits32(float f)
{
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char* argv[])
{
    if (argc < 2) {
        std::printf("usage: %s <file>\n", argv[0]);
        return 2;
    }
    int failures = 0;
    std::vector<TileCase> tiles;
    std::ifstream in(argv[1], std::ios::binary);
    std::string line;
    while (std::getline(in, line)) {
        if (line.compare(0, 5, "tile ") == 0) {
            std::istringstream ss(line.substr(5));
            std::string f[4];
            TileCase t{};
            ss >> f[0] >> f[1] >> f[2] >> f[3] >> t.w >> t.h;
            for (int k = 0; k < 4; k++) t.win[k] = std::strtof(f[k].c_str(), nullptr);
            if (!ss || t.w < 1 || t.h < 1) {
                std::printf("UNEXPECTED tile line [%s]\n", line.c_str());
                ++failures;
                continue;
            }
            tiles.push_back(t);
        } else if (line.compare(0, 5, "parse") == 0) {
            const std::string text = line.size() > 6 ? line.substr(6) : std::string();
            // a heap copy of exactly the text's size: a read past its end is the sanitizer's
            std::vector<char> copy(text.begin(), text.end());
            copy.push_back('\0');
            std::printf("parse %d\n", pf::parse_tile_depth(copy.data()));
        }
    }
    if (pf::parse_tile_depth(nullptr) != -1) ++failures;

    size_t total = 0;
    for (const TileCase& t : tiles) total += (size_t)t.w + (size_t)t.h;
    std::vector<double> tab(total, -1.0);
    size_t at = 0;
    for (const TileCase& t : tiles) {  // pf_set_tiles' packing
        pf::ray_tables(t.win[0], t.win[1], t.win[2], t.win[3], t.w, t.h, &tab[at], &tab[at + t.w]);
        at += (size_t)t.w + (size_t)t.h;
    }
    at = 0;
    for (const TileCase& t : tiles) {
        const double* cu = &tab[at];
        const double* rv = cu + t.w;
        std::printf("tile %d %d %08x\n", t.w, t.h, bits32(pf::ray_factor(cu[0], rv[0])));
        for (int i = 0; i < t.w + t.h; i++) {
            if (!(cu[i] >= 0.0)) ++failures;  // a square; -1.0 would be a slot never written
            std::printf("%016llx%c", bits64(cu[i]), i + 1 == t.w + t.h ? '\n' : ' ');
        }
        if (t.w == 1 && cu[0] != 0.0) ++failures;
        if (t.h == 1 && rv[0] != 0.0) ++failures;
        at += (size_t)t.w + (size_t)t.h;
    }
    std::printf(failures ? "ray_check FAILED\n" : "ray_check ok\n");
    return failures ? 1 : 0;
}
