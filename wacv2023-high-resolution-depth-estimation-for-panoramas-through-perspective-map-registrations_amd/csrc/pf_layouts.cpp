// pf_layouts.cpp -- the reference's tile tables and the layout-file parser (pf_layouts.hpp).
//
// The windows feed bit-exact geometry, so every table is built with the roundings of Main.cpp's
// main(): D2R is a double expression; `float margin = D2R(m)` rounds it once; a sector edge
// `float azi = D2R(k) - margin` is a double difference rounded once; a range edge
// `azi01 - margin` is a float difference.  The 4-fold table has no arithmetic at all: each
// component is one D2R(k) rounded to float.
#include "pf_layouts.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <fstream>

namespace pfl {
namespace {

constexpr double kMyPi = 3.14159265359;  // Basic.h:11
inline double d2r(double a) { return a / 180.0 * kMyPi; }  // Basic.h:14

// The generator the 5-fold and 3-fold tables share: nsec sectors with a margin, three zenith
// bands; tile order bands outer, sectors inner.
void sector_table(double margin_deg, int nsec, const double fz[3][2], const double rz[3][2],
                  std::vector<Tile>& tiles)
{
    const float margin = (float)d2r(margin_deg);
    const double step = 360.0 / nsec;
    std::vector<float> a0(nsec), a1(nsec);
    for (int i = 0; i < nsec; ++i) {
        a0[i] = (float)(d2r(step * i) - margin);
        a1[i] = (float)(d2r(step * (i + 1)) + margin);
    }
    tiles.clear();
    for (int b = 0; b < 3; ++b)
        for (int i = 0; i < nsec; ++i) {
            Tile t;
            t.fov[0] = a0[i];
            t.fov[1] = a1[i];
            t.fov[2] = (float)d2r(fz[b][0]);
            t.fov[3] = (float)d2r(fz[b][1]);
            t.range[0] = a1[i] - margin;
            t.range[1] = a0[i] + margin;
            t.range[2] = (float)d2r(rz[b][0]);
            t.range[3] = (float)d2r(rz[b][1]);
            tiles.push_back(t);
        }
}

void fold4_table(std::vector<Tile>& tiles)
{
    static const double fa[4][2] = {{-2, 92}, {88, 182}, {178, 272}, {268, 362}};
    static const double fz[3][2] = {{17, 109}, {44, 136}, {71, 163}};
    static const double ra[4][2] = {{90, 0}, {180, 90}, {270, 180}, {360, 270}};
    static const double rz[3][2] = {{25, 56}, {56, 124}, {124, 155}};
    tiles.clear();
    for (int b = 0; b < 3; ++b)
        for (int i = 0; i < 4; ++i) {
            Tile t;
            t.fov[0] = (float)d2r(fa[i][0]);
            t.fov[1] = (float)d2r(fa[i][1]);
            t.fov[2] = (float)d2r(fz[b][0]);
            t.fov[3] = (float)d2r(fz[b][1]);
            t.range[0] = (float)d2r(ra[i][0]);
            t.range[1] = (float)d2r(ra[i][1]);
            t.range[2] = (float)d2r(rz[b][0]);
            t.range[3] = (float)d2r(rz[b][1]);
            tiles.push_back(t);
        }
}

const char* const kNames[] = {"leres", "midas", "fold4", "fold3"};

inline bool is_blank(char ch)
{
    return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\v' || ch == '\f';
}
inline bool is_digit(char ch) { return ch >= '0' && ch <= '9'; }

// [+-]? (digits [. digits*]? | . digits) ([eE] [+-]? digits)?  -- plain decimal numbers only, so
// the accepted set does not depend on the C library's strtod extensions (hex floats, "nan").
bool is_decimal(const char* s, size_t n)
{
    size_t i = 0;
    if (i < n && (s[i] == '+' || s[i] == '-')) ++i;
    size_t nd = 0;
    while (i < n && is_digit(s[i])) ++i, ++nd;
    if (i < n && s[i] == '.') {
        ++i;
        size_t nf = 0;
        while (i < n && is_digit(s[i])) ++i, ++nf;
        if (nd == 0 && nf == 0) return false;
    } else if (nd == 0) {
        return false;
    }
    if (i < n && (s[i] == 'e' || s[i] == 'E')) {
        ++i;
        if (i < n && (s[i] == '+' || s[i] == '-')) ++i;
        size_t ne = 0;
        while (i < n && is_digit(s[i])) ++i, ++ne;
        if (ne == 0) return false;
    }
    return i == n;
}

}  // namespace

const char* const* names(int* count)
{
    if (count) *count = (int)(sizeof(kNames) / sizeof(kNames[0]));
    return kNames;
}

bool named(const std::string& name, std::vector<Tile>& tiles)
{
    if (name == "leres") {  // Main.cpp:788-843
        static const double fz[3][2] = {{18, 94}, {52, 128}, {86, 162}};
        static const double rz[3][2] = {{25, 60}, {60, 120}, {120, 155}};
        sector_table(3, 5, fz, rz, tiles);
        return true;
    }
    if (name == "midas") {  // Main.cpp:731-787
        static const double fz[3][2] = {{20, 78}, {61, 119}, {102, 160}};
        static const double rz[3][2] = {{25, 67}, {67, 113}, {113, 155}};
        sector_table(2, 5, fz, rz, tiles);
        return true;
    }
    if (name == "fold3") {  // Main.cpp:845-887
        static const double fz[3][2] = {{12, 120}, {36, 144}, {60, 168}};
        static const double rz[3][2] = {{26, 60}, {60, 120}, {120, 154}};
        sector_table(2, 3, fz, rz, tiles);
        return true;
    }
    if (name == "fold4") {  // Main.cpp:695-730
        fold4_table(tiles);
        return true;
    }
    return false;
}

bool load_file(const std::string& path, std::vector<Tile>& tiles, std::string& err)
{
    tiles.clear();
    std::ifstream in(path, std::ios::binary);
    if (!in) {
        err = "cannot open layout file " + path;
        return false;
    }
    std::string line;
    long long lineno = 0;
    while (std::getline(in, line)) {
        ++lineno;
        const size_t end = std::min(line.find('#'), line.size());
        double v[8];
        int nv = 0;
        size_t i = 0;
        while (true) {
            while (i < end && is_blank(line[i])) ++i;
            if (i >= end) break;
            size_t j = i;
            while (j < end && !is_blank(line[j])) ++j;
            if (nv == 8 || !is_decimal(line.data() + i, j - i)) {
                nv = -1;
                break;
            }
            v[nv++] = std::strtod(line.substr(i, j - i).c_str(), nullptr);
            i = j;
        }
        if (nv == 0) continue;  // blank or comment only
        if (nv != 8) {
            err = path + ":" + std::to_string(lineno) + ": want eight numbers (degrees)";
            return false;
        }
        if ((int)tiles.size() >= kMaxTiles) {
            err = path + ": more than " + std::to_string(kMaxTiles) + " tiles";
            return false;
        }
        Tile t;
        for (int k = 0; k < 8; ++k) {
            const double rad = d2r(v[k]);  // strtod overflows to infinity
            if (!std::isfinite(rad) || std::fabs(rad) > (double)FLT_MAX) {
                err = path + ":" + std::to_string(lineno) + ": value " + std::to_string(k + 1) +
                      " is not finite";
                return false;
            }
            (k < 4 ? t.fov[k] : t.range[k - 4]) = (float)rad;
        }
        tiles.push_back(t);
    }
    if (in.bad()) {
        err = "cannot read layout file " + path;
        return false;
    }
    if (tiles.empty()) {
        err = path + ": no tiles";
        return false;
    }
    return true;
}

bool resolve(const std::string& spec, std::vector<Tile>& tiles, std::string& err)
{
    if (named(spec, tiles)) return true;
    if (load_file(spec, tiles, err)) return true;
    err = "layout '" + spec + "' is neither a known name (leres, midas, fold4, fold3) nor a "
          "usable layout file: " + err;
    return false;
}

}  // namespace pfl
