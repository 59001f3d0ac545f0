// pf_valid.hpp -- the host side of the tile-pixel validity rule that is plain text and counting:
// the "LO:HI" value of PF_TILE_VALID / --tile-valid, and MergeDepthMaps' "[mask]" lines from the
// counts of pf_tile_valid_counts.  Host-only and header-only (no HIP include), so
// tests/cpp/valid_check.cpp builds it alone under a host sanitizer.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace pfv {

// "LO:HI": two floats as strtof reads them ("-inf", "inf" and "infinity" included), nothing
// before, between or after them but the one colon, neither NaN, LO < HI.  On failure err says
// why and lo / hi are left alone.
inline bool parse_range(const char* s, float& lo, float& hi, std::string& err)
{
    const auto fail = [&](const std::string& why) {
        err = std::string("bad tile validity range \"") + (s ? s : "") + "\": " + why +
              " (want LO:HI with LO < HI, e.g. 0:inf or -inf:inf)";
        return false;
    };
    if (!s || !*s) return fail("empty");
    const char* colon = std::strchr(s, ':');
    if (!colon || std::strchr(colon + 1, ':')) return fail("needs exactly one ':'");
    const std::string a(s, colon), b(colon + 1);
    float v[2];
    const std::string* part[2] = {&a, &b};
    for (int k = 0; k < 2; ++k) {
        const std::string& t = *part[k];
        if (t.empty() || t[0] == ' ' || t[0] == '\t' || t[0] == '\n')
            return fail(k ? "HI is missing" : "LO is missing");
        char* end = nullptr;
        v[k] = std::strtof(t.c_str(), &end);
        if (end != t.c_str() + t.size()) return fail(k ? "HI is no number" : "LO is no number");
        if (std::isnan(v[k])) return fail("NaN is no bound");
    }
    if (!(v[0] < v[1])) return fail("LO is not below HI");
    lo = v[0];
    hi = v[1];
    return true;
}

// valid / total: [ntiles][2] = {registration samples, pixels} as pf_tile_valid_counts writes them
// under the rule / under PF_VALID_ALL.  One line per tile that has invalid pixels:
//   [mask] tile <i>: <n> of <N> pixels invalid, <m> of <M> samples
// Counts that cannot be (negative, or more valid than there are) give an empty list and false.
inline bool mask_lines(const long long* valid, const long long* total, int ntiles,
                       std::vector<std::string>& lines)
{
    lines.clear();
    if (ntiles < 0 || (ntiles > 0 && (!valid || !total))) return false;
    for (int i = 0; i < ntiles; ++i) {
        const long long vs = valid[2 * i], vp = valid[2 * i + 1];
        const long long ts = total[2 * i], tp = total[2 * i + 1];
        if (vs < 0 || vp < 0 || vs > ts || vp > tp) {
            lines.clear();
            return false;
        }
        if (vp == tp) continue;
        char buf[160];
        std::snprintf(buf, sizeof(buf),
                      "[mask] tile %d: %lld of %lld pixels invalid, %lld of %lld samples", i,
                      tp - vp, tp, ts - vs, ts);
        lines.push_back(buf);
    }
    return true;
}

}  // namespace pfv
