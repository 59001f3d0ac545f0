// pf_weights.hpp -- the host side of the per-pixel tile weights that is plain text: the
// "tent" / "files:SUFFIX" value of PF_TILE_WEIGHTS / --tile-weights, the name of a tile's weight
// file, the size check's message and MergeDepthMaps' "[weights]" lines.  Host-only and header-only
// (no HIP include), so tests/cpp/weights_check.cpp builds it alone under a host sanitizer.
#pragma once

#include <cstdio>
#include <cstring>
#include <string>

namespace pfw {

enum { OFF = 0, TENT = 1, FILES = 2 };

// What the tiles' weights are: none, the blending tent (pf_tile_tent_weights), or one map per tile
// file F read from F + suffix.
struct Spec {
    int mode = OFF;
    std::string suffix;
};

// "off", "tent" or "files:SUFFIX" with a SUFFIX that is not empty and holds no path separator (it
// is appended to the tile's file name, never a path of its own).  On failure err says why and
// spec is left alone.
inline bool parse_spec(const char* s, Spec& spec, std::string& err)
{
    const auto fail = [&](const std::string& why) {
        err = std::string("bad tile weights \"") + (s ? s : "") + "\": " + why +
              " (want tent or files:SUFFIX, e.g. files:.w.pfm)";
        return false;
    };
    if (!s || !*s) return fail("empty");
    const std::string v(s);
    if (v == "off") {
        spec = Spec{};
        return true;
    }
    if (v == "tent") {
        spec.mode = TENT;
        spec.suffix.clear();
        return true;
    }
    static const char kFiles[] = "files:";
    if (v.compare(0, sizeof(kFiles) - 1, kFiles) != 0) return fail("unknown mode");
    const std::string suffix = v.substr(sizeof(kFiles) - 1);
    if (suffix.empty()) return fail("SUFFIX is missing");
    if (suffix.find('/') != std::string::npos || suffix.find('\\') != std::string::npos)
        return fail("SUFFIX holds a path separator");
    spec.mode = FILES;
    spec.suffix = suffix;
    return true;
}

// SetTileWeights' arguments as a Spec: mode OFF / TENT take no suffix, FILES needs one that
// parse_spec would take.
inline bool make_spec(int mode, const std::string& suffix, Spec& spec, std::string& err)
{
    if (mode == OFF) return parse_spec("off", spec, err);
    if (mode == TENT) return parse_spec("tent", spec, err);
    if (mode == FILES) return parse_spec(("files:" + suffix).c_str(), spec, err);
    err = "unknown tile weights mode " + std::to_string(mode) + " (want 0 off, 1 tent, 2 files)";
    return false;
}

// The weight map of the tile file F: F + SUFFIX.
inline std::string weight_file(const std::string& tile_file, const Spec& spec)
{
    return tile_file + spec.suffix;
}

// A weight map must have its tile's width and height.
inline bool size_matches(const std::string& file, int w, int h, int tile_w, int tile_h,
                         std::string& err)
{
    if (w == tile_w && h == tile_h) return true;
    err = "weight map " + file + " is " + std::to_string(w) + "x" + std::to_string(h) +
          ", its tile " + std::to_string(tile_w) + "x" + std::to_string(tile_h);
    return false;
}

// "[weights] tile <i>: <n> of <N> samples used, sum w <s>" from pf_register_weighted's summary
// {used samples, sum of w} and the tile's sample count.
inline std::string weights_line(int tile, double used, long long samples, double sum_w)
{
    char buf[160];
    std::snprintf(buf, sizeof(buf), "[weights] tile %d: %lld of %lld samples used, sum w %.6g",
                  tile, (long long)used, samples, sum_w);
    return buf;
}

}  // namespace pfw
