// pf_disp_weights.hpp -- the host side of the disparity tiles' per-pixel weights that is plain text:
// the "tent" / "files:SUFFIX" / "range:LO:HI" value of PF_DISPARITY_WEIGHTS / --disparity-weights,
// SetDisparityWeights' arguments, and what the switch cannot be combined with.  Host-only and
// header-only (no HIP include), so tests/cpp/disp_weights_check.cpp builds it alone under a host
// sanitizer.  pf_weights.hpp's parse_spec and pf_valid.hpp's parse_range do the parsing.
#pragma once

#include "pf_valid.hpp"
#include "pf_weights.hpp"

#include <string>

namespace pfdw {

enum { OFF = pfw::OFF, TENT = pfw::TENT, FILES = pfw::FILES, RANGE = 3 };

// What the disparity tiles' weights are: none, the blending tent, one map per tile file F read
// from F + suffix, or the validity rule lo < v < hi written as weights (pf_tile_range_weights).
struct Spec {
    int mode = OFF;
    std::string suffix;
    float lo = 0.0f, hi = 0.0f;
};

// "off", "tent", "files:SUFFIX" (pfw::parse_spec's rules) or "range:LO:HI" (pfv::parse_range's:
// two floats, "inf" included, LO < HI).  On failure err says why and spec is left alone.
inline bool parse_spec(const char* s, Spec& spec, std::string& err)
{
    const auto fail = [&](const std::string& why) {
        err = std::string("bad disparity weights \"") + (s ? s : "") + "\": " + why +
              " (want tent, files:SUFFIX or range:LO:HI, e.g. range:0:inf)";
        return false;
    };
    if (!s || !*s) return fail("empty");
    static const char kRange[] = "range:";
    if (std::strncmp(s, kRange, sizeof(kRange) - 1) == 0) {
        float lo, hi;
        std::string why;
        if (!pfv::parse_range(s + sizeof(kRange) - 1, lo, hi, why)) return fail("LO:HI is no range");
        spec.mode = RANGE;
        spec.suffix.clear();
        spec.lo = lo;
        spec.hi = hi;
        return true;
    }
    pfw::Spec w;
    std::string why;
    if (!pfw::parse_spec(s, w, why)) {
        const std::string v(s);
        if (v == "files:") return fail("SUFFIX is missing");
        if (v.compare(0, 6, "files:") == 0) return fail("SUFFIX holds a path separator");
        return fail("unknown mode");
    }
    spec = Spec{};
    spec.mode = w.mode;
    spec.suffix = w.suffix;
    return true;
}

// SetDisparityWeights' arguments as a Spec: OFF / TENT take no argument, FILES takes the SUFFIX,
// RANGE takes "LO:HI".
inline bool make_spec(int mode, const std::string& arg, Spec& spec, std::string& err)
{
    if (mode == OFF) return parse_spec("off", spec, err);
    if (mode == TENT) return parse_spec("tent", spec, err);
    if (mode == FILES) return parse_spec(("files:" + arg).c_str(), spec, err);
    if (mode == RANGE) return parse_spec(("range:" + arg).c_str(), spec, err);
    err = "unknown disparity weights mode " + std::to_string(mode) +
          " (want 0 off, 1 tent, 2 files, 3 range)";
    return false;
}

// The pfw::Spec of a TENT / FILES spec (the weight files are read as MergeDepthMaps reads them).
inline pfw::Spec as_tile_spec(const Spec& s)
{
    pfw::Spec w;
    w.mode = s.mode == RANGE ? pfw::OFF : s.mode;
    w.suffix = s.suffix;
    return w;
}

// What is on beside the switch, as the facade reads it from its environment and setters and as
// panofuse_main reads it from its flags.
struct Others {
    bool disparity_tiles = false, tile_valid = false, reg_loss = false, consistent = false;
    bool global_align = false, check_laplacian = false, tile_weights = false;
    bool smoothing = false, stitch = false;
};

// The first thing the weighted disparity calls have no form for, named as the facade's switch
// (cli false) or as panofuse_main's flag (cli true); nullptr: nothing clashes.
inline const char* clash(const Others& o, bool cli)
{
    if (!o.disparity_tiles) return cli ? "--tile-model depth" : "depth tiles";
    if (o.tile_valid) return cli ? "--tile-valid" : "PF_TILE_VALID / SetTileValidity";
    if (o.reg_loss) return cli ? "--reg-loss" : "PF_REG_LOSS / SetRegistrationLoss";
    if (o.consistent) return cli ? "--reg-consistent" : "PF_REG_CONSISTENT";
    if (o.global_align) return cli ? "--global-align" : "PF_GLOBAL_ALIGN";
    if (o.check_laplacian) return cli ? "--check-laplacian" : "PF_CHECK_LAPLACIAN";
    if (o.smoothing) return cli ? "--fusion smoothing" : "PF_FUSION=smoothing";
    if (o.stitch) return cli ? "--fusion stitch" : "PF_FUSION=stitch";
    if (o.tile_weights) return cli ? "--tile-weights" : "PF_TILE_WEIGHTS / SetTileWeights";
    return nullptr;
}

// The refusal's text.
inline std::string clash_message(const char* what, bool cli)
{
    return std::string(cli ? "--disparity-weights fits and fuses"
                           : "disparity weights (PF_DISPARITY_WEIGHTS / SetDisparityWeights) fit "
                             "and fuse") +
           " disparity tiles with per-pixel weights: not with " + what;
}

}  // namespace pfdw
