// The host-only part of the disparity tiles' weights (csrc/pf_disp_weights.hpp) as a stand-alone
// program for tests/test_disp_weights_sanitized.py, which builds it with
// -fsanitize=address,undefined and runs it as a child process.
//   disp_weights_check <cases file>
//     Every line "<ok|bad> <text>" (the text may be empty or very long) goes through parse_spec:
//     "<ok|bad> <1|0> <mode> <lo> <hi> <suffix>" is printed, and "UNEXPECTED" when the outcome is
//     not the announced one.  Then make_spec, as_tile_spec, clash and clash_message on fixed
//     values, and "disp_weights_check ok".
#include "pf_disp_weights.hpp"

#include <fstream>
#include <iostream>
#include <string>

static int g_bad = 0;

static void expect(bool cond, const char* what)
{
    if (cond) return;
    std::cout << "UNEXPECTED " << what << std::endl;
    g_bad++;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    std::string line;
    while (std::getline(in, line)) {
        const size_t sp = line.find(' ');
        const std::string want = line.substr(0, sp);
        const std::string text = sp == std::string::npos ? "" : line.substr(sp + 1);
        pfdw::Spec spec;
        spec.mode = 9;  // a failed parse leaves it alone
        spec.suffix = "kept";
        spec.lo = -5.0f;
        spec.hi = 5.0f;
        std::string err;
        const bool ok = pfdw::parse_spec(text.c_str(), spec, err);
        std::cout << want << (ok ? " 1 " : " 0 ") << spec.mode << " " << spec.lo << " " << spec.hi
                  << " " << spec.suffix << std::endl;
        expect(ok == (want == "ok"), "parse outcome");
        expect(ok || (spec.mode == 9 && spec.suffix == "kept" && spec.lo == -5.0f &&
                      spec.hi == 5.0f && !err.empty()),
               "failed parse wrote");
        expect(ok || err.find("want tent, files:SUFFIX or range:LO:HI") != std::string::npos,
               "message");
    }
    pfdw::Spec spec;
    std::string err;
    expect(pfdw::parse_spec(nullptr, spec, err) == false, "null text");
    expect(pfdw::make_spec(pfdw::OFF, "ignored", spec, err) && spec.mode == pfdw::OFF, "mode 0");
    expect(pfdw::make_spec(pfdw::TENT, "", spec, err) && spec.mode == pfdw::TENT, "mode 1");
    expect(pfdw::make_spec(pfdw::FILES, ".w.pfm", spec, err) && spec.mode == pfdw::FILES &&
               spec.suffix == ".w.pfm",
           "mode 2");
    expect(pfdw::as_tile_spec(spec).mode == pfw::FILES && pfdw::as_tile_spec(spec).suffix == ".w.pfm",
           "as_tile_spec of files");
    expect(pfdw::make_spec(pfdw::RANGE, "0:inf", spec, err) && spec.mode == pfdw::RANGE &&
               spec.lo == 0.0f && spec.hi > 3e38f && spec.suffix.empty(),
           "mode 3");
    expect(pfdw::as_tile_spec(spec).mode == pfw::OFF, "as_tile_spec of range");
    expect(!pfdw::make_spec(pfdw::RANGE, "", spec, err), "mode 3 without a range");
    expect(!pfdw::make_spec(pfdw::RANGE, "1:0", spec, err), "mode 3 with LO above HI");
    expect(!pfdw::make_spec(pfdw::FILES, "", spec, err), "mode 2 without a suffix");
    expect(!pfdw::make_spec(pfdw::FILES, "../x", spec, err), "mode 2 with a path");
    expect(!pfdw::make_spec(7, "", spec, err) && err.find("7") != std::string::npos, "mode 7");
    expect(!pfdw::make_spec(-2147483647 - 1, "", spec, err), "mode INT_MIN");
    expect(spec.mode == pfdw::RANGE && spec.lo == 0.0f, "failed make_spec wrote");

    pfdw::Others o;
    expect(std::string(pfdw::clash(o, true)) == "--tile-model depth", "depth tiles, cli");
    expect(std::string(pfdw::clash(o, false)) == "depth tiles", "depth tiles");
    o.disparity_tiles = true;
    expect(pfdw::clash(o, true) == nullptr && pfdw::clash(o, false) == nullptr, "nothing clashes");
    bool pfdw::Others::* const flags[] = {&pfdw::Others::tile_valid, &pfdw::Others::reg_loss,
                                          &pfdw::Others::consistent, &pfdw::Others::global_align,
                                          &pfdw::Others::check_laplacian, &pfdw::Others::smoothing,
                                          &pfdw::Others::stitch, &pfdw::Others::tile_weights};
    for (bool pfdw::Others::* f : flags) {
        pfdw::Others one;
        one.disparity_tiles = true;
        one.*f = true;
        const char* cli = pfdw::clash(one, true);
        const char* env = pfdw::clash(one, false);
        expect(cli && env && cli[0] == '-' && env[0] != '-', "a clash has both names");
        if (cli && env)
            std::cout << pfdw::clash_message(cli, true) << " | " << pfdw::clash_message(env, false)
                      << std::endl;
    }
    if (g_bad) return 1;
    std::cout << "disp_weights_check ok" << std::endl;
    return 0;
}
