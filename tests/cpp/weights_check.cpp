// The host-only part of the per-pixel tile weights (csrc/pf_weights.hpp) as a stand-alone program
// for tests/test_weights_sanitized.py, which builds it with -fsanitize=address,undefined and runs
// it as a child process.
//   weights_check <cases file>
//     Every line "<ok|bad> <text>" (the text may be empty or very long) goes through parse_spec:
//     "<ok|bad> <1|0> <mode> <suffix>" is printed, and "UNEXPECTED" when the outcome is not the
//     announced one.  Then make_spec, weight_file, size_matches and weights_line on fixed values,
//     and "weights_check ok".
#include "pf_weights.hpp"

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
        pfw::Spec spec;
        spec.mode = 9;  // a failed parse leaves it alone
        spec.suffix = "kept";
        std::string err;
        const bool ok = pfw::parse_spec(text.c_str(), spec, err);
        if (ok)
            std::cout << want << " 1 " << spec.mode << " " << spec.suffix << std::endl;
        else
            std::cout << want << " 0 " << spec.mode << " " << spec.suffix << std::endl;
        expect(ok == (want == "ok"), "parse outcome");
        expect(ok || (spec.mode == 9 && spec.suffix == "kept" && !err.empty()), "failed parse wrote");
    }
    pfw::Spec spec;
    std::string err;
    expect(pfw::parse_spec(nullptr, spec, err) == false, "null text");
    expect(pfw::make_spec(pfw::OFF, "ignored", spec, err) && spec.mode == pfw::OFF, "mode 0");
    expect(pfw::make_spec(pfw::TENT, "", spec, err) && spec.mode == pfw::TENT, "mode 1");
    expect(pfw::make_spec(pfw::FILES, ".w.pfm", spec, err) && spec.mode == pfw::FILES &&
               spec.suffix == ".w.pfm",
           "mode 2");
    expect(pfw::weight_file("dir/a.png", spec) == "dir/a.png.w.pfm", "weight_file");
    expect(!pfw::make_spec(pfw::FILES, "", spec, err), "mode 2 without a suffix");
    expect(!pfw::make_spec(pfw::FILES, "../x", spec, err), "mode 2 with a path");
    expect(!pfw::make_spec(7, "", spec, err) && err.find("7") != std::string::npos, "mode 7");
    expect(!pfw::make_spec(-2147483647 - 1, "", spec, err), "mode INT_MIN");
    expect(spec.mode == pfw::FILES && spec.suffix == ".w.pfm", "failed make_spec wrote");
    expect(pfw::size_matches("f", 64, 48, 64, 48, err), "equal sizes");
    err.clear();
    expect(!pfw::size_matches("dir/a.png.w.pfm", 48, 64, 64, 48, err) &&
               err == "weight map dir/a.png.w.pfm is 48x64, its tile 64x48",
           "size message");
    std::cout << pfw::weights_line(3, 1234.0, 4096, 617.25) << std::endl;
    std::cout << pfw::weights_line(2147483647, 9.0e15, 9223372036854775807LL, 1e300) << std::endl;
    std::cout << pfw::weights_line(0, 0.0, 0, 0.0) << std::endl;
    if (g_bad) return 1;
    std::cout << "weights_check ok" << std::endl;
    return 0;
}
