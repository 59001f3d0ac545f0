// valid_check -- the host-only part of the tile-pixel validity rule (csrc/pf_valid.hpp: the
// "LO:HI" parser of PF_TILE_VALID / --tile-valid and the "[mask]" lines' bookkeeping) under a host
// sanitizer: tests/test_valid_sanitized.py builds this file with
// -fsanitize=address,undefined -fno-sanitize-recover=all and runs it as a child process.
//
//   valid_check <file>
// <file> holds one case per line, "<want> <text>" with want = ok | bad and the text taken to the
// end of the line as it is (it may be empty or hold blanks).  Per case it prints
//   <want> <ok 0|1> <lo bits> <hi bits>
// Then the bookkeeping cases run, and it ends with "valid_check ok" (status 0) or
// "valid_check FAILED" (status 1).
#include "pf_valid.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

static uint32_t bits(float f)
{
    uint32_t u;
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
    std::ifstream in(argv[1], std::ios::binary);
    std::string line;
    while (std::getline(in, line)) {
        const size_t sp = line.find(' ');
        if (sp == std::string::npos) continue;
        const std::string want = line.substr(0, sp), text = line.substr(sp + 1);
        float lo = -1.0f, hi = -2.0f;
        std::string err;
        // a heap copy of exactly the text's size: a read past its end is the sanitizer's to find
        std::vector<char> copy(text.begin(), text.end());
        copy.push_back('\0');
        const bool ok = pfv::parse_range(copy.data(), lo, hi, err);
        if (ok != (want == "ok") || (!ok && err.empty()) || (ok && !(lo < hi)) ||
            (!ok && (lo != -1.0f || hi != -2.0f))) {
            std::printf("UNEXPECTED [%s]: ok=%d err=%s\n", text.c_str(), (int)ok, err.c_str());
            ++failures;
        }
        std::printf("%s %d %08x %08x\n", want.c_str(), (int)ok, bits(lo), bits(hi));
    }
    {
        float lo = 0, hi = 0;
        std::string err;
        if (pfv::parse_range(nullptr, lo, hi, err) || err.empty()) ++failures;
    }
    // the bookkeeping: {samples, pixels} per tile
    {
        const long long total[] = {100, 4096, 100, 4096, 90, 4096, 0, 0};
        const long long valid[] = {100, 4096, 60, 4000, 0, 0, 0, 0};
        std::vector<std::string> lines;
        if (!pfv::mask_lines(valid, total, 4, lines) || lines.size() != 2 ||
            lines[0] != "[mask] tile 1: 96 of 4096 pixels invalid, 40 of 100 samples" ||
            lines[1] != "[mask] tile 2: 4096 of 4096 pixels invalid, 90 of 90 samples")
            ++failures;
        for (const std::string& ln : lines) std::printf("%s\n", ln.c_str());
        if (!pfv::mask_lines(valid, total, 0, lines) || !lines.empty()) ++failures;
        if (!pfv::mask_lines(nullptr, nullptr, 0, lines)) ++failures;
        if (pfv::mask_lines(nullptr, total, 2, lines)) ++failures;
        if (pfv::mask_lines(valid, total, -1, lines)) ++failures;
        const long long more[] = {101, 4096};  // more valid samples than samples
        if (pfv::mask_lines(more, total, 1, lines) || !lines.empty()) ++failures;
        const long long neg[] = {5, -1};
        if (pfv::mask_lines(neg, total, 1, lines)) ++failures;
        const long long big_t[] = {1LL << 40, 1LL << 62}, big_v[] = {0, 1};
        if (!pfv::mask_lines(big_v, big_t, 1, lines) || lines.size() != 1) ++failures;
        for (const std::string& ln : lines) std::printf("%s\n", ln.c_str());
    }
    std::printf(failures ? "valid_check FAILED\n" : "valid_check ok\n");
    return failures ? 1 : 0;
}
