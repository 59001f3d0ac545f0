// layouts_check -- the host-only layouts unit (csrc/pf_layouts.cpp) under a host sanitizer:
// tests/test_layouts_sanitized.py builds this file and that unit with
// -fsanitize=address,undefined -fno-sanitize-recover=all and runs it as a child process.
//
//   layouts_check <dir>
// <dir> holds the files the test wrote: good_*.txt must parse, bad_*.txt must be rejected with a
// message.  For every file and for the four named tables it prints one line,
//   <name> <ntiles or -1> <fnv1a-64 of the tiles' float bits>
// so the test can hold the sanitized run to the unsanitized library, bit for bit.
#include "pf_layouts.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <string>
#include <vector>

static uint64_t hash_tiles(const std::vector<pfl::Tile>& tiles)
{
    uint64_t h = 1469598103934665603ull;
    for (const pfl::Tile& t : tiles) {
        unsigned char b[sizeof(pfl::Tile)];
        std::memcpy(b, &t, sizeof(b));
        for (unsigned char c : b) h = (h ^ c) * 1099511628211ull;
    }
    return h;
}

int main(int argc, char* argv[])
{
    if (argc < 2) {
        std::printf("usage: %s <dir>\n", argv[0]);
        return 2;
    }
    int failures = 0;
    int count = 0;
    const char* const* names = pfl::names(&count);
    for (int i = 0; i < count; ++i) {
        std::vector<pfl::Tile> tiles;
        if (!pfl::named(names[i], tiles)) ++failures;
        std::printf("%s %d %016llx\n", names[i], (int)tiles.size(),
                    (unsigned long long)hash_tiles(tiles));
    }
    {
        std::vector<pfl::Tile> tiles;
        std::string err;
        if (pfl::named("nosuch", tiles) || pfl::resolve("nosuch", tiles, err) || err.empty())
            ++failures;
    }
    std::vector<std::string> files;
    for (const auto& e : std::filesystem::directory_iterator(argv[1]))
        files.push_back(e.path().string());
    std::sort(files.begin(), files.end());
    for (const std::string& fn : files) {
        const std::string base = std::filesystem::path(fn).filename().string();
        std::vector<pfl::Tile> tiles;
        std::string err;
        const bool ok = pfl::resolve(fn, tiles, err);
        const bool want = base.rfind("good_", 0) == 0;
        if (ok != want || (!ok && err.empty()) || (ok && tiles.empty()) ||
            (int)tiles.size() > pfl::kMaxTiles) {
            std::printf("UNEXPECTED %s: ok=%d err=%s\n", base.c_str(), (int)ok, err.c_str());
            ++failures;
        }
        std::printf("%s %d %016llx\n", base.c_str(), ok ? (int)tiles.size() : -1,
                    (unsigned long long)hash_tiles(ok ? tiles : std::vector<pfl::Tile>()));
    }
    std::printf(failures ? "layouts_check FAILED\n" : "layouts_check ok\n");
    return failures ? 1 : 0;
}
