// pf_layouts.hpp -- the tile layouts the facade and the command line know: the reference's four
// tables of Main.cpp's main() and layout files.  Host only (no HIP, no pf_depth.h), so the unit
// builds and runs under a host sanitizer on its own (tests/cpp/layouts_check.cpp).
#pragma once

#include <string>
#include <vector>

namespace pfl {

// One tile: the viewing window {az_left, az_right, zen_top, zen_down} and the valid range
// {az_left, az_right, zen_up, zen_down}, radians, as the reference's Vec4f pair.
struct Tile {
    float fov[4];
    float range[4];
};

constexpr int kMaxTiles = 4096;  // pf_set_tiles' limit

// "leres" (Main.cpp:788-843, the active table), "midas" (:731-787), "fold4" (:695-730),
// "fold3" (:845-887), with the reference's float rounding; false for any other name.
bool named(const std::string& name, std::vector<Tile>& tiles);
const char* const* names(int* count);

// A layout file: one tile per line, eight decimal numbers in degrees (the window's az_left
// az_right zen_top zen_down, then the range's az_left az_right zen_up zen_down), separated by
// blanks; '#' starts a comment, blank lines are skipped.  Every value becomes (float)D2R(deg):
// computed in double, rounded once.  false with a message in `err` for a line that does not hold
// exactly eight numbers, a non-finite value, no tiles, or more than kMaxTiles tiles.
bool load_file(const std::string& path, std::vector<Tile>& tiles, std::string& err);

// A known name, else a readable layout file.
bool resolve(const std::string& spec, std::vector<Tile>& tiles, std::string& err);

}  // namespace pfl
