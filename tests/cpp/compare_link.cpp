// A caller of include/pf_depth.h for tests/test_compare_link.py: links against
// libpanofuse_depth.so and uses the entry points that came with ErrorCompare, none of which needs
// a GPU here.
//   compare_link <dir>
// 1. DepthNamespace::ErrorCompare with the reference's signature (Depth.h:318-319) on a gt file
//    that does not exist: must return false after "cannot load emap_gt? ..." -- the loads come
//    before any GPU call.  Prints "RET <0|1>".
// 2. EquirectangularMap::Save8bit of a hand-filled 5x3 map (float)i * 0.1f - 0.25f (values below
//    0 and above 1) to <dir>/save8.png.  Prints "SAVE <0|1>".
#include "../../include/pf_depth.h"

#include <cstdio>
#include <iostream>
#include <string>

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string dir(argv[1]);
    std::string gt = dir + "/no_such_gt.png", given = dir + "/no_such_given.png";
    const std::string shifted = dir + "/shifted.png";
    float v[7] = {0, 0, 0, 0, 0, 0, 0};
    const bool ret = DepthNamespace::ErrorCompare(gt, given, true, v[0], v[1], v[2], v[3], v[4],
                                                  v[5], v[6], 1, true, shifted.c_str());
    std::cout << "RET " << (ret ? 1 : 0) << std::endl;

    DepthNamespace::EquirectangularMap m;
    m.width = 5;
    m.height = 3;
    m.channels = 1;
    m.data = new float[15];
    for (int i = 0; i < 15; ++i) m.data[i] = (float)i * 0.1f - 0.25f;
    std::string out = dir + "/save8.png";
    std::cout << "SAVE " << (m.Save8bit(out) ? 1 : 0) << std::endl;
    return 0;
}
