// Calls the reference's own DepthNamespace::ErrorLaplacian on two image files and prints its five
// outputs at full precision.  Compiled by tools/make_edge_golden.py together with the unmodified
// reference Depth.cpp (never committed); Basic.h comes first, as in the reference's Main.cpp.
#include "Basic.h"
#include "ILMBase.h"
#include "Depth.h"
#define STB_IMAGE_IMPLEMENTATION
#include "stb_image.h"
#define STB_IMAGE_WRITE_IMPLEMENTATION
#include "stb_image_write.h"

#include <cstdio>

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    std::string gt(argv[1]), given(argv[2]);
    double v[5];
    if (!DepthNamespace::ErrorLaplacian(gt, given, v[0], v[1], v[2], v[3], v[4])) return 1;
    std::printf("EDGE %.17g %.17g %.17g %.17g %.17g\n", v[0], v[1], v[2], v[3], v[4]);
    return 0;
}
