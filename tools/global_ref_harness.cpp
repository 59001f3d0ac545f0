// Calls the reference's own DepthNamespace::SolveDepthToDepth2, MedianScaling and
// EquirectangularMap::CopyInvalidPixels on raw arrays read from files.  Compiled by
// tools/make_global_golden.py together with the unmodified reference Depth.cpp and the vendored
// Ceres (never committed); Basic.h comes first, as in the reference's Main.cpp.
//   global_ref_harness fit    <emap.f32> ew eh ec <data.u16> w h zr0 zr1
//       the reference's own "[SolveDepthToDepth2] ..." line, then "FIT a b c d" at %.9g
//   global_ref_harness median <m0.f32> w0 h0 c0 <m1.f32> w1 h1 c1 <out.f32>
//       "MED ret m0 m1" at %.9g; the scaled map 0 to <out.f32>
//   global_ref_harness mask   <dst.f32> w h c <ref.f32> rw rh rc <out.f32>
//       the masked map to <out.f32>
// zr0 / zr1 are the bit patterns of the two floats as unsigned decimal.
#include "Basic.h"
#include "ILMBase.h"
#include "Depth.h"
#define STB_IMAGE_IMPLEMENTATION
#include "stb_image.h"
#define STB_IMAGE_WRITE_IMPLEMENTATION
#include "stb_image_write.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

template <class T>
static T* read_all(const char* fn, size_t n)
{
    T* p = new T[n];
    FILE* f = std::fopen(fn, "rb");
    if (!f || std::fread(p, sizeof(T), n, f) != n) {
        std::fprintf(stderr, "cannot read %zu elements of %s\n", n, fn);
        std::exit(4);
    }
    std::fclose(f);
    return p;
}

static void load(DepthNamespace::EquirectangularMap& m, char** a)
{
    m.width = std::atoi(a[1]);
    m.height = std::atoi(a[2]);
    m.channels = std::atoi(a[3]);
    m.data = read_all<float>(a[0], (size_t)m.width * m.height * m.channels);
}

static void store(const DepthNamespace::EquirectangularMap& m, const char* fn)
{
    FILE* f = std::fopen(fn, "wb");
    if (!f) std::exit(5);
    std::fwrite(m.data, sizeof(float), (size_t)m.width * m.height * m.channels, f);
    std::fclose(f);
}

static float from_bits(const char* s)
{
    const unsigned u = (unsigned)std::strtoul(s, nullptr, 10);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string mode(argv[1]);
    if (mode == "fit" && argc == 11) {
        DepthNamespace::EquirectangularMap emap;
        load(emap, argv + 2);
        const int w = std::atoi(argv[7]), h = std::atoi(argv[8]);
        unsigned short* data = read_all<unsigned short>(argv[6], (size_t)w * h);
        Vec2f zr(from_bits(argv[9]), from_bits(argv[10]));
        Vec4f abcd(0, 0, 0, 0);
        if (!DepthNamespace::SolveDepthToDepth2(emap, data, w, h, zr, abcd)) return 1;
        std::cout.flush();
        std::printf("FIT %.9g %.9g %.9g %.9g\n", abcd[0], abcd[1], abcd[2], abcd[3]);
        delete[] data;
        return 0;
    }
    if (mode == "median" && argc == 11) {
        DepthNamespace::EquirectangularMap m0, m1;
        load(m0, argv + 2);
        load(m1, argv + 6);
        float a = 0, b = 0;
        const bool ok = DepthNamespace::MedianScaling(m0, m1, &a, &b);
        std::cout.flush();
        std::printf("MED %d %.9g %.9g\n", ok ? 1 : 0, a, b);
        store(m0, argv[10]);
        return 0;
    }
    if (mode == "mask" && argc == 11) {
        DepthNamespace::EquirectangularMap dst, ref;
        load(dst, argv + 2);
        load(ref, argv + 6);
        dst.CopyInvalidPixels(ref);
        store(dst, argv[10]);
        return 0;
    }
    return 2;
}
