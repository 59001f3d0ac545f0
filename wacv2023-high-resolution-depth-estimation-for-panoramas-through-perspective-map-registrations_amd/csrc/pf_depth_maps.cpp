// pf_depth_maps.cpp -- the host side of the DepthNamespace facade (include/pf_depth.h): the two
// map classes' loads, accessors, window geometry and moves, Metrics::Save/Print, the PNG writers
// and the free projections.  Host-only: no HIP include and no panofuse.h, so the plain host
// compiler builds it with pf_image.cpp and pf_jpeg.cpp (tests/test_maps_sanitized.py runs it
// under AddressSanitizer + UBSan).  The four map members that run on the GPU (CopyInvalidPixels,
// DispDepthConversion, Depth2DepthTransform, D2DTransform) are in pf_depth_gpu.cpp.
#include "../../include/pf_depth.h"
#include "pf_geom.hpp"
#include "pf_image.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>

Vec2f g_zenith_range((float)PF_D2R(26), (float)PF_D2R(154));  // Depth.cpp:22

bool Save16BitPNG(unsigned short* data, int width, int height, const char* filename)
{
    std::string err;
    if (!pfio::save_png16(filename, data, width, height, err)) {
        std::cout << "[Save16BitPNG] " << err << std::endl;
        return false;
    }
    return true;
}

bool Save8BitPNG(const unsigned char* data, int width, int height, const char* filename)
{
    std::string err;
    if (!pfio::save_png8_stb(filename, data, width, height, 1, err)) {
        std::cout << "[Save8BitPNG] " << err << std::endl;
        return false;
    }
    return true;
}

namespace DepthNamespace {

namespace {
// Both Loads (Depth.cpp:56-100, :304-351): the file's samples as floats in 0..1 (u8 / 255,
// u16 / 65535) in a new[] array that replaces `data`; `failed` is the caller's message prefix.
bool load_floats(const std::string& filename, const char* failed, int& width, int& height,
                 int& channels, float*& data)
{
    delete[] data;
    data = nullptr;
    pfio::Image im;
    std::string err;
    if (!pfio::load_image(filename, im, err)) {
        std::cout << failed << err << std::endl;
        return false;
    }
    width = im.w;
    height = im.h;
    channels = im.c;
    const size_t n = (size_t)width * height * channels;
    data = new float[n];
    if (im.is16)
        for (size_t i = 0; i < n; ++i) data[i] = (float)im.px16[i] / 65535.0f;
    else
        for (size_t i = 0; i < n; ++i) data[i] = (float)im.px8[i] / 255.0f;
    return true;
}
}  // namespace

// ---- EquirectangularMap (Depth.cpp:277-575) ----
EquirectangularMap::~EquirectangularMap() { delete[] data; }

bool EquirectangularMap::Load(std::string& filename, bool mono360)
{
    if (filename.size() >= 3 && filename.compare(filename.size() - 3, 3, "pfm") == 0)
        return LoadPfm(filename, mono360, mono360);
    return load_floats(filename, "[EquirectangularMap::Load] failed: ", width, height, channels,
                       data);
}

bool EquirectangularMap::LoadPfm(std::string& filename, bool flip_vertical, bool normalize,
                                 const char* save_png_filename)
{
    std::string err;
    float* img = pfio::load_pfm(filename, &width, &height, &channels, err);
    if (!img) {
        std::cout << "load_pfm() failed? " << err << std::endl;
        return false;
    }
    float mn = FLT_MAX, mx = -FLT_MAX;  // Depth.cpp:468-486
    const size_t n = (size_t)width * height * channels;
    for (size_t i = 0; i < n; ++i) {
        if (img[i] < mn) mn = img[i];
        if (img[i] > mx) mx = img[i];
    }
    delete[] data;
    data = new float[n];
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            for (int c = 0; c < channels; c++) {
                const int sy = flip_vertical ? height - 1 - y : y;
                float val = img[((size_t)sy * width + x) * channels + c];
                if (normalize) {
                    val = (val - mn) / (mx - mn);
                } else {  // cap to 0~10 (Depth.cpp:515-520)
                    if (val < 0) val = 0;
                    val = std::min(val / 10.0f, 10.0f);
                }
                data[((size_t)y * width + x) * channels + c] = val;
            }
    std::free(img);
    if (save_png_filename) {
        std::vector<uint8_t> d((size_t)width * height);
        for (size_t i = 0; i < d.size(); ++i) d[i] = (uint8_t)(data[i * channels] * 255.0f);
        if (!pfio::save_png8(save_png_filename, d.data(), width, height, 1, err))
            std::cout << "[LoadPfm] " << err << std::endl;
    }
    return true;
}

float EquirectangularMap::ValueAtCoord(float azi, float zen)  // Depth.cpp:551-556
{
    const int x = (int)(azi / (PF_MYPI_D * 2) * (float)(width - 1));
    const int y = (int)(zen / PF_MYPI_D * (float)(height - 1));
    return data[((size_t)y * width + x) * channels];
}

float EquirectangularMap::ValueAtXY(int x, int y) { return data[((size_t)y * width + x) * channels]; }

double EquirectangularMap::Avg()  // Depth.cpp:563-583
{
    double avg = 0;
    int count = 0;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const float val = data[((size_t)y * width + x) * channels];
            if (val > 0) {
                avg += val;
                count++;
            }
        }
    if (count == 0) return 0;
    avg /= (float)count;
    return avg;
}

bool EquirectangularMap::Save8bit(std::string& filename)  // Depth.cpp:612-635
{
    if (!data) return false;
    std::vector<uint8_t> d((size_t)width * height);
    for (size_t i = 0; i < d.size(); ++i) {
        float val = data[i * channels];
        if (val < 0) val = 0;
        if (val > 1) val = 1;
        const float p = val * 255.0f;
        d[i] = p != p ? 0 : (uint8_t)p;  // NaN: 0 (undefined in the reference)
    }
    return Save8BitPNG(d.data(), width, height, filename.c_str());
}

// ---- PerspectiveMap (Depth.cpp:45-274) ----
PerspectiveMap::~PerspectiveMap() { delete[] data; }

PerspectiveMap::PerspectiveMap(PerspectiveMap&& o) noexcept { *this = std::move(o); }

PerspectiveMap& PerspectiveMap::operator=(PerspectiveMap&& o) noexcept
{
    if (this != &o) {
        delete[] data;
        width = o.width;
        height = o.height;
        channels = o.channels;
        data = o.data;
        o.data = nullptr;
        azimuth_left = o.azimuth_left;
        azimuth_right = o.azimuth_right;
        zenith_top = o.zenith_top;
        zenith_down = o.zenith_down;
        ranges = o.ranges;
        middle = o.middle;
        hedge = o.hedge;
        vedge = o.vedge;
        corner0 = o.corner0;
        corner1 = o.corner1;
        corner2 = o.corner2;
        corner3 = o.corner3;
        window_set = o.window_set;
    }
    return *this;
}

bool PerspectiveMap::Load(std::string& filename)
{
    return load_floats(filename, "[PerspectiveMap::Load] failed! ", width, height, channels, data);
}

namespace {
Vec3f vec(const pfgeom::V3& v) { return Vec3f(v.x, v.y, v.z); }
pfgeom::V3 v3(const Vec3f& v) { return pfgeom::V3{v.x, v.y, v.z}; }
pfgeom::Window window_of(const PerspectiveMap& p)
{
    pfgeom::Window w;
    w.middle = v3(p.middle);
    w.hedge = v3(p.hedge);
    w.vedge = v3(p.vedge);
    w.corner0 = v3(p.corner0);
    w.corner1 = v3(p.corner1);
    w.corner2 = v3(p.corner2);
    w.corner3 = v3(p.corner3);
    return w;
}
}  // namespace

// The window geometry (Depth.cpp:120-155) on the host, bit-identical to the reference's (and to
// pf_set_tiles, which recomputes it when the map is handed to the library).
void PerspectiveMap::SetWindow(float aL, float aR, float zT, float zD)
{
    azimuth_left = aL;
    azimuth_right = aR;
    zenith_top = zT;
    zenith_down = zD;
    const pfgeom::Window w = pfgeom::set_window(aL, aR, zT, zD);
    middle = vec(w.middle);
    hedge = vec(w.hedge);
    vedge = vec(w.vedge);
    corner0 = vec(w.corner0);
    corner1 = vec(w.corner1);
    corner2 = vec(w.corner2);
    corner3 = vec(w.corner3);
    window_set = true;
}

Vec2f PerspectiveMap::ToSphericalCoord(float x, float y)  // Depth.cpp:157-166
{
    float az, zen;
    pfgeom::to_spherical_coord(window_of(*this), x, y, az, zen);
    return Vec2f(az, zen);
}

Vec2f PerspectiveMap::SphericalTo2D(float azimuth, float zenith)  // Depth.cpp:168-182
{
    float x, y;
    pfgeom::sph_to_2d(window_of(*this), azimuth, zenith, x, y);
    return Vec2f(x, y);
}

bool PerspectiveMap::Contain(float azimuth, float zenith)  // Depth.cpp:184-207
{
    const Vec2f xy = SphericalTo2D(azimuth, zenith);
    const float threshold = 1e-3f;
    return xy.x >= 0 - threshold && xy.x <= 1 + threshold && xy.y >= 0 - threshold &&
           xy.y <= 1 + threshold;
}

float PerspectiveMap::ValueAtXY(int x, int y) { return data[((size_t)y * width + x) * channels]; }

float PerspectiveMap::Value(float x, float y)  // Depth.cpp:111-118
{
    const int X = (int)(x * (float)(width - 1));
    const int Y = (int)(y * (float)(height - 1));
    return data[((size_t)Y * width + X) * channels];
}

// ---- free projection functions (Depth.cpp:2955-2971) ----
Vec3f SphericalToWorld(float azimuth, float zenith) { return vec(pfgeom::sph_to_world(azimuth, zenith)); }

Vec2f WorldToSpherical(Vec3f& p)
{
    pfgeom::V3 q = v3(p);
    float az, zen;
    pfgeom::world_to_sph(q, az, zen);
    p = vec(q);
    return Vec2f(az, zen);
}

// ---- Metrics (Depth.h:161-258) ----
bool Metrics::Save(const char* filename)
{
    FILE* fp = std::fopen(filename, "w+");
    if (!fp) {
        std::cout << "fopen failed?" << std::endl;
        return false;
    }
    auto row = [&](const char* name, float g, float r, bool rel_guard) {
        std::fprintf(fp, "%s_given: %f\n", name, g);
        std::fprintf(fp, "%s_result: %f\n", name, r);
        if (rel_guard) std::fprintf(fp, "%s diff: %f\n", name, (r - g) / g);
    };
    row("mse", mse_given, mse_result, mse_given != 0);
    row("mae", mae_given, mae_result, mae_given != 0);
    row("mre", mre_given, mre_result, mre_given != 0);
    row("mselog", mselog_given, mselog_result, mselog_given != 0);
    row("delta1", delta1_given, delta1_result, delta1_given != 0);
    row("delta2", delta2_given, delta2_result, delta2_given != 0);
    row("delta3", delta3_given, delta3_result, delta1_given != 0);  // sic, Depth.h:238
    std::fclose(fp);
    return true;
}

void Metrics::Print()
{
    std::cout << "RMSE " << std::sqrt(mse_given) << "->" << std::sqrt(mse_result) << " ("
              << (std::sqrt(mse_result) - std::sqrt(mse_given)) / std::sqrt(mse_given)
              << ") MAE " << mae_given << "->" << mae_result << " ("
              << (mae_result - mae_given) / mae_given << ") MRE " << mre_given << "->"
              << mre_result << " (" << (mre_result - mre_given) / mre_given << ") RMSElog "
              << std::sqrt(mselog_given) << "->" << std::sqrt(mselog_result) << " ("
              << (std::sqrt(mselog_result) - std::sqrt(mselog_given)) / std::sqrt(mselog_given)
              << ") deltas:" << delta1_given << "->" << delta1_result << "("
              << (delta1_result - delta1_given) << ") , " << delta2_given << "->"
              << delta2_result << "(" << (delta2_result - delta2_given) << ") , "
              << delta3_given << "->" << delta3_result << "(" << (delta3_result - delta3_given)
              << std::endl;
}

}  // namespace DepthNamespace
