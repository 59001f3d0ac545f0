// pf_depth_c.cpp -- the C-ABI helpers of include/pf_depth.h for the ctypes bindings and the
// tests: the loads, the decoders and writers behind them, the layouts as plain float arrays.
#include "pf_facade.hpp"
#include "pf_image.hpp"

#include <cstring>

extern "C" int pfd_load_map(const char* fn, int is_emap, float* out, long long cap, int* w, int* h,
                            int* c)
{
    std::string f(fn);
    DepthNamespace::EquirectangularMap e;
    DepthNamespace::PerspectiveMap p;
    const bool ok = is_emap ? e.Load(f) : p.Load(f);
    if (!ok) return -1;
    const int W = is_emap ? e.width : p.width, H = is_emap ? e.height : p.height,
              C = is_emap ? e.channels : p.channels;
    *w = W;
    *h = H;
    *c = C;
    const long long n = (long long)W * H * C;
    if (out && cap >= n) std::memcpy(out, is_emap ? e.data : p.data, sizeof(float) * n);
    return 0;
}

extern "C" int pfd_decode_image(const char* fn, void* out, long long cap, int* w, int* h, int* c,
                                int* is16)
{
    pfio::Image im;
    std::string err;
    if (!pfio::load_image(fn, im, err)) {
        std::cout << "[pfd_decode_image] " << err << std::endl;
        return -1;
    }
    *w = im.w;
    *h = im.h;
    *c = im.c;
    *is16 = im.is16 ? 1 : 0;
    const long long n = (long long)im.w * im.h * im.c * (im.is16 ? 2 : 1);
    if (!out || cap < n) return -2;
    std::memcpy(out, im.is16 ? (const void*)im.px16.data() : (const void*)im.px8.data(), n);
    return 0;
}

extern "C" int pfd_is_16_bit(const char* fn) { return pfio::is_16bit(fn) ? 1 : 0; }

extern "C" int pfd_save_jpeg(const char* fn, const uint8_t* px, int w, int h, int c, int quality,
                             int flip)
{
    std::string err;
    if (!pfio::save_jpeg(fn, px, w, h, c, quality, err, flip != 0)) {
        std::cout << "[pfd_save_jpeg] " << err << std::endl;
        return -1;
    }
    return 0;
}

extern "C" int pfd_save_png16(const char* fn, const uint16_t* data, int w, int h)
{
    return Save16BitPNG(const_cast<unsigned short*>(data), w, h, fn) ? 0 : -1;
}

extern "C" int pfd_layout(const char* name, float* fovs, float* ranges, int cap)
{
    std::vector<Vec4f> f, r;
    std::string err;
    if (!name || !pf_resolve_layout(name, f, r, &err)) {
        std::cout << "[pfd_layout] " << (name ? err : std::string("NULL name")) << std::endl;
        return -1;
    }
    const int n = (int)f.size();
    if ((fovs || ranges) && cap < n) return -1;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 4; ++k) {
            if (fovs) fovs[4 * i + k] = f[i][k];
            if (ranges) ranges[4 * i + k] = r[i][k];
        }
    return n;
}

extern "C" void pfd_leres_layout(float* fovs, float* ranges)
{
    pfd_layout("leres", fovs, ranges, 15);  // Main.cpp:788-843: 15 tiles
}

extern "C" void pfd_rgb_tile_size(const float* fov, int* w, int* h)
{
    pff::rgb_tile_size(Vec4f(fov[0], fov[1], fov[2], fov[3]), *w, *h);
}
