// pf_weight.hip -- per-pixel tile weights: the kernel that fills a weight set (k_tent_weights,
// pf_tile_tent_weights).  The kernels that read weights are the third registration form
// (k_register_weighted, pf_register.hip) and the weighted gathers (pf_targets.hip).
#include "pf_internal.hpp"

namespace pf {

// The classic blending tent in tile pixel space: for a w x h tile, pixel (x, y) gets
// min(t, m) / m with t = min(min(x + 1, w - x), min(y + 1, h - y)) and m = (min(w, h) + 1) / 2 in
// integers, one fp32 division, values in (0, 1].  Channel 0 of the tiles' element layout; the
// other channels are written 0.
__global__ void __launch_bounds__(256) k_tent_weights(const TileGeom* __restrict__ geom,
                                                      float* __restrict__ weights)
{
    const int p = blockIdx.y;
    const TileGeom g = geom[p];
    const long long npx = (long long)g.w * g.h;
    const int m = (min(g.w, g.h) + 1) / 2;
    float* o = weights + g.off;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npx;
         i += (long long)gridDim.x * 256) {
        const int x = (int)(i % g.w), y = (int)(i / g.w);
        const int t = min(min(x + 1, g.w - x), min(y + 1, g.h - y));
        o[i * g.c] = (float)min(t, m) / (float)m;
        for (int ch = 1; ch < g.c; ch++) o[i * g.c + ch] = 0.0f;
    }
}

void launch_tent_weights(hipStream_t s, const TileGeom* geom, int ntiles, long long tile_pixels,
                         float* weights)
{
    long long gx = (tile_pixels / (ntiles > 0 ? ntiles : 1) + 255) / 256;
    if (gx > 1024) gx = 1024;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(k_tent_weights, dim3((unsigned)gx, (unsigned)ntiles), dim3(256), 0, s, geom,
                       weights);
}

}  // namespace pf
