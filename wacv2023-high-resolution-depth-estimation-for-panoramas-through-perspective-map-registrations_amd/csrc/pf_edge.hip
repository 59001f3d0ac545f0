// Edge-fidelity metrics of a depth map against ground truth: DepthNamespace::ErrorLaplacian
// (Depth.cpp:2636-2953).  Per pixel (x, y) of the given map the reference compares, between the
// gt (sampled at X = (int)((float)x * ratio_x), Y likewise) and the given map,
//   * the 3x3 Laplacian  c - (l + r + u + d) / 4            (mse and mae), x in [1, w-2],
//   * Sobel X and Sobel Y                                   (mae each),    y in [1, h-2];
//   * a 5x5 LoG filter (13 taps)                            (mae),         [2, w-3] x [2, h-3].
// Every tap is a float widened to double and every expression is evaluated in fp64 in the
// reference's left-to-right order (the library is built with -ffp-contract=off), so the
// per-pixel terms are the reference's bit for bit.  A sample counts when its gt taps are valid
// ((double)tap >= 1e-4): the five cross taps for the Laplacian, all 25 for the LoG, and for Sobel
// the reference's list as written (Depth.cpp:2747-2748: val[0][1] and val[0][2] are tested twice,
// val[1][0] and val[2][0] never) -- reproduced, not corrected.
//
// One block per ETX x ETY tile of the given map; the tile plus a 2-pixel halo is staged in LDS.
// When the gt has the given map's size (ratio 1: the result-against-gt case) its tile is staged
// the same way, so each input is read from HBM once; any other ratio gathers the gt taps.  Sums:
// fp64 per lane, wave_sum, per-block partials in the workspace, one block per panorama adds them
// in a fixed order (no atomics: deterministic), as k_err_sums / k_err_final in pf_metrics.hip.
#include "pf_internal.hpp"

namespace pf {

namespace {

constexpr int EB = 256;               // threads per block
constexpr int EHALO = 2;              // the 5x5 window's reach
constexpr int ELW = EDGE_TILE_X + 2 * EHALO, ELH = EDGE_TILE_Y + 2 * EHALO;  // staged tile
constexpr int NES = 8;                // lap d^2, lap |d|, sobel x, sobel y, LoG, n_lap, n_sobel, n_lap5
constexpr int ERPT = EDGE_TILE_Y / (EB / EDGE_TILE_X);  // rows per thread
static_assert(EB % EDGE_TILE_X == 0 && (EDGE_TILE_X & (EDGE_TILE_X - 1)) == 0 && EDGE_TILE_X % 64 == 0 &&
                  EDGE_TILE_Y % (EB / EDGE_TILE_X) == 0,
              "whole waves per tile row, whole columns per thread");

struct EArgs {
    const float* gt;
    int gw, gh, gc;
    long long gstride;
    const float* gv;        // float given map (channel 0 of gvc) ...
    const uint16_t* gv16;   // ... or the u16 result
    int w, h, gvc;
    long long vstride;
    float rx, ry;           // (float)gt.width / (float)w, (float)gt.height / (float)h
    double *gt_lap, *gv_lap, *lap_ae;  // optional [batch][h][w] planes
};

__device__ __forceinline__ double edge_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The filters over a 5x5 window W[i][j] (column i, row j; the centre is W[2][2]).  The 3x3
// window val[a][b] of Depth.cpp:2702-2711 is W[a + 1][b + 1].
__device__ __forceinline__ double lap3(const double (&W)[5][5])
{  // Depth.cpp:2723, :2730
    return 1 * W[2][2] - (W[1][2] + W[3][2] + W[2][1] + W[2][3]) / 4;
}
__device__ __forceinline__ double sobel_x(const double (&W)[5][5])
{  // Depth.cpp:2753, :2768
    return W[1][1] - W[3][1] + 2 * W[1][2] - 2 * W[3][2] + W[1][3] - W[3][3];
}
__device__ __forceinline__ double sobel_y(const double (&W)[5][5])
{  // Depth.cpp:2754, :2769
    return W[1][1] + 2 * W[2][1] + W[3][1] - W[1][3] - 2 * W[2][3] - W[3][3];
}
__device__ __forceinline__ double log5(const double (&W)[5][5])
{  // Depth.cpp:2904-2906, :2935-2937
    return -1 * W[2][0] - 1 * W[1][1] - 2 * W[2][1] - 1 * W[3][1]
        - 1 * W[0][2] - 2 * W[1][2] + 16 * W[2][2] - 2 * W[3][2] - 1 * W[4][2]
        - 1 * W[1][3] - 2 * W[2][3] - 1 * W[3][3] - 1 * W[2][4];
}

// (double)tap < 1e-4 decided in fp32: 1e-4 lies strictly between two neighbouring floats, so the
// test is tap <= the lower one (false for NaN either way).
constexpr float VALID_BELOW = 0x1.a36e2ep-14f, VALID_FROM = 0x1.a36e30p-14f;
static_assert((double)VALID_BELOW < 1e-4 && (double)VALID_FROM >= 1e-4, "neighbours of 1e-4");
static_assert(__builtin_bit_cast(uint32_t, VALID_FROM) == __builtin_bit_cast(uint32_t, VALID_BELOW) + 1,
              "adjacent floats");

// One thread walks down a column of its tile, ERPT rows, with the 5x5 windows of both maps in
// registers (doubles): a step shifts the windows up one row and reads one new row of five taps
// per map, so a pixel costs 10 tap reads and conversions instead of 38.  bad[j] holds the
// validity bits of gt window row j (bit i = column i invalid).
// STAGED: the gt has the given map's geometry (rx == ry == 1, so X == x and Y == y exactly) and
// its tile sits in LDS beside the given map's; else the gt taps are gathered from memory, a tap
// outside the gt map reading as 0 (invalid) -- the range tests below skip those samples anyway.
template <bool STAGED>
__global__ __launch_bounds__(EB) void k_edge_sums(EArgs a, double* part)
{
    __shared__ float sv[ELH][ELW];
    __shared__ float sg[STAGED ? ELH : 1][STAGED ? ELW : 1];
    __shared__ double red[EB / 64][NES];
    const int b = blockIdx.z;
    const int x0 = blockIdx.x * EDGE_TILE_X, y0 = blockIdx.y * EDGE_TILE_Y;
    const float* gt = a.gt + (long long)b * a.gstride;

    // the tile and its halo; pixels outside the map are zeros that no counted sample reads
#pragma unroll 4
    for (int i = threadIdx.x; i < ELH * ELW; i += EB) {
        const int ly = i / ELW, lx = i - ly * ELW;
        const int x = x0 - EHALO + lx, y = y0 - EHALO + ly;
        float v = 0.0f, g = 0.0f;
        if (x >= 0 && x < a.w && y >= 0 && y < a.h) {
            const long long p = (long long)y * a.w + x;
            if (a.gv16)
                v = u16_unit(a.gv16[(long long)b * a.vstride + p]);  // Depth.cpp:322
            else
                v = a.gv[(long long)b * a.vstride + p * a.gvc];
            if (STAGED) g = gt[p * a.gc];
        }
        sv[ly][lx] = v;
        if (STAGED) sg[ly][lx] = g;
    }
    __syncthreads();

    double s[5] = {0, 0, 0, 0, 0};
    uint32_t cn[3] = {0, 0, 0};
    const int lx = threadIdx.x & (EDGE_TILE_X - 1);
    const int ly0 = (threadIdx.x / EDGE_TILE_X) * ERPT;
    const int x = x0 + lx;
    // inner columns (Depth.cpp:2687, :2841) and the range tests on the gt columns (:2698,
    // :2856; the 5x5 test as written leaves X3/X4 and Y3/Y4 unchecked, so the outermost tap is
    // bounded here as well: a sample is skipped, never read out of range)
    bool okx3 = x >= 1 && x <= a.w - 2, okx5 = x >= 2 && x <= a.w - 3;
    int IX[5] = {0, 0, 0, 0, 0};
    bool inx[5] = {true, true, true, true, true};
    if (!STAGED) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            IX[i] = (int)((float)(x - 2 + i) * a.rx);
            inx[i] = IX[i] >= 0 && IX[i] <= a.gw - 1;
        }
        okx3 = okx3 && !(IX[1] < 0 || IX[3] > a.gw - 1);
        okx5 = okx5 && !(IX[0] < 0 || IX[2] > a.gw - 1) && !(IX[4] > a.gw - 1);
    }

    double G[5][5], V[5][5];  // [column][row]
    uint32_t bad[5];
    int IY[5] = {0, 0, 0, 0, 0};
    // row j of the windows <- tile row r (map row y0 - 2 + r)
    auto load_row = [&](int j, int r) {
        uint32_t m = 0;
        if (!STAGED) IY[j] = (int)((float)(y0 - EHALO + r) * a.ry);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            float g = 0.0f;
            if (STAGED) {
                g = sg[r][lx + i];
            } else if (inx[i] && IY[j] >= 0 && IY[j] <= a.gh - 1) {
                g = gt[((long long)IY[j] * a.gw + IX[i]) * a.gc];
            }
            m |= (g <= VALID_BELOW ? 1u : 0u) << i;
            G[i][j] = (double)g;
            V[i][j] = (double)sv[r][lx + i];
        }
        bad[j] = m;
    };
#pragma unroll
    for (int j = 1; j < 5; ++j) load_row(j, ly0 + j - 1);

#pragma unroll
    for (int k = 0; k < ERPT; ++k) {
        const int ly = ly0 + k, y = y0 + ly;
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // the windows move down one row
#pragma unroll
            for (int i = 0; i < 5; ++i) G[i][j] = G[i][j + 1], V[i][j] = V[i][j + 1];
            bad[j] = bad[j + 1];
            IY[j] = IY[j + 1];
        }
        load_row(4, ly + 4);
        if (y >= a.h) break;  // block-uniform per wave: the rest of the column is outside
        bool ok3 = okx3 && y >= 1 && y <= a.h - 2;
        bool ok5 = okx5 && y >= 2 && y <= a.h - 3;
        if (!STAGED) {
            ok3 = ok3 && !(IY[1] < 0 || IY[3] > a.gh - 1);
            ok5 = ok5 && !(IY[0] < 0 || IY[2] > a.gh - 1) && !(IY[4] > a.gh - 1);
        }
        // Depth.cpp:2716: the five cross taps
        const bool lap_ok = ok3 && !((bad[1] & 0x04u) | (bad[2] & 0x0Eu) | (bad[3] & 0x04u));
        // Depth.cpp:2747-2748 as written: val[0][0], val[0][1], val[0][2], val[1][1], val[2][1],
        // val[1][2], val[2][2] (val[1][0] and val[2][0] are never tested); val[p][q] is column
        // p + 1 of row q + 1 here
        const bool sob_ok = ok3 && !((bad[1] & 0x02u) | (bad[2] & 0x0Eu) | (bad[3] & 0x0Eu));
        const bool log_ok = ok5 && !(bad[0] | bad[1] | bad[2] | bad[3] | bad[4]);

        const double gl = lap_ok ? lap3(G) : 0.0, vl = lap_ok ? lap3(V) : 0.0;
        const double d = gl - vl, ae = fabs(d);
        s[0] += d * d;  // pow(d, 2); an exact 0 where the sample does not count
        s[1] += ae;
        cn[0] += lap_ok;
        s[2] += sob_ok ? fabs(sobel_x(G) - sobel_x(V)) : 0.0;
        s[3] += sob_ok ? fabs(sobel_y(G) - sobel_y(V)) : 0.0;
        cn[1] += sob_ok;
        s[4] += log_ok ? fabs(log5(G) - log5(V)) : 0.0;
        cn[2] += log_ok;
        if (x < a.w && (a.gt_lap || a.gv_lap || a.lap_ae)) {  // Depth.cpp:2737-2742, 0 elsewhere
            const long long o = ((long long)b * a.h + y) * a.w + x;
            if (a.gt_lap) a.gt_lap[o] = gl;
            if (a.gv_lap) a.gv_lap[o] = vl;
            if (a.lap_ae) a.lap_ae[o] = ae;
        }
    }

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < NES; ++k) {
        const double v = edge_wave_sum(k < 5 ? s[k] : (double)cn[k - 5]);
        if (lane == 0) red[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NES) {
        double v = 0;
        for (int w = 0; w < EB / 64; ++w) v += red[w][threadIdx.x];
        const long long blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
        const long long nblk = (long long)gridDim.x * gridDim.y;
        part[((long long)b * nblk + blk) * NES + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(EB) void k_edge_final(const double* part, long long nblk,
                                                   pf_edge_metrics* out)
{
    const int b = blockIdx.x;
    __shared__ double col[NES];
    // column k by the 64 lanes of one wave (strided, then a fixed-shape tree): a fixed order
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = wv; k < NES; k += EB / 64) {
        double v = 0;
        for (long long i = lane; i < nblk; i += 64) v += part[((long long)b * nblk + i) * NES + k];
        v = edge_wave_sum(v);
        if (lane == 0) col[k] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    pf_edge_metrics m;
    m.n_lap = (int64_t)col[5];  // integer-valued sums: exact in any order
    m.n_sobel = (int64_t)col[6];
    m.n_lap5 = (int64_t)col[7];
    m.lap_mse = col[0] / (double)m.n_lap;  // Depth.cpp:2944-2948: 0 / 0 = NaN with no sample
    m.lap_mae = col[1] / (double)m.n_lap;
    m.sobelx_mae = col[2] / (double)m.n_sobel;
    m.sobely_mae = col[3] / (double)m.n_sobel;
    m.lap5_mae = col[4] / (double)m.n_lap5;
    out[b] = m;
}

long long edge_blocks(const EdgeJob& j)
{
    const long long tx = (j.w + EDGE_TILE_X - 1) / EDGE_TILE_X, ty = (j.h + EDGE_TILE_Y - 1) / EDGE_TILE_Y;
    return tx * ty;
}

}  // namespace

bool edge_staged(const EdgeJob& j) { return j.gw == j.w && j.gh == j.h; }

size_t edge_workspace_bytes(const EdgeJob& j)
{
    return sizeof(double) * NES * (size_t)edge_blocks(j) * j.batch + 256;
}

void launch_edge(hipStream_t s, const EdgeJob& j, void* ws, pf_edge_metrics* out)
{
    EArgs a;
    a.gt = j.gt;
    a.gw = j.gw;
    a.gh = j.gh;
    a.gc = j.gc;
    a.gstride = (long long)j.gw * j.gh * j.gc;
    a.gv = j.given;
    a.gv16 = j.given16;
    a.w = j.w;
    a.h = j.h;
    a.gvc = j.given16 ? 1 : j.gc_given;
    a.vstride = (long long)j.w * j.h * a.gvc;
    a.rx = (float)j.gw / (float)j.w;  // Depth.cpp:2654-2655
    a.ry = (float)j.gh / (float)j.h;
    a.gt_lap = j.gt_lap;
    a.gv_lap = j.given_lap;
    a.lap_ae = j.lap_ae;
    double* part = (double*)ws;
    const dim3 grid((j.w + EDGE_TILE_X - 1) / EDGE_TILE_X, (j.h + EDGE_TILE_Y - 1) / EDGE_TILE_Y,
                    j.batch);
    if (edge_staged(j))
        hipLaunchKernelGGL(k_edge_sums<true>, grid, dim3(EB), 0, s, a, part);
    else
        hipLaunchKernelGGL(k_edge_sums<false>, grid, dim3(EB), 0, s, a, part);
    hipLaunchKernelGGL(k_edge_final, dim3(j.batch), dim3(EB), 0, s, part, edge_blocks(j), out);
}

}  // namespace pf
