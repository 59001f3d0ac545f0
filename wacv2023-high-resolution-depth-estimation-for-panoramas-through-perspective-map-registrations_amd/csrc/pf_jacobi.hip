// pf_jacobi.hip -- register-streaming, temporally blocked damped-Jacobi engine for gfx950.
//
// The reference runs `iters` sweeps per level, each a full read-modify-write of the buffer
// (Depth.cpp:1680-1717).  Here one launch ("pass") advances the band by T sweeps:
//
//  * A wave owns a vertical strip of 128 virtual columns (two per lane, kJC) and streams down a
//    chunk of rows.  Step k consumes input row k - 1 (loaded 2-3 steps ahead; the L rows up to 3
//    steps ahead, straight into their ring: "Load schedule" below) and, for every sweep level t
//    = 1..T, produces row
//    k-2t of level t from rows k-2t-1..k-2t+1 of level t-1, which it keeps in registers (a 3-row
//    ring per level).  Horizontal neighbours cross lanes with DPP wave_shr/wave_shl moves.  L rows
//    come through a ring as well: in registers (JLag) or in per-stage LDS (JPipe); no barriers
//    inside a wave's stream.
//  * Columns are "virtual": virtual column x of row Y is linear pixel Y*w + x, so x < 0 or
//    x >= w wraps into the neighbouring row -- exactly the reference's buffer[yy*width + xx]
//    addressing (the seam quirk of SURVEY.md Appendix A item 5 comes out for free).
//  * Each strip carries a halo of Tp >= T virtual columns on both sides and each row chunk a halo
//    of T rows; values in the halo go stale sweep by sweep and are never stored.
//  * Only band pixels (h0*w <= i < (h1+1)*w) are stored.  A band pixel never reads a pixel
//    outside the band (covered pixels sit in rows h0+1..h1-1), so out-of-band cells may hold
//    anything.
//  * The first pass of a level reads its input straight from the level-0 seed (emap gather) or
//    the 2x nearest upsample of the previous level; the last pass of the last level writes the
//    u16 quantisation (Depth.cpp:1721-1736) instead of floats.
//
// Per pixel the arithmetic is the reference's, in its order, fp32, no contraction:
//   Lcur = ((((W*-1/4) + N*-1/4) + Ctr) + S*-1/4) + E*-1/4    (std::map key order)
//   t = b + (L - Lcur)*0.5;  b' = clamp01(t*(1-1e-4) + b*1e-4)
// with Lcur = L = 0 for an un-windowed pixel.  (The reference starts Lcur at 0; 0 + W*-1/4 can
// differ from W*-1/4 only in the sign of a zero, which cannot reach b' because b is never -0.)
//
// Variants that were built, measured slower (or no faster) on MI355X and removed; each result is
// in DESIGN.md §3, the code in this file's history:
//  * three and four columns per lane (general and packed forms);
//  * run-time gating of the levels a step does not need (the compile-time fill / drain stayed);
//  * non-temporal stores of the finished rows;
//  * JLag's L ring in LDS (the register ring is faster at every depth built);
//  * one drain copy per ring group, and the ring rotation by binary parts;
//  * the E tap as a DPP move plus a v_fmac_f32 instead of one v_fmac_f32_dpp.
// The numeric tunables below are what tools/build_variant.sh A/B builds still vary.
#include "pf_internal.hpp"

#include <cstdlib>
#include <cstring>

#ifndef PF_JLAG_WAVES
#define PF_JLAG_WAVES 1  // __launch_bounds__ min waves per SIMD of the lagged kernel
#endif
#ifndef PF_JPK_GROUP
#define PF_JPK_GROUP 3  // levels per stage-wise group of the packed form (VGPR bound: 3 waves/SIMD)
#endif
#ifndef PF_JFILL
// the first PF_JFILL 6-step groups of a row chunk's lagged fill run as their own unrolled steps
// with the levels they do not need compiled out (JLag::fill_from); 0 = off, -1 = per depth
#define PF_JFILL -1
#endif
#ifndef PF_JDRAIN
// the last PF_JDRAIN 6-step groups of a row chunk with the idle shallow levels compiled out (the
// last group alone holds 39 of the 45 idle level-steps at T = 10); 0 = off
#define PF_JDRAIN 1
#endif
#ifndef PF_JLAG_WAVES_FAST
// the packed passes: 3 waves per SIMD (<= 168 VGPRs).  With the drain compiled out (PF_JDRAIN)
// hipcc's free allocation lands at 168-171 (checked in the ISA); the bound holds it at 168
#define PF_JLAG_WAVES_FAST 3
#endif
#ifndef PF_JPIPE_FILL
#define PF_JPIPE_FILL 3  // fill groups of the pipelined engine (PF_JFILL = -1)
#endif
#ifndef PF_JLAG_PF
// steps of lead of JLag's input row loads, at most: 2 or 3.  The PF + 1 load buffers are
// indexed by ring group plus phase, so their period has to divide the L ring's R rows, not the
// 6-step unroll; a depth whose R it does not divide keeps 3 buffers (JLag::NB)
#define PF_JLAG_PF 3
#endif
// JPipe's lead for the input and L row loads: its buffers are indexed by phase alone, so the
// period PF + 1 must divide the 6-step unroll
#define PF_JPIPE_PF 2
static_assert(6 % (PF_JPIPE_PF + 1) == 0, "the 6-step unroll needs a load-buffer period dividing 6");
static_assert(PF_JLAG_PF == 2 || PF_JLAG_PF == 3, "JLag's input lead");

namespace pf {

namespace {

__device__ __forceinline__ float dpp_from_left(float v)
{  // lane i <- lane i-1 (wave_shr:1)
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_from_right(float v)
{  // lane i <- lane i+1 (wave_shl:1)
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x130, 0xF, 0xF, true));
}

typedef float f2 __attribute__((ext_vector_type(2)));

// A lane's column pair as one vector value: the general form reads the elements .v[j], the
// packed form operates on .v directly (an array member here defeats scalar replacement of the
// level rings and sends them to scratch).
struct Row {
    f2 v;
};

}  // namespace

// Source of a pass's input rows.
enum { SRC_BUF = 0, SRC_UPSAMPLE = 1, SRC_SEED = 2 };

// ---------------------------------------------------------------------------------------------
// Lagged streaming: sweep level t produces row k-2t at step k (two rows behind level t-1), so
// every level reads only rows finished in earlier steps and the 2T updates of a step are
// independent (no intra-step dependency chain).  Level t keeps a 3-row ring.  The step loop is
// unrolled by 6, over the R/6 groups of the L ring's period, so every register ring index is a
// compile-time constant.
//
// L rows live in a ring of R >= 2T+1 rows (row r in slot r % R): each L row is loaded from memory
// once and read T times from the ring.
//
// Load schedule.  Step k issues two 512-B row loads per wave: L row k + LL straight into its ring
// slot (LL = min(3, R - 2T - 1): that slot's old row was last read a step ago or earlier) and
// input row k + PF - 1 into one of NB = PF + 1 buffers indexed by ring group plus phase (PF = 3
// where 4 divides R, else 2).  The step's first instructions consume input row k - 1 and sanitise
// L row k - 2 in place, so both loads have had PF / LL + 2 steps.  Loads return in order, so the
// wait for the input row also waits for every load issued before it: at T = 10 a wave has 6 rows
// (3 KB) in flight at that wait (s_waitcnt vmcnt(6) in the ISA).  No L staging buffers: the
// T = 10 packed passes fit 3 waves per SIMD without scratch.  Measurements: DESIGN.md §3.
//
// Two arithmetic forms of the same update (bit-identical results):
//  * FAST (packed): the two columns of a lane are one v_pk_* operand pair; the taps that cross
//    lanes are scalar DPP ops (the count is at JLag::sweep_packed_group).  A packed op moves two
//    lanes of data at about the issue cost of a scalar op on gfx950 (tools/ubench/valu_rate.hip).
//    The un-windowed mask is geometric: t = fma(d, H, b) with H = 0.5 on windowed pixels and 0 on
//    un-windowed ones (0 * finite = 0, b + 0 = b exactly).  H = Hcol(column) * Hrow(row) needs
//    the host's separable-coverage certificate (prepare_levels in pf_layout.hip): a band pixel is
//    covered iff its row is in h0+1..h1-1 and its column in a fixed set that excludes column 0
//    (true of the reference's layouts: column 0 and the columns past the 359.9-degree cap are
//    uncovered).  L rows are sanitised in the ring so that d stays finite where H = 0: L is set
//    to 0 exactly there (the un-windowed marker is a NaN), and kept as loaded where H = 0.5, so
//    an infinite target on a covered pixel saturates the pixel to 0 or 1 as in the reference.
//  * general: scalar ops, mask from the marker in L (cmp + cndmask per pixel), any coverage.  It
//    runs where the certificate is missing, and under PF_JSLOW.
__device__ __forceinline__ f2 pk_add_clamp01(f2 a, f2 b)
{  // v_pk_add_f32 with the output clamp: both lanes clamped to [0, 1] (b' = clamp01(...))
    f2 r;
    asm("v_pk_add_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// a plain v_add_f32: keeps the backend from widening a lone add of two vector halves into a
// packed op plus a move
__device__ __forceinline__ float add_scalar(float a, float b)
{
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// acc + x[lane + 1] * q (lane 63: + 0 * q, bound_ctrl), one rounding: fma(x[lane+1], q, acc).
// The E tap of a lane's last column as one v_fmac_f32_dpp (the neighbour lane's value read
// through DPP inside the FMA): hipcc's DPP combiner folds a DPP move into a v_add_f32 but not
// into the tied-accumulator v_fmac_f32, so it is written out
__device__ __forceinline__ float fmac_from_right(float acc, float x, float q)
{
    asm("v_fmac_f32_dpp %0, %1, %2 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0"
        : "+v"(acc) : "v"(x), "v"(q));
    return acc;
}
// fma(a, b, c) as a plain v_fma_f32 (same reason: two scalar FMAs on the halves of a pair would
// otherwise become a packed FMA after a pair assembly)
__device__ __forceinline__ float fma_scalar(float a, float b, float c)
{
    float r;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

template <int T, int SRC, bool OUT16, bool FAST>
struct JLag {
    static constexpr int C = kJacobiCols;
    static_assert(C == 2, "a lane's columns are one pair: Row, the vector loads and stores, the wrap");
    // ring of R >= 2T+1 rows, R a multiple of 6: the loop body is unrolled over the R/6 groups
    // of 6 steps so every ring slot is a compile-time constant
    static constexpr int R = (2 * T + 1 + 5) / 6 * 6, NG = R / 6;
    // Input rows land in NB = PF + 1 buffers, PF steps ahead of the step that consumes them.  The
    // buffer of a row is a compile-time constant of the unrolled step if NB divides R (the index
    // is ring group plus phase): 4 buffers at T = 4, 5, 10 (R = 12, 24), 3 where 4 do not divide
    // R (R = 6 at T = 1, 2; R = 18 at T = 8), and in the seeded passes, whose gather holds more
    // address registers (T = 10: a 4th buffer puts 28-32 B per lane of scratch into their step
    // loop, 3 buffers none)
    static constexpr int NB =
        SRC != SRC_SEED && R % (PF_JLAG_PF + 1) == 0 ? PF_JLAG_PF + 1 : 3;
    static constexpr int PF = NB - 1;
    static_assert(R % NB == 0, "the input buffers' period must divide the ring's");
    // L row k + LL is loaded at step k, straight into its ring slot.  The slot held row
    // k + LL - R, which level T read for the last time at step k + LL - R + 2T <= k - 1, so the
    // slot is dead if LL <= R - 2T - 1: 3 steps at T = 1, 4, 10 and 1 step at T = 2, 5, 8.
    // Level 1 reads the row at step k + LL + 2, so an L load has LL + 2 steps to land
    static constexpr int LL = 3 < R - 2 * T - 1 ? 3 : R - 2 * T - 1;
    static_assert(LL >= 1 && LL <= R - 2 * T - 1, "the ring slot of L row k + LL must be dead at step k");
    // The L ring is in registers -- every slot index is a compile-time constant of the unrolled
    // step -- so no LDS store / load latency sits on a step's dependency chain.  Round 4: at
    // T = 10 the register ring took the packed pass from 132 VGPRs + 48 KB of LDS per 4-wave
    // workgroup to 166-167 VGPRs and no LDS -- the same 3 waves per SIMD -- and dropped the T LDS
    // reads per step: C3 Jacobi stage 3.37-3.38 -> 3.19-3.24 ms, 14.10-14.35k -> 14.75-14.81k
    // panoramas/s (three alternating rounds on one MI355X, profiles/r04/ab_lreg; recipe:
    // tools/gpu_round.sh ab).  JPipe keeps an LDS ring of its own.
    Row Lr[R];        // ring slot s = Lr[s]
    Row H[T][3];      // H[t][r % 3] = level t row r
    Row In[NB];       // input row k0 + s lands in In[s % NB] (issued at step k0 + s + 1 - PF)
    float hcol[C];  // FAST: H of the lane's columns: 0.5 (covered column) or 0
    float vq;       // -1/4 in a VGPR (the folded-DPP FMA takes its second operand from a VGPR)
    const JacobiPass* P;
    int w, xs0, vlo, vhi, r0, r1, h0, h1;
    int colbase;   // virtual column of lane 0 (wave-uniform)
    int lo;        // lane * C
    int rlo, rhi;  // rows loads are clamped to: the band [h0, h1].  A band pixel never reads a
                   // row outside it except as a neighbour of the un-windowed rows h0 / h1,
                   // whose update ignores its neighbours -- in the packed form through a zero
                   // factor, which needs the neighbours finite.  A halo lane's virtual columns
                   // past a row end still reach rows h0-1 / h1+1, which k_border keeps finite
    const float *src, *prev, *emap, *lnorm;
    float* dst;
    uint16_t* out;

    // Row k of a plane: a wave-uniform row pointer (SGPR arithmetic) plus the lane offset, so
    // the loads use the global_load saddr form with no per-lane address math.
    __device__ __forceinline__ Row load_row(const float* base_ptr, int k) const
    {
        Row r;
        int kc = k < rlo ? rlo : (k > rhi ? rhi : k);
        const float* rp = base_ptr + ((long long)kc * w + colbase);
        float2 q = *reinterpret_cast<const float2*>(rp + lo);
        r.v[0] = q.x; r.v[1] = q.y;
        return r;
    }

    __device__ __forceinline__ Row load_input(int k) const
    {
        if constexpr (SRC == SRC_BUF) {
            return load_row(src, k);
        } else {
            // Virtual column xs0 of row k is pixel (xr, Y) with |xs0 - xr| < w (the halo is
            // narrower than a row, jacobi_tcap), so the wrap is one compare, no division.
            // xs0 is even, so the lane's pair (2m, 2m+1) never straddles a row end and shares
            // one source pixel of the half-resolution level.
            // (Written as a loop over the lane's pairs, of which there is one: hipcc compiles
            // the straight-line form of the same statements to different code.)
            Row r;
#pragma unroll
            for (int j = 0; j < C; j += 2) {
                int xr = xs0 + j, Y = k;
                if (xr < 0) { xr += w; Y -= 1; }
                else if (xr >= w) { xr -= w; Y += 1; }
                float v0 = 0.0f, v1 = 0.0f;
                if (Y >= 0 && Y < P->h) {
                    if constexpr (SRC == SRC_UPSAMPLE) {
                        v0 = v1 = prev[(long long)(Y >> 1) * (w >> 1) + (xr >> 1)];
                    } else if (Y >= P->h0 && Y <= P->h1) {  // level-0 seed (Depth.cpp:1442-1465)
                        const int ro = P->erow[Y + 1];
                        v0 = emap[ro + P->ecol[xr + 1]];
                        v1 = emap[ro + P->ecol[xr + 2]];
                    }
                }
                r.v[j] = v0;
                r.v[j + 1] = v1;
            }
            return r;
        }
    }

    static constexpr int slot(int ph, int a) { return ((ph - a) % 3 + 3) % 3; }

    // the L ring: row k of the group sits in slot GB + PH (GB = group base mod R, compile-time);
    // level t reads row k - 2t.  The packed form sanitises a row (above) in its slot at step
    // row + 2, the step of its first read (level 1): the load has had LL + 2 steps by then, and
    // this is the only place that waits for it.  H = 0 in the lane's un-windowed columns (hcol)
    // and, in a pass that reaches them (ROWS), on rows h0 / h1; the rows past them are clamped
    // copies of those two (load_row), never stored, and are zeroed alike
    template <int GB, int PH, bool ROWS>
    __device__ __forceinline__ void ring_sanitise(int k)
    {
        Row& r = Lr[((GB + PH - 2) % R + R) % R];
        bool edge = false;
        if constexpr (ROWS) edge = k - 2 <= h0 || k - 2 >= h1;
#pragma unroll
        for (int j = 0; j < C; j++) r.v[j] = (edge || hcol[j] == 0.0f) ? 0.0f : r.v[j];
    }
    template <int GB, int PH, int TT>
    __device__ __forceinline__ Row ring_get() const
    {
        return Lr[((GB + PH - 2 * TT) % R + R) % R];
    }

    // Lv[t - TA] = L row of level t for t in [TA, TB] (compile-time t)
    template <int GB, int PH, int TA, int TB>
    __device__ __forceinline__ void ring_get_range(Row* Lv) const
    {
        if constexpr (TA <= TB) {
            Lv[0] = ring_get<GB, PH, TA>();
            ring_get_range<GB, PH, TA + 1, TB>(Lv + 1);
        }
    }

    // general form: T*C scalar updates, stage-wise so consecutive VALU instructions belong to
    // different updates (hides the dependent-issue latency)
    template <int PH>
    __device__ __forceinline__ void sweep_general(const Row* Lv, Row* nw) const
    {
        float Wl[T], Er[T];
#pragma unroll
        for (int t = 1; t <= T; t++) {
            Wl[t - 1] = dpp_from_left(H[t - 1][slot(PH, 2 * t)].v[C - 1]);
            Er[t - 1] = dpp_from_right(H[t - 1][slot(PH, 2 * t)].v[0]);
        }
        float cur[T][C];
#pragma unroll
        for (int t = 1; t <= T; t++)
#pragma unroll
            for (int j = 0; j < C; j++) {
                const Row& c = H[t - 1][slot(PH, 2 * t)];
                float W = j == 0 ? Wl[t - 1] : c.v[j - 1];
                cur[t - 1][j] = W + H[t - 1][slot(PH, 2 * t + 1)].v[j];
            }
        // Lcur = (((W*q + N*q) + b) + S*q) + E*q with q = -1/4.  Every product by q (and by 0.5
        // below) is exact -- a power-of-two scaling -- so fl(W*q + N*q) = q*fl(W+N) and
        // fl(a + x*q) = fma(x, q, a): the fused form rounds exactly where the reference rounds.
        // (Exact unless an operand is below 2^-124, which depths in [0,1] never reach here.)
#pragma unroll
        for (int t = 1; t <= T; t++)
#pragma unroll
            for (int j = 0; j < C; j++)
                cur[t - 1][j] = __builtin_fmaf(cur[t - 1][j], -0.25f, H[t - 1][slot(PH, 2 * t)].v[j]);
#pragma unroll
        for (int t = 1; t <= T; t++)
#pragma unroll
            for (int j = 0; j < C; j++)
                cur[t - 1][j] = __builtin_fmaf(H[t - 1][slot(PH, 2 * t - 1)].v[j], -0.25f, cur[t - 1][j]);
#pragma unroll
        for (int t = 1; t <= T; t++)
#pragma unroll
            for (int j = 0; j < C; j++) {
                const Row& c = H[t - 1][slot(PH, 2 * t)];
                float E = j == C - 1 ? Er[t - 1] : c.v[j + 1];
                cur[t - 1][j] = __builtin_fmaf(E, -0.25f, cur[t - 1][j]);
            }
        // un-windowed pixel (L = marker): Lcur = L = 0, so the step is exactly +0.  Masked with
        // an AND so the compiler keeps this straight-line (no exec-mask branch).
#pragma unroll
        for (int t = 1; t <= T; t++)
#pragma unroll
            for (int j = 0; j < C; j++) {
                const float Lx = Lv[t - 1].v[j];
                float d = Lx - cur[t - 1][j];
                uint32_t m = __float_as_uint(Lx) == PF_NAN_MARKER ? 0u : 0xFFFFFFFFu;
                cur[t - 1][j] = __uint_as_float(__float_as_uint(d) & m);
            }
#pragma unroll
        for (int t = 1; t <= T; t++)
#pragma unroll
            for (int j = 0; j < C; j++) {
                const float b = H[t - 1][slot(PH, 2 * t)].v[j];
                float tt = __builtin_fmaf(cur[t - 1][j], 0.5f, b);  // b + (L - Lcur)*0.5
                float v = tt * (1 - (float)1e-4) + b * (float)1e-4;
                // clamp01: b is never -0 or NaN here, so med3 equals the reference's compares
                nw[t - 1].v[j] = __builtin_amdgcn_fmed3f(v, 0.0f, 1.0f);
            }
    }

    // FAST form: the same update on the lane's column pair, stage-wise over groups of
    // PF_JPK_GROUP levels (bounds the live temporaries, i.e. the VGPR count).  The terms that
    // cross lanes are scalar ops: W + N of column 0 is one v_add_f32_dpp (the DPP move folded
    // into the add) and the E terms are two scalar FMAs, the rest packed.  Measured issue costs
    // on MI355X (tools/ubench/dpp_rate.hip, >= 2 waves/SIMD): v_pk_* 4.7 cycles, v_add/v_fma 2.8,
    // any DPP op 4.4 -- so per level and column pair 7 packed + 1 folded DPP + 1 DPP move +
    // 3 scalar (~50 cycles) against 9 packed + 2 DPP moves + 2 pair assemblies (~57).
    template <int PH, int T0, int T1, bool ROWS>
    __device__ __forceinline__ void sweep_packed_group(const Row* Lv, Row* nw, int k) const
    {
        constexpr int G = T1 - T0;
        const f2 q = {-0.25f, -0.25f};
        const f2 reg = {(float)1e-4, (float)1e-4};
        const f2 reg_ = {1 - (float)1e-4, 1 - (float)1e-4};
        f2 cur[G];
        // Lcur = (((W*q + N*q) + b) + S*q) + E*q, q = -1/4, as in sweep_general
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int t = T0 + 1 + g;
            const f2 c = H[t - 1][slot(PH, 2 * t)].v, n = H[t - 1][slot(PH, 2 * t + 1)].v;
            cur[g].x = dpp_from_left(c.y) + n.x;  // folds into v_add_f32_dpp
            cur[g].y = add_scalar(c.x, n.y);
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int t = T0 + 1 + g;
            cur[g] = __builtin_elementwise_fma(cur[g], q, H[t - 1][slot(PH, 2 * t)].v);
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int t = T0 + 1 + g;
            cur[g] = __builtin_elementwise_fma(H[t - 1][slot(PH, 2 * t - 1)].v, q, cur[g]);
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int t = T0 + 1 + g;
            const f2 c = H[t - 1][slot(PH, 2 * t)].v;
            cur[g].x = fma_scalar(c.y, vq, cur[g].x);
            cur[g].y = fmac_from_right(cur[g].y, c.x, vq);
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int t = T0 + 1 + g;
            // rows h0 and h1 are un-windowed (the host certified the rest of the band); only
            // passes whose row window reaches them (ROWS) pay for the test
            f2 hh = f2{hcol[0], hcol[1]};
            if constexpr (ROWS) {
                const int row = k - 2 * t;
                const float hr = (row == h0 || row == h1) ? 0.0f : 1.0f;
                hh = hh * hr;
            }
            cur[g] = __builtin_elementwise_fma(Lv[g].v - cur[g], hh, H[t - 1][slot(PH, 2 * t)].v);
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int t = T0 + 1 + g;
            nw[t - 1].v = pk_add_clamp01(cur[g] * reg_, H[t - 1][slot(PH, 2 * t)].v * reg);
        }
    }
    // Fill and drain.  Level t is only needed for rows [r0 - (T-t), r1 + (T-t)) of the chunk,
    // i.e. at steps k in [r0 - T + 3t, r1 + T + t); outside that window its row is never read by
    // a needed update (stencil closure), so its ring slots may hold stale rows there, read only
    // by unneeded updates.  10-30% of the updates of a chunk are of that kind at the default
    // depths (the lagged start fills T levels over 3T steps, the drain empties them over T).
    // They are dropped at compile time: the steps of the chunk's first and last groups are their
    // own instantiations (fill_from, drain_from below) that compute levels LA..NA only -- NA < T
    // in the fill, LA > 1 in the drain -- and the steady-state steps between compute all T.  (A
    // wave-uniform branch per level group and step did the same at run time and was slower,
    // DESIGN.md §3.)
    template <int PH, int GB, int T0, bool ROWS, int NA, int LA = 1>
    __device__ __forceinline__ void sweep_packed(Row* nw, int k) const
    {
        constexpr int T1 = T0 + PF_JPK_GROUP < T ? T0 + PF_JPK_GROUP : T;
        // the groups run from the deepest level down: level t+1 reads the oldest row of level
        // t's ring before level t overwrites it, so the new row can take that row's registers
        // (all reads of a step are rows of earlier steps, so the order is free)
        if constexpr (T1 < T) sweep_packed<PH, GB, T1, ROWS, NA, LA>(nw, k);
        constexpr int TB = T1 < NA ? T1 : NA;
        constexpr int TA = T0 > LA - 1 ? T0 : LA - 1;  // levels TA+1 .. TB
        if constexpr (TA < TB) {
            Row Lv[TB - TA];
            ring_get_range<GB, PH, TA + 1, TB>(Lv);
            sweep_packed_group<PH, TA, TB, ROWS>(Lv, nw, k);
        }
    }

    // Step k = (group base) + PH; GB = (group base - k0) mod R: ring slots count from the
    // chunk's first step, so they are compile-time constants without aligning k0.  NA < T only
    // in the fill (fill_from).
    template <int PH, bool ROWS, int GB, int NA = T, int LA = 1>
    __device__ __forceinline__ void step(int k)
    {
        // level-0 row k-1 (loaded PF steps ago) joins the ring
        H[0][slot(PH, 1)] = In[(GB + PH + NB - 1) % NB];
        // L row k-2, which level 1 reads in this step, is sanitised in its slot (rows before k0
        // are zero slots: harmless)
        if constexpr (FAST) ring_sanitise<GB, PH, ROWS>(k);
        // L row k + LL straight into its ring slot, which is dead by now (at LL above)
        Lr[(GB + PH + LL) % R] = load_row(lnorm, k + LL);
        // input row k + PF - 1 for a later step; its buffer held row k - 2, consumed last step
        In[(GB + PH + PF - 1) % NB] = load_input(k + PF - 1);
        Row nw[T];
        if constexpr (FAST) {
            sweep_packed<PH, GB, 0, ROWS, NA, LA>(nw, k);
        } else {
            static_assert(NA == T && LA == 1, "the general form has no fill / drain specialisation");
            Row Lv[T];
            ring_get_range<GB, PH, 1, T>(Lv);
            sweep_general<PH>(Lv, nw);
        }
#pragma unroll
        for (int t = 1; t < T; t++)
            if (t >= LA && t <= NA) H[t][slot(PH, 2 * t)] = nw[t - 1];  // idle: keeps its rows
        if constexpr (NA < T) return;  // no stored row before every level runs (fill_from)
        const int j = k - 2 * T;  // final-level row finished this step
        // xs0, vlo and vhi are even, so a lane's pair is inside [vlo, vhi) or outside: one
        // vector store per lane.
        if (j >= r0 && j < r1 && xs0 >= vlo && xs0 < vhi) {
            const long long rowb = (long long)j * w + colbase;
            if constexpr (OUT16) {
                // quantise (Depth.cpp:1721-1736); v is already in [0,1], truncating cast
                uint32_t qv[C];
#pragma unroll
                for (int p = 0; p < C; p++) qv[p] = (uint32_t)(nw[T - 1].v[p] * 65535.0f);
                *reinterpret_cast<uint32_t*>(out + rowb + lo) = qv[0] | (qv[1] << 16);
            } else {
                *reinterpret_cast<float2*>(dst + rowb + lo) = make_float2(nw[T - 1].v[0], nw[T - 1].v[1]);
            }
        }
    }

    // one group of 6 steps starting at k, k mod R == 6G
    template <bool ROWS, int G>
    __device__ __forceinline__ void group(int k)
    {
        step<0, ROWS, 6 * G>(k);
        step<1, ROWS, 6 * G>(k + 1);
        step<2, ROWS, 6 * G>(k + 2);
        step<3, ROWS, 6 * G>(k + 3);
        step<4, ROWS, 6 * G>(k + 4);
        step<5, ROWS, 6 * G>(k + 5);
    }
    // groups G..NG-1 of the unrolled ring period; returns false once k reaches kend
    template <bool ROWS, int G>
    __device__ __forceinline__ bool groups_from(int& k, int kend)
    {
        group<ROWS, G>(k);
        k += 6;
        if (k >= kend) return false;
        if constexpr (G + 1 < NG) return groups_from<ROWS, G + 1>(k, kend);
        else return true;
    }
    // The chunk's fill.  The stored rows [r0, r1) of level T read level t's rows
    // [r0 - (T - t), r1 + (T - t)) and nothing else; level t produces row k - 2t at step k, so
    // its first needed row comes at step r0 - T + 3t = k0 + 1 + 3t.  Before that (s = k - k0 <
    // 1 + 3t) level t feeds nothing that is stored.  The first NF groups therefore run as their
    // own unrolled steps with levels na(s) + 1 .. T compiled out; an idle level keeps its
    // zero-initialised rows, which only idle levels read (level t reads level t - 1 alone, which
    // is active from three steps earlier).  At T = 10: 175 of the ~2,100 level-steps of a
    // 183-row chunk.
    static constexpr int na(int s)
    {
        const int a = s >= 1 ? (s - 1) / 3 : 0;
        return a < T ? a : T;
    }
    static constexpr int NF_ALL = (3 * T + 1 + 5) / 6;  // groups with an idle level
    // hipcc's register allocation of the unrolled loop is erratic in the fill length: at T = 10,
    // 3 groups keep the step loop at 166-169 VGPRs (3 waves per SIMD) where 1 or 4 take 171-232;
    // at T = 8, 4 groups keep 140-143 where 3 take 188 (checked in the ISA)
    static constexpr int NF_AUTO = T == 8 ? 4 : 3;
    static constexpr int NF_SEL = PF_JFILL < 0 ? NF_AUTO : PF_JFILL;
    static constexpr int NF = !FAST ? 0 : (NF_SEL < NF_ALL ? NF_SEL : NF_ALL);
    template <bool ROWS, int F>
    __device__ __forceinline__ bool fill_from(int& k, int kend)
    {
        if constexpr (F < NF) {
            constexpr int GB = 6 * (F % NG);
            step<0, ROWS, GB, na(6 * F + 0)>(k);
            step<1, ROWS, GB, na(6 * F + 1)>(k + 1);
            step<2, ROWS, GB, na(6 * F + 2)>(k + 2);
            step<3, ROWS, GB, na(6 * F + 3)>(k + 3);
            step<4, ROWS, GB, na(6 * F + 4)>(k + 4);
            step<5, ROWS, GB, na(6 * F + 5)>(k + 5);
            k += 6;
            if (k >= kend) return false;
            return fill_from<ROWS, F + 1>(k, kend);
        } else {
            return true;
        }
    }
    // The chunk's drain, likewise: level t is last needed at step kend - 1 - (T - t), so in the
    // last T steps the shallow levels go idle one by one.  The last ND groups run as their own
    // steps with levels 1 .. la(p) - 1 compiled out, p = the step within those groups.  The
    // chunk's step count kend - k0 is not a multiple of 6: the groups end o = 0..5 steps past
    // kend, and la() assumes o = 0, the largest active set (a few idle level-steps remain when
    // o > 0; nothing needed is skipped).  The drain starts at a run-time ring group; its code is
    // written for group 0 and the ring is rotated to it first (ring_to_zero).
    static constexpr int ND_ALL = (T + 5) / 6;  // groups with an idle level (o = 0)
    static constexpr int ND = !(PF_JDRAIN && FAST) ? 0 : (PF_JDRAIN < ND_ALL ? PF_JDRAIN : ND_ALL);
    static constexpr int la(int p)
    {
        const int a = T - 6 * ND + p + 1;
        return a < 1 ? 1 : a;
    }
    template <bool ROWS, int I>
    __device__ __forceinline__ void drain_from(int& k)
    {
        if constexpr (I < ND) {
            constexpr int GB = 6 * (I % NG);
            step<0, ROWS, GB, T, la(6 * I + 0)>(k);
            step<1, ROWS, GB, T, la(6 * I + 1)>(k + 1);
            step<2, ROWS, GB, T, la(6 * I + 2)>(k + 2);
            step<3, ROWS, GB, T, la(6 * I + 3)>(k + 3);
            step<4, ROWS, GB, T, la(6 * I + 4)>(k + 4);
            step<5, ROWS, GB, T, la(6 * I + 5)>(k + 5);
            k += 6;
            drain_from<ROWS, I + 1>(k);
        }
    }
    // the drain code is written for ring group 0: the L ring is rotated so that the drain's
    // first group sits at slot 0 (a register permutation once per chunk), instead of one copy of
    // the drain per ring group (which took the T = 10 pass from 166 to 214 VGPRs)
    // Up to LL of the permuted slots have their load in flight: the register dependency orders
    // that (one wait per chunk).  The input buffers are brought to the same phase: SH % NB is 0,
    // or 2 where the drain starts at an odd ring group with 4 buffers
    template <int SH>
    __device__ __forceinline__ void ring_rotate()
    {
        Row t[R];
#pragma unroll
        for (int x = 0; x < R; x++) t[x] = Lr[(x + SH) % R];
#pragma unroll
        for (int x = 0; x < R; x++) Lr[x] = t[x];
        if constexpr (SH % NB != 0) {
            Row u[NB];
#pragma unroll
            for (int x = 0; x < NB; x++) u[x] = In[(x + SH) % NB];
#pragma unroll
            for (int x = 0; x < NB; x++) In[x] = u[x];
        }
    }
    template <int G>
    __device__ __forceinline__ void ring_to_zero(int g)
    {  // g = the ring group the drain starts at
        if constexpr (G < NG) {
            if (g == G) ring_rotate<6 * G>();
            else ring_to_zero<G + 1>(g);
        }
    }
    // the drain from ring group g.  (The group is computed by the caller whether it is used or
    // not, NG == 1: hipcc orders a few of the drain's instructions differently without it.)
    template <bool ROWS>
    __device__ __forceinline__ void drain(int g, int& k)
    {
        if constexpr (NG > 1) ring_to_zero<1>(g);
        drain_from<ROWS, 0>(k);
    }
    // the step loop from the chunk's first step k0 (ring group 0): the fill, whole groups up to
    // the drain (or to the end, for a chunk too short for both), the drain
    template <bool ROWS>
    __device__ __forceinline__ void run(int k0, int kend)
    {
        int k = k0;
        const int gt = (kend - k0 + 5) / 6;  // groups of the chunk
        const bool dr = ND > 0 && gt >= NF + ND;
        if (!fill_from<ROWS, 0>(k, kend)) return;
        const int kd = dr ? k0 + 6 * (gt - ND) : kend;
        if (k < kd) {
            bool more = true;
            if constexpr (NF % NG != 0) more = groups_from<ROWS, NF % NG>(k, kd);
            while (more) more = groups_from<ROWS, 0>(k, kd);
        }
        if (dr) drain<ROWS>(__builtin_amdgcn_readfirstlane((gt - ND) % NG), k);
    }
};

template <int T, int SRC, bool OUT16, bool FAST>
__global__ void __launch_bounds__(256, FAST ? PF_JLAG_WAVES_FAST : PF_JLAG_WAVES)
k_jlag(JacobiPass P)
{
    using S_t = JLag<T, SRC, OUT16, FAST>;
    constexpr int C = S_t::C;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int job = blockIdx.x * 4 + wave;
    if (job >= P.nstrips * P.nchunks) return;  // wave-uniform
    const int b = blockIdx.y;
    const int strip = job % P.nstrips, chunk = job / P.nstrips;
    S_t S;
    S.P = &P;
    S.w = P.w;
    S.h0 = P.h0;
    S.h1 = P.h1;
    S.colbase = strip * P.V - P.Tp;
    S.lo = lane * C;
    S.vq = -0.25f;
    asm volatile("" : "+v"(S.vq));
    S.rlo = P.h0;
    S.rhi = P.h1;
    S.xs0 = strip * P.V - P.Tp + lane * C;
    S.vlo = strip * P.V;
    S.vhi = min(S.vlo + P.V, P.w);
    S.r0 = P.row_lo + chunk * P.rows_per_chunk;
    S.r1 = min(S.r0 + P.rows_per_chunk, P.row_hi);
    S.src = P.src + b * P.sstride;
    S.prev = P.prev + b * P.pstride;
    S.emap = P.emap + b * P.estride;
    S.lnorm = P.lnorm + b * P.lstride;
    S.dst = P.dst + b * P.dstride;
    S.out = P.out + b * P.ostride;
    // H of the lane's two columns.  Column 0 is un-windowed (certified), so the only halo cell
    // that can reach a stored pixel is virtual column w (pixel (0, Y+1), the east tap of column
    // w-1 -- the seam quirk), whose H is 0; other halo cells get 0 too (never read).
#pragma unroll
    for (int j = 0; j < C; j++) S.hcol[j] = 0.0f;
    if constexpr (FAST) {
        // xs0 and w are even, so the lane's two columns are both inside or both outside
        if (S.xs0 >= 0 && S.xs0 < P.w)
#pragma unroll
            for (int j = 0; j < C; j++) S.hcol[j] = P.hcol[S.xs0 + j];
    }
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int j = 0; j < C; j++) S.H[t][q].v[j] = 0.0f;
#pragma unroll
    for (int q = 0; q < S_t::NB; q++)
#pragma unroll
        for (int j = 0; j < C; j++) S.In[q].v[j] = 0.0f;
#pragma unroll
    for (int q = 0; q < S_t::R; q++)
#pragma unroll
        for (int j = 0; j < C; j++) S.Lr[q].v[j] = 0.0f;
    // steps k0 .. kend: level 0 needs rows from r0 - T, the last output row r1-1 finishes at
    // step r1 - 1 + 2T.  Ring slots count from k0 (JLag::step), so k0 needs no alignment.
    const int k0 = S.r0 - T - 1;
    const int kend = S.r1 + 2 * T;
    // prime the rows the first steps consume before their in-loop loads land (the rest are
    // loaded PF / LL steps ahead inside step()).  The ring slots of rows before k0 stay zero:
    // they only feed halo/stale cells, like the zero-initialised level rows.  Input row k0 + r
    // sits in buffer r and L row k0 + r in ring slot r (both count from k0).
#pragma unroll
    for (int r = 0; r + 1 < S_t::PF; r++) S.In[r] = S.load_input(k0 + r);
#pragma unroll
    for (int r = 0; r < S_t::LL; r++) S.Lr[r] = S.load_row(S.lnorm, k0 + r);
    // rows computed by some level of this pass: k - 2t for k in [k0, kend + 5], t in [1, T]
    const int wlo = k0 - 2 * T, whi = kend + 3;
    const bool rows = (S.h0 >= wlo && S.h0 <= whi) || (S.h1 >= wlo && S.h1 <= whi);
    if (!FAST || rows) S.template run<true>(k0, kend);
    else S.template run<false>(k0, kend);
}

// ---------------------------------------------------------------------------------------------
// Pipelined passes: the T = S*TS sweep levels of one strip-chunk are split over the S waves of a
// workgroup.  Wave (stage) s owns levels s*TS+1 .. (s+1)*TS and runs the lagged stream of JLag
// over them; the input of its first level is its predecessor's last level, whose new row the
// predecessor leaves in a double-buffered LDS slot every step (one workgroup barrier per step).
// Against JLag at the same T: S times the waves per strip-chunk at 1/S of the register rings, so
// the small levels fill the chip with fewer row chunks (less vertical halo) and every level gets
// more waves per SIMD to hide the load/LDS latency behind.  Same arithmetic, same order: every
// pixel's value is bit-identical to JLag's (and the reference's).
static constexpr int md(int a, int m) { return ((a % m) + m) % m; }

template <int TS, int S, int SI, int SRC, bool OUT16>
struct JPipe {
    static constexpr int C = kJacobiCols;
    static constexpr int T = TS * S;
    static constexpr int TB = SI * TS + 1, TE = TB + TS - 1;  // own levels
    static constexpr int PF = PF_JPIPE_PF, NB = PF_JPIPE_PF + 1;
    static constexpr int R = (2 * TS + 1 + 5) / 6 * 6;  // L ring rows (multiple of 6)
    static constexpr int NG = R / 6;
    static constexpr int G = PF_JPK_GROUP;
    Row H[TS][3];  // H[l][row % 3]: level TB-1+l (l = 0: the input level of this stage)
    Row In[NB];    // stage 0: level-0 input row r in In[r % NB]
    Row Lin[NB];   // L row r in Lin[r % NB], put into the LDS ring PF steps after its load
    float* lring;     // this stage's ring: R rows of 64*C floats (row r in slot r % R)
    const float* xin; // stage > 0: the predecessor's exchange slots [2][64*C]
    float* xout;      // stage < S-1: this stage's exchange slots
    int lane_c;
    float hcol[C];
    float vq;  // -1/4 in a VGPR, as JLag::vq
    const JacobiPass* P;
    int w, xs0, vlo, vhi, r0, r1, h0, h1, colbase, lo, rlo, rhi;
    const float *src, *prev, *emap, *lnorm;
    float* dst;
    uint16_t* out;

    __device__ __forceinline__ Row load_row(const float* base_ptr, int k) const
    {
        Row r;
        int kc = k < rlo ? rlo : (k > rhi ? rhi : k);
        const float2 q = *reinterpret_cast<const float2*>(base_ptr + ((long long)kc * w + colbase) + lo);
        r.v[0] = q.x; r.v[1] = q.y;
        return r;
    }
    __device__ __forceinline__ Row load_input(int k) const
    {  // as JLag::load_input
        if constexpr (SRC == SRC_BUF) {
            return load_row(src, k);
        } else {
            Row r;
            int xr = xs0, Y = k;
            if (xr < 0) { xr += w; Y -= 1; }
            else if (xr >= w) { xr -= w; Y += 1; }
            float v0 = 0.0f, v1 = 0.0f;
            if (Y >= 0 && Y < P->h) {
                if constexpr (SRC == SRC_UPSAMPLE) {
                    v0 = v1 = prev[(long long)(Y >> 1) * (w >> 1) + (xr >> 1)];
                } else if (Y >= P->h0 && Y <= P->h1) {
                    const int ro = P->erow[Y + 1];
                    v0 = emap[ro + P->ecol[xr + 1]];
                    v1 = emap[ro + P->ecol[xr + 2]];
                }
            }
            r.v[0] = v0;
            r.v[1] = v1;
            return r;
        }
    }
    __device__ __forceinline__ void lds_put(float* p, Row r) const
    {  // L rows sanitised as they enter the ring (the packed form's H = 0 trick, JLag)
        r.v[0] = __builtin_isfinite(r.v[0]) ? r.v[0] : 0.0f;
        r.v[1] = __builtin_isfinite(r.v[1]) ? r.v[1] : 0.0f;
        *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
    }
    __device__ __forceinline__ Row lds_get(const float* p) const
    {
        Row r;
        const float2 q = *reinterpret_cast<const float2*>(p);
        r.v[0] = q.x; r.v[1] = q.y;
        return r;
    }

    // own levels T0 < t <= T1 (global indices) of step k (phase PH), packed form of JLag
    template <int PH, int T0, int T1, bool ROWS>
    __device__ __forceinline__ void sweep_group(const Row* Lv, Row* nw, int k) const
    {
        constexpr int NGR = T1 - T0;
        const f2 q = {-0.25f, -0.25f};
        const f2 reg = {(float)1e-4, (float)1e-4};
        const f2 reg_ = {1 - (float)1e-4, 1 - (float)1e-4};
        f2 cur[NGR];
#pragma unroll
        for (int g = 0; g < NGR; g++) {
            const int t = T0 + 1 + g, l = t - TB;  // reads ring H[l] = level t-1
            const f2 c = H[l][md(PH - 2 * t, 3)].v, n = H[l][md(PH - 2 * t - 1, 3)].v;
            cur[g].x = dpp_from_left(c.y) + n.x;
            cur[g].y = add_scalar(c.x, n.y);
        }
#pragma unroll
        for (int g = 0; g < NGR; g++) {
            const int t = T0 + 1 + g, l = t - TB;
            cur[g] = __builtin_elementwise_fma(cur[g], q, H[l][md(PH - 2 * t, 3)].v);
        }
#pragma unroll
        for (int g = 0; g < NGR; g++) {
            const int t = T0 + 1 + g, l = t - TB;
            cur[g] = __builtin_elementwise_fma(H[l][md(PH - 2 * t + 1, 3)].v, q, cur[g]);
        }
#pragma unroll
        for (int g = 0; g < NGR; g++) {
            const int t = T0 + 1 + g, l = t - TB;
            const f2 c = H[l][md(PH - 2 * t, 3)].v;
            cur[g].x = fma_scalar(c.y, vq, cur[g].x);
            cur[g].y = fmac_from_right(cur[g].y, c.x, vq);
        }
#pragma unroll
        for (int g = 0; g < NGR; g++) {
            const int t = T0 + 1 + g, l = t - TB;
            f2 hh = f2{hcol[0], hcol[1]};
            if constexpr (ROWS) {
                const int row = k - 2 * t;
                const float hr = (row == h0 || row == h1) ? 0.0f : 1.0f;
                hh = hh * hr;
            }
            cur[g] = __builtin_elementwise_fma(Lv[t - TB].v - cur[g], hh, H[l][md(PH - 2 * t, 3)].v);
        }
#pragma unroll
        for (int g = 0; g < NGR; g++) {
            const int t = T0 + 1 + g, l = t - TB;
            nw[t - TB].v = pk_add_clamp01(cur[g] * reg_, H[l][md(PH - 2 * t, 3)].v * reg);
        }
    }
    // own levels T0 < t <= min(T1, NA): levels past NA are idle in the fill (JLag::fill_from)
    template <int PH, int T0, bool ROWS, int NA>
    __device__ __forceinline__ void sweep(const Row* Lv, Row* nw, int k) const
    {
        constexpr int T1 = T0 + G < TE ? T0 + G : TE;
        constexpr int TB_ = T1 < NA ? T1 : NA;
        if constexpr (T0 < TB_) sweep_group<PH, T0, TB_, ROWS>(Lv, nw, k);
        if constexpr (T1 < TE) sweep<PH, T1, ROWS, NA>(Lv, nw, k);
    }

    // step k = (group base) + PH, GB = (group base - k0) mod R (ring slots count from the
    // chunk's first step, as in JLag); levels past NA idle (the fill)
    template <int PH, bool ROWS, int GB, int NA = T>
    __device__ __forceinline__ void step(int k)
    {
        // the input level's row k - 2TB + 1 joins ring H[0]
        if constexpr (SI == 0) {
            H[0][md(PH - 1, 3)] = In[md(PH - 1, NB)];
        } else {
            H[0][md(PH - 2 * TB + 1, 3)] = lds_get(xin + md(PH - 1, 2) * (64 * C) + lane_c);
        }
        // L row q = k - 2TB + 2 enters the ring; rows k - 2t (t = TB..TE) are read from it
        constexpr int QO = -2 * TB + 2;
        lds_put(lring + md(GB + PH + QO, R) * (64 * C) + lane_c, Lin[md(PH + QO, NB)]);
        Row Lv[TS];
#pragma unroll
        for (int t = TB; t <= TE; t++) Lv[t - TB] = lds_get(lring + md(GB + PH - 2 * t, R) * (64 * C) + lane_c);
        Lin[md(PH + QO + PF, NB)] = load_row(lnorm, k + QO + PF);
        if constexpr (SI == 0) In[md(PH + PF - 1, NB)] = load_input(k + PF - 1);
        Row nw[TS];
        sweep<PH, TB - 1, ROWS, NA>(Lv, nw, k);
#pragma unroll
        for (int t = TB; t < TE; t++)
            if (t <= NA) H[t - TB + 1][md(PH - 2 * t, 3)] = nw[t - TB];
        if constexpr (SI < S - 1) {
            if constexpr (TE <= NA)  // else the next stage's first level is idle too
                *reinterpret_cast<float2*>(xout + md(PH, 2) * (64 * C) + lane_c) =
                    make_float2(nw[TS - 1].v[0], nw[TS - 1].v[1]);
        } else if constexpr (NA == T) {
            const int j = k - 2 * T;  // final-level row finished this step
            if (j >= r0 && j < r1 && xs0 >= vlo && xs0 < vhi) {
                const long long rowb = (long long)j * w + colbase;
                if constexpr (OUT16) {
                    const uint32_t q0 = (uint32_t)(nw[TS - 1].v[0] * 65535.0f);
                    const uint32_t q1 = (uint32_t)(nw[TS - 1].v[1] * 65535.0f);
                    *reinterpret_cast<uint32_t*>(out + rowb + lo) = q0 | (q1 << 16);
                } else {
                    *reinterpret_cast<float2*>(dst + rowb + lo) =
                        make_float2(nw[TS - 1].v[0], nw[TS - 1].v[1]);
                }
            }
        }
        __syncthreads();  // the exchange row of this step is visible to the next stage
    }

    template <bool ROWS, int GI>
    __device__ __forceinline__ void group(int k)
    {
        step<0, ROWS, 6 * GI>(k);
        step<1, ROWS, 6 * GI>(k + 1);
        step<2, ROWS, 6 * GI>(k + 2);
        step<3, ROWS, 6 * GI>(k + 3);
        step<4, ROWS, 6 * GI>(k + 4);
        step<5, ROWS, 6 * GI>(k + 5);
    }
    template <bool ROWS, int GI>
    __device__ __forceinline__ bool groups_from(int& k, int kend)
    {
        group<ROWS, GI>(k);
        k += 6;
        if (k >= kend) return false;
        if constexpr (GI + 1 < NG) return groups_from<ROWS, GI + 1>(k, kend);
        else return true;
    }
    // the fill as JLag::fill_from: level t idle for steps s = k - k0 < 1 + 3t (every stage runs
    // the same steps, so the barriers still pair up)
    static constexpr int na(int s)
    {
        const int a = s >= 1 ? (s - 1) / 3 : 0;
        return a < T ? a : T;
    }
    static constexpr int NF_ALL = (3 * T + 1 + 5) / 6;
    static constexpr int NF_SEL = PF_JFILL < 0 ? PF_JPIPE_FILL : PF_JFILL;
    static constexpr int NF = NF_SEL < NF_ALL ? NF_SEL : NF_ALL;
    template <bool ROWS, int F>
    __device__ __forceinline__ bool fill_from(int& k, int kend)
    {
        if constexpr (F < NF) {
            constexpr int GB = 6 * (F % NG);
            step<0, ROWS, GB, na(6 * F + 0)>(k);
            step<1, ROWS, GB, na(6 * F + 1)>(k + 1);
            step<2, ROWS, GB, na(6 * F + 2)>(k + 2);
            step<3, ROWS, GB, na(6 * F + 3)>(k + 3);
            step<4, ROWS, GB, na(6 * F + 4)>(k + 4);
            step<5, ROWS, GB, na(6 * F + 5)>(k + 5);
            k += 6;
            if (k >= kend) return false;
            return fill_from<ROWS, F + 1>(k, kend);
        } else {
            return true;
        }
    }
    template <bool ROWS>
    __device__ __forceinline__ void run(int k0, int kend)
    {
        int k = k0;
        bool more = fill_from<ROWS, 0>(k, kend);
        if constexpr (NF % NG != 0) {
            if (more) more = groups_from<ROWS, NF % NG>(k, kend);
        }
        while (more) more = groups_from<ROWS, 0>(k, kend);
    }
};

template <int TS, int S, int SI, int SRC, bool OUT16>
__device__ __forceinline__ void jpipe_stage(const JacobiPass& P, int lane, int b, int strip,
                                            int chunk, float* lring, float* xchg)
{
    using S_t = JPipe<TS, S, SI, SRC, OUT16>;
    constexpr int T = S_t::T, C = S_t::C;
    S_t St;
    St.P = &P;
    St.w = P.w;
    St.h0 = P.h0;
    St.h1 = P.h1;
    St.colbase = strip * P.V - P.Tp;
    St.lo = lane * C;
    St.lane_c = lane * C;
    St.vq = -0.25f;
    asm volatile("" : "+v"(St.vq));
    St.rlo = P.h0;  // as JLag::rlo
    St.rhi = P.h1;
    St.xs0 = strip * P.V - P.Tp + lane * C;
    St.vlo = strip * P.V;
    St.vhi = min(St.vlo + P.V, P.w);
    St.r0 = P.row_lo + chunk * P.rows_per_chunk;
    St.r1 = min(St.r0 + P.rows_per_chunk, P.row_hi);
    St.src = P.src + b * P.sstride;
    St.prev = P.prev + b * P.pstride;
    St.emap = P.emap + b * P.estride;
    St.lnorm = P.lnorm + b * P.lstride;
    St.dst = P.dst + b * P.dstride;
    St.out = P.out + b * P.ostride;
    St.lring = lring + SI * (S_t::R * 64 * C);
    St.xin = SI > 0 ? xchg + (SI - 1) * (2 * 64 * C) : nullptr;
    St.xout = SI < S - 1 ? xchg + SI * (2 * 64 * C) : nullptr;
    St.hcol[0] = St.hcol[1] = 0.0f;
    if (St.xs0 >= 0 && St.xs0 < P.w) { St.hcol[0] = P.hcol[St.xs0]; St.hcol[1] = P.hcol[St.xs0 + 1]; }
#pragma unroll
    for (int l = 0; l < TS; l++)
#pragma unroll
        for (int q = 0; q < 3; q++) St.H[l][q].v = f2{0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < S_t::NB; q++) { St.In[q].v = f2{0.0f, 0.0f}; St.Lin[q].v = f2{0.0f, 0.0f}; }
    const int k0 = St.r0 - T - 1;  // ring slots count from k0: no alignment (JLag)
    const int kend = St.r1 + 2 * T;
    constexpr int QO = -2 * S_t::TB + 2;
    if constexpr (SI == 0) {
#pragma unroll
        for (int r = 0; r + 1 < S_t::PF; r++) St.In[md(r, S_t::NB)] = St.load_input(k0 + r);
    }
#pragma unroll
    for (int r = 0; r < S_t::PF; r++) St.Lin[md(QO + r, S_t::NB)] = St.load_row(St.lnorm, k0 + QO + r);
    const int wlo = k0 - 2 * T, whi = kend + 3;
    const bool rows = (St.h0 >= wlo && St.h0 <= whi) || (St.h1 >= wlo && St.h1 <= whi);
    // rows is uniform over the workgroup (it depends on the chunk only), so every stage takes the
    // same branch and runs the same number of steps (= barriers)
    if (rows) St.template run<true>(k0, kend);
    else St.template run<false>(k0, kend);
}

template <int TS, int S, int SRC, bool OUT16>
__global__ void __launch_bounds__(64 * S) k_jpipe(JacobiPass P)
{
    constexpr int C = kJacobiCols, R = JPipe<TS, S, 0, SRC, OUT16>::R;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int job = blockIdx.x;
    if (job >= P.nstrips * P.nchunks) return;  // uniform over the workgroup
    const int b = blockIdx.y;
    const int strip = job % P.nstrips, chunk = job / P.nstrips;
    __shared__ float lring[S * R * 64 * C];
    __shared__ float xchg[(S > 1 ? S - 1 : 1) * 2 * 64 * C];
    // the exchange slots are read one step before they are first written (those rows only
    // feed halo cells); zero them so the stale cells are finite and deterministic
    for (int i = threadIdx.x; i < (S > 1 ? S - 1 : 1) * 2 * 64 * C; i += 64 * S) xchg[i] = 0.0f;
    __syncthreads();
    if (wave == 0) jpipe_stage<TS, S, 0, SRC, OUT16>(P, lane, b, strip, chunk, lring, xchg);
    if constexpr (S > 1) { if (wave == 1) jpipe_stage<TS, S, (S > 1 ? 1 : 0), SRC, OUT16>(P, lane, b, strip, chunk, lring, xchg); }
    if constexpr (S > 2) { if (wave == 2) jpipe_stage<TS, S, (S > 2 ? 2 : 0), SRC, OUT16>(P, lane, b, strip, chunk, lring, xchg); }
    if constexpr (S > 3) { if (wave == 3) jpipe_stage<TS, S, (S > 3 ? 3 : 0), SRC, OUT16>(P, lane, b, strip, chunk, lring, xchg); }
}

#if !defined(PF_JPART) || PF_JPART == 0
// Out-of-band rows of a level: 0 (level 0, Depth.cpp:1449-1452) or the nearest upsample of the
// previous level (Depth.cpp:1467-1485); stored to both ping-pong buffers, or quantised into the
// u16 output on the last level (where the ping-pong buffers get only the rows h0-1 and h1+1).
__global__ void __launch_bounds__(256) k_border(const float* __restrict__ prev, long long pstride,
                                                LevelDims L, float* __restrict__ a,
                                                float* __restrict__ bb, long long stride,
                                                uint16_t* __restrict__ out, long long ostride)
{
    // one panorama's level plane is < 2^31 pixels (the host checks out_w * out_h), so the
    // pixel arithmetic is 32-bit: no 64-bit division in the index split
    const int top = L.h0 * L.w;
    const int bot = (L.h - 1 - L.h1) * L.w;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= top + bot) return;
    const int b = blockIdx.y;
    const int y = i < top ? i / L.w : L.h1 + 1 + (i - top) / L.w;
    const int x = i < top ? i - y * L.w : (i - top) - (y - L.h1 - 1) * L.w;
    const int o = y * L.w + x;
    float v = 0.0f;
    if (prev) v = prev[b * pstride + (y / 2) * (L.w / 2) + x / 2];
    if (out) {
        float q = v;
        if (q < 0) q = 0;
        if (q > 1) q = 1;
        out[b * ostride + o] = (uint16_t)(q * 65535.0f);
        // the rows next to the band: a pass's loads clamp rows to [h0, h1], but a halo lane's
        // virtual columns past either row end still reach rows h0-1 / h1+1 (the neighbours of
        // the un-windowed rows, whose zero factor needs them finite; JLag::rlo)
        if (a && (y == L.h0 - 1 || y == L.h1 + 1)) {
            a[b * stride + o] = v;
            bb[b * stride + o] = v;
        }
    } else {
        a[b * stride + o] = v;
        bb[b * stride + o] = v;
    }
}

// The same for widths divisible by 4: a thread owns 4 consecutive pixels of a row (one float2
// load of the half-resolution level, 16-B float / 8-B u16 stores).  The per-pixel scalar form
// stored 2 B per lane on the last level (0.09 ms per C3 step at level 2, ~1.2 TB/s).
__global__ void __launch_bounds__(256) k_border4(const float* __restrict__ prev, long long pstride,
                                                 LevelDims L, float* __restrict__ a,
                                                 float* __restrict__ bb, long long stride,
                                                 uint16_t* __restrict__ out, long long ostride)
{
    const int top = L.h0 * L.w;
    const int bot = (L.h - 1 - L.h1) * L.w;
    const int i = 4 * ((int)blockIdx.x * 256 + (int)threadIdx.x);
    if (i >= top + bot) return;
    const int b = blockIdx.y;
    const int y = i < top ? i / L.w : L.h1 + 1 + (i - top) / L.w;
    const int x = i < top ? i - y * L.w : (i - top) - (y - L.h1 - 1) * L.w;
    const int o = y * L.w + x;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (prev) {  // x is a multiple of 4: the pair x/2, x/2+1 is one aligned float2
        const float2 q = *reinterpret_cast<const float2*>(prev + b * pstride + (y / 2) * (L.w / 2) + x / 2);
        v = make_float4(q.x, q.x, q.y, q.y);
    }
    if (out) {
        const float e[4] = {v.x, v.y, v.z, v.w};
        uint32_t u[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float q = e[k];
            if (q < 0) q = 0;
            if (q > 1) q = 1;
            u[k] = (uint32_t)(uint16_t)(q * 65535.0f);
        }
        *reinterpret_cast<uint2*>(out + b * ostride + o) = make_uint2(u[0] | (u[1] << 16), u[2] | (u[3] << 16));
        if (a && (y == L.h0 - 1 || y == L.h1 + 1)) {  // see k_border
            *reinterpret_cast<float4*>(a + b * stride + o) = v;
            *reinterpret_cast<float4*>(bb + b * stride + o) = v;
        }
    } else {
        *reinterpret_cast<float4*>(a + b * stride + o) = v;
        *reinterpret_cast<float4*>(bb + b * stride + o) = v;
    }
}

#endif

// ---------------------------------------------------------------------------------------------
// The lagged passes of one sweep depth T are built in their own translation unit (the Makefile
// compiles this file once per T with -DPF_JPART=T, and once with PF_JPART=0 for the rest), so the
// 70-odd k_jlag instantiations compile in parallel.
#define PF_JCAT2(a, b) a##b
#define PF_JCAT(a, b) PF_JCAT2(a, b)
#define PF_JDECL(T)                                                                            \
    void PF_JCAT(jlag_launch_t, T)(hipStream_t s, const JacobiPass& P, int batch, bool fast);  \
    int PF_JCAT(jlag_waves_t, T)(bool fast);
PF_JDECL(1) PF_JDECL(2) PF_JDECL(4) PF_JDECL(5) PF_JDECL(8) PF_JDECL(10)

#if defined(PF_JPART) && PF_JPART > 0
template <int T, int SRC, bool OUT16, bool FAST>
static void launch_pass_cts(hipStream_t s, const JacobiPass& P, int batch)
{
    long long jobs = (long long)P.nstrips * P.nchunks;
    dim3 grid((unsigned)((jobs + 3) / 4), batch);
    hipLaunchKernelGGL((k_jlag<T, SRC, OUT16, FAST>), grid, dim3(256), 0, s, P);
}

template <int T, bool FAST>
static void launch_pass_ct(hipStream_t s, const JacobiPass& P, int batch)
{
    if (P.out_mode) {
        if (P.src_mode == SRC_BUF) launch_pass_cts<T, SRC_BUF, true, FAST>(s, P, batch);
        else if (P.src_mode == SRC_UPSAMPLE) launch_pass_cts<T, SRC_UPSAMPLE, true, FAST>(s, P, batch);
        else launch_pass_cts<T, SRC_SEED, true, FAST>(s, P, batch);
    } else {
        if (P.src_mode == SRC_BUF) launch_pass_cts<T, SRC_BUF, false, FAST>(s, P, batch);
        else if (P.src_mode == SRC_UPSAMPLE) launch_pass_cts<T, SRC_UPSAMPLE, false, FAST>(s, P, batch);
        else launch_pass_cts<T, SRC_SEED, false, FAST>(s, P, batch);
    }
}

template <int T, bool FAST>
static int waves_per_cu_t()
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &nb, reinterpret_cast<const void*>(k_jlag<T, SRC_BUF, false, FAST>), 256, 0) != hipSuccess)
        nb = 1;
    return nb * 4;
}

void PF_JCAT(jlag_launch_t, PF_JPART)(hipStream_t s, const JacobiPass& P, int batch, bool fast)
{
    if (fast) launch_pass_ct<PF_JPART, true>(s, P, batch);
    else launch_pass_ct<PF_JPART, false>(s, P, batch);
}

int PF_JCAT(jlag_waves_t, PF_JPART)(bool fast)
{
    return fast ? waves_per_cu_t<PF_JPART, true>() : waves_per_cu_t<PF_JPART, false>();
}
#else  // PF_JPART == 0: dispatch, the pipelined engine, the border kernel

bool jstream_supported_T(int T) { return T == 1 || T == 2 || T == 4 || T == 5 || T == 8 || T == 10; }

static int waves_per_cu_c(int T, bool fast)
{
    switch (T) {
        case 1: return jlag_waves_t1(fast);
        case 2: return jlag_waves_t2(fast);
        case 4: return jlag_waves_t4(fast);
        case 5: return jlag_waves_t5(fast);
        case 8: return jlag_waves_t8(fast);
        default: return jlag_waves_t10(fast);
    }
}

// Resident waves per CU of the pass kernel at depth T (used to size the grid to whole rounds).
int jstream_waves_per_cu(int T, bool fast)
{
    static int cache[2][11] = {{0}};
    if (T < 1 || T > 10 || !jstream_supported_T(T)) return 4;
    int& c = cache[fast ? 1 : 0][T];
    if (!c) c = waves_per_cu_c(T, fast);
    return c;
}

void launch_jstream(hipStream_t s, const JacobiPass& P, int T, int batch, bool fast)
{
    switch (T) {
        case 1: jlag_launch_t1(s, P, batch, fast); break;
        case 2: jlag_launch_t2(s, P, batch, fast); break;
        case 4: jlag_launch_t4(s, P, batch, fast); break;
        case 5: jlag_launch_t5(s, P, batch, fast); break;
        case 8: jlag_launch_t8(s, P, batch, fast); break;
        default: jlag_launch_t10(s, P, batch, fast); break;
    }
}

// Pipelined passes (k_jpipe): T = S * TS.
template <int TS, int S>
static void launch_pipe_ts(hipStream_t s, const JacobiPass& P, int batch)
{
    dim3 grid((unsigned)(P.nstrips * P.nchunks), batch);
    if (P.out_mode) {
        if (P.src_mode == SRC_BUF) hipLaunchKernelGGL((k_jpipe<TS, S, SRC_BUF, true>), grid, dim3(64 * S), 0, s, P);
        else if (P.src_mode == SRC_UPSAMPLE) hipLaunchKernelGGL((k_jpipe<TS, S, SRC_UPSAMPLE, true>), grid, dim3(64 * S), 0, s, P);
        else hipLaunchKernelGGL((k_jpipe<TS, S, SRC_SEED, true>), grid, dim3(64 * S), 0, s, P);
    } else {
        if (P.src_mode == SRC_BUF) hipLaunchKernelGGL((k_jpipe<TS, S, SRC_BUF, false>), grid, dim3(64 * S), 0, s, P);
        else if (P.src_mode == SRC_UPSAMPLE) hipLaunchKernelGGL((k_jpipe<TS, S, SRC_UPSAMPLE, false>), grid, dim3(64 * S), 0, s, P);
        else hipLaunchKernelGGL((k_jpipe<TS, S, SRC_SEED, false>), grid, dim3(64 * S), 0, s, P);
    }
}

// (S, TS) pairs the pipelined engine is built for; T = S * TS
bool jpipe_supported(int S, int TS) { return S == 2 && (TS == 5 || TS == 4); }

void launch_jpipe(hipStream_t s, const JacobiPass& P, int S, int TS, int batch)
{
    if (S == 2 && TS == 5) launch_pipe_ts<5, 2>(s, P, batch);
    else if (S == 2 && TS == 4) launch_pipe_ts<4, 2>(s, P, batch);
}

template <int TS, int S>
static int pipe_waves_per_cu_t()
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &nb, reinterpret_cast<const void*>(k_jpipe<TS, S, SRC_BUF, false>), 64 * S, 0) != hipSuccess)
        nb = 1;
    return nb * S;
}

int jpipe_waves_per_cu(int S, int TS)
{
    static int cache[2] = {0, 0};
    const int i = TS == 5 ? 0 : 1;
    if (!cache[i]) cache[i] = TS == 5 ? pipe_waves_per_cu_t<5, 2>() : pipe_waves_per_cu_t<4, 2>();
    (void)S;
    return cache[i];
}

void launch_border(hipStream_t s, const float* prev, long long pstride, LevelDims L, float* a,
                   float* b, long long stride, uint16_t* out, long long ostride, int batch)
{
    long long n = (long long)(L.h0 + (L.h - 1 - L.h1)) * L.w;
    if (n <= 0) return;
    // the vector form needs 4 | w (then the plane strides are multiples of 4 too: aligned stores)
    if (L.w % 4 == 0 && stride % 4 == 0 && ostride % 4 == 0 && pstride % 2 == 0) {
        dim3 grid((unsigned)((n / 4 + 255) / 256), batch);
        hipLaunchKernelGGL(k_border4, grid, dim3(256), 0, s, prev, pstride, L, a, b, stride, out,
                           ostride);
        return;
    }
    dim3 grid((unsigned)((n + 255) / 256), batch);
    hipLaunchKernelGGL(k_border, grid, dim3(256), 0, s, prev, pstride, L, a, b, stride, out,
                       ostride);
}

#endif  // PF_JPART

}  // namespace pf
