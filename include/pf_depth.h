/*
 * pf_depth.h -- the reference's C++ entry points for the fusion path (Depth.h), served by
 * libpanofuse_depth.so on top of the C-ABI of panofuse.h.  A caller of the reference's
 * DepthNamespace (Main.cpp:592, :663) recompiles against this header and links
 * -lpanofuse_depth -lpanofuse; the arithmetic runs in the HIP kernels of libpanofuse.
 *
 * Entry points and the reference interface each one replaces:
 *   EquirectangularMap::{Load, LoadPfm, ValueAtCoord, ValueAtXY, Avg, CopyInvalidPixels,
 *                        DispDepthConversion, Save8bit}                Depth.h:9-59
 *   PerspectiveMap::{Load, SetWindow, Value, ValueAtXY, ToSphericalCoord, SphericalTo2D,
 *                    Contain, Azimuth/ZenithMin/Max, D2DTransform, Depth2DepthTransform}
 *                    and the cached window members middle/hedge/vedge/corner0-3
 *                                                                      Depth.h:61-158
 *   Metrics::{Save, Print}                                             Depth.h:161-250
 *   MergeDepthMaps                                                     Depth.h:286-289
 *   SolveDisparityToDepth (declared there, defined here)               Depth.h:293-294
 *   SolveDepthToDepth                                                  Depth.h:297-298
 *   SolveDepthToDepth2                                                 Depth.h:300-301
 *   SolveDepthAll                                                      Depth.h:306-307
 *   SolveDepthBySmoothing                                              Depth.h:309
 *   ErrorData / ErrorEmap                                              Depth.h:313-316
 *   ErrorCompare                                                       Depth.h:318-319
 *   ErrorLaplacian                                                     Depth.h:321-323
 *   SphericalToWorld / WorldToSpherical                                Depth.h:326-329
 *   MedianScaling                                                      Depth.h:337
 *   Save16BitPNG                                                       Depth.cpp:27-32
 *   g_zenith_range                                                     Depth.cpp:22
 *
 * Ownership follows the reference: the map classes own `data` (new[]), MergeDepthMaps
 * allocates and frees its own u16 output, SolveDepthAll writes a caller buffer of W*H u16.
 * Errors: false returns with a message on std::cout, as the reference prints its diagnostics.
 * Threading: one host thread per device (the facade keeps one pf_ctx per device).
 *
 * The window geometry and projections (SetWindow, ToSphericalCoord, SphericalTo2D, Contain,
 * SphericalToWorld, WorldToSpherical) are host fp32 code with the reference's Imath semantics
 * and glibc calls (csrc/pf_geom.hpp), bit-identical to it; the per-pixel path runs on the GPU.
 *
 * Extensions (not in the reference): MergeDisparityMaps, MergeDepthMaps for disparity tiles;
 * TransformResult, the cubic of SolveDepthToDepth2 applied to the u16 result; StitchDepthMaps and
 * CheckLaplacian, the two `if (false)` diagnostics of MergeDepthMaps / SolveDepthAll as calls.
 * MergeDepthMaps / MergeDisparityMaps read three environment switches (panofuse_main sets them
 * from --fusion, --save-stitch, --check-laplacian): PF_FUSION=laplacian|smoothing|stitch chooses
 * what fills the result (Depth.cpp:904-922, :851; laplacian, the default, is the reference's
 * active path; smoothing and stitch run on the registered tiles), PF_SAVE_STITCH=1 also writes
 * <out>.pmap.png (:859), PF_CHECK_LAPLACIAN=1 prints "[SolveDepthAll] check Laplacian err:<err>"
 * (:1757) after the fusion and is refused with any other PF_FUSION.
 * SetTileValidity (an extension too) sets the tile-pixel validity rule of the library
 * (pf_set_tile_validity, include/panofuse.h): SolveDepthToDepth, SolveDepthAll, MergeDepthMaps,
 * StitchDepthMaps and CheckLaplacian then skip the tile pixels outside (lo, hi);
 * SolveDisparityToDepth, MergeDisparityMaps and SolveDepthBySmoothing fail with the library's
 * message while it is on.  MergeDepthMaps also reads PF_TILE_VALID=LO:HI (panofuse_main
 * --tile-valid; "-inf" / "inf" allowed, a malformed value is an error), which holds for that call,
 * and under the rule prints "[mask] tile <i>: <n> of <N> pixels invalid, <m> of <M> samples" per
 * tile that has invalid pixels.
 *
 * Not provided: a SolveDisparityToDepth over several active maps (a joint nonlinear solve), the
 * triangulation/subdivision members (vertices, faces, subd_*: never used on the path).
 */
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#ifndef PF_DEPTH_NO_VEC
/* The vector types of the reference's ILMBase.h:14-16 (`typedef Imath::Vec4<float> Vec4f`, ...)
 * for callers that do not include Imath.  They are declared as class templates in namespace
 * Imath with Imath's layout (public x, y[, z[, w]] of T, ImathVec.h:63-66, 259-262, 563-566),
 * so the entry points below mangle exactly as the reference's do
 * (`DepthNamespace::MergeDepthMaps(..., std::vector<Imath::Vec4<float>>&, ..., Imath::Vec2<float>&,
 * ...)`): libpanofuse_depth.so is built with these, and a caller that includes the real
 * ILMBase.h first and then this header with -DPF_DEPTH_NO_VEC (as Main.cpp:13-15 includes
 * ILMBase.h before Depth.h) links against the same symbols.  Like Imath's, the copy
 * constructors are user-provided (ImathVec.h:96, 294, 507), which makes the types non-trivial for
 * calls: a Vec2f returned by value travels through a hidden pointer in both builds, so the
 * calling convention matches as well as the names.  Every member is inline (and hidden
 * in the library: -fvisibility-inlines-hidden), so nothing here competes with the real Imath.
 * The operations are the ones a caller of the window members uses, with Imath's arithmetic
 * (ImathVec.h:1467-1486 dot/cross, :1631-1700 length with lengthTiny, normalize by division). */
#include <cmath>
#include <limits>
namespace Imath {
template <class T>
class Vec2 {
public:
    T x, y;
    Vec2() : x(0), y(0) {}
    explicit Vec2(T a) : x(a), y(a) {}
    Vec2(T a, T b) : x(a), y(b) {}
    Vec2(const Vec2& v) : x(v.x), y(v.y) {}
    const Vec2& operator=(const Vec2& v) { x = v.x; y = v.y; return *this; }
    T& operator[](int i) { return (&x)[i]; }
    const T& operator[](int i) const { return (&x)[i]; }
    T dot(const Vec2& v) const { return x * v.x + y * v.y; }
    T length() const
    {
        const T l2 = dot(*this);
        if (l2 < T(2) * std::numeric_limits<T>::min()) {  // lengthTiny
            T ax = x >= T(0) ? x : -x, ay = y >= T(0) ? y : -y;
            const T mx = ax < ay ? ay : ax;
            if (mx == T(0)) return T(0);
            ax /= mx;
            ay /= mx;
            return mx * std::sqrt(ax * ax + ay * ay);
        }
        return std::sqrt(l2);
    }
};
template <class T>
class Vec3 {
public:
    T x, y, z;
    Vec3() : x(0), y(0), z(0) {}
    explicit Vec3(T a) : x(a), y(a), z(a) {}
    Vec3(T a, T b, T c) : x(a), y(b), z(c) {}
    Vec3(const Vec3& v) : x(v.x), y(v.y), z(v.z) {}
    const Vec3& operator=(const Vec3& v) { x = v.x; y = v.y; z = v.z; return *this; }
    T& operator[](int i) { return (&x)[i]; }
    const T& operator[](int i) const { return (&x)[i]; }
    Vec3 operator+(const Vec3& v) const { return Vec3(x + v.x, y + v.y, z + v.z); }
    Vec3 operator-(const Vec3& v) const { return Vec3(x - v.x, y - v.y, z - v.z); }
    Vec3 operator*(T s) const { return Vec3(x * s, y * s, z * s); }
    T dot(const Vec3& v) const { return x * v.x + y * v.y + z * v.z; }
    Vec3 cross(const Vec3& v) const
    {
        return Vec3(y * v.z - z * v.y, z * v.x - x * v.z, x * v.y - y * v.x);
    }
    T length() const
    {
        const T l2 = dot(*this);
        if (l2 < T(2) * std::numeric_limits<T>::min()) {  // lengthTiny
            T ax = x >= T(0) ? x : -x, ay = y >= T(0) ? y : -y, az = z >= T(0) ? z : -z;
            T mx = ax;
            if (mx < ay) mx = ay;
            if (mx < az) mx = az;
            if (mx == T(0)) return T(0);
            ax /= mx;
            ay /= mx;
            az /= mx;
            return mx * std::sqrt(ax * ax + ay * ay + az * az);
        }
        return std::sqrt(l2);
    }
    const Vec3& normalize()  /* in place, returns *this */
    {
        const T l = length();
        if (l != T(0)) {
            x /= l;
            y /= l;
            z /= l;
        }
        return *this;
    }
};
template <class T>
inline Vec3<T> operator*(T s, const Vec3<T>& v) { return Vec3<T>(s * v.x, s * v.y, s * v.z); }
template <class T>
class Vec4 {
public:
    T x, y, z, w;
    Vec4() : x(0), y(0), z(0), w(0) {}
    explicit Vec4(T a) : x(a), y(a), z(a), w(a) {}
    Vec4(T a, T b, T c, T d) : x(a), y(b), z(c), w(d) {}
    Vec4(const Vec4& v) : x(v.x), y(v.y), z(v.z), w(v.w) {}
    const Vec4& operator=(const Vec4& v) { x = v.x; y = v.y; z = v.z; w = v.w; return *this; }
    T& operator[](int i) { return (&x)[i]; }
    const T& operator[](int i) const { return (&x)[i]; }
};
}  // namespace Imath
typedef Imath::Vec2<float> Vec2f;
typedef Imath::Vec3<float> Vec3f;
typedef Imath::Vec4<float> Vec4f;
#endif

#define PF_MYPI_D 3.14159265359          /* Basic.h:11 */
#define PF_D2R(a) ((a) / 180.0 * PF_MYPI_D) /* Basic.h:14 */

extern Vec2f g_zenith_range; /* Depth.cpp:22 Vec2f(D2R(26), D2R(154)) */

bool Save16BitPNG(unsigned short* data, int width, int height, const char* filename);
/* A one-channel 8-bit PNG with the bytes of stbi_write_png(filename, width, height, 1, data,
 * width), the call that ErrorCompare and Save8bit make (Depth.cpp:2596, :632). */
bool Save8BitPNG(const unsigned char* data, int width, int height, const char* filename);

namespace DepthNamespace {

class EquirectangularMap {
public:
    int width = 0, height = 0, channels = 0;
    float* data = nullptr; /* [height][width][channels], 0..1 */

    EquirectangularMap() = default;
    ~EquirectangularMap();
    EquirectangularMap(const EquirectangularMap&) = delete;
    EquirectangularMap& operator=(const EquirectangularMap&) = delete;

    bool Load(std::string& filename, bool mono360 = false);
    bool LoadPfm(std::string& filename, bool flip_vertical, bool normalize,
                 const char* save_png_filename = nullptr);
    float ValueAtCoord(float azimuth, float zenith);
    float ValueAtXY(int x, int y);
    double Avg();
    /* mark invalid pixels from a reference emap (Depth.h:52, Depth.cpp:703-725), on the GPU
     * (pf_copy_invalid): channel 0 of ref_emap at (int((float)x * ratio_x), int((float)y *
     * ratio_y)) is copied into channel 0 of this map where it is < 1e-4 or >= 1 - 1e-4 */
    void CopyInvalidPixels(EquirectangularMap& ref_emap);
    /* disparity <-> depth (Depth.cpp:587-610) on the GPU (pf_disp_depth_convert): channel 0 becomes
     * 1 / v where (double)fabsf(v) >= 1e-5 -- once per channel of the map, as the reference's loop
     * over the channels converts channel 0 each time */
    void DispDepthConversion();
    /* channel 0, clamped to 0..1, as (unsigned char)(v * 255.0f) in a one-channel 8-bit PNG with
     * stbi_write_png's bytes (Depth.cpp:612-635); NaN becomes 0.  Returns false when the file
     * cannot be written (the reference returns true regardless). */
    bool Save8bit(std::string& filename);
};

class PerspectiveMap {
public:
    int width = 0, height = 0, channels = 0;
    float* data = nullptr;
    /* the FOVs of the viewing window (SetWindow arguments, Depth.h:70-73) */
    float azimuth_left = 0, azimuth_right = 0, zenith_top = 0, zenith_down = 0;
    Vec4f ranges; /* valid {azi_left, azi_right, zen_up, zen_down} (Depth.h:76) */
    /* the cached quadrilateral window of SetWindow (Depth.h:87-93) */
    Vec3f middle, hedge, vedge;
    Vec3f corner0, corner1, corner2, corner3;
    bool window_set = false;

    PerspectiveMap() = default;
    ~PerspectiveMap();
    PerspectiveMap(PerspectiveMap&& o) noexcept;
    PerspectiveMap& operator=(PerspectiveMap&& o) noexcept;
    PerspectiveMap(const PerspectiveMap&) = delete;
    PerspectiveMap& operator=(const PerspectiveMap&) = delete;

    bool Load(std::string& filename);
    void SetWindow(float AzimuthLeft, float AzimuthRight, float ZenithTop, float ZenithDown);
    float Value(float x, float y);
    Vec2f ToSphericalCoord(float x, float y);       /* Depth.cpp:157-166 */
    Vec2f SphericalTo2D(float azimuth, float zenith); /* Depth.cpp:168-182 */
    bool Contain(float azimuth, float zenith);        /* Depth.cpp:184-207 */
    float AzimuthMin() { return azimuth_left < azimuth_right ? azimuth_left : azimuth_right; }
    float AzimuthMax() { return azimuth_left > azimuth_right ? azimuth_left : azimuth_right; }
    float ZenithMin() { return zenith_top < zenith_down ? zenith_top : zenith_down; }
    float ZenithMax() { return zenith_top > zenith_down ? zenith_top : zenith_down; }
    float ValueAtXY(int x, int y);                    /* Depth.cpp:209-212 */
    /* Y = c / (a X + b) + d on channel 0 (Depth.h:155, Depth.cpp:214-243: X a disparity in 0-1,
     * clamped to [1e-4, 1 - 1e-4]; Y clamped to 0-1); runs on the GPU (pf_disparity_transform) */
    void D2DTransform(Vec4f abcd);
    void Depth2DepthTransform(Vec4f& abcd); /* runs on the GPU (pf_depth_transform) */
};

class Metrics {
public:
    float mse_given = 0, mse_result = 0, mae_given = 0, mae_result = 0, mre_given = 0,
          mre_result = 0, mselog_given = 0, mselog_result = 0, delta1_given = 0,
          delta1_result = 0, delta2_given = 0, delta2_result = 0, delta3_given = 0,
          delta3_result = 0;
    bool Save(const char* filename);
    void Print();
};

bool MergeDepthMaps(std::string& equirectangular_map_filename,
                    std::vector<std::string>& perspective_map_filenames,
                    std::string& out_filename, std::vector<Vec4f>& perspective_map_FOVs,
                    std::vector<Vec4f>& perspective_map_ranges, int out_width,
                    Vec2f& zenith_range, std::string* equirectangular_map_groundtruth = nullptr,
                    Metrics* metrics = nullptr, int* time_Reg = nullptr,
                    int* time_Laplacian = nullptr);

/* EXTENSION (not in the reference): MergeDepthMaps for tiles that hold relative inverse depth
 * in 0-1 (MiDaS / DPT).  Every tile is registered alone with SolveDisparityToDepth's model and
 * mapped to depth by D2DTransform; everything else (fusion, files written, metrics, timers) is
 * MergeDepthMaps'. */
bool MergeDisparityMaps(std::string& equirectangular_map_filename,
                        std::vector<std::string>& perspective_map_filenames,
                        std::string& out_filename, std::vector<Vec4f>& perspective_map_FOVs,
                        std::vector<Vec4f>& perspective_map_ranges, int out_width,
                        Vec2f& zenith_range,
                        std::string* equirectangular_map_groundtruth = nullptr,
                        Metrics* metrics = nullptr, int* time_Reg = nullptr,
                        int* time_Laplacian = nullptr);

/* Depth.h:291-294: the disparity-to-depth transform y = c / (a x + b) + d (x a tile's disparity,
 * y the baseline's depth) with c fixed at 1, as the reference's FunctorDisparity2Depth
 * (Depth.cpp:1044-1073) has it; abcd = (a, b, 1, d) for D2DTransform.  Exactly one map may be
 * active: more (or none) returns false with a message. */
bool SolveDisparityToDepth(EquirectangularMap& emap, std::vector<PerspectiveMap>& pmaps,
                           std::vector<bool>& pmaps_actives, Vec2f& zenith_range, Vec4f& abcd);

bool SolveDepthToDepth(EquirectangularMap& emap, std::vector<PerspectiveMap>& pmaps,
                       std::vector<bool>& pmaps_actives, Vec2f& zenith_range, Vec4f& abcd);

/* EXTENSION (the reference registers every map to the baseline on its own, so neighbours never
 * meet): the cubics of all maps fitted at once, each to the baseline and to its neighbours where
 * their windows overlap, lambda >= 0 weighing the overlap term (pf_register_consistent,
 * include/panofuse.h; lambda = 0 is the independent least squares).  abcd_out[i] belongs to
 * pmaps[i]; the maps are not modified.  Prints the library's message and returns false under
 * SetTileValidity, SetRegistrationLoss or SetTileDepth(1), for a bad lambda, and when the joint
 * system is singular. */
bool SolveDepthToDepthConsistent(EquirectangularMap& emap, std::vector<PerspectiveMap>& pmaps,
                                 Vec2f& zenith_range, double lambda, std::vector<Vec4f>& abcd_out);
/* EXTENSION: how much the maps disagree where they overlap (pf_overlap_stats).  One entry per
 * ordered pair (p, q) with overlap samples, in ascending (p, q): over the registration samples of
 * map p that fall inside map q's window, d = T_p(value in p) - T_q(value in q) with T the
 * Depth2DepthTransform of abcds (one Vec4f per map; an empty vector: the values as they are). */
struct TileOverlapStat {
    int p, q;
    double count, sum, sum_sq, max_abs;  /* of d over the samples counted */
    double nan_count;                    /* samples left out: a NaN on either side */
};
bool TileOverlapStats(std::vector<PerspectiveMap>& pmaps, std::vector<Vec4f>& abcds,
                      Vec2f& zenith_range, std::vector<TileOverlapStat>& stats_out);

/* Depth.h:300-301, Depth.cpp:1158-1259: the final global registration of a fused u16 result
 * (data [height][width]) to the baseline emap: one cubic fitted on every pixel of the band rows by
 * the reference's LM from (0, 0, 1, 0), on the GPU (pf_register_global).  Prints the reference's
 * "[SolveDepthToDepth2] abcd:(a b c d) cost:<initial>-><final>" line.  data is not modified. */
bool SolveDepthToDepth2(EquirectangularMap& emap, unsigned short* data, int width, int height,
                        Vec2f& zenith_range, Vec4f& abcd);
/* EXTENSION (not in the reference, which leaves the use of SolveDepthToDepth2's abcd to the
 * caller): Depth2DepthTransform's cubic on the band rows of the u16 result, in place, on the GPU
 * (pf_result_transform): v = (float)d / 65535.0f, Y clamped to 0-1, NaN becomes 0,
 * d = (unsigned short)(Y * 65535.0f); the other rows are left untouched. */
bool TransformResult(unsigned short* data, int width, int height, Vec2f& zenith_range,
                     Vec4f& abcd);

bool SolveDepthAll(EquirectangularMap& emap, std::vector<PerspectiveMap>& pmaps,
                   unsigned short* data, int& out_width, int& out_height, Vec2f& zenith_range,
                   const char* Laplacian_filename = nullptr);
// Depth.h:309, Depth.cpp:1773-1878: the reference's alternate solver (tiles written into the
// grid, 500 Gauss-Seidel smoothing iterations near the tile-box edges), on the GPU, bit-exact.
bool SolveDepthBySmoothing(std::vector<PerspectiveMap>& pmaps, unsigned short* data,
                           int& out_width, int& out_height, Vec2f& zenith_range);
/* EXTENSION (not in the reference, which reads every tile pixel as depth): the tile-pixel
 * validity rule of every later call of this facade, process-wide.  on: a raw tile value v
 * (channel 0) counts only if lo < v && v < hi in fp32 -- NaN never does; lo = -INFINITY,
 * hi = INFINITY rejects exactly NaN and +-Inf, lo = 0 also holes written as 0.  off (the default):
 * every pixel is read.  false (and a message) for on with !(lo < hi). */
bool SetTileValidity(bool on, float lo, float hi);
/* EXTENSION (the reference passes NULL as the loss, Depth.cpp:1232, 1393): the robust loss of the
 * tile registrations of every later call of this facade, process-wide (pf_set_register_loss,
 * include/panofuse.h): kind 0 none (the default), 1 Ceres' HuberLoss(a), 2 SoftLOneLoss(a), a
 * finite and > 0.  Honoured by MergeDepthMaps, SolveDepthToDepth with one active map,
 * MergeDisparityMaps and SolveDisparityToDepth; SolveDepthToDepth with several active maps and
 * SolveDepthToDepth2 print the library's message and return false while it is set.
 * MergeDepthMaps / MergeDisparityMaps also read PF_REG_LOSS=huber:A|softl1:A (panofuse_main
 * --reg-loss), which holds for that call, and under a loss print per tile "[robust] tile <i>: <m>
 * of <n> samples beyond a=<A>, cost <c0> -> <c1>, <it> iterations, <termination>".  false (and a
 * message) for an unknown kind or a bad scale. */
bool SetRegistrationLoss(int kind, double a);
/* EXTENSION (the reference reads every tile value as ray distance): what the tiles of every later
 * call of this facade hold, process-wide (pf_set_tile_depth, include/panofuse.h): kind 0 ray
 * distance (the default), 1 planar depth, i.e. depth along the optical axis as perspective depth
 * networks predict it.  Under planar depth MergeDepthMaps / MergeDisparityMaps register with the
 * per-pixel ray factor, transform the uploaded tiles and fuse, stitch or smooth those, and print
 * "[tile-depth] planar: ray factor up to <max> over <n> tiles"; SolveDepthToDepth with one active
 * map and SolveDisparityToDepth fit with the factor; the calls that hand the library a transform to
 * fuse into its gather, and SolveDepthToDepth with several active maps, print the library's message
 * and return false.  MergeDepthMaps / MergeDisparityMaps also read PF_TILE_DEPTH=planar|ray
 * (panofuse_main --tile-depth), which holds for that call.  false (and a message) for another
 * kind. */
bool SetTileDepth(int kind);
/* EXTENSION (the reference's registration functors carry a Weight that its only call site sets to
 * 1.0f, Depth.cpp:1044-1150, 1366-1375): per-pixel tile weights for every later MergeDepthMaps of
 * this facade, process-wide (pf_register_weighted / pf_fuse_weighted, include/panofuse.h).  mode 0
 * off (the default), 1 the blending tent of every tile (pf_tile_tent_weights), 2 files: the weight
 * map of a tile file F is F + suffix: a PNG read as a tile is (samples in 0-1), or a PFM read raw
 * (its floats as stored, rows in file order, top row first), channel 0 of either, and of the
 * tile's width and height, else MergeDepthMaps names the file and returns false.  A weight that is
 * not in (0, +inf) switches its pixel off; weights in {0, 1} are the validity rule.
 * MergeDepthMaps then registers every tile by weighted least squares, fuses the weighted Laplacian
 * targets and prints per tile "[weights] tile <i>: <n> of <N> samples used, sum w <s>".  It also
 * reads PF_TILE_WEIGHTS=tent|files:SUFFIX (panofuse_main --tile-weights), which holds for that
 * call.  With weights on it returns false, before any file is read, together with
 * SetTileValidity, SetRegistrationLoss, SetTileDepth(1), PF_REG_CONSISTENT, PF_GLOBAL_ALIGN,
 * PF_CHECK_LAPLACIAN or PF_FUSION=smoothing|stitch; MergeDisparityMaps does so always.  false (and
 * a message) for another mode, or for mode 2 with an empty suffix or one that holds a path
 * separator. */
bool SetTileWeights(int mode, const std::string& suffix = "");
/* EXTENSION: per-pixel weights for the disparity tiles of every later MergeDisparityMaps of this
 * facade, process-wide (pf_register_disparity_weighted / pf_merge_disparity_weighted,
 * include/panofuse.h).  mode 0 off (the default), 1 the blending tent, 2 files: arg is the SUFFIX of
 * SetTileWeights' weight files, 3 range: arg is "LO:HI" and a pixel counts iff LO < v < HI
 * (pf_tile_range_weights on the uploaded tiles; "0:inf" drops the disparity-0 sky a network
 * writes).  MergeDisparityMaps then fits every tile by weighted least squares, fuses the weighted
 * Laplacian targets of the transformed tiles and prints SetTileWeights' "[weights] tile <i>: ..."
 * lines.  It also reads PF_DISPARITY_WEIGHTS=tent|files:SUFFIX|range:LO:HI (panofuse_main
 * --disparity-weights), which holds for that call.  Accepted with SetTileDepth(1).  With the switch
 * on, MergeDisparityMaps returns false, before any file is read, together with SetTileValidity,
 * SetRegistrationLoss, PF_REG_CONSISTENT, PF_GLOBAL_ALIGN, PF_CHECK_LAPLACIAN,
 * PF_FUSION=smoothing|stitch or SetTileWeights, and MergeDepthMaps (depth tiles) does so always.
 * false (and a message) for another mode or a malformed arg. */
bool SetDisparityWeights(int mode, const std::string& arg = "");
/* EXTENSION (in the reference an `if (false)` block of MergeDepthMaps, Depth.cpp:817-865): the
 * direct stitch of the tiles as they are into data (width * height u16) -- every pixel takes the
 * first map whose range box contains it, no fusion -- on the GPU (pf_stitch), bit-exact. */
bool StitchDepthMaps(std::vector<PerspectiveMap>& pmaps, unsigned short* data, int& width,
                     int& height);
/* EXTENSION (in the reference an `if (false)` block of SolveDepthAll, Depth.cpp:1738-1758): runs
 * the fusion of the maps as they are and returns, per level, the squared distance between the
 * solved plane's 5-point Laplacian and the level's targets, summed in the reference's order
 * (pf_fuse_check).  err_per_level.back() is the number the reference prints as
 * "[SolveDepthAll] check Laplacian err:"; the coarser levels' are the same formula. */
bool CheckLaplacian(EquirectangularMap& emap, std::vector<PerspectiveMap>& pmaps, int width,
                    int height, Vec2f& zenith_range, std::vector<float>& err_per_level);

bool ErrorData(EquirectangularMap& emap_gt, unsigned short* data, int data_width,
               int data_height, float& mse, float& mae, float& mre, float& mse_log,
               float& delta1, float& delta2, float& delta3, int align_way, bool cap_depth,
               Vec2f* least_square_shift = nullptr, float* median_shift_factor = nullptr);
bool ErrorEmap(EquirectangularMap& emap_gt, EquirectangularMap& emap_given, float& mse,
               float& mae, float& mre, float& mse_log, float& delta1, float& delta2,
               float& delta3, int align_way, bool cap_depth,
               Vec2f* least_square_shift = nullptr, float* median_shift_factor = nullptr);

/* Two-file comparison (Depth.cpp:2460-2634), on the GPU (pf_error_compare, whose comment in
 * panofuse.h has the chain step by step).  The gt is loaded with Load(fn), the baseline with
 * Load(fn, true) (a mono360 PFM is flipped and normalised to 0..1); a load failure prints the
 * reference's "cannot load emap_gt? ..." / "cannot load emap_baseline? ..." and returns false
 * before any GPU call.  DispDepthCompare == false: ErrorEmap(gt, baseline, align_way, cap_depth),
 * and with a file name the baseline as an 8-bit PNG.  DispDepthCompare == true: the baseline is a
 * disparity; it is least-squares-aligned to the gt's disparity, converted to depth, clipped to
 * [0, 10], scored with ErrorEmap(align_way, cap_depth), and its non-black pixels, normalised to
 * their min..max (printed as "DispDepthCompare emap_baseline minmax:..."), are written as an
 * 8-bit PNG, followed by "[ErrorCompare] <ret> saved shifted emap:...".
 * Where the reference's behaviour is undefined, this is the rule: a null shifted_filename in
 * disparity mode writes no file (the reference passes it to stbi_write_png); a product above 255
 * saturates to 255; NaN becomes 0 in the 8-bit plane; every comparison otherwise follows IEEE as
 * the source reads, so a NaN is not black, does not move the min / max and stays NaN in the depth
 * plane. */
bool ErrorCompare(std::string& gt_filename, std::string& baseline_filename, bool DispDepthCompare,
                  float& mse, float& mae, float& mre, float& mselog, float& delta1, float& delta2,
                  float& delta3, int align_way, bool cap_depth,
                  const char* shifted_filename = nullptr);
/* The same for maps already in memory (neither is modified).  fit: the disparity fit {s, o};
 * minmax: {vmin, vmax} of the non-black pixels; shifted: the 8-bit plane [height][width] of the
 * baseline; n_nonblack: the number of pixels that were normalised (nothing is written to a file,
 * nothing is printed). */
bool ErrorCompare(EquirectangularMap& emap_gt, EquirectangularMap& emap_baseline,
                  bool DispDepthCompare, float& mse, float& mae, float& mre, float& mselog,
                  float& delta1, float& delta2, float& delta3, int align_way, bool cap_depth,
                  Vec2f* fit = nullptr, Vec2f* minmax = nullptr,
                  std::vector<unsigned char>* shifted = nullptr, int* n_nonblack = nullptr);

/* Edge-fidelity errors between a ground-truth map and a given map, both loaded with
 * EquirectangularMap::Load (Depth.cpp:2636-2953): mse and mae of the 3x3 Laplacian, mae of
 * Sobel X, Sobel Y and of the 5x5 LoG filter, computed on the GPU (pf_error_laplacian) and
 * printed as the reference's "[ErrorLap] ..." line.  The three file-name arguments are accepted
 * and ignored: the reference's own writing of those images is commented out (Depth.cpp:2779-2830),
 * so it never produces them either.  (pf_error_laplacian returns the three Laplacian maps as
 * device planes for callers that want them.) */
bool ErrorLaplacian(std::string& gt_filename, std::string& baseline_filename,
                    double& Laplacian_mse, double& Laplacian_mae, double& SobelX_mae,
                    double& SobelY_mae, double& Laplacian5x5_mae,
                    std::string* gt_Laplacian_fn = nullptr,
                    std::string* baseline_Laplacian_fn = nullptr,
                    std::string* Laplacian_ae_fn = nullptr);
/* The same for maps already in memory; counts (optional): long long[3] = the numbers of
 * Laplacian, Sobel and 5x5 samples behind the means. */
bool ErrorLaplacian(EquirectangularMap& emap_gt, EquirectangularMap& emap_baseline,
                    double& Laplacian_mse, double& Laplacian_mae, double& SobelX_mae,
                    double& SobelY_mae, double& Laplacian5x5_mae, long long* counts = nullptr);

/* spherical coord. (radians) to 3d position (Depth.cpp:2955-2958) */
Vec3f SphericalToWorld(float azimuth, float zenith);
/* 3d position to spherical coord.; p is normalized in place (Depth.cpp:2960-2971) */
Vec2f WorldToSpherical(Vec3f& p);

/* median scaling emap0 toward emap1 (Depth.h:337, Depth.cpp:637-701), on the GPU
 * (pf_median_scale): channel 0 of emap0 is multiplied by median1 / median0 on its valid pixels
 * (!(v < 1e-4 || v >= 1 - 1e-4)); the medians are the order statistics at index n / 2 of the
 * valid values.  Where the reference's behaviour is undefined, this is the rule: NaN counts as
 * invalid, and a map without any valid pixel returns false after the reference's
 * "MedianScaling: zero val0_median ??" line, before any GPU call, with nothing written. */
bool MedianScaling(EquirectangularMap& emap0, EquirectangularMap& emap1,
                   float* emap0_median = nullptr, float* emap1_median = nullptr);

}  // namespace DepthNamespace

/* The mode-0 driver (Main.cpp:331-687 CreateDepthPanoramas) over std::filesystem; tile_ext is
 * "png" (MiDaS naming, Main.cpp:570-573), "jpg" (LeReS naming, :576-578) or "auto".  The tile
 * layout is the one PF_LAYOUT names in the environment (panofuse_main --layout NAME|FILE: leres,
 * midas, fold4, fold3 or a layout file, see pf_resolve_layout), by default the LeReS layout of
 * Main.cpp:788-843; an unusable PF_LAYOUT returns 2 before any GPU call.  After the first fused
 * panorama the layout is audited once (pf_layout_audit) and every level with taps outside their
 * tile prints "[layout] level L (WxH): N taps outside their tile (clamped)", in place of the
 * reference's per-tap "oops!".  With PF_TILE_MODEL=disparity in the environment
 * (panofuse_main --tile-model disparity) the tiles are disparities: MergeDisparityMaps.  shard / nshards: this process takes the panoramas
 * shard, shard + nshards, ... of the sorted folder (one process per GPU, no communication).
 * With PF_GLOBAL_ALIGN=1 in the environment (panofuse_main --global-align) MergeDepthMaps and
 * MergeDisparityMaps run SolveDepthToDepth2 and TransformResult's cubic on the fused result before
 * it is written and scored.
 * With PF_EDGE_METRICS=1 in the environment (panofuse_main --edge-metrics) each panorama also
 * gets <raw>.edges.txt: ErrorLaplacian of the result and of the baseline against the gt.
 * Returns the process exit code. */
int pf_create_depth_panoramas(const std::string& rgb_folder, const std::string& gt_folder,
                              const std::string& baseline_folder,
                              const std::string& result_folder, const std::string& tile_dir,
                              const std::string& tile_ext, int out_width, int shard = 0,
                              int nshards = 1);
/* The RGB tile export of mode 0 (Main.cpp:399-430 + SaveCubeMap :242-326): every panorama of
 * rgb_folder (8/16-bit PNG, PGM/PPM) warped on the GPU (pf_warp_rgb) into the tiles of the
 * layout PF_LAYOUT names (as above; by default the 15 LeReS tiles), each
 * 1024 x round(1024/aspect) px, written as <tile_dir>/<raw>.<a0>_<a1>_<z0>_<z1>.jpg (rows
 * top-first, like the reference's flipped write; baseline JPEG at quality 100, 4:4:4, as the
 * reference's stbi_write_jpg call ends up, Main.cpp:319-320). */
int pf_export_rgb_tiles(const std::string& rgb_folder, const std::string& tile_dir);
/* The active LeReS layout (Main.cpp:788-843): 15 FOVs and ranges. */
void pf_leres_layout(std::vector<Vec4f>& fovs, std::vector<Vec4f>& ranges);
/* The reference's four tables by name, with its float rounding: "leres" (Main.cpp:788-843),
 * "midas" (:731-787, 15 tiles), "fold4" (:695-730, 12 tiles), "fold3" (:845-887, 9 tiles); tile
 * order bands outer, sectors inner.  false for an unknown name. */
bool pf_named_layout(const std::string& name, std::vector<Vec4f>& fovs,
                     std::vector<Vec4f>& ranges);
/* A layout file: one tile per line, eight numbers in degrees (the window's az_left az_right
 * zen_top zen_down, then the range's az_left az_right zen_up zen_down); '#' starts a comment,
 * blank lines are skipped.  Every value becomes (float)D2R(deg), computed in double and rounded
 * once: a file with fold4's degrees is fold4 bit for bit, while leres / midas / fold3 come from
 * float additions and are in general not reproduced by their rounded degrees.  false with a
 * message in *err for a line without exactly eight numbers, a non-finite value, no tiles or more
 * than 4096 tiles. */
bool pf_load_layout_file(const std::string& path, std::vector<Vec4f>& fovs,
                         std::vector<Vec4f>& ranges, std::string* err);
/* A known name, else a layout file (what --layout and PF_LAYOUT take). */
bool pf_resolve_layout(const std::string& spec, std::vector<Vec4f>& fovs,
                       std::vector<Vec4f>& ranges, std::string* err);

/* C-ABI helpers (ctypes bindings, tests): load a map as EquirectangularMap::Load (is_emap = 1)
 * or PerspectiveMap::Load (0) into out (float, capacity `cap`; dims always written; returns -1
 * on a load failure); write a 16-bit gray PNG as Save16BitPNG; the LeReS layout as 15x4
 * floats each. */
extern "C" int pfd_load_map(const char* fn, int is_emap, float* out, long long cap, int* w,
                            int* h, int* c);
extern "C" int pfd_save_png16(const char* fn, const uint16_t* data, int w, int h);
/* the tile writer of the RGB export: the bytes of stbi_write_jpg(fn, w, h, c, px, quality) with
 * stbi_flip_vertically_on_write(flip) (Main.cpp:319-320), c = 1..4 channels, rows top-first */
extern "C" int pfd_save_jpeg(const char* fn, const uint8_t* px, int w, int h, int c, int quality,
                             int flip);
/* the image decoders behind Load (stbi_load / stbi_load_16 with req_comp 0, Depth.cpp:56-100):
 * native samples (u8, or u16 when *is16) into out (capacity cap bytes); -1 load failure, -2 out
 * too small (dims written either way).  pfd_is_16_bit = stbi_is_16_bit. */
extern "C" int pfd_decode_image(const char* fn, void* out, long long cap, int* w, int* h, int* c,
                                int* is16);
extern "C" int pfd_is_16_bit(const char* fn);
extern "C" void pfd_leres_layout(float* fovs, float* ranges);
/* pf_resolve_layout for bindings: the tiles of a named table or a layout file as 4 floats each
 * into fovs / ranges (capacity `cap` tiles each; either may be NULL to ask for the count only).
 * Returns the tile count, or -1 (unknown name / rejected file, message on stdout; or cap too
 * small). */
extern "C" int pfd_layout(const char* name, float* fovs, float* ranges, int cap);
/* The export's tile size for a window (SaveCubeMap's viewport): w = 1024,
 * h = round(1024 / aspect). */
extern "C" void pfd_rgb_tile_size(const float* fov, int* w, int* h);
