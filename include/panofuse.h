/*
 * panofuse.h -- C-ABI of the MI355X (gfx950) panorama-depth fusion library (libpanofuse.so).
 *
 * Drop-in for the reference's DepthNamespace hot path (Depth.h:286-307 and the OpenGL E->P
 * render of Main.cpp:242-326).  Plain pointers and sizes only; every data pointer is a DEVICE
 * pointer (hipMalloc'd memory or a torch tensor's data_ptr()) owned by the caller, and every
 * call is stream-ordered on the context's stream.  Calls return PF_OK (0) or a negative PF_E*
 * code; pf_last_error() gives the message.  A context is bound to one device and one stream and
 * is not thread-safe: use one context per host thread per device.
 *
 * Batched layout in HBM (row-major, row 0 = zenith 0):
 *   emap  [batch][eh][ew][ec]           fp32 baseline equirectangular depth in [0,1]
 *   tiles [batch][sum_i th_i*tw_i*tc]   fp32 perspective tiles, tile i at offset sum_{j<i}
 *   out   [batch][out_h][out_w]         u16 fused panorama
 *   coeffs[batch][ntiles][4]            fp32 {a,b,c,d} of y = a x^3 + b x^2 + c x + d
 */
#ifndef PANOFUSE_H
#define PANOFUSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_OK 0
#define PF_EINVAL (-1)     /* bad argument, shape or layout */
#define PF_ENOMEM (-2)     /* device allocation failed */
#define PF_EHIP (-3)       /* HIP runtime error */
#define PF_ESTATE (-4)     /* call order (e.g. no tiles set) */
#define PF_EDEGENERATE (-5) /* a tile box with x0 == x1 (the reference loops forever there) */
#define PF_ETIMEOUT (-6)   /* a resident-kernel hand-off wait timed out: the output of that
                            * fusion (or row-band smoothing) is invalid (see pf_jres_errors);
                            * reported by pf_synchronize, and by the next pf_fuse / pf_merge /
                            * pf_solve_smoothing once the timed-out call has finished */

typedef struct pf_ctx pf_ctx;

/* {azimuth_left, azimuth_right, zenith_top, zenith_down} in radians.  As a viewing window
 * this is PerspectiveMap::SetWindow's argument list (Depth.cpp:120); as a valid range it is
 * PerspectiveMap::ranges (Depth.h:82). */
typedef struct pf_window {
    float az_left, az_right, zen_top, zen_down;
} pf_window;

/* Synthetic stand-in for the external depth net (not part of the reference): per tile,
 * d' = clamp01(alpha*d + (kappa*d)*d + beta + sigma*u), u uniform in [-1,1) hashed from
 * (seed, pixel) -- seed unique per (panorama, layout-wide tile) -- as the oracle's pfo_hash32.
 * Used only to manufacture benchmark tiles from a ground-truth pano. */
typedef struct pf_response {
    float alpha, kappa, beta, sigma;
    uint32_t seed, pad;
} pf_response;

int pf_create(int device, pf_ctx** out);
void pf_destroy(pf_ctx* ctx);
const char* pf_last_error(const pf_ctx* ctx);
/* hipStream_t to order all work on (NULL = the null stream). */
int pf_set_stream(pf_ctx* ctx, void* hip_stream);
/* Waits for the context stream.  Returns PF_ETIMEOUT (message in pf_last_error) when a fusion
 * enqueued since the last report had a resident-kernel wait time out, i.e. its u16 output is
 * invalid -- the reference's "return false" on a failed merge (Depth.cpp:767-778). */
int pf_synchronize(pf_ctx* ctx);
const char* pf_version(void);

/* Tile layout.  Replaces PerspectiveMap::SetWindow + ranges (Depth.cpp:780-786).
 * cap_ranges != 0 applies MergeDepthMaps' MIN2(range, D2R(359.9)) to ranges[0..1]
 * (Depth.cpp:783-784).  tile_c = channels per tile pixel (channel 0 is used, as Value() does). */
int pf_set_tiles(pf_ctx* ctx, const pf_window* fovs, const pf_window* ranges, int ntiles,
                 const int* tile_w, const int* tile_h, int tile_c, int cap_ranges);

/* Registration solver for degree 3 (the reference's cubic FunctorDepth2Depth3):
 *   PF_SOLVER_LM (default) -- the reference's Ceres 1.13 Levenberg-Marquardt (DENSE_SCHUR,
 *     default options, from (1,1,1,1); Depth.cpp:1270-1274, 1399-1404), run per tile from the
 *     fp64 moment sums of its samples;
 *   PF_SOLVER_NORMAL -- the exact least-squares minimiser (fp64 normal equations).
 * Lower degrees always take the normal equations (the reference has no lower-degree solve). */
#define PF_SOLVER_NORMAL 0
#define PF_SOLVER_LM 1
int pf_set_solver(pf_ctx* ctx, int solver);

/* Tile-pixel validity rule (an extension: the reference reads every tile pixel as depth).  Real
 * tiles hold NaN / Inf from a depth net, holes and sky masks written as 0, letter-box bars, or
 * pixels a caller masked with NaN; read as depth, one such pixel spoils the whole band.
 *   PF_VALID_ALL (default)  every pixel is read, as the reference does: every entry point
 *                           launches the kernels and returns the bits it always did;
 *   PF_VALID_RANGE          a raw tile value v (channel 0, before any transform) is valid iff
 *                           lo < v && v < hi, compared in fp32; NaN fails both.  Needs lo < hi.
 * lo = -INFINITY, hi = +INFINITY rejects exactly NaN and +-Inf (an arbitrary mask is expressed by
 * writing NaN); lo = 0 also rejects holes written as 0; hi = 1 rejects saturated pixels.
 * Under PF_VALID_RANGE:
 *   pf_register, pf_register_joint, pf_merge's registration: a sample whose raw tile value is
 *     invalid or whose baseline value is not finite is skipped (it adds nothing to the moment
 *     sums).  A problem left with fewer than degree + 1 samples, or whose solution is not finite,
 *     gets four quiet NaNs as coefficients (fp32 and fp64).  apply != 0 transforms the valid
 *     pixels and writes NaN into the invalid ones, which so stay invalid under any later lo / hi.
 *   pf_fuse, pf_merge, pf_fuse_targets, pf_fuse_check (and pf_fuse_level on their targets): tile
 *     p contributes to a pixel of a panorama iff all five taps of its stencil are valid -- the
 *     raw value passes the rule and, with coeffs, the transformed value is finite, so a tile with
 *     NaN coefficients drops out.  The covering tiles are counted per pixel and panorama; a pixel
 *     left with none is un-windowed: it keeps its seed / upsampled value and is a boundary for
 *     its neighbours.  Coverage then depends on the data, so the levels run the marker-reading
 *     Jacobi passes, not the packed form or the resident kernel.  The baseline emap
 *     must be finite where the fusion seeds from it: documented, not checked.
 *   pf_stitch: a pixel takes the first tile whose box holds it and whose sampled value is valid
 *     (as a tap above); 0 if there is none.
 *   They return PF_ESTATE, never silently ignoring the rule: pf_register_disparity,
 *     pf_merge_disparity, pf_solve_smoothing, and the sharded pieces that derive coverage from the
 *     layout alone: pf_fuse_partial, pf_fuse_partial_rows, pf_fuse_coverage_rows,
 *     pf_fuse_multicover, pf_fuse_multicover_patch. */
#define PF_VALID_ALL 0
#define PF_VALID_RANGE 1
int pf_set_tile_validity(pf_ctx* ctx, int mode, float lo, float hi);

/* Valid counts under the context's rule: counts [batch][ntiles][2] (DEVICE, long long) =
 * {registration samples pf_register keeps, valid pixels} per panorama and tile; with
 * PF_VALID_ALL the totals.  Stream-ordered. */
int pf_tile_valid_counts(pf_ctx* ctx, const float* tiles, const float* emap, int ew, int eh,
                         int ec, int batch, float zr0, float zr1, long long* counts);

/* SolveDepthToDepth (Depth.cpp:1261-1414) for every tile with only that tile active
 * (MergeDepthMaps' loop, Depth.cpp:794-805), fp64 least squares of degree `degree`
 * (3 = the reference's FunctorDepth2Depth3, with the context's solver; 1 = scale/shift);
 * coeffs may be NULL.  coeffs64 (optional, [batch][ntiles][4] doubles) receives the unrounded
 * solution.  apply != 0 then runs Depth2DepthTransform (Depth.cpp:245-274) on the tiles. */
int pf_register(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, float* tiles,
                int batch, float zr0, float zr1, int degree, int apply, float* coeffs,
                double* coeffs64);

/* SolveDepthToDepth with several active maps (Depth.cpp:1261-1414: the sample grids of every
 * active tile in one least-squares problem): active is a HOST int[ntiles] mask; coeffs
 * ([batch][4] floats) / coeffs64 ([batch][4] doubles) are device pointers (either may be NULL). */
int pf_register_joint(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, const float* tiles,
                      int batch, float zr0, float zr1, int degree, const int* active,
                      float* coeffs, double* coeffs64);

/* SolveDepthAll (Depth.cpp:1416-1771): multi-level Laplacian-target scatter + damped Jacobi,
 * u16 output.  coeffs (optional, from pf_register with apply = 0) fuses Depth2DepthTransform
 * into the tile gather instead of rewriting the tiles. */
int pf_fuse(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, const float* tiles,
            const float* coeffs, int batch, int out_w, int out_h, float zr0, float zr1,
            uint16_t* out);

/* MergeDepthMaps core (Depth.cpp:789-913) without file I/O: pf_register (degree 3) then
 * pf_fuse with the transform fused.  Tiles are left untouched; coeffs (optional) receives the
 * per-tile abcd. */
int pf_merge(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, const float* tiles,
             int batch, int out_w, float zr0, float zr1, float* coeffs, uint16_t* out);

/* Disparity tiles (MiDaS / DPT: relative inverse depth in 0-1).  The reference declares
 * SolveDisparityToDepth (Depth.h:293-294) without defining it; this is its model
 * (FunctorDisparity2Depth, Depth.cpp:1044-1073: y = 1/(a x + b) + d, weight 1) fitted on
 * SolveDepthToDepth's samples by the same Ceres 1.13 Levenberg-Marquardt (DENSE_SCHUR, default
 * options, from (1,1,1)), every tile alone as in MergeDepthMaps' loop.  fp64 throughout, in a
 * fixed summation order, so the result is reproducible bit for bit.
 *   coeffs   (optional) [batch][ntiles][4] floats  abcd = (a, b, 1, d), the order D2DTransform reads
 *   coeffs64 (optional) [batch][ntiles][4] doubles the unrounded solution
 *   summary  (optional) [batch][ntiles][4] doubles {initial cost, final cost, iterations,
 *            termination: 0 no convergence, 1 function, 2 parameter, 3 gradient tolerance,
 *            4 minimum radius, 5 failure}
 * apply != 0 then runs D2DTransform (Depth.cpp:214-243) on the tiles. */
int pf_register_disparity(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, float* tiles,
                          int batch, float zr0, float zr1, int apply, float* coeffs,
                          double* coeffs64, double* summary);

/* PerspectiveMap::D2DTransform (Depth.cpp:214-243) on device data, in place: channel 0 of npix
 * pixels becomes clamp01(c / (a * clampX + b) + d) in fp32, NaN kept; abcd: 4 HOST floats. */
int pf_disparity_transform(pf_ctx* ctx, float* data, long long npix, int channels,
                           const float* abcd);

/* MergeDepthMaps' compute core for disparity tiles (an extension: the reference has no such
 * driver): pf_register_disparity, D2DTransform into a context-owned copy of the tiles, then
 * pf_fuse on that copy without coefficients.  The caller's tiles are left untouched; coeffs
 * (optional) receives the per-tile abcd. */
int pf_merge_disparity(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, const float* tiles,
                       int batch, int out_w, float zr0, float zr1, float* coeffs, uint16_t* out);

/* ---- robust registration (an extension: the reference passes NULL as the loss at both call
 * sites, Depth.cpp:1232, 1393; a user of it writes new ceres::HuberLoss(a) there) ----
 *
 * The per-tile fits above are unweighted least squares, and one gross outlier (a depth edge, glass,
 * sky, a mirror: finite, in range and wrong, so no validity rule removes it) bends the cubic.
 * With a loss set, the tile registrations minimise sum 0.5 rho(r^2) by the same Ceres 1.13
 * Levenberg-Marquardt, with Ceres' loss semantics (s = r^2 of the unscaled residual, b = a a):
 *   PF_LOSS_HUBER  (loss_function.h:177, loss_function.cc:47-61)
 *     s > b:  rho = 2 a sqrt(s) - b, rho' = max(DBL_MIN, a / sqrt(s));  else rho = s, rho' = 1
 *   PF_LOSS_SOFTL1 (loss_function.h:193, loss_function.cc:63-70), c = 1 / b, t = sqrt(1 + s c)
 *     rho = 2 b (t - 1), rho' = max(DBL_MIN, 1 / t)
 * rho'' <= 0 for both, so Corrector (corrector.cc:81-85) scales the residual and the Jacobian row
 * by sqrt(rho') and nothing else; the cost term is 0.5 rho (residual_block.cc:164-166).  The
 * gradient, J'J, the Jacobi scaling, the model cost change and every tolerance are formed from
 * the corrected quantities.  A loss cannot be carried by the 15 moment sums of the cubic, so the
 * cubic runs sample-wise (k_register_robust, csrc/pf_robust.hip) in the fixed summation order of
 * the disparity fit: reproducible bit for bit.  CauchyLoss, ArctanLoss, TolerantLoss
 * and the others need log, atan2 or exp in fp64, whose device and glibc versions are not the same
 * bits: out of scope.
 *
 * a must be finite and > 0 for a loss (PF_EINVAL otherwise) and is ignored for PF_LOSS_NONE.
 * With PF_LOSS_NONE (the default, also after a loss was set and unset) every entry point launches
 * the kernels and returns the bits it always did.  With a loss set:
 *   pf_register, pf_register_ex, pf_merge   run the sample-wise kernel; they need degree == 3 and
 *     PF_SOLVER_LM (PF_EINVAL otherwise).  The start is (1,1,1,1).  apply and the transform fused
 *     into the fusion are unchanged.  Under PF_VALID_RANGE a sample whose raw tile value fails the
 *     rule or whose baseline value is not finite is skipped; a problem left with fewer than 4
 *     samples, or with a non-finite solution, gets four quiet NaNs and termination 5.
 *   pf_register_disparity, pf_merge_disparity   fit their model under the loss; the summary of
 *     pf_register_disparity then has the 6 entries of pf_register_ex's.
 *   pf_register_joint, pf_register_global   return PF_ESTATE: the robust joint and global solves
 *     are out of scope. */
#define PF_LOSS_NONE 0 /* default */
#define PF_LOSS_HUBER 1
#define PF_LOSS_SOFTL1 2
int pf_set_register_loss(pf_ctx* ctx, int kind, double a);

/* pf_register with a per-tile solver summary (optional, DEVICE, [batch][ntiles][6] doubles):
 * {initial cost, final cost, iterations, termination as pf_register_disparity's, samples used,
 * inliers = samples with r^2 <= a^2 at the returned coefficients}.  summary is allowed only while
 * a loss is set (PF_EINVAL otherwise); with summary == NULL this is pf_register. */
int pf_register_ex(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, float* tiles,
                   int batch, float zr0, float zr1, int degree, int apply, float* coeffs,
                   double* coeffs64, double* summary);

/* ---- planar-depth tiles (an extension: the reference reads every tile value as ray distance) ----
 *
 * Perspective depth networks (LeReS, MiDaS / DPT, ZoeDepth, ...) predict planar depth: distance
 * along the optical axis.  The baseline panorama and the fused result hold ray distance: distance
 * from the camera centre.  On SetWindow's plane at unit distance (Depth.cpp:120-155) tile pixel
 * (x, y) sits at pos = corner0 + x hedge + y vedge, and the two differ by the factor
 *   k = |pos| = sqrt(1 + (tx (1 - 2x))^2 + (ty (2y - 1))^2),  tx = tan(daz / 2), ty = tan(dzen / 2),
 * which depends on the pixel's position, so no per-tile function of the value can carry it.
 *
 * pf_set_tiles builds, per tile, cu[i] = (tx (1 - 2 i / (w-1)))^2 and rv[j] = (ty (2 j / (h-1) - 1))^2
 * in fp64 from the fp32 window (pixel i is x = i / (w-1), the inverse of Value()'s truncating
 * index).  The factor has one definition: kf(i, j) = (float)sqrt(1.0 + cu[i] + rv[j]), the adds and
 * the sqrt in fp64, rounded once to fp32; the registrations use K = (double)kf.
 *
 * Under PF_TILE_DEPTH_PLANAR:
 *   pf_register, pf_register_ex, pf_register_disparity   fit K T(x) to the baseline, T the per-tile
 *     cubic or 1/(a x + b) + d: the residual is K m - y and the Jacobian row is K times the plain
 *     one, in the plain fits' summation order, for every combination of solver, degree, validity
 *     rule and loss that runs in ray mode.  apply != 0 writes clamp01(kf * T32(x)): T32 is the fp32
 *     value of Depth2DepthTransform / D2DTransform before its final clamp, then one fp32 multiply,
 *     then the clamp; NaN stays NaN and, under the validity rule, an invalid pixel becomes NaN.
 *   pf_merge, pf_merge_disparity   register, apply into a context-owned copy of the tiles and fuse
 *     that copy without coefficients; the caller's tiles are untouched and coeffs receives the
 *     planar fit.  Under the validity rule the copy is fused under (-inf, +inf): its invalid
 *     pixels are the NaNs apply wrote, and a value clamped to 0 or 1 is valid.
 *   The fused-transform gathers have no factor: pf_fuse, pf_fuse_targets, pf_fuse_check, pf_stitch,
 *     pf_solve_smoothing, pf_fuse_partial, pf_fuse_partial_rows and pf_fuse_multicover return
 *     PF_ESTATE when coeffs != NULL, and run as ever with coeffs == NULL (the tiles are then ray
 *     distance already).  pf_register_joint returns PF_ESTATE.  Everything else is unaffected.
 * With PF_TILE_DEPTH_RAY (the default, also after PLANAR was set and unset) every entry point
 * launches the kernels and returns the bits it always did. */
#define PF_TILE_DEPTH_RAY 0     /* default: tiles hold ray distance, as the reference assumes */
#define PF_TILE_DEPTH_PLANAR 1  /* tiles hold depth along the optical axis */
int pf_set_tile_depth(pf_ctx* ctx, int kind);          /* unknown kind: PF_EINVAL */
/* The tables of one tile of the stored layout: HOST out, cu[tile_w], rv[tile_h]. */
int pf_tile_ray_tables(pf_ctx* ctx, int tile, double* cu, double* rv);
/* kf of every tile pixel: DEVICE out, one float per tile pixel (no channels), tiles in layout
 * order, rows top-first.  Works in either mode.  Stream-ordered. */
int pf_tile_ray_factor(pf_ctx* ctx, float* k);

/* ---- overlap-consistent registration (an extension: the reference registers every tile to the
 * baseline on its own, Depth.cpp:794-805, and neighbouring tiles never meet) ----
 *
 * Two neighbours can each fit the blurry baseline well and still disagree where they overlap; the
 * stitch shows that as seams, and the fusion can only average the conflicting targets.  The cubic
 * is linear in its coefficients, so "fit the baseline and agree with your neighbours" is one linear
 * least-squares problem per panorama in 4 ntiles unknowns, c_p the cubic of tile p:
 *   E(c) = sum_p sum_{s in S_p} (u_s.c_p - y_s)^2
 *        + lambda sum_{(p,q)} sum_{s in O_pq} (u_s.c_p - v_s.c_q)^2
 * S_p: the registration samples of tile p exactly as pf_register reads them, u = (X^3, X^2, X, 1),
 * X and y clamped to [1e-4, 1 - 1e-4] in fp64.  O_pq, for an ordered pair p != q: the samples of
 * S_p whose grid direction, projected into tile q by SphericalTo2D with the tabulated trig values of
 * tile p's grid, has dir.middle > 0 and 0 <= x <= 1 and 0 <= y <= 1 in fp32, with no clamping;
 * v is the same row of tile q's value at Value(x, y).  The pairs with |O_pq| > 0 are listed in
 * ascending (p, q).
 *
 * The overlap table depends on the layout, the tile sizes and the zenith range only; it is built on
 * the first call that needs it (two deterministic passes: count, then fill in sample order) and
 * cached until pf_set_tiles or another zenith range replaces the registration grids.
 *   pf_overlap_pairs  HOST counts: the pairs and the pair samples of all pairs together.
 *   pf_overlap_table  DEVICE copies: pairs [npairs][4] ints {p, q, first, count} and index
 *                     [nsamples][2] ints {element in tile p, element in tile q} (offsets inside the
 *                     tile, channel 0), pair after pair, each in ascending sample order of p.
 *   pf_overlap_stats  stats [batch][npairs][5] doubles {count, sum d, sum d^2, max |d|, samples
 *                     left out because a side is NaN}, d = (double)T32_p - (double)T32_q with T32
 *                     Depth2DepthTransform's fp32 value under coeffs ([batch][ntiles][4] floats),
 *                     or the raw tile values with coeffs == NULL.
 *   pf_register_consistent  the minimiser of E: the 15 moment sums of pf_register per tile, 36
 *     moment sums per pair (u u', v v', u v'), the normal equations assembled in a fixed order and
 *     solved by an in-place right-looking Cholesky factorisation with column-oriented substitutions,
 *     one workgroup per panorama, all in fp64 + - * / sqrt in a fixed order:
 *     reproducible bit for bit.  lambda must be finite and >= 0 (PF_EINVAL otherwise); lambda = 0 is
 *     the exact per-tile least squares (PF_SOLVER_NORMAL's minimiser by another elimination).
 *       coeffs   (optional) [batch][ntiles][4] floats, coeffs64 (optional) the unrounded doubles
 *       summary  (optional) [batch][4] doubles {data cost, pair cost, pair samples, status}: the
 *                first sum of E and the second without its factor lambda, both at the returned
 *                fp64 coefficients, evaluated from the moment sums; status 1: a pivot was not > 0
 *                or the solution is not finite -- every coefficient of that panorama is a quiet
 *                NaN, as are the two costs; other panoramas of the batch are unaffected.
 *     apply != 0 then runs Depth2DepthTransform on the tiles, as pf_register's.
 * All four return PF_ESTATE while the validity rule (pf_set_tile_validity), a loss
 * (pf_set_register_loss) or PF_TILE_DEPTH_PLANAR (pf_set_tile_depth) is on: their consistent forms
 * are out of scope and the modes are never silently ignored.  No existing entry point changes. */
int pf_overlap_pairs(pf_ctx* ctx, float zr0, float zr1, int* npairs, long long* nsamples);
int pf_overlap_table(pf_ctx* ctx, float zr0, float zr1, int* pairs, int* index);
int pf_overlap_stats(pf_ctx* ctx, const float* tiles, const float* coeffs, int batch, float zr0,
                     float zr1, double* stats);
int pf_register_consistent(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, float* tiles,
                           int batch, float zr0, float zr1, double lambda, int apply,
                           float* coeffs, double* coeffs64, double* summary);

/* ---- per-pixel tile weights ----------------------------------------------------------------------
 *
 * An extension: a confidence per tile pixel (a network's uncertainty map, a border falloff, a
 * segmentation mask per panorama) for the registration and the fusion.  The reference carries the
 * hook and never uses it: every registration functor multiplies its residual by a Weight
 * (Depth.cpp:1044-1150) and the only call site passes 1.0f (Depth.cpp:1366-1375).
 *
 * weights   DEVICE floats in the tiles' own element layout (tile p at its offset, the same strides,
 *           any channel count); only the channel-0 element of a pixel is read.  wbatch == 1: one
 *           set of tile_elems floats for the whole batch; wbatch == batch: one set per panorama;
 *           anything else, or NULL, is PF_EINVAL.
 * usable    u(w) = w if 0 < w && w < +inf in fp32, else 0: NaN, negatives and zero mean "not here".
 *
 * Weights in {0, 1} are the validity rule (pf_set_tile_validity): with NaN written under the zeros
 * the three calls equal their counterparts under the rule (-inf, +inf) bit for bit, and with every
 * weight 1.0f they equal pf_register / pf_fuse / pf_merge bit for bit.
 *
 *   pf_tile_tent_weights  fills one set (tile_elems floats, 0 in the non-zero channels) with the
 *     blending tent in tile pixel space: for a w x h tile at pixel (x, y), t = min(min(x + 1, w - x),
 *     min(y + 1, h - y)), m = (min(w, h) + 1) / 2 in integers, weight = (float)min(t, m) / (float)m.
 *   pf_register_weighted  weighted least squares, degree 3, by the reference's LM from the moment
 *     sums (PF_SOLVER_LM only: PF_EINVAL otherwise).  A sample is used iff u(w) > 0 at its tile
 *     element, its raw tile value is finite and its baseline value is finite; a used sample adds
 *     (double)w times each of pf_register's 15 terms, in pf_register's order.  This is
 *     Weight = sqrt(w) in the reference's FunctorDepth2Depth3.  Fewer than 4 used samples, or a
 *     non-finite solution: four quiet NaNs.
 *       summary  (optional) [batch][ntiles][2] doubles {used samples, sum of w}
 *     apply != 0 then runs Depth2DepthTransform on the tiles, as pf_register's.
 *   pf_fuse_weighted  SolveDepthAll with weighted Laplacian targets.  A tap counts iff u(w) > 0 and
 *     its (transformed, if coeffs) value is finite; tile p contributes to a pixel iff all five taps
 *     of its stencil count, with wmin = the smallest of their five weights; the target is
 *     sum(wmin * Lp) * (1 / sum(wmin)) over the contributing tiles in index order (fp32, separate
 *     multiply and add), and a pixel without a contributing tile has no target, as an uncovered
 *     one.  Coverage then depends on the data, so the Jacobi levels take their general passes.
 *   pf_merge_weighted  pf_register_weighted (no apply) + pf_fuse_weighted with its coefficients.
 *
 * All four return PF_ESTATE while the validity rule (pf_set_tile_validity), a loss
 * (pf_set_register_loss) or PF_TILE_DEPTH_PLANAR (pf_set_tile_depth) is on.  Disparity tiles have
 * their own weighted forms (below).  Smoothing, stitch, the joint, consistent and global
 * registrations and the sharded fusion have no weighted form.  Layouts of more than 2^30 tile
 * elements per panorama are PF_EINVAL in the two fusing calls.  No existing entry point changes. */
int pf_tile_tent_weights(pf_ctx* ctx, float* weights);
int pf_register_weighted(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, float* tiles,
                         const float* weights, int wbatch, int batch, float zr0, float zr1,
                         int apply, float* coeffs, double* coeffs64, double* summary);
int pf_fuse_weighted(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, const float* tiles,
                     const float* weights, int wbatch, const float* coeffs, int batch, int out_w,
                     int out_h, float zr0, float zr1, uint16_t* out);
int pf_merge_weighted(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, const float* tiles,
                      const float* weights, int wbatch, int batch, int out_w, float zr0,
                      float zr1, float* coeffs, uint16_t* out);

/* ---- per-pixel weights for disparity tiles ------------------------------------------------------
 *
 * The weighted forms of pf_register_disparity / pf_merge_disparity: weights, wbatch and u(w) as
 * above.  A network writes sky as disparity ~ 0, which the fit clamps to 1e-4 and which then bends
 * y = 1/(a x + b) + d for the whole tile; weights say "this pixel does not count".
 *
 *   pf_tile_range_weights  the validity rule written as a weight set per panorama: weights
 *     (DEVICE output, [batch][tile_elems] floats) gets 1.0f at the channel-0 element of a pixel
 *     whose raw value has lo < v && v < hi in fp32 (NaN fails), 0.0f everywhere else, the other
 *     channels included.  Stream-ordered; refuses nothing but bad arguments.
 *   pf_register_disparity_weighted  pf_register_disparity's fit (same samples, clamps, start
 *     (1, 1, 1) and LM) as weighted least squares.  A sample is used iff u(w) > 0 at its tile
 *     element, its raw tile value is finite and its baseline value is finite; a used sample adds
 *     W = (double)u(w) times each of the ten terms of a Jacobian evaluation (W * (0.5 * (r * r)) in
 *     a trial), multiply and add apart in fp64; any other sample adds nothing.  Lane l of 256 owns
 *     samples l, l + 256, ... used or not, then pf_register_disparity's halving tree, so with every
 *     weight 1.0f and finite data coeffs, coeffs64 and the first four summary entries are
 *     pf_register_disparity's bit for bit.  Fewer than 3 used samples (no fit is run: both costs
 *     are NaN, 0 iterations), or a solution that is not finite: four quiet NaNs in coeffs and
 *     coeffs64 and termination 5.
 *       summary  (optional) [batch][ntiles][6] doubles {initial cost, final cost, iterations,
 *                termination, used samples, sum of W (fp64, the same lane order and tree)}
 *     apply != 0 then runs D2DTransform on every pixel of the tiles, as pf_register_disparity's.
 *   pf_merge_disparity_weighted  copies the tiles into a context-owned buffer, runs the call above
 *     with apply on the copy and fuses the copy as pf_fuse_weighted does with coeffs == NULL and
 *     the same weights.  The caller's tiles stay untouched; a tile left with NaN coefficients
 *     transforms to NaN and drops out of every pixel.
 *
 * Under PF_TILE_DEPTH_PLANAR (pf_set_tile_depth) the terms are the planar fit's, K (q + d) with the
 * sample's ray factor K, times W, and apply composes D2DTransform with the ray factor.  The
 * validity rule (pf_set_tile_validity) or a loss (pf_set_register_loss) is PF_ESTATE in the two
 * fitting calls, checked before anything else; NULL weights, a wbatch that is neither 1 nor batch
 * and, for the merge, more than 2^30 tile elements are PF_EINVAL. */
int pf_tile_range_weights(pf_ctx* ctx, const float* tiles, int batch, float lo, float hi,
                          float* weights);
int pf_register_disparity_weighted(pf_ctx* ctx, const float* emap, int ew, int eh, int ec,
                                   float* tiles, const float* weights, int wbatch, int batch,
                                   float zr0, float zr1, int apply, float* coeffs,
                                   double* coeffs64, double* summary);
int pf_merge_disparity_weighted(pf_ctx* ctx, const float* emap, int ew, int eh, int ec,
                                const float* tiles, const float* weights, int wbatch, int batch,
                                int out_w, float zr0, float zr1, float* coeffs, uint16_t* out);

/* ---- post-fusion calibration (no tile layout needed; all pointers are device pointers) ----
 *
 * SolveDepthToDepth2 (Depth.cpp:1158-1259): one cubic per panorama from the fused u16 result
 * data [batch][out_h][out_w] to the baseline emap [batch][eh][ew][ec] (channel 0), on every pixel
 * of rows h0..h1 (the band of pf_level_info's last level): x = (float)data / 65535.0f,
 * y = ValueAtCoord of the pixel's spherical coordinate, both clamped to [1e-4, 1 - 1e-4] in fp64.
 * The reference's Ceres 1.13 Levenberg-Marquardt (DENSE_SCHUR, default options) from (0, 0, 1, 0),
 * evaluated from 15 fp64 moment sums taken in a fixed order (chunks of 16,384 samples),
 * so the result is reproducible bit for bit.  The rows must exist (h1 <= out_h - 1).
 *   coeffs   (optional) [batch][4] floats   abcd = Vec4f(vars) (Depth.cpp:1251)
 *   coeffs64 (optional) [batch][4] doubles  the unrounded solution
 *   summary  (optional) [batch][4] doubles  as pf_register_disparity's
 * apply != 0 then runs pf_result_transform with the fitted coefficients. */
int pf_register_global(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, uint16_t* data,
                       int batch, int out_w, int out_h, float zr0, float zr1, int apply,
                       float* coeffs, double* coeffs64, double* summary);

/* The cubic on the u16 result, in place (an extension: the reference fits abcd with
 * SolveDepthToDepth2 and leaves the use to the caller).  Rows h0..h1 only: v = (float)d / 65535.0f,
 * Depth2DepthTransform's map (Depth.cpp:256-271) in fp32, NaN becomes 0, d = (u16)(Y * 65535.0f).
 * coeffs: DEVICE [batch][4] floats. */
int pf_result_transform(pf_ctx* ctx, uint16_t* data, int batch, int out_w, int out_h, float zr0,
                        float zr1, const float* coeffs);

/* MedianScaling (Depth.cpp:637-701): channel 0 of map0 [batch][h0][w0][c0] is scaled by
 * m1 / m0 (fp32) on its valid pixels, where m0 / m1 are the order statistics at index n / 2 of
 * the valid values of map0 / map1 (an exact selection: what nth_element leaves there), valid
 * meaning !(v < 1e-4 || v >= 1 - 1e-4) in double; NaN counts as invalid.
 *   medians (optional) [batch][2] floats {m0, m1}
 *   status  (optional) [batch] ints: 0 ok; 1 a map has no valid pixel (the reference indexes an
 *           empty vector there): medians 0, nothing written */
int pf_median_scale(pf_ctx* ctx, float* map0, int w0, int h0, int c0, const float* map1, int w1,
                    int h1, int c1, int batch, float* medians, int* status);

/* EquirectangularMap::CopyInvalidPixels (Depth.cpp:703-725): for every pixel (x, y) of dst
 * [batch][h][w][c], channel 0 of ref [batch][rh][rw][rc] at X = int((float)x * ((float)rw /
 * (float)w)), Y likewise, is copied into channel 0 of dst where it is < 1e-4 or >= 1 - 1e-4
 * (NaN is not copied).  X / Y are clamped to the last column / row. */
int pf_copy_invalid(pf_ctx* ctx, float* dst, int w, int h, int c, const float* ref, int rw,
                    int rh, int rc, int batch);

/* E->P depth warp: tile pixel (X,Y) -> ToSphericalCoord(X/(W-1), Y/(H-1)) (Depth.cpp:157-166)
 * -> bilinear sample of pano [batch][ph][pw] at (az/2pi*(pw-1), zen/pi*(ph-1)).  resp
 * ([batch][ntiles], optional) applies the synthetic depth-net response. */
int pf_warp_depth(pf_ctx* ctx, const float* pano, int pw, int ph, int batch,
                  const pf_response* resp, float* tiles);

/* E->P RGB warp (Main.cpp:242-326 SaveCubeMap + SphereMesh.cpp:154-210 texture mapping):
 * u8 RGB pano [batch][ph][pw][3] -> tiles [batch][sum_i th_i*tw_i*3], GL camera conventions,
 * GL_LINEAR + GL_REPEAT, rows top-first. */
int pf_warp_rgb(pf_ctx* ctx, const uint8_t* pano, int pw, int ph, int batch, uint8_t* tiles);

/* SolveDepthBySmoothing (Depth.cpp:1773-1878; Depth.h:309), the reference's alternate solver
 * (not called by mode 0): every tile written into the out_w x out_h grid (a later tile
 * overwrites an earlier one), 500 in-place Gauss-Seidel smoothing iterations on the pixels within
 * 10 of a tile-box edge in rows [floor(h*zr0/MYPI), ceil(h*zr1/MYPI)], u16 quantisation.
 * tiles: [batch][tile_elems] float (channel 0 read); coeffs: NULL, or [batch][ntiles][4] applied
 * as Depth2DepthTransform on the fly; out: [batch][out_h][out_w] u16.  Bit-exact.  The
 * row-band form's hand-off waits are bounded: a timeout makes the output invalid and is reported
 * as PF_ETIMEOUT by pf_synchronize (or the next call), as for the fusions. */
int pf_solve_smoothing(pf_ctx* ctx, const float* tiles, const float* coeffs, int batch,
                       int out_w, int out_h, float zr0, float zr1, uint16_t* out);

/* The direct tile stitch (Depth.cpp:817-865, `if (false)` in the reference): the "no blending"
 * baseline.  Every pixel of every row takes the value of the FIRST tile (ascending order) whose
 * range box contains it -- x0 = round(r0 / (2 MYPI) * (W-1)), x1, y0, y1 likewise in double from
 * the ranges as pf_set_tiles stored them; inside when min(x0,x1) <= x <= max(x0,x1) and
 * y0 <= y <= y1, both ends inclusive, no zenith band -- read at SphericalTo2D of the fusion
 * grid's (az, zen) through Value's truncated index (an index that leaves the tile is clamped;
 * the reference reads out of bounds there).  A pixel under no tile is 0.  Quantisation as the
 * fusion's: clamp to [0, 1], (u16)(v * 65535.0f), NaN -> 0.
 * tiles: [batch][tile_elems] float (channel 0 read); coeffs: NULL, or [batch][ntiles][4] applied
 * as Depth2DepthTransform on the fly; out: [batch][out_h][out_w] u16.  Bit-exact. */
int pf_stitch(pf_ctx* ctx, const float* tiles, const float* coeffs, int batch, int out_w,
              int out_h, uint16_t* out);

/* The Laplacian self-check of SolveDepthAll (Depth.cpp:1738-1758, `if (false)` in the
 * reference) on given planes: for y = h0+1 .. h1-1, x = 1 .. w-2 in row-major order, from
 * err = 0.0f,  Lcur = val - (((left + right) + up) + down) / 4.0f,  d = Lcur - L  (fp32),
 * err = (float)((double)err + (double)d * (double)d)  -- the reference's float chain, bit for
 * bit.  L is the pixel's normalised target, 0 where lnorm carries the un-windowed marker.
 *   buf   [batch][h][w] float   a level's plane after its sweeps
 *   lnorm [batch][h][w] float   the targets as pf_fuse_targets writes them
 *   err   [batch] float, device
 * PF_EINVAL unless 0 <= h0, h0 + 2 <= h1 <= h - 1 and w >= 3.  Needs no tile layout. */
int pf_laplacian_residual(pf_ctx* ctx, const float* buf, const float* lnorm, int w, int h, int h0,
                          int h1, int batch, float* err);

/* The fusion of one panorama (pf_fuse with batch 1) with the self-check after every level: per
 * level pf_fuse_targets, pf_fuse_level and pf_laplacian_residual on that level's plane and
 * targets.  err: [nlevels] float, device; err[nlevels - 1] is the number the reference prints as
 * "[SolveDepthAll] check Laplacian err:", the coarser levels' are the same formula on their own
 * targets (an extension).  out (optional): [out_h][out_w] u16, equal to pf_fuse's bit for bit. */
int pf_fuse_check(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, const float* tiles,
                  const float* coeffs, int out_w, int out_h, float zr0, float zr1, float* err,
                  uint16_t* out);

/* ---- multi-GPU fusion of one panorama (tiles sharded over ranks) ----
 * pf_fuse_partial scatters the Laplacian targets of tiles [t0, t1) for level `level` into
 * lsum/cnt ([out levels h][w] fp32 and fp32 counts); the caller sums them over ranks
 * (RCCL reduce), then pf_fuse_finish_level runs normalisation + Jacobi on the summed grids. */
int pf_level_info(int out_w, int out_h, float zr0, float zr1, int level, int* w, int* h,
                  int* h0, int* h1, int* iters, int* nlevels);
int pf_fuse_partial(pf_ctx* ctx, const float* tiles, const float* coeffs, int t0, int t1,
                    int out_w, int out_h, float zr0, float zr1, int level, float* lsum,
                    float* cnt);
/* buf: the level's buffer (in: seed/upsampled values, out: after the sweeps).  When
 * level == nlevels-1, out (if not NULL) receives the u16 quantisation. */
int pf_fuse_seed(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, const float* prev,
                 int out_w, int out_h, float zr0, float zr1, int level, float* buf);
int pf_fuse_finish_level(pf_ctx* ctx, const float* lsum, const float* cnt, int out_w,
                         int out_h, float zr0, float zr1, int level, float* buf,
                         uint16_t* out);
/* pf_fuse_seed + pf_fuse_finish_level in one: the level is seeded (level 0 from emap, else
 * the 2x upsample of prev, the previous level's plane) inside its first sweep pass, as
 * pf_merge does it, with no seeded plane and no full-plane copies.  buf receives the level
 * (every row), except on the last level with out != NULL, where only out is written.  cnt ==
 * NULL: lsum holds the normalised targets (pf_fuse_targets).  The replicated levels of the
 * row-sharded C5 flow (pf_dist.fuse_row_sharded).  Round 5. */
int pf_fuse_level(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, const float* prev,
                  const float* lsum, const float* cnt, int out_w, int out_h, float zr0,
                  float zr1, int level, float* buf, uint16_t* out);
/* One level's normalised targets (every tile, one panorama; [h_l][w_l] fp32, the band rows
 * written) -- what pf_fuse_level takes as lsum with cnt == NULL, when no partial sums need to
 * travel (the one-rank row-sharded fusion).  Round 5. */
int pf_fuse_targets(pf_ctx* ctx, const float* tiles, const float* coeffs, int out_w, int out_h,
                    float zr0, float zr1, int level, float* lnorm);
/* Exactness of the summed grids.  Per pixel the reference adds the covering tiles' Laplacians
 * one at a time (Depth.cpp:1609-1617); summing per-rank partials reproduces that for pixels
 * covered by at most two tiles, not for the few covered by three or more (sector corners on
 * shared band rows: 7 pixels per level in the C5 layout).  pf_fuse_multicover lists their
 * (pixel, tile) pairs (count in *npairs; contrib == NULL: count only) and writes contrib[i] =
 * the contribution of pair i's tile if it lies in [t0, t1), else 0; summing contrib over ranks
 * (exact: one non-zero per pair) and pf_fuse_multicover_patch then rewrites those pixels of
 * the summed lsum in the reference's single-thread order (tiles ascending). */
int pf_fuse_multicover(pf_ctx* ctx, const float* tiles, const float* coeffs, int t0, int t1,
                       int out_w, int out_h, float zr0, float zr1, int level, float* contrib,
                       int* npairs);
int pf_fuse_multicover_patch(pf_ctx* ctx, int out_w, int out_h, float zr0, float zr1, int level,
                             const float* contrib, float* lsum);

/* ---- row-band sharding of one level's Jacobi over ranks (pf_dist.py) ----
 * Every rank holds full-size level buffers but owns the rows [row0, row1) of the band [h0, h1].
 * pf_fuse_normalize: the normalised targets of (summed) pf_fuse_partial grids.
 * pf_fuse_border: the rows outside [h0, h1] (0 at level 0, else the nearest upsample of prev)
 *   into both ping-pong buffers a and b, or into the u16 out on the last level (and then, if
 *   a / b are given, their rows h0-1 and h1+1, which the passes' halo lanes read).
 * pf_fuse_band_plan: the sweep depths T[0..n) of the level's passes (returns n), a function of
 *   (level, nbands) only, so every rank derives the same plan.  A level whose zenith band
 *   touches rows 1 / h-2, or whose width is odd or too narrow for a strip, has no band passes
 *   (the one-call path sweeps it launch by launch): PF_EINVAL, naming the reason.  T == NULL with
 *   cap == 0 asks for the count alone and returns 0 for such a level, with no error -- a
 *   sharded flow replicates it (pf_fuse_level) instead of sweeping it in bands.
 * pf_fuse_band_pass: one pass of depth T over rows [row0, row1): reads rows row0-T-1 .. row1+T
 *   of src (src_mode 0), or of the upsample of prev (1) or the emap seed (2, level 0) for the
 *   first pass; writes rows [row0, row1) of dst, or of the u16 out (when out != NULL: the last
 *   pass of the last level).  Between passes the caller refreshes the T+1 halo rows on each side
 *   from the neighbouring bands. */
int pf_fuse_normalize(pf_ctx* ctx, const float* lsum, const float* cnt, int out_w, int out_h,
                      float zr0, float zr1, int level, float* lnorm);
int pf_fuse_border(pf_ctx* ctx, const float* prev, int out_w, int out_h, float zr0, float zr1,
                   int level, float* a, float* b, uint16_t* out);
int pf_fuse_band_plan(pf_ctx* ctx, int out_w, int out_h, float zr0, float zr1, int level,
                      int nbands, int* T, int cap);
int pf_fuse_band_pass(pf_ctx* ctx, const float* emap, int ew, int eh, int ec, const float* prev,
                      const float* lnorm, int src_mode, const float* src, float* dst,
                      uint16_t* out, int out_w, int out_h, float zr0, float zr1, int level, int T,
                      int row0, int row1);
/* Row-restricted pieces of the sharded fusion (round 5): a rank computes only the rows it sweeps
 * plus their halo, and the rows its own tiles contribute to its neighbours'.
 * pf_fuse_partial_rows: pf_fuse_partial's sums of tiles [t0, t1) on rows [row0, row1) of the
 *   level only (rows of the range outside the band [h0, h1] get zero sums and counts; nothing is
 *   written outside the range).
 * pf_fuse_coverage_rows: the coverage count n of ALL tiles on rows [row0, row1) (layout-only:
 *   a rank counts its rows itself instead of receiving the other ranks' counts).
 * pf_fuse_normalize_rows: pf_fuse_normalize on rows [row0, row1) only.
 * pf_fuse_tile_rows: [*ymin, *ymax] = the rows where tiles [t0, t1) have non-zero partial sums at
 *   this level (*ymin > *ymax when none); host only, from the cached boxes.
 * pf_rows_add: dst[i] += src[i], i < n (a received partial-sum segment; exact where a pixel is
 *   covered by at most two tiles -- the rest is pf_fuse_multicover's).
 * pf_rows_add_batch: the same for `count` segments (dst[k], src[k], n[k]: host arrays of device
 *   pointers and sizes) in one launch; the segments must not overlap. */
int pf_fuse_partial_rows(pf_ctx* ctx, const float* tiles, const float* coeffs, int t0, int t1,
                         int out_w, int out_h, float zr0, float zr1, int level, int row0,
                         int row1, float* lsum, float* cnt);
int pf_fuse_coverage_rows(pf_ctx* ctx, int out_w, int out_h, float zr0, float zr1, int level,
                          int row0, int row1, float* cnt);
int pf_fuse_normalize_rows(pf_ctx* ctx, const float* lsum, const float* cnt, int out_w,
                           int out_h, float zr0, float zr1, int level, int row0, int row1,
                           float* lnorm);
int pf_fuse_tile_rows(pf_ctx* ctx, int out_w, int out_h, float zr0, float zr1, int level, int t0,
                      int t1, int* ymin, int* ymax);
int pf_rows_add(pf_ctx* ctx, float* dst, const float* src, long long n);
int pf_rows_add_batch(pf_ctx* ctx, float* const* dst, const float* const* src,
                      const long long* n, int count);

/* ---- stage timing (hipEvents on the context stream; replaces the reference's timeGetTime
 * brackets around registration and fusion, Depth.cpp:792-808, 907-916) ----
 * While enabled, every entry point records an event pair around each stage it launches.
 * pf_profile_read synchronises, then writes PF_NSTAGES entries of: elapsed ms, algorithmic
 * bytes (SURVEY.md section 8d accounting) and kernel launches; it resets the accumulators. */
#define PF_STAGE_WARP 0
#define PF_STAGE_REGISTER 1
#define PF_STAGE_SEED 2
#define PF_STAGE_TARGETS 3
#define PF_STAGE_JACOBI 4
#define PF_STAGE_QUANTIZE 5
#define PF_STAGE_METRICS 6
#define PF_NSTAGES 7
int pf_profile_enable(pf_ctx* ctx, int on);
int pf_profile_read(pf_ctx* ctx, double* ms, double* bytes, long long* launches);

/* ---- cross-stream ordering (no reference counterpart) ----
 * Makes `hip_stream` (another stream on the same device) wait until level `level` of the
 * context's most recently enqueued fusion (pf_fuse / pf_merge) has finished its sweeps, e.g. to
 * start memory-bound work beside the finer levels instead of beside the coarse one.  Returns
 * PF_EINVAL if no fusion with that many levels was enqueued on this context. */
int pf_stream_wait_level(pf_ctx* ctx, int level, void* hip_stream);

/* ---- Jacobi engine selection (no reference counterpart; every engine is bit-identical) ----
 * mode 1 (default; the environment variable PF_JRES=0 changes the default to 0): levels of
 * width 256 or 512 with the separable-coverage certificate run all their sweeps in one resident
 * launch, in row_blocks blocks per panorama (0: chosen by the cost model); mode 0: the
 * streaming temporally blocked passes everywhere. */
int pf_set_jacobi_engine(pf_ctx* ctx, int mode, int row_blocks);

/* ---- Jacobi pass planning for concurrent fusions (no reference counterpart) ----
 * The streaming passes cut each level's band into row chunks by a cost model of the chip's wave
 * slots (more chunks: more waves, but every chunk re-runs a T-row fill).  Contexts whose fusions
 * run concurrently on one GPU (several fusion lanes) each see only part
 * of the chip: `share` (0 < share <= 1, default 1) is the fraction this context's plans count
 * on, so they take fewer, longer chunks -- less total work.  Results are bit-identical for any
 * share (the chunking never changes a value).  PF_EINVAL for a share outside (0, 1]. */
int pf_set_jacobi_share(pf_ctx* ctx, double share);

/* ---- resident level kernel health (no reference counterpart) ----
 * The coarse fusion level runs all its sweeps in one launch whose row blocks trade halo rows
 * through device memory (pf_jres.hip).  Its waits are bounded: a wait that times out is counted
 * here instead of hanging the device (the level's result is then invalid).  Synchronises the
 * context stream; returns the count since the context was created (>= 0) or an error code. */
int pf_jres_errors(pf_ctx* ctx);
/* Test hook (no reference counterpart): in the context's NEXT resident launch, row block 0 of
 * every panorama withholds its hand-off flag and every wait gives up after 2^spin_log2 polls
 * (spin_log2 in [4, 24]), so the neighbouring blocks time out: the fusion must then report
 * PF_ETIMEOUT.  The launch after that runs normally. */
int pf_debug_jres_fault(pf_ctx* ctx, int spin_log2);
/* The same hook for the context's NEXT row-band smoothing launch (pf_solve_smoothing with more
 * than one row block per panorama): row block 0 never publishes its steps, its neighbour's wait
 * gives up after 2^spin_log2 polls (and stops waiting for the rest of the launch), and
 * pf_synchronize / the next call reports PF_ETIMEOUT. */
int pf_debug_smooth_fault(pf_ctx* ctx, int spin_log2);

/* ---- parity probes (bit-exact index maps) ----
 * For level `level` of out_w: per covered pixel and tap k (5 taps in std::map order), the
 * linear tile index (Y*W+X)*C of the tap for the first covering tile, -1 elsewhere.
 * tap_index: [out_h_level][w][5] int32 device buffer.  lsum/cnt as pf_fuse_partial. */
int pf_probe_taps(pf_ctx* ctx, int out_w, int out_h, float zr0, float zr1, int level,
                  int32_t* tap_index);
/* The E->P warps' coordinate maps, exactly as pf_warp_depth / pf_warp_rgb build and cache them
 * (host code, glibc transcendentals as the reference calls them; no context or GPU needed).
 * HOST buffers, one tile of tile_w x tile_h with viewing window *fov, panorama pw x ph:
 *   pf_probe_warp_coords: wxy[h*w] = x0 | y0 << 16, wfxy[h*w][2] = (fx, fy) -- the bilinear
 *     corner and weights of ToSphericalCoord (Depth.cpp:157-166) at ValueAtCoord's convention;
 *   pf_probe_rgb_taps: taps[h*w][4] = {ix0 | iy0 << 16, ix1 | iy1 << 16, ax bits, ay bits} --
 *     the GL_REPEAT corners and GL_LINEAR weights of SaveCubeMap's camera ray (Main.cpp:246-269,
 *     fs_perspective.txt:67-73). */
int pf_probe_warp_coords(const pf_window* fov, int tile_w, int tile_h, int pw, int ph,
                         uint32_t* wxy, float* wfxy);
int pf_probe_rgb_taps(const pf_window* fov, int tile_w, int tile_h, int pw, int ph,
                      uint32_t* taps);

/* ---- layout audit ----
 * What the tiles set by pf_set_tiles do at one level of an out_w x out_h fusion, counted on the
 * GPU with the fusion's own tables (the level's host sin/cos tables and boxes) and projection:
 * the verdict is about the taps pf_fuse reads, not about a second projection.  Taps are counted
 * per (tile, pixel of its box, tap of the five-point mask), as the reference would visit them. */
typedef struct pf_level_audit {
    int w, h, h0, h1;             /* as pf_level_info */
    long long taps_outside;       /* taps whose SphericalTo2D result leaves [0,1]^2 (tested on the
                                     unclamped floats): the reference prints "oops!" and reads
                                     past the tile there (Depth.cpp:1595-1604) */
    long long taps_clamped;       /* taps whose Value() index (Y*W+X)*C left the tile buffer and
                                     was clamped to [0, W*H*C - C]; depends on the tile size */
    long long covered;            /* pixels with at least one covering tile */
    long long uncovered_interior; /* rows h0+1..h1-1, columns 1..w-1, covered by no tile */
    int max_cover;                /* most tiles over one pixel */
    int seam;                     /* 1 if column w-1 is covered (the seam read, SURVEY App. A
                                     item 5) */
} pf_level_audit;
/* out: HOST struct; the call synchronizes the context's stream. */
int pf_layout_audit(pf_ctx* ctx, int out_w, int out_h, float zr0, float zr1, int level,
                    pf_level_audit* out);

/* ---- accuracy metrics ----
 * ErrorData (Depth.cpp:1980-2213) when given16 != NULL: the u16 result [batch][h][w];
 * ErrorEmap (Depth.cpp:2215-2458) when given != NULL: a float map [batch][h][w][given_c]
 * (channel 0).  gt: [batch][gh][gw][gc] float in 0..1 (channel 0).  Rows
 * [(int)(zr0/MYPI*h), (int)(zr1/MYPI*h)] are compared, gt < 1e-4 is skipped, cap_depth caps
 * both at 10 m; align_way 0 = none, 1 = median shift (exact medians), 2 = least squares.
 * out: DEVICE array of batch pf_metrics.  Replaces the reference's float outputs
 * (mse, mae, mre, mselog, delta1..3) and the optional median_shift_factor / least_square_shift. */
typedef struct pf_metrics {
    float mse, mae, mre, mselog, delta1, delta2, delta3;
    float median_shift;          /* gt_median / given_median (align_way 1), else 1 */
    float ls_s, ls_o;            /* least_square {s, o} (align_way 2), else 0 */
    float gt_median, given_median;
    int32_t n, nlog;             /* num_compares, num_log_compares */
    int32_t reserved[2];
} pf_metrics;
int pf_error_metrics(pf_ctx* ctx, const float* gt, int gw, int gh, int gc, const float* given,
                     const uint16_t* given16, int w, int h, int given_c, int batch, float zr0,
                     float zr1, int align_way, int cap_depth, pf_metrics* out);
/* Summation order of the means (mse, mae, mre, mselog) and of the least-squares sums:
 *   PF_METRICS_TREE (the C-ABI's default) -- fp64 partial sums in a fixed tree: deterministic,
 *     0.9 ms per 64 panoramas at C3, means within 1e-5 relative of exact fp64 sums (and within
 *     1e-2 of the reference's drifting float sums).
 *   PF_METRICS_SEQUENTIAL -- "bit-exact means": the reference's order, row-major float
 *     accumulators (mse and mselog through a double add, Depth.cpp:2119-2123, 2178-2186);
 *     bit-exact to it (mselog within 1e-5: device log10f).  The per-pixel terms are formed by
 *     producer waves beside verified fp32 chains: ~7.4 ms per 64-panorama call at C3.
 * The facade (include/pf_depth.h) and panofuse_main default to PF_METRICS_SEQUENTIAL, the order
 * the reference prints; PF_METRICS_ORDER=tree / --metrics-order tree select the tree. */
#define PF_METRICS_TREE 0
#define PF_METRICS_SEQUENTIAL 1
int pf_set_metrics_order(pf_ctx* ctx, int order);

/* ---- edge-fidelity metrics: ErrorLaplacian (Depth.cpp:2636-2953) ----
 * Error of the 3x3 Laplacian (mse, mae), of Sobel X and Sobel Y (mae) and of the 5x5 LoG filter
 * (mae) between gt [batch][gh][gw][gc] (channel 0) and a given map of w x h pixels: a float map
 * [batch][h][w][given_c] (channel 0) or the u16 result given16 [batch][h][w], read as
 * (float)v / 65535.0f -- exactly one of the two.  Per given pixel (x, y) the gt taps sit at
 * X = (int)((float)x * ((float)gw / (float)w)), Y likewise; the 3x3 samples run over
 * [1, w-2] x [1, h-2], the 5x5 samples over [2, w-3] x [2, h-3].  Taps are floats widened to
 * double and the filters are evaluated in fp64 in the reference's operand order, so every
 * per-pixel term and every count is the reference's; the means are fixed-order fp64 tree sums
 * (deterministic; within 2 * w*h * 2^-53 relative of the exact sum of the terms).  A sample
 * counts when its gt taps are valid ((double)tap >= 1e-4): the five cross taps (Laplacian), all
 * 25 (LoG), and for Sobel the reference's list as written (Depth.cpp:2747-2748 never tests
 * val[1][0] and val[2][0]).  A mean over no sample is NaN (0 / 0), as in the reference; maps
 * narrower or shorter than 3 are legal and give exactly that.
 * out: DEVICE array of batch pf_edge_metrics.  gt_lap / given_lap / lap_ae: DEVICE double
 * [batch][h][w] planes or NULL -- the gt Laplacian, the given map's Laplacian and their absolute
 * error (Depth.cpp:2666-2683, :2737-2742), zero where the Laplacian sample is invalid or outside
 * the inner region.  Stream-ordered. */
typedef struct pf_edge_metrics {
    double lap_mse, lap_mae, sobelx_mae, sobely_mae, lap5_mae;
    int64_t n_lap, n_sobel, n_lap5;
} pf_edge_metrics;                       /* 64 bytes */
int pf_error_laplacian(pf_ctx* ctx, const float* gt, int gw, int gh, int gc, const float* given,
                       const uint16_t* given16, int w, int h, int given_c, int batch,
                       pf_edge_metrics* out, double* gt_lap, double* given_lap, double* lap_ae);

/* ---- two-map comparison: ErrorCompare (Depth.cpp:2460-2634; Depth.h:318-319) ----
 * Scores a given map [batch][h][w][given_c] (channel 0) against gt [batch][gh][gw][gc] (channel 0)
 * and makes the 8-bit picture the reference saves.  All arithmetic is fp32, one rounding per
 * operation; conv(a, C) is DispDepthConversion of a C-channel map: where (double)fabsf(v) >= 1e-5,
 * v = 1.0f / v, C times over (the reference loops over the channels but converts channel 0 each
 * time, so a 3-channel map is inverted three times and a 2-channel map twice).
 *   disp_depth == 0 (depth against depth): m = ErrorEmap(gt, given, align_way, cap_depth);
 *     shifted = (unsigned char)(max(v, 0) * 255.0f) of the given map, depth = the given map's
 *     channel 0; fit_s = fit_o = 0, vmin = FLT_MAX, vmax = -FLT_MAX, n_nonblack = 0.
 *   disp_depth != 0 (the given map is a disparity, e.g. a mono360 PFM):
 *     1. gt_disp = conv(gt, gc);
 *     2. {fit_s, fit_o} = the least-squares {s, o} of ErrorEmap(gt_disp, given, 2, no cap);
 *     3. v = given * fit_s + fit_o (multiply, then add);  4. v = conv(v, given_c);
 *     5. v < 0 -> 0, v > 10 -> 10: the `depth` plane;
 *     6. m = ErrorEmap(gt, v, align_way, cap_depth);
 *     7. vmin / vmax over the pixels with (double)fabsf(v) >= 1e-4 ("non-black"), from
 *        FLT_MAX / -FLT_MAX;  8. those pixels become (v - vmin) / (vmax - vmin);
 *     9. shifted = (unsigned char)(max(v, 0) * 255.0f).
 * Where the reference's behaviour is undefined: a product above 255 saturates to 255; NaN becomes 0
 * in the u8 plane; every comparison otherwise follows IEEE as the source reads, so a NaN is not
 * black (it counts in n_nonblack), does not move vmin / vmax and stays NaN in the depth plane; the
 * facade writes no file for a null file name in disparity mode.
 * The order set by pf_set_metrics_order applies to both inner ErrorEmap calls.  given is not
 * written.  out: DEVICE array of batch pf_compare; depth: DEVICE float [batch][h][w] or NULL;
 * shifted: DEVICE uint8 [batch][h][w] or NULL.  Stream-ordered, no host round trip: the fit and
 * vmin / vmax stay on the device between the kernels. */
typedef struct pf_compare {
    pf_metrics m;            /* the final ErrorEmap call */
    float fit_s, fit_o;      /* disparity fit {s, o}; 0, 0 in depth mode */
    float vmin, vmax;        /* FLT_MAX, -FLT_MAX when no pixel qualified or in depth mode */
    int32_t n_nonblack;      /* pixels that were normalised */
    int32_t reserved[3];
} pf_compare;                /* 96 bytes */
int pf_error_compare(pf_ctx* ctx, const float* gt, int gw, int gh, int gc, const float* given,
                     int w, int h, int given_c, int batch, float zr0, float zr1, int disp_depth,
                     int align_way, int cap_depth, pf_compare* out, float* depth,
                     uint8_t* shifted);
/* EquirectangularMap::DispDepthConversion (Depth.cpp:587-610) in place: conv(data, channels) on
 * channel 0 of npix pixels of a DEVICE buffer with `channels` interleaved channels. */
int pf_disp_depth_convert(pf_ctx* ctx, float* data, long long npix, int channels);

/* Depth2DepthTransform of one map (Depth.cpp:245-274): channel 0 of npix pixels of a DEVICE
 * buffer with `channels` interleaved channels, X = clamp(v, 1e-4, 1-1e-4),
 * v' = clamp01(a X^3 + b X^2 + c X + d) in the reference's fp32 order; abcd is a HOST float[4]. */
int pf_depth_transform(pf_ctx* ctx, float* data, long long npix, int channels, const float* abcd);

#ifdef __cplusplus
}
#endif
#endif
