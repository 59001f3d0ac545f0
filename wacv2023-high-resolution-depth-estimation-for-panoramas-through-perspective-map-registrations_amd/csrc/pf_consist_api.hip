// pf_consist_api.hip -- the entry points of the overlap-consistent registration (pf_consist.hip):
// pf_overlap_pairs, pf_overlap_table, pf_overlap_stats, pf_register_consistent.
#include "pf_ctx.hpp"

#include <cmath>
#include <cstdlib>

using namespace pf;

namespace {

// The new entry points have no form under the validity rule, a loss or planar tiles: checked
// first, so the refusal names the setter whatever else the call lacks.
int check_plain_modes(pf_ctx* c, const char* entry)
{
    int rc;
    if (!c) return PF_EINVAL;
    if ((rc = check_unmasked(c, entry))) return rc;
    if ((rc = check_no_loss(c, entry))) return rc;
    if (c->tile_depth != PF_TILE_DEPTH_RAY)
        return fail(c, PF_ESTATE,
                    "%s has no planar-depth form: call pf_set_tile_depth(ctx, PF_TILE_DEPTH_RAY) "
                    "first",
                    entry);
    return PF_OK;
}

// The overlap table of the stored layout's registration grids for this zenith range, built on
// first use: count (k_paircount), scan on the host, fill (k_pairidx).  Synchronises when it builds.
int prepare_pairs(pf_ctx* c, float zr0, float zr1)
{
    int rc;
    if ((rc = prepare_registration(c, zr0, zr1))) return rc;
    if ((rc = check_reg_grids(c, nullptr))) return rc;
    if (c->pair_valid) return PF_OK;
    const int nt = c->ntiles;
    const size_t ncell = (size_t)nt * nt;
    if ((rc = ensure(c, c->pair_counts, sizeof(int) * ncell))) return rc;
    const TileGeom* geom = (const TileGeom*)c->geom.p;
    const RegGrid* reg = (const RegGrid*)c->reg.p;
    const GridCol* rcols = (const GridCol*)c->rcols.p;
    const GridRow* rrows = (const GridRow*)c->rrows.p;
    launch_paircount(c->stream, geom, reg, rcols, rrows, nt, (int*)c->pair_counts.p);
    HIPCHK(c, hipGetLastError());
    std::vector<int> counts(ncell);
    HIPCHK(c, hipMemcpyAsync(counts.data(), c->pair_counts.p, sizeof(int) * ncell,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pairs_h.clear();
    long long total = 0;
    for (int p = 0; p < nt; p++)
        for (int q = 0; q < nt; q++) {
            const int n = counts[(size_t)p * nt + q];
            if (n <= 0) continue;
            if (total + n > INT32_MAX)
                return fail(c, PF_EINVAL, "the layout has more than 2^31 overlap samples");
            const int row[4] = {p, q, (int)total, n};
            c->pairs_h.insert(c->pairs_h.end(), row, row + 4);
            total += n;
        }
    c->pair_samples = total;
    if ((rc = upload(c, c->pair_list, c->pairs_h))) return rc;
    if ((rc = ensure(c, c->pair_index, sizeof(int2) * (size_t)(total > 0 ? total : 1)))) return rc;
    const int npairs = (int)(c->pairs_h.size() / 4);
    if (npairs > 0) {
        launch_pairidx(c->stream, geom, reg, rcols, rrows, (const int*)c->pair_list.p, npairs,
                       (int2*)c->pair_index.p);
        HIPCHK(c, hipGetLastError());
    }
    c->pair_valid = true;
    return PF_OK;
}

}  // namespace

extern "C" {

int pf_overlap_pairs(pf_ctx* c, float zr0, float zr1, int* npairs, long long* nsamples)
{
    int rc;
    if ((rc = check_plain_modes(c, "pf_overlap_pairs"))) return rc;
    if ((rc = check_common(c, 1))) return rc;
    if ((rc = prepare_pairs(c, zr0, zr1))) return rc;
    if (npairs) *npairs = (int)(c->pairs_h.size() / 4);
    if (nsamples) *nsamples = c->pair_samples;
    return PF_OK;
}

int pf_overlap_table(pf_ctx* c, float zr0, float zr1, int* pairs, int* index)
{
    int rc;
    if ((rc = check_plain_modes(c, "pf_overlap_table"))) return rc;
    if ((rc = check_common(c, 1))) return rc;
    if (!pairs || !index) return fail(c, PF_EINVAL, "pf_overlap_table: pairs/index is NULL");
    if ((rc = prepare_pairs(c, zr0, zr1))) return rc;
    if (!c->pairs_h.empty())
        HIPCHK(c, hipMemcpyAsync(pairs, c->pair_list.p, sizeof(int) * c->pairs_h.size(),
                                 hipMemcpyDeviceToDevice, c->stream));
    if (c->pair_samples > 0)
        HIPCHK(c, hipMemcpyAsync(index, c->pair_index.p, sizeof(int2) * (size_t)c->pair_samples,
                                 hipMemcpyDeviceToDevice, c->stream));
    return PF_OK;
}

int pf_overlap_stats(pf_ctx* c, const float* tiles, const float* coeffs, int batch, float zr0,
                     float zr1, double* stats)
{
    int rc;
    if ((rc = check_plain_modes(c, "pf_overlap_stats"))) return rc;
    if ((rc = check_common(c, batch))) return rc;
    if (!tiles || !stats) return fail(c, PF_EINVAL, "pf_overlap_stats: tiles/stats is NULL");
    if ((rc = prepare_pairs(c, zr0, zr1))) return rc;
    const int npairs = (int)(c->pairs_h.size() / 4);
    if (npairs == 0) return PF_OK;
    StageTimer t(c, PF_STAGE_REGISTER, batch * 16.0 * (double)c->pair_samples, 1);
    launch_overlap_stats(c->stream, (const TileGeom*)c->geom.p, (const int*)c->pair_list.p, npairs,
                         c->ntiles, (const int2*)c->pair_index.p, tiles, c->tile_elems, coeffs,
                         stats, batch);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_register_consistent(pf_ctx* c, const float* emap, int ew, int eh, int ec, float* tiles,
                           int batch, float zr0, float zr1, double lambda, int apply,
                           float* coeffs, double* coeffs64, double* summary)
{
    int rc;
    if ((rc = check_plain_modes(c, "pf_register_consistent"))) return rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles) return fail(c, PF_EINVAL, "tiles is NULL");
    if (!(std::isfinite(lambda) && lambda >= 0.0))
        return fail(c, PF_EINVAL, "pf_register_consistent: lambda must be finite and >= 0 (got %g)",
                    lambda);
    if ((rc = prepare_pairs(c, zr0, zr1))) return rc;
    const int nt = c->ntiles, npairs = (int)(c->pairs_h.size() / 4);
    const int nps = pair_sums_per_pair(), nds = register_sums_per_tile();
    if ((rc = ensure(c, c->reg_sums, sizeof(double) * nds * nt * batch))) return rc;
    if ((rc = ensure(c, c->pair_sums, sizeof(double) * nps * (size_t)(npairs > 0 ? npairs : 1) * batch)))
        return rc;
    // PF_CONSIST_WORKSPACE (tests): the global-workspace form of the solve for any layout
    const char* force = getenv("PF_CONSIST_WORKSPACE");
    const bool in_lds = consist_fits_lds(nt) && !(force && force[0] == '1');
    double* ws = nullptr;
    if (!in_lds) {
        if ((rc = ensure(c, c->consist_ws, sizeof(double) * consist_workspace_doubles(nt) * batch)))
            return rc;
        ws = (double*)c->consist_ws.p;
    }
    float* cf = coeffs;
    if (!cf) {
        if ((rc = ensure(c, c->coeffs, sizeof(float) * 4 * nt * batch))) return rc;
        cf = (float*)c->coeffs.p;
    }
    const int2* sidx = reg_sample_index(c, ew, eh, ec);  // before the stage timer: built once
    double nsamp = 0;
    for (const RegGrid& g : c->reg_h) nsamp += (double)(g.cols + 1) * (g.rows + 1);
    const TileGeom* geom = (const TileGeom*)c->geom.p;
    StageTimer t(c, PF_STAGE_REGISTER,
                 batch * (8.0 * nsamp + 16.0 * (double)c->pair_samples +
                          (apply ? 8.0 * (double)c->tile_elems / c->tile_c : 0.0)),
                 (npairs > 0 ? 3 : 2) + (apply ? 1 : 0));
    // the data moments: k_register's launch, handing its 15 sums out
    launch_register(c->stream, geom, (const RegGrid*)c->reg.p, (const GridCol*)c->rcols.p,
                    (const GridRow*)c->rrows.p, nt, emap, ew, eh, ec, (long long)ew * eh * ec,
                    tiles, c->tile_elems, 3, c->solver, nullptr, nullptr, batch,
                    (double*)c->reg_sums.p, nullptr, sidx);
    if (npairs > 0)
        launch_pair_moments(c->stream, geom, (const int*)c->pair_list.p, npairs,
                            (const int2*)c->pair_index.p, tiles, c->tile_elems,
                            (double*)c->pair_sums.p, batch);
    launch_consist_solve(c->stream, (const double*)c->reg_sums.p, (const double*)c->pair_sums.p,
                         (const int*)c->pair_list.p, npairs, nt, lambda, (double)c->pair_samples,
                         ws, cf, coeffs64, summary, batch);
    if (apply)
        launch_apply_cubic(c->stream, geom, nt, c->tile_elems / c->tile_c, tiles, c->tile_elems,
                           cf, batch);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

}  // extern "C"
