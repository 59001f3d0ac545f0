// pf_plan.hip -- the Jacobi cost model and pass planner, and the resident-kernel planner.  The
// planners only: nothing here touches a stream.
#include "pf_ctx.hpp"

#include <cstdlib>

using namespace pf;

// SIMDs the pass plans of this context count on: the chip times the context's share
static int plan_simds(const pf_ctx* c)
{
    const int n = (int)(4.0 * c->num_cu * c->jacobi_share + 0.5);
    return n < 4 ? 4 : n;
}

// Jacobi pass geometry: lanes own kJacobiCols columns, strips carry a Tp-column halo (Tp >= T,
// rounded to the column count so vector rows stay aligned); the sweep depth and row chunking of
// every pass come from the cost model of plan_level().  Env overrides for tuning runs: PF_JT
// (largest T), PF_JOVH (per-step overhead in update units).
struct JacobiTuning {
    int Tmax = 10;
    double step_overhead = 3.0, lone_cycles = 4.0;  // swept on MI355X (profiles/r02/jacobi; recipe: tools/gpu_round.sh ab)
    double pipe_overhead = 1.0;   // pipelined engine: barrier + exchange per step, update units
    // per pass, in the cost units of best_chunks (~10 ns each at C3): a launch's fixed cost
    // (dispatch, ramp, drain; a few us).  Without it the planner cut the batch-1 levels into
    // hundreds of tiny passes (C5 on one GPU: 173 passes, Jacobi 2.11 ms; with it 63 passes,
    // 1.60 ms; C2 latency 0.97 -> 0.82 ms; the batch-64 plans are unchanged).  PF_JLAUNCH=...
    double launch_cost = 300.0;
};

// The tunables, read from the environment once per process.
static const JacobiTuning& jacobi_tuning()
{
    static const JacobiTuning tune = [] {
        JacobiTuning t;
        if (const char* e = getenv("PF_JT")) t.Tmax = atoi(e);
        if (const char* e = getenv("PF_JOVH")) t.step_overhead = atof(e);
        if (const char* e = getenv("PF_JC1")) t.lone_cycles = atof(e);
        if (const char* e = getenv("PF_JPOVH")) t.pipe_overhead = atof(e);
        if (const char* e = getenv("PF_JLAUNCH")) t.launch_cost = atof(e);
        if (t.Tmax < 1) t.Tmax = 1;
        return t;
    }();
    return tune;
}

// One pass: depth T, nchunks row chunks.  Its nstrips*batch*nchunks waves each run
// rows_per_chunk + 3T + ~4 steps of T updates per column (lagged levels, halo, 6-step alignment), and
// they run in ceil(waves / resident) rounds, so the pass costs ~ rounds * steps * (T + o) with o
// the per-step overhead (loads, LDS ring, store) in update units.  Whole rounds matter: at the
// small levels a "one wave per slot" grid left the last round 20-80% empty.
static PassPlan best_chunks(int T, int band_rows, int w, int batch, int per_simd, int nsimd,
                            int stages = 1)
{
    const JacobiTuning& tune = jacobi_tuning();
    const double c1 = tune.lone_cycles;
    const double ovh = tune.step_overhead + (stages > 1 ? tune.pipe_overhead : 0.0);
    // VALU work of one step of one wave in update units: T/stages levels
    const double work = (double)T / stages;
    PassPlan best;
    best.T = T;
    best.stages = stages;
    best.cost = 1e300;
    const long long per = (long long)strip_geometry(T, w).nstrips * batch;
    const long long slots = (long long)per_simd * nsimd;
    for (int n = 1; n <= band_rows; n++) {
        const int rows = (band_rows + n - 1) / n;
        if (n > 1 && (band_rows + rows - 1) / rows < n) continue;  // same as a smaller n
        // rounds of resident waves; in each, a SIMD holding W waves issues one VALU
        // instruction per 2 cycles shared among them, and a lone wave one per ~c1 cycles
        const long long waves = per * n * stages;
        double cyc = 0;
        for (long long left = waves; left > 0; left -= slots) {
            const long long in_round = left < slots ? left : slots;
            const double W = (double)((in_round + nsimd - 1) / nsimd);
            cyc += (2.0 * W > c1 ? 2.0 * W : c1);
        }
        const double cost = cyc * (rows + 3.0 * T + 4.0) * (work + ovh);
        if (cost < best.cost) {
            best.cost = cost;
            best.nchunks = n;
        }
    }
    return best;
}

// Sweep depths for a level: a shortest-path split of `iters` into passes from the supported
// menu (<= tcap), each with its best chunking.
std::vector<PassPlan> pf::plan_level(pf_ctx* c, const LevelDims& L, int tcap, int batch,
                                     bool fast, int band_rows)
{
    const JacobiTuning& tune = jacobi_tuning();
    static const int menu[] = {10, 8, 5, 4, 2, 1};
    if (band_rows <= 0) band_rows = L.h1 - L.h0 + 1;
    PassPlan opt[11];
    for (int T : menu)
        if (T <= tcap && jstream_supported_T(T))
            opt[T] = best_chunks(T, band_rows, L.w, batch, jstream_waves_per_cu(T, fast) / 4,
                                 4 * c->num_cu);
    // the pipelined engine (2 waves per strip-chunk), packed form only; PF_JPIPE=0 disables it,
    // PF_JPIPE=1 takes it wherever it exists, otherwise the cost model decides
    static const char* pe = getenv("PF_JPIPE");
    const int pmode = pe ? atoi(pe) : 2;
    if (fast && pmode != 0)
        for (int T : menu) {
            if (T > tcap || T % 2 || !jpipe_supported(2, T / 2)) continue;
            PassPlan pp = best_chunks(T, band_rows, L.w, batch, jpipe_waves_per_cu(2, T / 2) / 4,
                                      4 * c->num_cu, 2);
            if (pmode == 1 || pp.cost < opt[T].cost || !jstream_supported_T(T)) opt[T] = pp;
        }
    if (fast && pmode == 1)  // forced: the single-wave engine only where no pipe fits
        for (int T : menu)
            if (opt[T].stages == 1) opt[T].cost *= 1e6;
    // tuning runs: PF_JTONLY<w>=T restricts the level of width w to depth-T passes (and depths 1
    // and 2 for a remainder)
    char tkey[32];
    snprintf(tkey, sizeof(tkey), "PF_JTONLY%d", L.w);
    const int tonly = getenv(tkey) ? atoi(getenv(tkey)) : 0;
    std::vector<double> dp(L.iters + 1, 1e300);
    std::vector<int> choice(L.iters + 1, 1);
    dp[0] = 0;
    for (int r = 1; r <= L.iters; r++)
        for (int T : menu) {
            if (T > r || T > tcap || !jstream_supported_T(T)) continue;
            if (tonly && T != tonly && T > 2) continue;
            const double v = dp[r - T] + opt[T].cost + tune.launch_cost;
            if (v < dp[r]) {
                dp[r] = v;
                choice[r] = T;
            }
        }
    std::vector<PassPlan> plan;
    for (int r = L.iters; r > 0; r -= choice[r]) plan.push_back(opt[choice[r]]);
    // a context that shares the chip with concurrent fusions (pf_set_jacobi_share) keeps the
    // depths and engines chosen for the whole chip and re-chunks its streaming passes for its
    // share: fewer, longer row chunks
    if (c->jacobi_share < 1.0)
        for (PassPlan& pp : plan)
            if (pp.stages == 1)
                pp.nchunks = best_chunks(pp.T, band_rows, L.w, batch,
                                         jstream_waves_per_cu(pp.T, fast) / 4, plan_simds(c))
                                 .nchunks;
    // tuning runs: PF_JN<w> forces the row chunking of the level of width w
    char key[32];
    snprintf(key, sizeof(key), "PF_JN%d", L.w);
    if (const char* e = getenv(key))
        for (PassPlan& pp : plan) pp.nchunks = atoi(e) > 0 ? atoi(e) : pp.nchunks;
    return plan;
}

// Largest sweep depth the streaming engine may use on this level: its halo rows must stay inside
// [1, h-2] (loads clamp rows into that range) and a strip (plus halo) must fit in a row.
int pf::jacobi_tcap(const LevelDims& L)
{
    int cap = jacobi_tuning().Tmax;
    char key[32];  // tuning runs: PF_JT<w> caps the sweep depth of the level of width w
    snprintf(key, sizeof(key), "PF_JT%d", L.w);
    if (const char* e = getenv(key)) cap = atoi(e) > 0 ? atoi(e) : cap;
    if (L.h0 - 1 < cap) cap = L.h0 - 1;
    if (L.h - 2 - L.h1 < cap) cap = L.h - 2 - L.h1;
    while (cap >= 1) {
        int Tp = (cap + 3) / 4 * 4;
        if (128 - Tp <= L.w && L.w % 2 == 0) break;
        cap--;
    }
    return cap;
}

PassPlan pf::plan_band_pass(pf_ctx* c, const LevelDims& L, int T, int band_rows, bool fast)
{
    return best_chunks(T, band_rows, L.w, 1, jstream_waves_per_cu(T, fast) / 4, plan_simds(c));
}

JresPlan pf::jres_plan(pf_ctx* c, const LevelDims& L, int batch, bool fast)
{
    JresPlan jp;
    static const char* env = getenv("PF_JRES");  // "0": streaming passes only (A/B runs)
    const int mode = c->jres_mode >= 0 ? c->jres_mode : (env && atoi(env) == 0 ? 0 : 1);
    if (mode == 0 || !fast || batch < 1) return jp;
    const int rows = jres_region_rows(L.w);  // region rows of one workgroup
    if (rows <= 0 || L.iters < 1) return jp;
    // resident blocks per CU at widths 256 and 512 (jres_region_rows supports no other), for the
    // full and the half-height region
    static int bpc_w[2][2] = {{-1, -1}, {-1, -1}};
    const int wi = L.w == 256 ? 0 : 1;
    const int band = L.h1 - L.h0 + 1;
    // cost in sweep units: the blocks run in ceil(blocks / resident) rounds of residency, each
    // sweep costs one unit (fixed region size), each K-sweep hand-off ~2.5 units (measured
    // hand-off latency on MI355X is 2-3 us against ~1.2 us per sweep)
    static const double xcost = getenv("PF_JRES_X") ? atof(getenv("PF_JRES_X")) : 2.5;
    static const int nb_env = getenv("PF_JRES_NB") ? atoi(getenv("PF_JRES_NB")) : 0;
    const int nb_force = c->jres_nb > 0 ? c->jres_nb : nb_env;
    // a sweep of the half-height region costs each wave ~half the updates, plus the fixed
    // barrier / edge exchange (PF_JRES_HALFCOST: its cost in full-region sweeps)
    static const double hcost = getenv("PF_JRES_HALFCOST") ? atof(getenv("PF_JRES_HALFCOST")) : 0.6;
    double best = 1e300;
    for (int hv = 0; hv < 2; hv++) {
        const int rows_h = hv ? jres_region_rows(L.w, true) : rows;
        if (rows_h <= 0) continue;
        if (bpc_w[wi][hv] < 0) bpc_w[wi][hv] = jres_blocks_per_cu(L.w, hv == 1);
        const int bpc = bpc_w[wi][hv];  // of the instantiation this choice launches
        if (bpc < 1) continue;
        const double sweep = hv ? hcost : 1.0;
        for (int nb = 1; nb <= band && nb <= 64; nb++) {
            if (nb_force > 0 && nb != nb_force) continue;
            const int core = (band + nb - 1) / nb;
            if ((band + core - 1) / core != nb) continue;
            int K;
            if (nb == 1) {
                if (core > rows_h) continue;
                K = L.iters;
            } else {
                K = (rows_h - core) / 2;
                if (K > core) K = core;
                if (K > L.iters) K = L.iters;
                if (K < 1) continue;
            }
            const int rounds = (L.iters + K - 1) / K;
            const long long resident = (long long)c->num_cu * bpc;
            const long long waves = ((long long)batch * nb + resident - 1) / resident;
            const double cost = (double)waves * (L.iters * sweep + (rounds - 1) * xcost);
            if (cost < best) {
                best = cost;
                jp.on = true;
                jp.nb = nb;
                jp.core = core;
                jp.K = K;
                jp.rounds = rounds;
                jp.half = hv == 1;
            }
        }
    }
    return jp;
}
