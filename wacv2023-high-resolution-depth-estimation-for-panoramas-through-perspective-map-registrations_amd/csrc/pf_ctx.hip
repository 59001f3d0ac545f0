// pf_ctx.hip -- the context of the C-ABI (include/panofuse.h): create and destroy, the setters,
// profiling and synchronisation, and the PF_ETIMEOUT reporting of the resident kernels.
#include "pf_ctx.hpp"

#include <cstdlib>

using namespace pf;

extern "C" {

const char* pf_version(void) { return "panofuse 0.1 (gfx950)"; }

int pf_create(int device, pf_ctx** out)
{
    if (!out) return PF_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return PF_EHIP;
    if (hipSetDevice(device) != hipSuccess) return PF_EHIP;
    pf_ctx* c = new pf_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        c->num_cu = prop.multiProcessorCount;
    *out = c;
    return PF_OK;
}

void pf_destroy(pf_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto& s : c->spans) {
        (void)hipEventDestroy(s.a);
        (void)hipEventDestroy(s.b);
    }
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_level)
        if (e) (void)hipEventDestroy(e);
    if (c->jres_err_h) (void)hipHostFree(c->jres_err_h);
    delete c;  // frees every DevBuf of the context and of its level cache
}

const char* pf_last_error(const pf_ctx* c) { return c ? c->err.c_str() : "null context"; }

int pf_stream_wait_level(pf_ctx* c, int level, void* hip_stream)
{
    if (!c || level < 0 || level >= c->nlev_recorded || !c->ev_level[level]) return PF_EINVAL;
    HIPCHK(c, hipStreamWaitEvent((hipStream_t)hip_stream, c->ev_level[level], 0));
    return PF_OK;
}

int pf_set_jacobi_share(pf_ctx* c, double share)
{
    if (!c || !(share > 0.0 && share <= 1.0)) return PF_EINVAL;
    c->jacobi_share = share;
    return PF_OK;
}

int pf_set_jacobi_engine(pf_ctx* c, int mode, int row_blocks)
{
    if (!c || mode < 0 || mode > 1 || row_blocks < 0) return PF_EINVAL;
    c->jres_mode = mode;
    c->jres_nb = row_blocks;
    return PF_OK;
}

}  // extern "C"

// PF_ETIMEOUT once for every new batch of timed-out resident-kernel waits whose count has
// reached the host (the copy queued behind each resident launch); never blocks.
int pf::jres_check(pf_ctx* c)
{
    if (!c->jres_err_h || !__atomic_load_n(c->jres_err_h, __ATOMIC_ACQUIRE)) return PF_OK;
    __atomic_store_n(c->jres_err_h, 0u, __ATOMIC_RELEASE);
    return fail(c, PF_ETIMEOUT, "resident kernel (Jacobi level or row-band smoothing): "
                "hand-off wait(s) timed out (%d resident-Jacobi timeouts so far on this context, "
                "pf_jres_errors); the output of that call is invalid", pf_jres_errors(c));
}

// The coherent pinned PF_ETIMEOUT flag shared by the resident Jacobi kernel and the row-band
// smoothing kernel: allocated and zeroed once (hipHostMalloc does not promise zeroed memory);
// PF_JRES_ERRHOST=0 leaves it out (timeouts then only count into pf_jres_errors).
int pf::ensure_err_host(pf_ctx* c)
{
    static const bool errhost = !(getenv("PF_JRES_ERRHOST") && atoi(getenv("PF_JRES_ERRHOST")) == 0);
    if (c->jres_err_h || !errhost) return PF_OK;
    HIPCHK(c, hipHostMalloc((void**)&c->jres_err_h, sizeof(uint32_t),
                            hipHostMallocMapped | hipHostMallocCoherent));
    __atomic_store_n(c->jres_err_h, 0u, __ATOMIC_RELEASE);
    return PF_OK;
}

extern "C" {

int pf_debug_smooth_fault(pf_ctx* c, int spin_log2)
{
    if (!c || spin_log2 < 4 || spin_log2 > 24) return PF_EINVAL;
    c->smooth_fault = spin_log2;
    return PF_OK;
}

int pf_debug_jres_fault(pf_ctx* c, int spin_log2)
{
    if (!c || spin_log2 < 4 || spin_log2 > 24) return PF_EINVAL;
    c->jres_fault = spin_log2;
    return PF_OK;
}

int pf_jres_errors(pf_ctx* c)
{
    if (!c) return PF_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!c->jres_sync.p) return 0;
    uint32_t n = 0;
    HIPCHK(c, hipMemcpy(&n, (const uint32_t*)c->jres_sync.p + 1, sizeof(n), hipMemcpyDeviceToHost));
    return (int)(n & 0x7FFFFFFF);
}

int pf_set_solver(pf_ctx* c, int solver)
{
    if (!c) return PF_EINVAL;
    if (solver != PF_SOLVER_LM && solver != PF_SOLVER_NORMAL)
        return fail(c, PF_EINVAL, "pf_set_solver: unknown solver %d", solver);
    c->solver = solver;
    return PF_OK;
}

int pf_set_stream(pf_ctx* c, void* s)
{
    if (!c) return PF_EINVAL;
    c->stream = (hipStream_t)s;
    return PF_OK;
}

int pf_profile_enable(pf_ctx* c, int on)
{
    if (!c) return PF_EINVAL;
    double ms[PF_NSTAGES], by[PF_NSTAGES];
    long long ln[PF_NSTAGES];
    int rc = pf_profile_read(c, ms, by, ln);  // drains and recycles pending spans
    c->prof_on = on != 0;
    return rc;
}

int pf_profile_read(pf_ctx* c, double* ms, double* bytes, long long* launches)
{
    if (!c) return PF_EINVAL;
    for (int s = 0; s < PF_NSTAGES; s++) {
        if (ms) ms[s] = 0;
        if (bytes) bytes[s] = 0;
        if (launches) launches[s] = 0;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto& s : c->spans) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, s.a, s.b));
        if (ms) ms[s.stage] += t;
        if (bytes) bytes[s.stage] += s.bytes;
        if (launches) launches[s.stage] += s.launches;
        c->event_pool.push_back(s.a);
        c->event_pool.push_back(s.b);
    }
    c->spans.clear();
    return PF_OK;
}

int pf_synchronize(pf_ctx* c)
{
    if (!c) return PF_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return jres_check(c);
}

}  // extern "C"
