// pmc_tuning.hip -- the switch table of include/pmc_tuning.h
#include "pmc_context.h"

// ---- tuning switches (include/pmc_tuning.h): a process-wide table set through pmc_tuning_set; the library reads three settings
// from the environment (PMC_NUM_SLOTS, PMC_NUM_GROUPS, PMC_STAT_POOL_BLOCKS) and nothing else
namespace
{
    std::mutex g_tuneMutex;
    // name -> value; the values live in a pool that is never shrunk, so that a pointer handed out by pmcTune stays valid when another
    // host thread sets or clears switches meanwhile (one host thread per device drives pmc_create / pmc_run_primary in the CLI and in
    // the multi-device tests).  A switch is SAMPLED where it is used -- the table layouts at pmc_create, the kernel selection at
    // pmc_run_primary: changing switches while a context is being created or is running gives that context either value.
    std::map<std::string, const std::string*>& tuneTable()
    {
        static std::map<std::string, const std::string*> table;
        return table;
    }
    const std::string* internTuneValue(const char* value)
    {
        static std::deque<std::string> pool;
        for (const auto& v : pool)
            if (v == value) return &v;
        pool.emplace_back(value);
        return &pool.back();
    }
}
// the value of a tuning switch, or null (the pointer stays valid for the life of the process)
extern "C" const char* pmcTune(const char* name)
{
    std::lock_guard<std::mutex> lock(g_tuneMutex);
    auto& table = tuneTable();
    auto at = table.find(name);
    return at == table.end() ? nullptr : at->second->c_str();
}
extern "C" int pmc_tuning_set(const char* name, const char* value)
{
    if (!name) return PMC_ERR_INVALID;
    std::lock_guard<std::mutex> lock(g_tuneMutex);
    if (value)
        tuneTable()[name] = internTuneValue(value);
    else
        tuneTable().erase(name);
    return PMC_OK;
}
extern "C" void pmc_tuning_clear(void)
{
    std::lock_guard<std::mutex> lock(g_tuneMutex);
    tuneTable().clear();
}

extern "C" int pmc_tune_dipole_cosines(pmc_ctx* ctx, const double* u, int64_t n, double* cos_out)
{
    if (!ctx || n < 0 || (n > 0 && (!u || !cos_out))) return fail(PMC_ERR_INVALID, "pmc_tune_dipole_cosines: invalid argument");
    if (n == 0) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    double* d = nullptr;
    HIP_TRY(hipMalloc(&d, sizeof(double) * size_t(2 * n)));
    hipError_t e = hipMemcpyAsync(d, u, sizeof(double) * size_t(n), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = pmcLaunchDipoleCosines(d, n, d + n, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(cos_out, d + n, sizeof(double) * size_t(n), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    hipFree(d);
    if (e != hipSuccess) return hipFail(e, "pmc_tune_dipole_cosines");
    return PMC_OK;
}

extern "C" int pmc_tune_source_velocities(pmc_ctx* ctx, int32_t source, const double* r, int64_t n, double* v_out)
{
    if (!ctx || n < 0 || (n > 0 && (!r || !v_out))) return fail(PMC_ERR_INVALID, "pmc_tune_source_velocities: invalid argument");
    if (source < 0 || source >= ctx->dev.num_sources) return fail(PMC_ERR_INVALID, "pmc_tune_source_velocities: no such source");
    if (n == 0) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    double* d = nullptr;
    HIP_TRY(hipMalloc(&d, sizeof(double) * size_t(6 * n)));
    hipError_t e = hipSuccess;
    if (ctx->sceneDirty)
    {
        // (the scene in constant memory, as pmc_trace_ray brings it up to date)
        e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = pmcUploadScene(ctx->slot, &ctx->dev, ctx->stream);
        if (e == hipSuccess) ctx->sceneDirty = false;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d, r, sizeof(double) * size_t(3 * n), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = pmcLaunchSourceVelocities(ctx->slot, source, d, n, d + 3 * n, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(v_out, d + 3 * n, sizeof(double) * size_t(3 * n), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    hipFree(d);
    if (e != hipSuccess) return hipFail(e, "pmc_tune_source_velocities");
    return PMC_OK;
}
