// pmc_tuning.hip -- the switch table and the test aids of include/pmc_tuning.h
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

// ---- test aids of the log kernels (include/pmc_tuning.h): the counting sort and the reduce kernels on logs the host supplies
namespace
{
    constexpr int64_t LOG_MAX_ENTRIES = int64_t(1) << 24;

    // what is wrong with a host-supplied log, or null: every kernel behind these aids reads whole chunks of keys and values and fills[chunk]
    const char* logProblem(const uint32_t* keys, const double* vals, const uint32_t* fills, int64_t n)
    {
        if (!keys || !vals) return "null array";
        if (n <= 0 || n > LOG_MAX_ENTRIES || n % PMC_RF_LOG_CHUNK) return "the number of entries must be a positive multiple of the chunk, at most 2^24";
        for (int64_t t = 0; fills && t < n / PMC_RF_LOG_CHUNK; ++t)
            if (fills[t] > (uint32_t)PMC_RF_LOG_CHUNK) return "a chunk filled beyond its size";
        return nullptr;
    }

    // the log on the device, the zeroed buffers of its partitioned copy and the sort's counters
    struct DeviceLog
    {
        uint32_t *keys, *sortedKeys, *fills;
        double *vals, *sortedVals;
        unsigned long long* temp;
    };
    hipError_t stageLog(CallBuffers& B, hipStream_t stream, const uint32_t* keys, const double* vals, const uint32_t* fills, int64_t n, int numParts, DeviceLog& L)
    {
        L = DeviceLog{};
        hipError_t e = B.get(size_t(n), &L.keys, keys);
        if (e == hipSuccess) e = B.get(size_t(n), &L.vals, vals);
        if (e == hipSuccess && fills) e = B.get(size_t(n / PMC_RF_LOG_CHUNK), &L.fills, fills);
        if (e == hipSuccess) e = B.get(size_t(n), &L.sortedKeys);
        if (e == hipSuccess) e = B.get(size_t(n), &L.sortedVals);
        if (e == hipSuccess) e = B.get(pmcRfTempBytes(numParts) / sizeof(unsigned long long), &L.temp);
        if (e == hipSuccess) e = hipMemsetAsync(L.sortedKeys, 0, size_t(n) * sizeof(uint32_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(L.sortedVals, 0, size_t(n) * sizeof(double), stream);
        return e;
    }

    // the scene in constant memory, as pmc_trace_ray brings it up to date
    hipError_t sceneUpToDate(pmc_ctx* ctx)
    {
        if (!ctx->sceneDirty) return hipSuccess;
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = pmcUploadScene(ctx->slot, &ctx->dev, ctx->stream);
        if (e == hipSuccess) ctx->sceneDirty = false;
        return e;
    }
}

extern "C" int pmc_tune_log_geometry(pmc_ctx* ctx, pmc_log_geometry_values* out)
{
    if (!ctx || !out) return fail(PMC_ERR_INVALID, "pmc_tune_log_geometry: invalid argument");
    const LogPlan L = pmcLogPlan(ctx);
    pmcLogConstants(out);
    out->cell_slots = ctx->dev.cell_slots;
    out->rf_num_lambda = ctx->dev.rf_store ? ctx->dev.rf_num_lambda : 0;
    out->rf_keys = L.rfKeys, out->rf_parts = L.rfParts, out->rf_logged = L.rfLogged ? 1 : 0;
    out->stat_records = L.statRecords, out->stat_parts = L.statParts, out->stat_logged = L.statLogged ? 1 : 0;
    out->max_entries = LOG_MAX_ENTRIES;
    return PMC_OK;
}

extern "C" int pmc_tune_log_partition(pmc_ctx* ctx, int32_t stat, int32_t num_parts, const uint32_t* keys, const double* vals, const uint32_t* fills, int64_t n,
                                      uint32_t* sorted_keys, double* sorted_vals, uint64_t* start)
{
    if (!ctx || !sorted_keys || !sorted_vals || !start || (stat != 0 && stat != 1)) return fail(PMC_ERR_INVALID, "pmc_tune_log_partition: invalid argument");
    if (num_parts < 1 || num_parts > pmcRfMaxParts())
        return fail(PMC_ERR_INVALID, "pmc_tune_log_partition: between 1 and " + std::to_string(pmcRfMaxParts()) + " partitions");
    if (const char* problem = logProblem(keys, vals, fills, n)) return fail(PMC_ERR_INVALID, std::string("pmc_tune_log_partition: ") + problem);
    HIP_TRY(hipSetDevice(ctx->device));
    CallBuffers B;
    DeviceLog L;
    hipError_t e = stageLog(B, ctx->stream, keys, vals, fills, n, num_parts, L);
    if (e == hipSuccess) e = pmcLaunchLogPartition(stat, L.keys, L.vals, L.sortedKeys, L.sortedVals, (unsigned long long)n, num_parts, L.temp, ctx->numCU, L.fills, ctx->stream);
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "start[] is copied as it stands");
    if (e == hipSuccess) e = hipMemcpyAsync(start, L.temp + num_parts, sizeof(uint64_t) * (size_t(num_parts) + 1), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sorted_keys, L.sortedKeys, sizeof(uint32_t) * size_t(n), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sorted_vals, L.sortedVals, sizeof(double) * size_t(n), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t done = hipStreamSynchronize(ctx->stream);  // (whatever was enqueued has finished before the buffers go)
    if (e == hipSuccess) e = done;
    if (e != hipSuccess) return hipFail(e, "pmc_tune_log_partition");
    return PMC_OK;
}

extern "C" int pmc_tune_rf_log_flush(pmc_ctx* ctx, const uint32_t* keys, const double* vals, int64_t n)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "pmc_tune_rf_log_flush: invalid argument");
    const LogPlan plan = pmcLogPlan(ctx);
    if (!plan.rfLogged || !ctx->dev.rf || !ctx->dev.cell_ext) return fail(PMC_ERR_INVALID, "pmc_tune_rf_log_flush: this context has no logged radiation field");
    if (const char* problem = logProblem(keys, vals, nullptr, n)) return fail(PMC_ERR_INVALID, std::string("pmc_tune_rf_log_flush: ") + problem);
    HIP_TRY(hipSetDevice(ctx->device));
    CallBuffers B;
    DeviceLog L;
    hipError_t e = stageLog(B, ctx->stream, keys, vals, nullptr, n, int(plan.rfParts), L);
    if (e == hipSuccess) e = sceneUpToDate(ctx);
    if (e == hipSuccess)
        e = pmcLaunchRfFlush(ctx->slot, L.keys, L.vals, L.sortedKeys, L.sortedVals, (unsigned long long)n, int(plan.rfParts), L.temp, ctx->numCU, ctx->stream);
    const hipError_t done = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = done;
    if (e != hipSuccess) return hipFail(e, "pmc_tune_rf_log_flush");
    return PMC_OK;
}

extern "C" int pmc_tune_stat_log_flush(pmc_ctx* ctx, const uint32_t* keys, const double* vals, const uint32_t* fills, int64_t n, double* acc_out)
{
    if (!ctx || !acc_out) return fail(PMC_ERR_INVALID, "pmc_tune_stat_log_flush: invalid argument");
    const LogPlan plan = pmcLogPlan(ctx);
    if (!plan.statLogged || !ctx->dev.stat_acc) return fail(PMC_ERR_INVALID, "pmc_tune_stat_log_flush: this context has no logged statistics");
    if (const char* problem = logProblem(keys, vals, fills, n)) return fail(PMC_ERR_INVALID, std::string("pmc_tune_stat_log_flush: ") + problem);
    HIP_TRY(hipSetDevice(ctx->device));
    CallBuffers B;
    DeviceLog L;
    const size_t records = size_t(plan.statRecords);
    std::vector<double> acc(records * 8);  // (the accumulator's records are 64 bytes: five sums and three words that stay zero)
    hipError_t e = stageLog(B, ctx->stream, keys, vals, fills, n, int(plan.statParts), L);
    if (e == hipSuccess) e = sceneUpToDate(ctx);
    if (e == hipSuccess)
        e = pmcLaunchStatFlush(ctx->slot, L.keys, L.vals, L.sortedKeys, L.sortedVals, (unsigned long long)n, int(plan.statParts), L.temp, ctx->numCU, L.fills,
                               ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(acc.data(), ctx->dev.stat_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    // (the accumulator is empty between two segments; cleared also when something above has failed)
    const hipError_t cleared = hipMemsetAsync(ctx->dev.stat_acc, 0, acc.size() * sizeof(double), ctx->stream);
    const hipError_t done = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = cleared;
    if (e == hipSuccess) e = done;
    if (e != hipSuccess) return hipFail(e, "pmc_tune_stat_log_flush");
    for (size_t r = 0; r < records; ++r)
        for (int p = 0; p < 5; ++p) acc_out[r * 5 + p] = acc[r * 8 + p];
    return PMC_OK;
}

extern "C" int pmc_tune_cell_numbering(pmc_ctx* ctx, int32_t* ext_out)
{
    if (!ctx || !ext_out) return fail(PMC_ERR_INVALID, "pmc_tune_cell_numbering: invalid argument");
    if (!ctx->dev.cell_ext || ctx->dev.cell_slots <= 0) return fail(PMC_ERR_INVALID, "pmc_tune_cell_numbering: this grid has no device numbering");
    HIP_TRY(hipSetDevice(ctx->device));
    hipError_t e = hipMemcpyAsync(ext_out, ctx->dev.cell_ext, sizeof(int32_t) * size_t(ctx->dev.cell_slots), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hipFail(e, "pmc_tune_cell_numbering");
    return PMC_OK;
}
