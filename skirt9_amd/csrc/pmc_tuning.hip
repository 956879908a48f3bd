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
    hipError_t e = sceneUpToDate(ctx);
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

// ---- test aids of the scalar device functions (include/pmc_tuning.h): one lane per host-supplied argument tuple
namespace
{
    constexpr int64_t PRIMITIVE_MAX_TUPLES = int64_t(1) << 20;

    // doubles per argument tuple and per result of every PMC_FN_*
    const int DEVICE_FUNCTION_WIDTHS[PMC_FN_COUNT][2] = {{2, 1}, {2, 1}, {2, 1}, {2, 2}, {1, 1}, {2, 3}, {5, 3}, {1, 1}, {2, 1}, {5, 1}, {4, 1}, {2, 1}, {7, 1}};

    // what is wrong with the tuple count and the buffers of an aid, or null
    const char* tupleProblem(int64_t n, const void* in, const void* out)
    {
        if (n < 0 || n > PRIMITIVE_MAX_TUPLES) return "between 0 and 2^20 tuples";
        if (n > 0 && (!in || !out)) return "null buffer";
        return nullptr;
    }

    // `count` elements of a result brought to the host after everything enqueued on the context's stream
    template<typename T> hipError_t fetch(pmc_ctx* ctx, hipError_t e, T* host, const T* device, size_t count)
    {
        if (e == hipSuccess) e = hipMemcpyAsync(host, device, sizeof(T) * count, hipMemcpyDeviceToHost, ctx->stream);
        return e;
    }
    hipError_t finish(pmc_ctx* ctx, hipError_t e)
    {
        const hipError_t done = hipStreamSynchronize(ctx->stream);  // (whatever was enqueued has finished before the buffers go)
        return e == hipSuccess ? done : e;
    }
}

extern "C" int pmc_tune_device_function_widths(int32_t function, int32_t* width_in, int32_t* width_out)
{
    if (function < 0 || function >= PMC_FN_COUNT || !width_in || !width_out)
        return fail(PMC_ERR_INVALID, "pmc_tune_device_function_widths: unknown function " + std::to_string(function) + ", or a null pointer");
    *width_in = DEVICE_FUNCTION_WIDTHS[function][0];
    *width_out = DEVICE_FUNCTION_WIDTHS[function][1];
    return PMC_OK;
}

extern "C" int pmc_tune_device_function(pmc_ctx* ctx, int32_t function, const double* args, int64_t n, double* out)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "pmc_tune_device_function: no context");
    if (function < 0 || function >= PMC_FN_COUNT) return fail(PMC_ERR_INVALID, "pmc_tune_device_function: unknown function " + std::to_string(function));
    if (const char* problem = tupleProblem(n, args, out)) return fail(PMC_ERR_INVALID, std::string("pmc_tune_device_function: ") + problem);
    if (n == 0) return PMC_OK;
    const int widthIn = DEVICE_FUNCTION_WIDTHS[function][0], widthOut = DEVICE_FUNCTION_WIDTHS[function][1];
    HIP_TRY(hipSetDevice(ctx->device));
    CallBuffers B;
    double *dArgs = nullptr, *dOut = nullptr;
    hipError_t e = B.get(size_t(n) * widthIn, &dArgs, args);
    if (e == hipSuccess) e = B.get(size_t(n) * widthOut, &dOut);
    if (e == hipSuccess) e = sceneUpToDate(ctx);
    if (e == hipSuccess) e = pmcLaunchDeviceFunction(ctx->slot, function, dArgs, widthIn, n, dOut, widthOut, ctx->stream);
    e = finish(ctx, fetch(ctx, e, out, dOut, size_t(n) * widthOut));
    if (e != hipSuccess) return hipFail(e, "pmc_tune_device_function");
    return PMC_OK;
}

extern "C" int pmc_tune_locate(pmc_ctx* ctx, int32_t kind, const double* nodes, int32_t num_nodes, const double* x, int64_t n, int32_t* index_out)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "pmc_tune_locate: no context");
    if (kind < 0 || kind > 2) return fail(PMC_ERR_INVALID, "pmc_tune_locate: unknown kind " + std::to_string(kind));
    if (!nodes || num_nodes < 2) return fail(PMC_ERR_INVALID, "pmc_tune_locate: a table has at least 2 nodes");
    if (const char* problem = tupleProblem(n, x, index_out)) return fail(PMC_ERR_INVALID, std::string("pmc_tune_locate: ") + problem);
    if (n == 0) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallBuffers B;
    double *dNodes = nullptr, *dX = nullptr;
    int32_t* dOut = nullptr;
    hipError_t e = B.get(size_t(num_nodes), &dNodes, nodes);
    if (e == hipSuccess) e = B.get(size_t(n), &dX, x);
    if (e == hipSuccess) e = B.get(size_t(n), &dOut);
    if (e == hipSuccess) e = pmcLaunchLocate(kind, dNodes, num_nodes, dX, n, dOut, ctx->stream);
    e = finish(ctx, fetch(ctx, e, index_out, dOut, size_t(n)));
    if (e != hipSuccess) return hipFail(e, "pmc_tune_locate");
    return PMC_OK;
}

extern "C" int pmc_tune_instrument(pmc_ctx* ctx, int32_t instrument, pmc_instrument_values* out, double* border, int32_t* ellv)
{
    if (!ctx || !out) return fail(PMC_ERR_INVALID, "pmc_tune_instrument: invalid argument");
    if (instrument < 0 || instrument >= ctx->dev.num_instruments) return fail(PMC_ERR_INVALID, "pmc_tune_instrument: no such instrument");
    const DevInstrument& I = ctx->dev.inst[instrument];
    out->costheta = I.costheta, out->sintheta = I.sintheta, out->cosphi = I.cosphi, out->sinphi = I.sinphi, out->cosomega = I.cosomega, out->sinomega = I.sinomega;
    out->xpmin = I.xpmin, out->xpsiz = I.xpsiz, out->ypmin = I.ypmin, out->ypsiz = I.ypsiz;
    out->aperture_r2 = I.aperture_r2, out->zp1 = I.zp1;
    out->nxp = I.nxp, out->nyp = I.nyp, out->num_border = I.num_border, out->num_lambda = I.num_lambda;
    out->include_sed = I.include_sed, out->include_ifu = I.include_ifu;
    if (!border && !ellv) return PMC_OK;
    if (!I.border || !I.ellv || I.num_border < 0) return fail(PMC_ERR_INVALID, "pmc_tune_instrument: the instrument has no wavelength grid on the device");
    HIP_TRY(hipSetDevice(ctx->device));
    hipError_t e = hipSuccess;
    if (border && I.num_border > 0) e = fetch(ctx, e, border, I.border, size_t(I.num_border));
    if (ellv) e = fetch(ctx, e, ellv, I.ellv, size_t(I.num_border) + 1);
    e = finish(ctx, e);
    if (e != hipSuccess) return hipFail(e, "pmc_tune_instrument");
    return PMC_OK;
}

extern "C" int pmc_tune_detector(pmc_ctx* ctx, int32_t instrument, const double* r, int64_t n, int32_t* pixel_out, int32_t* inside_out)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "pmc_tune_detector: no context");
    if (instrument < 0 || instrument >= ctx->dev.num_instruments) return fail(PMC_ERR_INVALID, "pmc_tune_detector: no such instrument");
    if (const char* problem = tupleProblem(n, r, pixel_out)) return fail(PMC_ERR_INVALID, std::string("pmc_tune_detector: ") + problem);
    if (n > 0 && !inside_out) return fail(PMC_ERR_INVALID, "pmc_tune_detector: null buffer");
    if (n == 0) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallBuffers B;
    double* dR = nullptr;
    int32_t *dPixel = nullptr, *dInside = nullptr;
    hipError_t e = B.get(size_t(3 * n), &dR, r);
    if (e == hipSuccess) e = B.get(size_t(n), &dPixel);
    if (e == hipSuccess) e = B.get(size_t(n), &dInside);
    if (e == hipSuccess) e = sceneUpToDate(ctx);
    if (e == hipSuccess) e = pmcLaunchDetector(ctx->slot, instrument, dR, n, dPixel, dInside, ctx->stream);
    e = fetch(ctx, e, pixel_out, dPixel, size_t(n));
    e = finish(ctx, fetch(ctx, e, inside_out, dInside, size_t(n)));
    if (e != hipSuccess) return hipFail(e, "pmc_tune_detector");
    return PMC_OK;
}

extern "C" int pmc_tune_wavelength_bins(pmc_ctx* ctx, int32_t instrument, const double* lambda, int64_t n, int32_t* ell_out)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "pmc_tune_wavelength_bins: no context");
    if (instrument < 0 || instrument >= ctx->dev.num_instruments) return fail(PMC_ERR_INVALID, "pmc_tune_wavelength_bins: no such instrument");
    const DevInstrument& I = ctx->dev.inst[instrument];
    if (!I.ellv || I.num_border < 0 || (I.num_border > 0 && !I.border))
        return fail(PMC_ERR_INVALID, "pmc_tune_wavelength_bins: the instrument has no wavelength grid on the device");
    if (const char* problem = tupleProblem(n, lambda, ell_out)) return fail(PMC_ERR_INVALID, std::string("pmc_tune_wavelength_bins: ") + problem);
    if (n == 0) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallBuffers B;
    double* dLambda = nullptr;
    int32_t* dEll = nullptr;
    hipError_t e = B.get(size_t(n), &dLambda, lambda);
    if (e == hipSuccess) e = B.get(size_t(n), &dEll);
    if (e == hipSuccess) e = sceneUpToDate(ctx);
    if (e == hipSuccess) e = pmcLaunchWavelengthBins(ctx->slot, instrument, dLambda, n, dEll, ctx->stream);
    e = finish(ctx, fetch(ctx, e, ell_out, dEll, size_t(n)));
    if (e != hipSuccess) return hipFail(e, "pmc_tune_wavelength_bins");
    return PMC_OK;
}

extern "C" int pmc_tune_angular_probabilities(pmc_ctx* ctx, int32_t source, const double* k, int64_t n, double* p_out, int32_t* kind_out, double* axis_out,
                                              double* cos_delta_out)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "pmc_tune_angular_probabilities: no context");
    if (source < 0 || source >= ctx->dev.num_sources) return fail(PMC_ERR_INVALID, "pmc_tune_angular_probabilities: no such source");
    const DevSource& Q = ctx->dev.src[source];
    if (Q.angular_kind != PMC_ANGULAR_LASER && Q.angular_kind != PMC_ANGULAR_CONICAL && Q.angular_kind != PMC_ANGULAR_NETZER)
        return fail(PMC_ERR_INVALID, "pmc_tune_angular_probabilities: the source emits isotropically");
    if (const char* problem = tupleProblem(n, k, p_out)) return fail(PMC_ERR_INVALID, std::string("pmc_tune_angular_probabilities: ") + problem);
    if (kind_out) *kind_out = Q.angular_kind;
    for (int a = 0; axis_out && a < 3; ++a) axis_out[a] = Q.angular_axis[a];
    if (cos_delta_out) *cos_delta_out = Q.angular_cos_delta;
    if (n == 0) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallBuffers B;
    double *dK = nullptr, *dP = nullptr;
    hipError_t e = B.get(size_t(3 * n), &dK, k);
    if (e == hipSuccess) e = B.get(size_t(n), &dP);
    if (e == hipSuccess) e = sceneUpToDate(ctx);
    if (e == hipSuccess) e = pmcLaunchAngularProbabilities(ctx->slot, source, dK, n, dP, ctx->stream);
    e = finish(ctx, fetch(ctx, e, p_out, dP, size_t(n)));
    if (e != hipSuccess) return hipFail(e, "pmc_tune_angular_probabilities");
    return PMC_OK;
}
