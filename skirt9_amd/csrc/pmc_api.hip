// pmc_api.hip -- the extern "C" ABI of include/pmc.h: context life time (pmc_create: the context's resources, the tuning switches of scene
// creation, the device-side configuration -- LDS limits, launch geometry, slot count), frames, radiation field, counters.
// What pmc_create makes of the scene -- validation, DevScene, every table -- is the plain host code of
// pmc_scene_build.h and pmc_tables.h, which writes through the context as its TableSink; the generation loop (pmc_run_primary) lives in
// pmc_run.hip, the RCCL calls in pmc_comm.hip, the switch table of include/pmc_tuning.h in pmc_tuning.hip, the ray tracer, the ray
// integrator and the point sampler in pmc_probe.hip; pmc_context.h is what they share.
#include "pmc_context.h"
#include "pmc_scene_build.h"
#include <memory>

namespace
{
    thread_local std::string t_error;
    // constant-memory scene slots (pmc_kernels.hip c_scene): every device has its own copy of the symbol, so the table
    // of live contexts is per device; guarded, because contexts may be created from one host thread per GPU
    constexpr int MAX_DEVICES = 64;
    bool g_slotUsed[MAX_DEVICES][PMC_MAX_CONTEXTS] = {{false}};
    std::mutex g_slotMutex;
}

// error text of the calling thread, for the other translation units of the library (pmc_sampler.hip)
void pmcSetError(const std::string& message)
{
    t_error = message;
}


extern "C" {

int pmc_abi_version(void)
{
    return PMC_ABI_VERSION;
}

// what this binary was built with (the Makefile hands its HIPFLAGS over): results are bit-compatible with the reference only under
// -ffp-contract=off (the reference build has no fused multiply-add), and the detector atomics are hardware f64 adds
// only under -munsafe-fp-atomics
#define PMC_STRINGIFY2(x) #x
#define PMC_STRINGIFY(x) PMC_STRINGIFY2(x)
#ifndef PMC_BUILD_FLAGS
#define PMC_BUILD_FLAGS "unknown (not built by the Makefile)"
#endif
const char* pmc_build_info(void)
{
    return "libpmc ABI " PMC_STRINGIFY(PMC_ABI_VERSION) ", gfx950, " __VERSION__ ", flags: " PMC_BUILD_FLAGS
#if defined(__FP_FAST_FMA) || defined(__FAST_MATH__)
           " [fast-math macros defined]"
#endif
        ;
}

namespace
{
    // a * b + c with run-time operands: 0 when the product is rounded before the sum (-ffp-contract=off), -2^-60 when the compiler fused the two
    __global__ void contractionProbeKernel(double a, double b, double c, double* out) { out[0] = a * b + c; }

    // one launch per process and device, at the first pmc_create: a binary whose compiler contracted a * b + c computes other last bits than
    // the reference in every optical depth and exit distance, silently; it is refused instead
    int checkContraction(int device)
    {
        static std::mutex m;
        static bool checked[64] = {false};
        std::lock_guard<std::mutex> lock(m);
        if (device >= 0 && device < 64 && checked[device]) return PMC_OK;
        double* d = nullptr;
        double h = 1.;
        if (hipMalloc(&d, sizeof(double)) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipMalloc failed");
        hipLaunchKernelGGL(contractionProbeKernel, dim3(1), dim3(1), 0, 0, 1. + 0x1p-30, 1. - 0x1p-30, -1., d);
        const hipError_t e = hipMemcpy(&h, d, sizeof(double), hipMemcpyDeviceToHost);
        hipFree(d);
        if (e != hipSuccess) return hipFail(e, "contraction self-test");
        if (h != 0.)
            return fail(PMC_ERR_DEVICE, std::string("this libpmc.so was compiled with floating-point contraction (a * b + c fused): its results would differ from "
                                                    "the reference's in the last bits everywhere; rebuild with -ffp-contract=off.  ") + pmc_build_info());
        if (device >= 0 && device < 64) checked[device] = true;
        return PMC_OK;
    }
}

const char* pmc_last_error(void)
{
    return t_error.c_str();
}

int64_t pmc_frame_layout_of(const pmc_scene* scene, int32_t instrument, pmc_frame_layout* out)
{
    if (!scene) return fail(PMC_ERR_INVALID, "null scene");
    return pmc_layout_compute(scene, instrument, out);
}

void pmc_destroy(pmc_ctx* ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    for (int g = 0; g < PMC_MAX_GROUPS; ++g)
    {
        if (ctx->groupStream[g]) hipStreamSynchronize(ctx->groupStream[g]);
        if (ctx->peelStream[g]) hipStreamSynchronize(ctx->peelStream[g]);
    }
    for (void* p : ctx->allocations) hipFree(p);
    for (void* p : ctx->slotAllocations) hipFree(p);
    for (void* p : ctx->segmentAllocations) hipFree(p);
    if (ctx->readback) hipHostFree(ctx->readback);
    for (hipEvent_t e : {ctx->evStart, ctx->evStop})
        if (e) hipEventDestroy(e);
    for (int g = 0; g < PMC_MAX_GROUPS; ++g)
    {
        for (hipEvent_t e : {ctx->evA[g], ctx->evB[g], ctx->evC[g], ctx->evJoin[g], ctx->evProp[g]})
            if (e) hipEventDestroy(e);
        if (g > 0 && ctx->groupStream[g]) hipStreamDestroy(ctx->groupStream[g]);
        if (ctx->peelStream[g]) hipStreamDestroy(ctx->peelStream[g]);
    }
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    if (ctx->slot >= 0)
    {
        std::lock_guard<std::mutex> lock(g_slotMutex);
        g_slotUsed[ctx->device][ctx->slot] = false;
    }
    delete ctx;
}

}  // extern "C"

// ---- pmc_create: checkScene | context resources | the tables of pmc_scene_build.h, with the context as their sink | device-side configuration
namespace
{
    // the switches that scene creation reads (SceneSwitches, pmc_tables.h), once
    SceneSwitches readSceneSwitches()
    {
        SceneSwitches sw;
        sw.treeAsBinTree = pmcTune("PMC_TREE_AS_BINTREE") != nullptr;
        sw.noMono = pmcTune("PMC_NO_MONO") != nullptr;
        sw.propNoCheckpoints = pmcTune("PMC_PROP_NO_CHECKPOINTS") != nullptr;
        sw.voroNoPeelKernel = pmcTune("PMC_VORO_NO_PEEL_KERNEL") != nullptr;
        sw.voroNoDeferredScan = pmcTune("PMC_VORO_NO_DEFERRED_SCAN") != nullptr;
        sw.voroNoCull = pmcTune("PMC_VORO_NO_CULL") != nullptr;
        sw.voroNoPropKernel = pmcTune("PMC_VORO_NO_PROP_KERNEL") != nullptr;
        sw.voroNoConeTables = pmcTune("PMC_VORO_NO_CONE_TABLES") != nullptr;
        sw.voroNoObserverLists = pmcTune("PMC_VORO_NO_OBSERVER_LISTS") != nullptr;
        sw.voroConeCullOnly = pmcTune("PMC_VORO_CONE_CULL_ONLY") != nullptr;
        // (cells with more entries than a link can name say so in their header; the switch lowers the limit: a test of that path)
        if (const char* v = pmcTune("PMC_VORO_LINK_COUNT_MAX")) sw.voroLinkCountMax = std::min<uint32_t>(sw.voroLinkCountMax, (uint32_t)std::max(0, atoi(v)));
        if (const char* v = pmcTune("PMC_CELL_ORDER")) sw.cellOrderRef = !strcmp(v, "ref");
        if (const char* v = pmcTune("PMC_CELL_SHUFFLE")) sw.cellShuffle = atoi(v);
        if (const char* v = pmcTune("PMC_WALK_BLOCKS_PER_CU")) sw.walkBlocksPerCU = std::max(1, atoi(v));
        if (const char* v = pmcTune("PMC_PEEL_BLOCKS_PER_CU")) sw.peelBlocksPerCU = std::max(1, atoi(v));
        return sw;
    }

    struct DestroyContext
    {
        void operator()(pmc_ctx* ctx) const { pmc_destroy(ctx); }
    };
    using ContextPtr = std::unique_ptr<pmc_ctx, DestroyContext>;

    // a context on `device` with its slot in the per-device table, streams, events and pinned readback
    int makeContext(int device, ContextPtr& made)
    {
        if (device >= MAX_DEVICES) return fail(PMC_ERR_UNSUPPORTED, "device index beyond the context table");
        ContextPtr ctx(new pmc_ctx());
        ctx->device = device;
        {
            std::lock_guard<std::mutex> lock(g_slotMutex);
            for (int sl = 0; sl < PMC_MAX_CONTEXTS && ctx->slot < 0; ++sl)
                if (!g_slotUsed[device][sl])
                {
                    g_slotUsed[device][sl] = true;
                    ctx->slot = sl;
                }
        }
        if (ctx->slot < 0) return fail(PMC_ERR_NOMEM, "too many live pmc contexts (at most " + std::to_string(PMC_MAX_CONTEXTS) + ")");
        auto makeStream = [](hipStream_t* out) { return hipStreamCreateWithPriority(out, hipStreamDefault, 0); };
        if (makeStream(&ctx->stream) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipStreamCreate failed");
        ctx->groupStream[0] = ctx->stream;
        for (int g = 1; g < PMC_MAX_GROUPS; ++g)
            if (makeStream(&ctx->groupStream[g]) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipStreamCreate failed");
        for (int g = 0; g < PMC_MAX_GROUPS; ++g)
            if (makeStream(&ctx->peelStream[g]) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipStreamCreate failed");
        for (hipEvent_t* ev : {&ctx->evStart, &ctx->evStop})
            if (hipEventCreate(ev) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipEventCreate failed");
        for (int g = 0; g < PMC_MAX_GROUPS; ++g)
            for (hipEvent_t* ev : {&ctx->evA[g], &ctx->evB[g], &ctx->evC[g], &ctx->evJoin[g], &ctx->evProp[g]})
                if (hipEventCreate(ev) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipEventCreate failed");
        if (const char* env = getenv("PMC_NUM_GROUPS"))
        {
            ctx->numGroups = std::min(PMC_MAX_GROUPS, std::max(1, atoi(env)));
            ctx->groupsConfigured = true;  // (an explicit setting: also a Voronoi scene runs with it)
        }
        if (hipHostMalloc(reinterpret_cast<void**>(&ctx->readback), PMC_MAX_GROUPS * sizeof(GroupReadback)) != hipSuccess)
            return fail(PMC_ERR_DEVICE, "hipHostMalloc failed");
        made = std::move(ctx);
        return PMC_OK;
    }

    // what the device decides: the kernels' LDS limits, the launch geometry of the persistent walk kernels, the number of packet slots
    int configureDevice(pmc_ctx* ctx, const SceneSwitches& sw)
    {
        const DevScene& D = ctx->dev;
        if (pmcConfigureKernels(ctx->walkLds, ctx->launchLds) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipFuncSetAttribute failed");
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return fail(PMC_ERR_DEVICE, "hipGetDeviceProperties failed");
        ctx->numCU = prop.multiProcessorCount;
        ctx->block = 256;
        ctx->wide = D.grid_kind == PMC_GRID_OCTREE && D.lmax > 10;
        // persistent walk kernels: as many workgroups as stay resident (the transition / launch kernels of the other
        // slot group get the CUs between generations)
        int perCU = pmcWalkBlocksPerCU(D.grid_kind, D.grid_kind == PMC_GRID_OCTREE ? 2 : 0, ctx->wide,
                                       D.grid_kind == PMC_GRID_OCTREE ? pmcPropBlock() : ctx->block, ctx->walkLds);
        if (perCU < 1) perCU = 1;
        // (octree propagation kernel: ONE workgroup of 256 lanes per CU.  The walk kernels are bound by the memory system's
        // rate of random gathers, which falls when too many of them are in flight -- 32 MB table, 8 / 16 / 32 waves per CU:
        // 1.9 / 0.94 / 0.83e11 records/s, profiles/microbench/gather_modes_mi355x.txt -- and the kernels of three slot groups
        // overlap; 1 / 2 / 3 per CU: 697 / 720 / 756 ms per 1e8 packets)
        if (sw.walkBlocksPerCU) perCU = std::min(perCU, sw.walkBlocksPerCU);  // tuning aid
        else perCU = std::min(perCU, D.grid_kind == PMC_GRID_OCTREE ? 1 : 3);
        ctx->grid = ctx->numCU * perCU;
        if (D.grid_kind == PMC_GRID_OCTREE)
        {
            int peelPerCU = pmcWalkBlocksPerCU(D.grid_kind, 1, ctx->wide, pmcPeelBlock(), ctx->walkLds);
            // (one workgroup of 512 lanes per CU: with the pipelined step more resident waves only queue up in the memory
            // system -- 1 / 2 / 3 per CU: 97 / 111 / 124 ms per 5e7 packets, profiles/README.md)
            peelPerCU = std::min(std::max(peelPerCU, 1), 1);
            if (sw.peelBlocksPerCU) peelPerCU = sw.peelBlocksPerCU;
            ctx->peelGrid = ctx->numCU * peelPerCU;
        }
        // packet slots: 24 Mi histories in flight (about 1.7 KB of state per slot with one statistics-recording instrument: 40 GB of the 288).  A
        // segment of 1e8 packets then runs 83 generations instead of the 177 of 8 Mi slots -- fewer launches, fewer ragged kernel tails -- and gains
        // 3-7 % (8 / 12 / 16 / 24 / 32 Mi: 2.00 / 2.05 / 2.05 / 2.07 / 2.07e8 packets/s, profiles/sweeps/r05_d3_slots.txt)
        ctx->numSlots = 24 * 1024 * 1024;
        if (const char* env = getenv("PMC_NUM_SLOTS"))
        {
            ctx->numSlots = std::max<int64_t>(1024, atoll(env));
            ctx->slotsConfigured = true;
        }
        return PMC_OK;
    }
}

extern "C" {

int pmc_create(const pmc_scene* scene, int32_t device, pmc_ctx** out)
{
    return pmc_create_ext(scene, nullptr, device, out);
}

int pmc_create_ext(const pmc_scene* scene, const pmc_scene_ext* ext, int32_t device, pmc_ctx** out)
{
    if (!scene || !out) return fail(PMC_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc = PMC_OK;
    SceneExtension extension;
    if ((rc = checkScene(*scene, ext, extension))) return rc;
    if (pmcExperimentBuild())
    {
        static std::atomic<bool> said{false};
        if (!said.exchange(true)) fprintf(stderr, "libpmc: this library was built with an ablation / perturbation macro (a tuning experiment): its results are NOT those of the engine\n");
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
        return fail(PMC_ERR_DEVICE, "no HIP device available: the MI355X engine cannot run (there is no CPU fallback)");
    if (device < 0 || device >= count) return fail(PMC_ERR_INVALID, "invalid device index");
    HIP_TRY(hipSetDevice(device));
    if ((rc = checkContraction(device))) return rc;

    ContextPtr ctx;  // (destroyed with everything it holds by then, unless it is handed out)
    if ((rc = makeContext(device, ctx))) return rc;
    const SceneSwitches switches = readSceneSwitches();
    SceneTables tables;
    if ((rc = buildSceneTables(*scene, extension, switches, *ctx, ctx->dev, tables))) return rc;
    ctx->frameSize = tables.frameSize;
    ctx->rfSize = tables.rfSize;
    ctx->frames = ctx->dev.frames;
    ctx->walkLds = tables.lds.walkBytes, ctx->transitionLds = tables.lds.transitionBytes, ctx->launchLds = tables.lds.launchBytes;
    if ((rc = configureDevice(ctx.get(), switches))) return rc;
    *out = ctx.release();
    return PMC_OK;
}

int pmc_set_launch(pmc_ctx* ctx, int32_t block, int32_t grid)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (block > 0)
    {
        if (block % 64 || block > 256) return fail(PMC_ERR_INVALID, "block must be a multiple of 64 and at most 256");
        ctx->block = block;
    }
    if (grid > 0) ctx->grid = grid;
    return PMC_OK;
}

int pmc_set_num_slots(pmc_ctx* ctx, int64_t num_slots)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (num_slots < 1 || num_slots > (int64_t(1) << 30)) return fail(PMC_ERR_INVALID, "num_slots out of range");
    ctx->numSlots = num_slots;
    ctx->slotsConfigured = true;
    return PMC_OK;
}

int pmc_bind_frames(pmc_ctx* ctx, double* device_ptr, int64_t num_doubles)
{
    if (!ctx || !device_ptr) return fail(PMC_ERR_INVALID, "null argument");
    if (num_doubles != ctx->frameSize) return fail(PMC_ERR_INVALID, "frame buffer size mismatch");
    ctx->frames = device_ptr;
    ctx->dev.frames = device_ptr;
    ctx->sceneDirty = true;
    return PMC_OK;
}

int pmc_clear_frames(pmc_ctx* ctx)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->frames, 0, size_t(ctx->frameSize) * sizeof(double), ctx->stream));
    return PMC_OK;
}

int pmc_set_progress(pmc_ctx* ctx, pmc_progress_fn report, void* user, double interval_seconds)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    ctx->progress = report;
    ctx->progressUser = user;
    ctx->progressInterval = interval_seconds > 0. ? interval_seconds : 0.;
    return PMC_OK;
}

int pmc_sync(pmc_ctx* ctx)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PMC_OK;
}

int pmc_last_kernel_ms(pmc_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return fail(PMC_ERR_INVALID, "null argument");
    if (!ctx->timed) return fail(PMC_ERR_INVALID, "no segment has been run yet");
    *ms = ctx->walkMs;
    return PMC_OK;
}

int pmc_last_timing(pmc_ctx* ctx, float* total_ms, float* walk_ms, float* transition_ms, int32_t* generations)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null argument");
    if (!ctx->timed) return fail(PMC_ERR_INVALID, "no segment has been run yet");
    if (total_ms) *total_ms = ctx->totalMs;
    if (walk_ms) *walk_ms = ctx->walkMs;
    if (transition_ms) *transition_ms = ctx->transitionMs;
    if (generations) *generations = ctx->generations;
    return PMC_OK;
}

int pmc_last_walk_timing(pmc_ctx* ctx, float* peel_ms, float* prop_ms)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null argument");
    if (!ctx->timed) return fail(PMC_ERR_INVALID, "no segment has been run yet");
    if (peel_ms) *peel_ms = ctx->peelMs;
    if (prop_ms) *prop_ms = ctx->propMs;
    return PMC_OK;
}

int pmc_walk_work(pmc_ctx* ctx, pmc_walk_work_values* out)
{
    if (!ctx || !out) return fail(PMC_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    unsigned long long host[6];
    HIP_TRY(hipMemcpy(host, ctx->dev.counters + PMC_CTR_WALKWORK, sizeof(host), hipMemcpyDeviceToHost));
    out->peel_wave_steps = host[0], out->peel_lane_steps = host[1], out->peel_rounds = host[2];
    out->prop_wave_steps = host[3], out->prop_lane_steps = host[4], out->prop_rounds = host[5];
    return PMC_OK;
}

int pmc_debug_tables(pmc_ctx* ctx, pmc_debug_table_values* out)
{
    if (!ctx || !out) return fail(PMC_ERR_INVALID, "null argument");
    if (ctx->dev.grid_kind != PMC_GRID_OCTREE) return fail(PMC_ERR_INVALID, "not an octree scene");
    out->cell_table = ctx->dev.cell_tab;
    out->cell_slots = ctx->dev.cell_slots;
    out->loose_base = ctx->dev.cell_slots;
    out->task_cell = ctx->dev.tasks.cell;
    out->num_slots = ctx->allocatedSlots;
    return PMC_OK;
}

int pmc_download(pmc_ctx* ctx, double* host_frames, int64_t num_doubles)
{
    if (!ctx || !host_frames) return fail(PMC_ERR_INVALID, "null argument");
    if (num_doubles != ctx->frameSize) return fail(PMC_ERR_INVALID, "frame buffer size mismatch");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(host_frames, ctx->frames, size_t(num_doubles) * sizeof(double), hipMemcpyDeviceToHost));
    return PMC_OK;
}

double* pmc_frames_device(pmc_ctx* ctx)
{
    return ctx ? ctx->frames : nullptr;
}

int64_t pmc_frames_size(pmc_ctx* ctx)
{
    return ctx ? ctx->frameSize : 0;
}

int64_t pmc_radiation_field_size(pmc_ctx* ctx)
{
    return ctx ? ctx->rfSize : 0;
}

double* pmc_radiation_field_device(pmc_ctx* ctx)
{
    return ctx ? ctx->dev.rf : nullptr;
}

int pmc_bind_radiation_field(pmc_ctx* ctx, double* device_ptr, int64_t num_doubles)
{
    if (!ctx || !device_ptr) return fail(PMC_ERR_INVALID, "null argument");
    if (!ctx->rfSize) return fail(PMC_ERR_INVALID, "the scene does not store the radiation field");
    if (num_doubles != ctx->rfSize) return fail(PMC_ERR_INVALID, "radiation field size mismatch");
    ctx->dev.rf = device_ptr;
    ctx->sceneDirty = true;
    return PMC_OK;
}

int pmc_download_radiation_field(pmc_ctx* ctx, double* host_rf, int64_t num_doubles)
{
    if (!ctx || !host_rf) return fail(PMC_ERR_INVALID, "null argument");
    if (!ctx->rfSize) return fail(PMC_ERR_INVALID, "the scene does not store the radiation field");
    if (num_doubles != ctx->rfSize) return fail(PMC_ERR_INVALID, "radiation field size mismatch");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(host_rf, ctx->dev.rf, size_t(num_doubles) * sizeof(double), hipMemcpyDeviceToHost));
    return PMC_OK;
}

int pmc_clear_radiation_field(pmc_ctx* ctx)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (!ctx->rfSize) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->dev.rf, 0, size_t(ctx->rfSize) * sizeof(double), ctx->stream));
    return PMC_OK;
}

int pmc_counters(pmc_ctx* ctx, pmc_counter_values* out)
{
    if (!ctx || !out) return fail(PMC_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    unsigned long long host[PMC_NUM_COUNTERS];
    HIP_TRY(hipMemcpy(host, ctx->dev.counters, sizeof(host), hipMemcpyDeviceToHost));
    out->histories = host[0];
    out->paths = host[1];
    out->cell_visits = host[2];
    out->detector_updates = host[3];
    out->scatterings = host[4];
    out->stat_overflows = host[5];
    out->rewalk_visits = host[6];
    if (pmcTune("PMC_PROFILE_DUMP"))
    {
        // work counters of the octree walk kernels: lane utilisation = lane_steps / (64 wave_steps)
        const unsigned long long* w = host + PMC_CTR_WALKWORK;
        fprintf(stderr, "PMC_PROFILE peel: wave_steps %llu lane_steps %llu (%.1f %% of the lanes) service_rounds %llu\n", w[0], w[1],
                w[0] ? 100. * double(w[1]) / (64. * double(w[0])) : 0., w[2]);
        fprintf(stderr, "PMC_PROFILE prop: wave_steps %llu lane_steps %llu (%.1f %% of the lanes) service_rounds %llu\n", w[3], w[4],
                w[3] ? 100. * double(w[4]) / (64. * double(w[3])) : 0., w[5]);
    }
#ifdef PMC_PROFILE
    if (pmcTune("PMC_PROFILE_DUMP"))
    {
        for (int k = 0; k < 2; ++k)
        {
            const unsigned long long* t = host + 208 + 8 * k;
            fprintf(stderr, "PMC_PROFILE %s phases (wave cycles): gather %llu tau+position %llu descent %llu walls %llu inside+exit %llu "
                            "service-finish+claim %llu service-loads %llu loop %llu\n", k ? "prop" : "peel", t[0], t[1], t[2], t[3], t[4], t[5],
                    t[6], t[7]);
        }
        for (int k = 0; k < 2; ++k)
        {
            const unsigned long long* c = host + 224 + 8 * k;
            fprintf(stderr, "PMC_PROFILE %s census (lane events): literal-algorithm steps %llu, edge %llu, descents %llu over %llu levels, octet links %llu, "
                            "hit %llu, exit %llu\n", k ? "prop" : "peel", c[0], c[2], c[3], c[4], c[5], c[6], c[7]);
        }
        fprintf(stderr, "PMC_PROFILE transition (wave cycles): stage %llu mode-load %llu cycle-tail %llu append %llu loads+detect %llu scatter %llu start-cycle %llu flush %llu\n",
                host[192], host[193], host[194], host[195], host[196], host[197], host[198], host[199]);
        fprintf(stderr, "PMC_PROFILE launch (wave cycles): stage %llu list %llu stats-flush %llu start-cycle %llu draw+sample %llu - %llu flush %llu\n",
                host[200], host[201], host[202], host[203], host[204], host[205], host[206]);
    }
#endif
    return PMC_OK;
}

int pmc_reset_counters(pmc_ctx* ctx)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->dev.counters, 0, PMC_NUM_COUNTERS * sizeof(unsigned long long), ctx->stream));
    ctx->overflowsSeen = 0;
    ctx->internalErrorsSeen = 0;
    return PMC_OK;
}

}  // extern "C"
