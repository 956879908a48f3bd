// pmc_probe.hip -- the probe calls of include/pmc.h: the single-ray tracer (pmc_trace_ray), the batched ray integrals (pmc_integrate_rays,
// pmc_integrate_weighted_rays) and the point sampler (pmc_sample_cells).  Each runs kernels of pmc_ray.inc / pmc_locate.inc outside the photon
// loop, in the frame that pmc_context.h holds once: the scene up to date, the buffers and the event pair of the call, the cell records of a pass.
#include "pmc_context.h"

extern "C" int pmc_trace_ray(pmc_ctx* ctx, const double r[3], const double k[3], int32_t* m, double* ds, int32_t cap, int32_t* n)
{
    if (!ctx || !r || !k || !m || !ds || !n || cap < 0) return fail(PMC_ERR_INVALID, "invalid argument");
    HIP_TRY(hipSetDevice(ctx->device));
    // octree: the ray is traced with BOTH flavours of the step (direction in scalar registers as in the peel-off kernel,
    // in vector registers as in the propagation kernel); they must agree bit for bit
    const int flavours = ctx->dev.grid_kind == PMC_GRID_OCTREE ? 2 : 1;
    const size_t room = size_t(std::max(cap, 1));
    int32_t* dm = nullptr;
    double* dds = nullptr;
    int32_t* dn = nullptr;
    double* dk = nullptr;
    CallBuffers scratch;
    HIP_TRY(scratch.get(room * flavours, &dm));
    HIP_TRY(scratch.get(room * flavours, &dds));
    HIP_TRY(scratch.get(size_t(flavours), &dn));
    HIP_TRY(scratch.get(size_t(3), &dk));
    hipError_t e = hipMemcpy(dk, k, 3 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = sceneUpToDate(ctx);
    for (int f = 0; f < flavours && e == hipSuccess; ++f)
        e = pmcLaunchTrace(ctx->slot, ctx->dev.grid_kind, ctx->wide, f, r, k, dk, dm + f * room, dds + f * room, cap, dn + f, ctx->walkLds,
                           ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hipFail(e, "trace kernel");
    int32_t count[2] = {0, 0};
    hipMemcpy(count, dn, sizeof(int32_t) * flavours, hipMemcpyDeviceToHost);
    *n = count[0];
    const int32_t got = std::min(*n, cap);
    hipMemcpy(m, dm, sizeof(int32_t) * got, hipMemcpyDeviceToHost);
    hipMemcpy(ds, dds, sizeof(double) * got, hipMemcpyDeviceToHost);
    if (flavours == 2)
    {
        std::vector<int32_t> m2(got);
        std::vector<double> ds2(got);
        hipMemcpy(m2.data(), dm + room, sizeof(int32_t) * got, hipMemcpyDeviceToHost);
        hipMemcpy(ds2.data(), dds + room, sizeof(double) * got, hipMemcpyDeviceToHost);
        if (count[1] != count[0] || std::memcmp(m2.data(), m, sizeof(int32_t) * got) || std::memcmp(ds2.data(), ds, sizeof(double) * got))
            return fail(PMC_ERR_DEVICE, "octree traversal: the scalar-direction and vector-direction steps disagree on this ray");
    }
    return PMC_OK;
}

// pmc_integrate_rays (cell_weights == nullptr: sums [num_rays][num_values]) and pmc_integrate_weighted_rays (sums [num_rays][1 + num_values]: a pass
// carries the weight and PMC_INTEGRATE_PASS_VALUES - 1 values; the sum of the weights is the same in every pass and is taken from the first)
static int integrateRays(pmc_ctx* ctx, const std::string& name, int64_t num_rays, const double* origins, const double* directions, int32_t num_values,
                         const double* cell_weights, const double* cell_values, double* sums)
{
    const bool weighted = cell_weights != nullptr;
    if (num_rays < 0) return fail(PMC_ERR_INVALID, name + ": negative number of rays");
    if (num_values < 0) return fail(PMC_ERR_INVALID, name + ": negative number of values");
    if (num_rays > 0 && (!origins || !directions)) return fail(PMC_ERR_INVALID, name + ": null ray arrays");
    if (num_values > 0 && !cell_values) return fail(PMC_ERR_INVALID, name + ": null cell values");
    if (num_rays > 0 && (num_values > 0 || weighted) && !sums) return fail(PMC_ERR_INVALID, name + ": null result array");
    ctx->integrateMs = 0.f;
    ctx->integrateLaneSteps = ctx->integrateWaveSteps = 0;
    if (num_rays == 0 || (num_values == 0 && !weighted)) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(sceneUpToDate(ctx));
    const DevScene& D = ctx->dev;
    constexpr int W = CellRecords::W;
    CellRecords cells;
    if (int rc = cells.prepare(D, name, true)) return rc;
    const int64_t batchMax = PMC_INTEGRATE_BATCH_RAYS;
    const size_t batchRoom = size_t(std::min(num_rays, batchMax));
    CallBuffers scratch;
    double *dOrigins = nullptr, *dDirections = nullptr, *dQ = nullptr, *dSums = nullptr;
    unsigned long long* dWork = nullptr;
    const int workWords = pmcProbeWorkWords();
    HIP_TRY(scratch.get(3 * batchRoom, &dOrigins));
    HIP_TRY(scratch.get(3 * batchRoom, &dDirections));
    HIP_TRY(scratch.get(cells.slots * W, &dQ));
    HIP_TRY(scratch.get(W * batchRoom, &dSums));
    HIP_TRY(scratch.get(size_t(workWords), &dWork));
    EventPair timer;
    if (int rc = timer.create()) return rc;
    const int lead = weighted ? 1 : 0;                // members of a record (and of a ray's sums) in front of the caller's values
    const int perPass = W - lead;                     // caller's values per pass
    const size_t stride = size_t(lead + num_values);  // the caller's sums per ray
    const int numPasses = std::max((num_values + perPass - 1) / perPass, 1);
    // one record on the host, built when the pass changes: once per pass where the rays are one batch or the values one pass
    std::vector<double> q(cells.slots * W), part(W * batchRoom);
    int built = -1;
    std::vector<unsigned long long> work(workWords);
    unsigned long long capped = 0;
    hipError_t e = hipSuccess;
    for (int64_t first = 0; first < num_rays && e == hipSuccess; first += batchMax)
    {
        const size_t n = size_t(std::min(batchMax, num_rays - first));
        e = hipMemcpy(dOrigins, origins + 3 * first, 3 * n * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dDirections, directions + 3 * first, 3 * n * sizeof(double), hipMemcpyHostToDevice);
        const int grid = persistentGrid(ctx, n);
        for (int pass = 0; pass < numPasses && e == hipSuccess; ++pass)
        {
            const int v0 = pass * perPass, nv = std::min(perPass, num_values - v0);
            if (pass != built) cells.build(q.data(), pass, num_values, cell_weights, cell_values);
            built = pass;
            e = hipMemcpy(dQ, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemsetAsync(dWork, 0, workWords * sizeof(unsigned long long), ctx->stream);
            if (e == hipSuccess) e = timer.start(ctx->stream);
            if (e == hipSuccess)
                e = pmcLaunchIntegrate(ctx->slot, D.grid_kind, ctx->wide, lead, dOrigins, dDirections, dQ, dSums, n, dWork, grid, ctx->walkLds, ctx->stream);
            if (e == hipSuccess) e = timer.stop(ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e == hipSuccess) e = hipMemcpy(part.data(), dSums, W * n * sizeof(double), hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(work.data(), dWork, workWords * sizeof(unsigned long long), hipMemcpyDeviceToHost);
            if (e != hipSuccess) break;
            ctx->integrateMs += timer.elapsedMs();
            capped += work[1];
            ctx->integrateLaneSteps += work[2];
            ctx->integrateWaveSteps += work[3];
            for (size_t i = 0; i < n; ++i)
            {
                if (weighted && pass == 0) sums[(size_t(first) + i) * stride] = part[i * W];
                for (int j = 0; j < nv; ++j) sums[(size_t(first) + i) * stride + size_t(lead + v0 + j)] = part[i * W + lead + j];
            }
        }
    }
    if (e != hipSuccess) return hipFail(e, name.c_str());
    if (capped)
        return fail(PMC_ERR_DEVICE, name + ": " + std::to_string(capped) + " ray walk(s) were still inside the grid after " + std::to_string(PMC_RAY_STEP_CAP) + " cells (traversal error)");
    return PMC_OK;
}

extern "C" {

int pmc_integrate_rays(pmc_ctx* ctx, int64_t num_rays, const double* origins, const double* directions, int32_t num_values, const double* cell_values,
                       double* sums)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    return integrateRays(ctx, "pmc_integrate_rays", num_rays, origins, directions, num_values, nullptr, cell_values, sums);
}

int pmc_integrate_weighted_rays(pmc_ctx* ctx, int64_t num_rays, const double* origins, const double* directions, int32_t num_values,
                                const double* cell_weights, const double* cell_values, double* sums)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (!cell_weights) return fail(PMC_ERR_INVALID, "pmc_integrate_weighted_rays: null cell weights");
    return integrateRays(ctx, "pmc_integrate_weighted_rays", num_rays, origins, directions, num_values, cell_weights, cell_values, sums);
}

int pmc_last_integrate_work(pmc_ctx* ctx, float* kernel_ms, uint64_t* lane_steps, uint64_t* wave_steps)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (kernel_ms) *kernel_ms = ctx->integrateMs;
    if (lane_steps) *lane_steps = ctx->integrateLaneSteps;
    if (wave_steps) *wave_steps = ctx->integrateWaveSteps;
    return PMC_OK;
}

// the point sampler (pmc_locate.inc): the points go through the device in chunks of PMC_SAMPLE_CHUNK_POINTS, located once per chunk, the values
// gathered in passes of PMC_INTEGRATE_PASS_VALUES at the cells of the chunk.  Device memory of a call: 3 + PMC_INTEGRATE_PASS_VALUES doubles and two
// int32 per point of a chunk (64 MiB), and one pass of cell values
int pmc_sample_cells(pmc_ctx* ctx, int64_t num_points, const double* positions, int32_t num_values, const double* cell_values, double* values,
                     int32_t* cells)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (num_points < 0) return fail(PMC_ERR_INVALID, "pmc_sample_cells: negative number of points");
    if (num_values < 0) return fail(PMC_ERR_INVALID, "pmc_sample_cells: negative number of values");
    if (num_points > 0 && !positions) return fail(PMC_ERR_INVALID, "pmc_sample_cells: null positions");
    if (num_values > 0 && !cell_values) return fail(PMC_ERR_INVALID, "pmc_sample_cells: null cell values");
    if (num_points > 0 && num_values > 0 && !values) return fail(PMC_ERR_INVALID, "pmc_sample_cells: null result array");
    ctx->sampleMs = 0.f;
    for (size_t i = 0, n = 3 * size_t(num_points); i < n; ++i)
        if (!std::isfinite(positions[i]))
            return fail(PMC_ERR_INVALID, "pmc_sample_cells: coordinate " + std::to_string(i % 3) + " of point " + std::to_string(i / 3) + " is not finite");
    if (num_points == 0 || (num_values == 0 && !cells)) return PMC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(sceneUpToDate(ctx));
    const DevScene& D = ctx->dev;
    constexpr int W = CellRecords::W;
    CellRecords records;
    if (int rc = records.prepare(D, "pmc_sample_cells", num_values > 0)) return rc;
    const size_t slots = records.slots;
    const int64_t chunkMax = PMC_SAMPLE_CHUNK_POINTS;
    const size_t chunkRoom = size_t(std::min(num_points, chunkMax));
    CallBuffers scratch;
    double *dPositions = nullptr, *dQ = nullptr, *dValues = nullptr;
    int32_t *dWalkCells = nullptr, *dCells = nullptr;
    HIP_TRY(scratch.get(3 * chunkRoom, &dPositions));
    HIP_TRY(scratch.get(chunkRoom, &dWalkCells));
    HIP_TRY(scratch.get(chunkRoom, &dCells));
    if (num_values > 0)
    {
        HIP_TRY(scratch.get(slots * W, &dQ));
        HIP_TRY(scratch.get(W * chunkRoom, &dValues));
    }
    EventPair timer;
    if (int rc = timer.create()) return rc;
    const auto timed = [&](hipError_t launched) {
        hipError_t e = launched;
        if (e == hipSuccess) e = timer.stop(ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) ctx->sampleMs += timer.elapsedMs();
        return e;
    };
    const int numPasses = (num_values + W - 1) / W;
    const size_t numChunks = size_t((num_points + chunkMax - 1) / chunkMax);
    // the records of every pass, built once on the host; with one pass they are uploaded once, with several once per chunk and pass (the
    // located cells of a chunk stay on the device for its passes, which is what bounds the device memory)
    std::vector<double> q(size_t(numPasses) * slots * W), part(num_values > 0 ? W * chunkRoom : 0);
    for (int pass = 0; pass < numPasses; ++pass) records.build(q.data() + size_t(pass) * slots * W, pass, num_values, nullptr, cell_values);
    hipError_t e = hipSuccess;
    for (size_t chunk = 0; chunk < numChunks && e == hipSuccess; ++chunk)
    {
        const size_t first = chunk * size_t(chunkMax);
        const size_t n = std::min(size_t(chunkMax), size_t(num_points) - first);
        e = hipMemcpy(dPositions, positions + 3 * first, 3 * n * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = timer.start(ctx->stream);
        if (e == hipSuccess)
            e = timed(pmcLaunchLocateCells(ctx->slot, D.grid_kind, ctx->wide, dPositions, dWalkCells, dCells, n, persistentGrid(ctx, n), ctx->walkLds, ctx->stream));
        if (e == hipSuccess && cells) e = hipMemcpy(cells + first, dCells, n * sizeof(int32_t), hipMemcpyDeviceToHost);
        for (int pass = 0; pass < numPasses && e == hipSuccess; ++pass)
        {
            const int v0 = pass * W, nv = std::min(W, num_values - v0);
            if (chunk == 0 || numPasses > 1)
                e = hipMemcpy(dQ, q.data() + size_t(pass) * slots * W, slots * W * sizeof(double), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = timer.start(ctx->stream);
            if (e == hipSuccess) e = timed(pmcLaunchGatherCells(dWalkCells, dQ, dValues, n, nv, int((n + 255) / 256), ctx->stream));
            if (e == hipSuccess) e = hipMemcpy(part.data(), dValues, size_t(nv) * n * sizeof(double), hipMemcpyDeviceToHost);
            if (e != hipSuccess) break;
            for (int j = 0; j < nv; ++j) std::memcpy(values + size_t(v0 + j) * size_t(num_points) + first, part.data() + size_t(j) * n, n * sizeof(double));
        }
    }
    if (e != hipSuccess) return hipFail(e, "pmc_sample_cells");
    return PMC_OK;
}

int pmc_last_sample_ms(pmc_ctx* ctx, float* kernel_ms)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (kernel_ms) *kernel_ms = ctx->sampleMs;
    return PMC_OK;
}

}  // extern "C"
