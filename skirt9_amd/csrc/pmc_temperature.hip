// pmc_temperature.hip -- dust temperatures from the stored radiation field (pmc_dust_temperatures): the energy balance of every cell and dust
// component, EquilibriumDustEmissionCalculator::equilibriumTemperature (EquilibriumDustEmissionCalculator.cpp:120-130) over
// MediumSystem::meanIntensity (MediumSystem.cpp:1370-1380), and the mass-weighted mean of MediumSystem::indicativeTemperature (:1401-1427).
//
// The table rf[m * num_lambda + ell] lies in device memory, a cell's row contiguous.  A lane per cell that walked its own row would read at a
// stride of 8 * num_lambda bytes; instead a workgroup stages the rows of its 256 cells through LDS in tiles of up to TEMP_TILE = 8 bins, and
// every lane then adds up its own row.  What the staging loads look like: rows of up to 8 bins are staged whole -- the 256 rows are ONE
// contiguous block and consecutive lanes read consecutive addresses --; of longer rows a tile takes a run of 8 bins (64 bytes) per row, the
// runs 8 * num_lambda bytes apart, so a wave's load touches eight 64-byte segments (half lines, the other half of which the next tile takes).
// With this tile the kernel moves 2.1 TB/s at 50 bins and 1.9 TB/s at 6 (profiles/sweeps/dust_temperature.md); a wider tile, which would
// ask for whole lines at more LDS, has not been tried.  The order of the sum is the
// reference's -- from the last bin down to the first, the way the valarray expression is summed -- and no sum is shared between lanes, so
// the result is the host's (skh_dust_temperatures) bit for bit.  The small tables (bin widths, cross sections, Planck-integrated absorption
// and the temperature grid, about 8 KB per component) are kept in LDS.
#include "pmc_context.h"

namespace
{
    constexpr int TEMP_BLOCK = 256;  // cells of a workgroup
    constexpr int TEMP_TILE = 8;     // bins of a staged tile (rows padded to TEMP_TILE + 1 doubles in LDS)

    struct TempArgs
    {
        const double* rf;           // [numCells][numLambda]
        const double* width;        // [numLambda]
        const double* sigma;        // [H][numLambda]
        const double* planckabs;    // [H][numT]
        const double* temperature;  // [numT]
        const double* cellFactor;   // [numCells]
        const double* rho;          // [H][numCells]
        double* out;                // [H + 1][numCells]
        int numCells, numLambda, numT, H;
    };

    size_t tempLdsBytes(int H, int L, int NT)
    {
        return (size_t(L) + size_t(H) * L + size_t(H) * NT + size_t(NT) + size_t(TEMP_BLOCK) * (TEMP_TILE + 1)) * sizeof(double);
    }

    // NR::clampedValue<NR::interpolateLinLin>(x, xv, yv) (NR.hpp:168-173, 328-331, 394-401) for x > 0 on tables of n >= 2 points
    __device__ __forceinline__ double clampedLinLin(double x, const double* xv, const double* yv, int n)
    {
        int i;
        if (x == xv[n - 1])
            i = n - 2;
        else
        {
            int jl = -1, ju = n;
            while (ju - jl > 1)
            {
                const int jm = (ju + jl) >> 1;
                if (x < xv[jm])
                    ju = jm;
                else
                    jl = jm;
            }
            i = jl;
        }
        if (i < 0) return yv[0];
        if (i >= n - 1) return yv[n - 1];
        const double x1 = xv[i], x2 = xv[i + 1], f1 = yv[i], f2 = yv[i + 1];
        return f1 + ((x - x1) / (x2 - x1)) * (f2 - f1);
    }

    __global__ __launch_bounds__(TEMP_BLOCK) void cellTemperatureKernel(const TempArgs A)
    {
        extern __shared__ double lds[];
        const int L = A.numLambda, NT = A.numT, H = A.H;
        double* sWidth = lds;               // [L]
        double* sSigma = sWidth + L;        // [H][L]
        double* sPlanck = sSigma + H * L;   // [H][NT]
        double* sTemp = sPlanck + H * NT;   // [NT]
        double* sTile = sTemp + NT;         // [TEMP_BLOCK][TEMP_TILE + 1]
        const int tid = threadIdx.x;
        for (int i = tid; i < L; i += TEMP_BLOCK) sWidth[i] = A.width[i];
        for (int i = tid; i < H * L; i += TEMP_BLOCK) sSigma[i] = A.sigma[i];
        for (int i = tid; i < H * NT; i += TEMP_BLOCK) sPlanck[i] = A.planckabs[i];
        for (int i = tid; i < NT; i += TEMP_BLOCK) sTemp[i] = A.temperature[i];
        // (the first barrier of the tile loop below also covers the tables)

        const int numTiles = (L + TEMP_TILE - 1) / TEMP_TILE;
        for (long long base = (long long)blockIdx.x * TEMP_BLOCK; base < A.numCells; base += (long long)gridDim.x * TEMP_BLOCK)
        {
            const int rows = (int)(A.numCells - base < TEMP_BLOCK ? A.numCells - base : TEMP_BLOCK);
            const bool valid = tid < rows;
            const long long m = base + tid;
            const double factor = valid ? A.cellFactor[m] : 0.;
            double sum[PMC_MAX_MEDIA];
#pragma unroll
            for (int h = 0; h < PMC_MAX_MEDIA; ++h) sum[h] = 0.;
            bool first = true;
            for (int t = numTiles - 1; t >= 0; --t)
            {
                const int l0 = t * TEMP_TILE;
                const int tl = L - l0 < TEMP_TILE ? L - l0 : TEMP_TILE;
                __syncthreads();  // the tile is free again
                const int count = rows * tl;
                for (int i = tid; i < count; i += TEMP_BLOCK)
                {
                    const int r = i / tl, c = i - r * tl;
                    sTile[r * (TEMP_TILE + 1) + c] = A.rf[(size_t)(base + r) * L + l0 + c];
                }
                __syncthreads();
                if (valid)
                    for (int c = tl - 1; c >= 0; --c)
                    {
                        const int ell = l0 + c;
                        const double w = sWidth[ell];
                        const double J = sTile[tid * (TEMP_TILE + 1) + c] * factor / w;
#pragma unroll
                        for (int h = 0; h < PMC_MAX_MEDIA; ++h)
                            if (h < H)
                            {
                                const double term = sSigma[h * L + ell] * J * w;
                                sum[h] = first ? term : sum[h] + term;
                            }
                        first = false;
                    }
            }
            if (valid)
            {
                double sumRhoT = 0., sumRho = 0.;
#pragma unroll
                for (int h = 0; h < PMC_MAX_MEDIA; ++h)
                    if (h < H)
                    {
                        const double rho = A.rho[(size_t)h * A.numCells + m];
                        double T = 0.;
                        if (rho > 0. && sum[h] > 0.) T = clampedLinLin(sum[h], sPlanck + h * NT, sTemp, NT);
                        A.out[(size_t)h * A.numCells + m] = T;
                        if (rho > 0.)
                        {
                            sumRhoT += rho * T;
                            sumRho += rho;
                        }
                    }
                A.out[(size_t)H * A.numCells + m] = sumRho > 0. ? sumRhoT / sumRho : 0.;
            }
        }
    }
}

extern "C" {

int pmc_dust_temperatures(pmc_ctx* ctx, const pmc_dust_heating* T, double* out)
{
    if (!ctx || !T || !out) return fail(PMC_ERR_INVALID, "pmc_dust_temperatures: null argument");
    if (!ctx->rfSize) return fail(PMC_ERR_INVALID, "pmc_dust_temperatures: the scene does not store the radiation field");
    if (T->num_components > PMC_MAX_MEDIA)
        return fail(PMC_ERR_UNSUPPORTED, "pmc_dust_temperatures: more than " + std::to_string(PMC_MAX_MEDIA) + " dust components");
    if (T->num_components < 1 || T->num_temperatures < 2) return fail(PMC_ERR_INVALID, "pmc_dust_temperatures: empty tables");
    if (T->num_cells != ctx->dev.num_cells || T->num_lambda != ctx->dev.rf_num_lambda || int64_t(T->num_cells) * T->num_lambda != ctx->rfSize)
        return fail(PMC_ERR_INVALID, "pmc_dust_temperatures: the tables do not match the radiation field of the scene (cells, wavelength bins)");
    if (!T->width || !T->sigma || !T->planckabs || !T->temperature || !T->cell_factor || !T->mass_density)
        return fail(PMC_ERR_INVALID, "pmc_dust_temperatures: null table");
    const int H = T->num_components, L = T->num_lambda, NT = T->num_temperatures;
    const size_t numCells = size_t(T->num_cells);
    const size_t lds = tempLdsBytes(H, L, NT);
    if (lds > size_t(160) * 1024)
        return fail(PMC_ERR_UNSUPPORTED, "pmc_dust_temperatures: the tables (" + std::to_string(lds) + " bytes) do not fit the LDS of a workgroup");
    ctx->temperatureMs = 0.f;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // (tables beyond the 64 KiB a kernel may use unasked: the limit is a property of the kernel on the current device, always raised to the
    // same cap, so that calls on several contexts of a device cannot lower it under one another)
    if (lds > size_t(64) * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&cellTemperatureKernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CallBuffers buffers;
    TempArgs A{};
    double *dWidth = nullptr, *dSigma = nullptr, *dPlanck = nullptr, *dTemp = nullptr, *dFactor = nullptr, *dRho = nullptr, *dOut = nullptr;
    HIP_TRY(buffers.get(size_t(L), &dWidth, T->width));
    HIP_TRY(buffers.get(size_t(H) * L, &dSigma, T->sigma));
    HIP_TRY(buffers.get(size_t(H) * NT, &dPlanck, T->planckabs));
    HIP_TRY(buffers.get(size_t(NT), &dTemp, T->temperature));
    HIP_TRY(buffers.get(numCells, &dFactor, T->cell_factor));
    HIP_TRY(buffers.get(size_t(H) * numCells, &dRho, T->mass_density));
    HIP_TRY(buffers.get(size_t(H + 1) * numCells, &dOut));
    A.rf = ctx->dev.rf, A.width = dWidth, A.sigma = dSigma, A.planckabs = dPlanck, A.temperature = dTemp, A.cellFactor = dFactor, A.rho = dRho, A.out = dOut;
    A.numCells = T->num_cells, A.numLambda = L, A.numT = NT, A.H = H;
    EventPair timer;
    if (int rc = timer.create()) return rc;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((numCells + TEMP_BLOCK - 1) / TEMP_BLOCK, size_t(ctx->numCU) * 8));
    hipError_t e = timer.start(ctx->stream);
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(cellTemperatureKernel, dim3(grid), dim3(TEMP_BLOCK), lds, ctx->stream, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = timer.stop(ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out, dOut, size_t(H + 1) * numCells * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hipFail(e, "pmc_dust_temperatures");
    ctx->temperatureMs = timer.elapsedMs();
    return PMC_OK;
}

int pmc_last_temperature_ms(pmc_ctx* ctx, float* kernel_ms)
{
    if (!ctx) return fail(PMC_ERR_INVALID, "null context");
    if (kernel_ms) *kernel_ms = ctx->temperatureMs;
    return PMC_OK;
}

}  // extern "C"
