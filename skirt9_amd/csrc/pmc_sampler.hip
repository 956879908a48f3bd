// pmc_sampler.hip -- setup-time density of an imported medium on the MI355X (include/pmc.h, pmc_sampler_*): smoothed particles, and
// the cells of an adaptive mesh (second half of this file).
//
// One lane per sample position: locate the block of the search grid (three binary searches over the separation arrays,
// staged in LDS), then walk the block's particle list IN ORDER and accumulate kernel(u) * rho -- exactly the loop of
// ParticleSnapshot::density (SKIRT/core/ParticleSnapshot.cpp:233-243), so that the sums come out bit-identical to the
// host's (IEEE f64 add / mul / div / sqrt, -ffp-contract=off, no transcendental function in the cubic-spline and
// uniform kernels).  Compute-bound f64 work with gathers from the particle table (40 B per particle, L2 / Infinity-Cache
// resident for 10^6 particles); positions and results stream over PCIe in batches.
#include "../../include/pmc.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

extern "C" const char* pmc_last_error(void);
void pmcSetError(const std::string& message);  // pmc_api.hip

// The frame of a sampler, whatever the kind of its tables: positions and results cross in batches through two buffers on one stream; the
// kind (second half of this file) adds its tables to `allocations` and the launch of its kernel.
struct pmc_sampler
{
    int device{0};
    hipStream_t stream{nullptr};
    long long batch{0};
    double* dpos{nullptr};  // [batch][3]
    double* dout{nullptr};  // [batch]
    std::vector<void*> allocations;
    // only for a kind whose kernel can fail at a position: the lowest index of such a position, or all ones, and the sentence to report it with
    unsigned long long* dfailed{nullptr};
    const char* failedSentence{nullptr};
    // the kind's kernel on `stream`, in `blocks` workgroups of 256, for the m positions in dpos of which the first has the index `first`
    std::function<void(const pmc_sampler&, int blocks, long long m, long long first)> launch;
};

namespace
{
    struct DevParticles
    {
        int32_t kernel;
        int32_t nb;
        const double* particle;
        const double* grid;  // xgrid | ygrid | zgrid, (nb + 1) each
        const long long* block_start;
        const int32_t* block_list;
    };

    // NR::locateClip on a separation array (NR.hpp:152-159).  (Its own copy: written as pmc_kernels.hip writes its locateClip, on locateBasic,
    // the compiler emits other bytes for sampleDensityKernel; and this form there changes 34 of that file's kernels.)
    __device__ __forceinline__ int locateClip(const double* xv, int n, double x)
    {
        if (x < xv[0]) return 0;
        int jl = -1, ju = n - 1;
        while (ju - jl > 1)
        {
            const int jm = (ju + jl) >> 1;
            if (x < xv[jm])
                ju = jm;
            else
                jl = jm;
        }
        return jl;
    }

    // CubicSplineSmoothingKernel::density (CubicSplineSmoothingKernel.cpp:40-50), UniformSmoothingKernel::density
    template<int KERNEL> __device__ __forceinline__ double kernelDensity(double u)
    {
        if (KERNEL == PMC_KERNEL_CUBIC_SPLINE)
        {
            if (u < 0.0 || u >= 1.0)
                return 0.0;
            else if (u < 0.5)
                return 8.0 / M_PI * (1.0 - 6.0 * u * u * (1.0 - u));
            else
                return 8.0 / M_PI * 2.0 * (1.0 - u) * (1.0 - u) * (1.0 - u);
        }
        if (u < 0.0 || u > 1.0) return 0.0;
        return 0.75 / M_PI;
    }

    template<int KERNEL>
    __global__ __launch_bounds__(256) void sampleDensityKernel(DevParticles P, const double* __restrict__ positions, long long n,
                                                               double* __restrict__ density)
    {
        extern __shared__ double grid[];  // 3 (nb + 1) separation points
        const int ng = 3 * (P.nb + 1);
        for (int i = threadIdx.x; i < ng; i += blockDim.x) grid[i] = P.grid[i];
        __syncthreads();
        const double* xg = grid;
        const double* yg = grid + (P.nb + 1);
        const double* zg = yg + (P.nb + 1);
        for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (long long)gridDim.x * blockDim.x)
        {
            const double x = positions[3 * s], y = positions[3 * s + 1], z = positions[3 * s + 2];
            const int i = locateClip(xg, P.nb + 1, x);
            const int j = locateClip(yg, P.nb + 1, y);
            const int k = locateClip(zg, P.nb + 1, z);
            const long long b = ((long long)i * P.nb + j) * P.nb + k;
            double sum = 0.;
            const long long e = P.block_start[b + 1];
            for (long long q = P.block_start[b]; q < e; ++q)
            {
                const double* p = P.particle + 5 * (long long)P.block_list[q];
                const double dx = x - p[0], dy = y - p[1], dz = z - p[2];
                const double u = sqrt(dx * dx + dy * dy + dz * dz) / p[3];
                sum += kernelDensity<KERNEL>(u) * p[4];
            }
            density[s] = sum > 0. ? sum : 0.;
        }
    }

    // ---------------------------------------------------------------- adaptive mesh
    //
    // One lane per position descends the tree of AdaptiveMeshSnapshot::Node::leaf (SKIRT/core/AdaptiveMeshSnapshot.cpp:108-148).  A node
    // is ONE 64-byte aligned record -- box, dimensions, link -- so that a level of the descent costs one 64-byte request per lane: the
    // record of the estimated child, which serves the `contains` test of Node::child and, when it passes, is the node of the next level.
    // The top levels are shared by all lanes (the root is a broadcast) and stay in the vector L1 / L2; the deep levels are gathers, and
    // positions of one cell (100 samples each in the setup phase) are neighbours in the batch, so their lanes walk the same records.  Plain
    // f64 in the reference's expression order (-ffp-contract=off); no LDS.
    struct alignas(64) MeshNode
    {
        double xmin, ymin, zmin, xmax, ymax, zmax;
        int32_t nx, ny, nz;  // 0, 0, 0: leaf
        int32_t link;        // nonleaf: id of child 0; leaf: cell index
    };
    static_assert(sizeof(MeshNode) == 64, "one node per 64-byte line");

    struct DevMesh
    {
        const MeshNode* node;
        const double* cell_density;
        int32_t depth;  // levels below the root: the cap of the descent
    };

    // the record as four 16-byte loads
    __device__ __forceinline__ MeshNode loadNode(const MeshNode* node, int32_t id)
    {
        const double2* d = reinterpret_cast<const double2*>(node + id);
        const double2 a = d[0], b = d[1], c = d[2];
        const int4 t = *reinterpret_cast<const int4*>(d + 3);
        MeshNode n;
        n.xmin = a.x, n.ymin = a.y, n.zmin = b.x, n.xmax = b.y, n.ymax = c.x, n.zmax = c.y;
        n.nx = t.x, n.ny = t.y, n.nz = t.z, n.link = t.w;
        return n;
    }

    // Box::contains (SKIRT/utils/Box.hpp:99-102): the box is closed; false for a coordinate that is not a number
    __device__ __forceinline__ bool holds(const MeshNode& n, double x, double y, double z)
    {
        return x >= n.xmin && x <= n.xmax && y >= n.ymin && y <= n.ymax && z >= n.zmin && z <= n.zmax;
    }

    // Box::cellIndices (Box.hpp:171-176) for one axis: the product first, then the quotient
    __device__ __forceinline__ int childIndex(int n, double x, double lo, double hi)
    {
        return max(0, min(n - 1, static_cast<int>(n * (x - lo) / (hi - lo))));
    }

    __global__ __launch_bounds__(256) void sampleMeshDensityKernel(DevMesh M, const double* __restrict__ positions, long long n, long long first,
                                                                   double* __restrict__ density, unsigned long long* __restrict__ failed)
    {
        for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (long long)gridDim.x * blockDim.x)
        {
            const double x = positions[3 * s], y = positions[3 * s + 1], z = positions[3 * s + 2];
            MeshNode node = loadNode(M.node, 0);
            double rho = 0.;
            if (holds(node, x, y, z))  // Node::leaf: outside the root box there is no cell
            {
                bool lost = false;
                for (int level = 0; level < M.depth && node.nx != 0; ++level)
                {
                    // Node::child: estimate the child, correct the indices by one if the point is not in it
                    int i = childIndex(node.nx, x, node.xmin, node.xmax);
                    int j = childIndex(node.ny, y, node.ymin, node.ymax);
                    int k = childIndex(node.nz, z, node.zmin, node.zmax);
                    MeshNode child = loadNode(M.node, node.link + (k * node.ny + j) * node.nx + i);
                    if (!holds(child, x, y, z))
                    {
                        if (x < child.xmin)
                            i--;
                        else if (x > child.xmax)
                            i++;
                        if (y < child.ymin)
                            j--;
                        else if (y > child.ymax)
                            j++;
                        if (z < child.zmin)
                            k--;
                        else if (z > child.zmax)
                            k++;
                        // (an index outside the node's children: the reference reads outside its list here)
                        if (i < 0 || i >= node.nx || j < 0 || j >= node.ny || k < 0 || k >= node.nz)
                        {
                            lost = true;
                            break;
                        }
                        child = loadNode(M.node, node.link + (k * node.ny + j) * node.nx + i);
                        if (!holds(child, x, y, z))
                        {
                            lost = true;
                            break;
                        }
                    }
                    node = child;
                }
                // a nonleaf node after `depth` levels cannot happen with the depth worked out from the table: the cap only bounds the loop
                if (lost || node.nx != 0)
                    atomicMin(failed, static_cast<unsigned long long>(first + s));
                else
                    rho = M.cell_density[node.link];
            }
            density[s] = rho;
        }
    }
}

namespace
{
    int failSampler(int code, const std::string& message)
    {
        pmcSetError(message);
        return code;
    }
    // the common failure path of the create functions
    int failAllocation(pmc_sampler* s, const char* kind)
    {
        pmc_sampler_destroy(s);
        return failSampler(PMC_ERR_NOMEM, std::string("device allocation for the ") + kind + " sampler failed");
    }
    // the frame on `device`, after the kind's checks of its tables: stream and batch buffers, and the word for failed positions if the kind wants one
    int openSampler(int32_t device, bool wantsFailWord, const char* kind, pmc_sampler** out)
    {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
            return failSampler(PMC_ERR_DEVICE, "no HIP device available: the device sampler cannot run");
        if (device < 0 || device >= count) return failSampler(PMC_ERR_INVALID, "invalid device index");
        if (hipSetDevice(device) != hipSuccess) return failSampler(PMC_ERR_DEVICE, "hipSetDevice failed");
        pmc_sampler* s = new pmc_sampler();
        s->device = device;
        s->batch = 1 << 22;
        const bool ok = hipMalloc(reinterpret_cast<void**>(&s->dpos), size_t(s->batch) * 3 * sizeof(double)) == hipSuccess
                        && hipMalloc(reinterpret_cast<void**>(&s->dout), size_t(s->batch) * sizeof(double)) == hipSuccess
                        && (!wantsFailWord || hipMalloc(reinterpret_cast<void**>(&s->dfailed), sizeof(unsigned long long)) == hipSuccess)
                        && hipStreamCreate(&s->stream) == hipSuccess;
        if (!ok) return failAllocation(s, kind);
        *out = s;
        return PMC_OK;
    }
    template<typename T> bool uploadTo(pmc_sampler* s, const T* host, size_t count, const T** out)
    {
        void* d = nullptr;
        if (hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return false;
        s->allocations.push_back(d);
        if (count && hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return false;
        *out = static_cast<const T*>(d);
        return true;
    }
}

extern "C" {

int pmc_sampler_create(const pmc_particles* P, int32_t device, pmc_sampler** out)
{
    if (!P || !out) return failSampler(PMC_ERR_INVALID, "null argument");
    *out = nullptr;
    if (P->kernel != PMC_KERNEL_CUBIC_SPLINE && P->kernel != PMC_KERNEL_UNIFORM)
        return failSampler(PMC_ERR_UNSUPPORTED, "smoothing kernel not supported by the device sampler");
    if (P->num_particles < 1 || P->num_blocks < 1 || !P->particle || !P->xgrid || !P->ygrid || !P->zgrid || !P->block_start
        || !P->block_list)
        return failSampler(PMC_ERR_INVALID, "particle tables are missing");
    if (3 * size_t(P->num_blocks + 1) * sizeof(double) > 64 * 1024)
        return failSampler(PMC_ERR_UNSUPPORTED, "search grid with more than 2729 blocks per axis");
    pmc_sampler* s = nullptr;
    if (const int code = openSampler(device, false, "particle", &s)) return code;
    const size_t nb = size_t(P->num_blocks), nb3 = nb * nb * nb;
    std::vector<double> grid;
    grid.insert(grid.end(), P->xgrid, P->xgrid + nb + 1);
    grid.insert(grid.end(), P->ygrid, P->ygrid + nb + 1);
    grid.insert(grid.end(), P->zgrid, P->zgrid + nb + 1);
    std::vector<long long> starts(P->block_start, P->block_start + nb3 + 1);
    DevParticles dev{};
    dev.kernel = P->kernel;
    dev.nb = P->num_blocks;
    if (!(uploadTo(s, P->particle, 5 * size_t(P->num_particles), &dev.particle) && uploadTo(s, grid.data(), grid.size(), &dev.grid)
          && uploadTo(s, starts.data(), starts.size(), &dev.block_start) && uploadTo(s, P->block_list, size_t(P->block_start[nb3]), &dev.block_list)))
        return failAllocation(s, "particle");
    const size_t lds = grid.size() * sizeof(double);
    s->launch = [dev, lds](const pmc_sampler& f, int blocks, long long m, long long) {
        if (dev.kernel == PMC_KERNEL_CUBIC_SPLINE)
            hipLaunchKernelGGL(sampleDensityKernel<PMC_KERNEL_CUBIC_SPLINE>, dim3(blocks), dim3(256), lds, f.stream, dev, f.dpos, m, f.dout);
        else
            hipLaunchKernelGGL(sampleDensityKernel<PMC_KERNEL_UNIFORM>, dim3(blocks), dim3(256), lds, f.stream, dev, f.dpos, m, f.dout);
    };
    *out = s;
    return PMC_OK;
}

int pmc_sampler_density(pmc_sampler* s, const double* positions, int64_t n, double* density)
{
    if (!s || n < 0) return failSampler(PMC_ERR_INVALID, "invalid argument");
    if (n == 0) return PMC_OK;
    if (!positions || !density) return failSampler(PMC_ERR_INVALID, "null buffer");
    if (hipSetDevice(s->device) != hipSuccess) return failSampler(PMC_ERR_DEVICE, "hipSetDevice failed");
    const unsigned long long none = ~0ull;
    unsigned long long failed = none;
    if (s->dfailed && hipMemsetAsync(s->dfailed, 0xff, sizeof(failed), s->stream) != hipSuccess)
        return failSampler(PMC_ERR_DEVICE, "hipMemset of the sampler's error word failed");
    for (int64_t first = 0; first < n; first += s->batch)
    {
        const long long m = std::min<long long>(s->batch, n - first);
        if (hipMemcpyAsync(s->dpos, positions + 3 * first, size_t(m) * 3 * sizeof(double), hipMemcpyHostToDevice, s->stream) != hipSuccess)
            return failSampler(PMC_ERR_DEVICE, "hipMemcpy of the sample positions failed");
        const int blocks = int(std::min<long long>((m + 255) / 256, 256 * 16));
        s->launch(*s, blocks, m, (long long)first);
        if (hipGetLastError() != hipSuccess) return failSampler(PMC_ERR_DEVICE, "launch of the density sampling kernel failed");
        if (hipMemcpyAsync(density + first, s->dout, size_t(m) * sizeof(double), hipMemcpyDeviceToHost, s->stream) != hipSuccess
            || hipStreamSynchronize(s->stream) != hipSuccess)
            return failSampler(PMC_ERR_DEVICE, "density sampling kernel failed");
    }
    if (s->dfailed)
    {
        if (hipMemcpyAsync(&failed, s->dfailed, sizeof(failed), hipMemcpyDeviceToHost, s->stream) != hipSuccess
            || hipStreamSynchronize(s->stream) != hipSuccess)
            return failSampler(PMC_ERR_DEVICE, "density sampling kernel failed");
        if (failed != none) return failSampler(PMC_ERR_DEVICE, s->failedSentence + (" (position " + std::to_string(failed) + ")"));
    }
    return PMC_OK;
}

int pmc_sampler_create_mesh(const pmc_adaptive_mesh* M, int32_t device, pmc_sampler** out)
{
    if (!M || !out) return failSampler(PMC_ERR_INVALID, "null argument");
    *out = nullptr;
    if (M->num_nodes < 1 || M->num_cells < 1 || !M->node_box || !M->node_dims || !M->node_link || !M->cell_density)
        return failSampler(PMC_ERR_INVALID, "adaptive mesh tables are missing");
    // ---- the table, before any device call: every index the kernel forms from it stays inside it; the depth of the tree in the same pass
    // (a child id is above its parent's, so the depth of a node is final when the pass reaches it)
    const int64_t numNodes = M->num_nodes;
    std::vector<MeshNode> nodes(static_cast<size_t>(numNodes));
    std::vector<int32_t> depth(static_cast<size_t>(numNodes), 0);
    int32_t maxDepth = 0;
    for (int64_t id = 0; id != numNodes; ++id)
    {
        const int32_t* dims = M->node_dims + 3 * id;
        const int32_t link = M->node_link[id];
        const std::string where = " (node " + std::to_string(id) + ")";
        if (dims[0] == 0 && dims[1] == 0 && dims[2] == 0)
        {
            if (link < 0 || link >= M->num_cells) return failSampler(PMC_ERR_INVALID, "adaptive mesh: leaf link outside the cells" + where);
        }
        else
        {
            if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return failSampler(PMC_ERR_INVALID, "adaptive mesh: dimension below 1" + where);
            const int64_t plane = int64_t(dims[0]) * dims[1];
            if (plane > INT32_MAX || plane * dims[2] > INT32_MAX)
                return failSampler(PMC_ERR_INVALID, "adaptive mesh: product of the dimensions overflows" + where);
            const int64_t count = plane * dims[2];
            if (link <= id) return failSampler(PMC_ERR_INVALID, "adaptive mesh: child id not above its parent's" + where);
            if (link + count > numNodes) return failSampler(PMC_ERR_INVALID, "adaptive mesh: child range outside the table" + where);
            const int32_t below = depth[size_t(id)] + 1;
            for (int64_t c = link; c != link + count; ++c) depth[size_t(c)] = std::max(depth[size_t(c)], below);
            maxDepth = std::max(maxDepth, below);
        }
        const double* box = M->node_box + 6 * id;
        MeshNode& node = nodes[size_t(id)];
        node.xmin = box[0], node.ymin = box[1], node.zmin = box[2], node.xmax = box[3], node.ymax = box[4], node.zmax = box[5];
        node.nx = dims[0], node.ny = dims[1], node.nz = dims[2], node.link = link;
    }
    pmc_sampler* s = nullptr;
    if (const int code = openSampler(device, true, "mesh", &s)) return code;
    DevMesh dev{};
    dev.depth = maxDepth;
    // (hipMalloc returns memory aligned to more than the 64 bytes of a record)
    if (!(uploadTo(s, nodes.data(), nodes.size(), &dev.node) && uploadTo(s, M->cell_density, size_t(M->num_cells), &dev.cell_density)))
        return failAllocation(s, "mesh");
    s->failedSentence = "Can't locate the appropriate child node";  // AdaptiveMeshSnapshot.cpp:133
    s->launch = [dev](const pmc_sampler& f, int blocks, long long m, long long first) {
        hipLaunchKernelGGL(sampleMeshDensityKernel, dim3(blocks), dim3(256), 0, f.stream, dev, f.dpos, m, first, f.dout, f.dfailed);
    };
    *out = s;
    return PMC_OK;
}

void pmc_sampler_destroy(pmc_sampler* s)
{
    if (!s) return;
    hipSetDevice(s->device);
    if (s->stream) hipStreamDestroy(s->stream);
    for (void* p : s->allocations) hipFree(p);
    if (s->dpos) hipFree(s->dpos);
    if (s->dout) hipFree(s->dout);
    if (s->dfailed) hipFree(s->dfailed);
    delete s;
}
}
