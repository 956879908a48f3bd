// adaptive_mesh.cpp -- see adaptive_mesh.hpp
#include "adaptive_mesh.hpp"
#include <algorithm>
#include <limits>
#include <stdexcept>

namespace skh
{
    namespace
    {
        const char* const cannotLocate = "Can't locate the appropriate child node";

        bool boxContains(const double* b, Vec3 r)
        {
            return r.x >= b[0] && r.x <= b[3] && r.y >= b[1] && r.y <= b[4] && r.z >= b[2] && r.z <= b[5];
        }
    }

    // AdaptiveMeshSnapshot::Node::Node (AdaptiveMeshSnapshot.cpp:29-64): the line of this node, then its children in the order k, j, i.
    // The children get their ids -- consecutive ones -- and their boxes before the first of them is read.
    void AdaptiveMeshSnapshot::readNode(int node, ColumnTextFile& file, std::vector<Array>& properties)
    {
        int nx = 0, ny = 0, nz = 0;
        if (file.readNonLeaf(nx, ny, nz))
        {
            // (the reference sizes its child list with the product as it comes)
            if (nx < 1 || ny < 1 || nz < 1) throw std::runtime_error("Nonleaf subdivision specifiers should be positive");
            const int64_t count = static_cast<int64_t>(nx) * ny * nz;
            if (nx > 32768 || ny > 32768 || nz > 32768 || count + numNodes() > std::numeric_limits<int32_t>::max() / 8)
                throw std::runtime_error("Too many nodes in adaptive mesh data");
            const int first = numNodes();
            const Box extent = boxOf(node);
            _dims[3 * static_cast<size_t>(node)] = nx, _dims[3 * static_cast<size_t>(node) + 1] = ny, _dims[3 * static_cast<size_t>(node) + 2] = nz;
            _link[node] = first;
            _box.resize(_box.size() + 6 * count);
            _dims.resize(_dims.size() + 3 * count, 0);
            _link.resize(_link.size() + count, -1);
            double* box = &_box[6 * static_cast<size_t>(first)];
            for (int k = 0; k < nz; k++)
                for (int j = 0; j < ny; j++)
                    for (int i = 0; i < nx; i++)
                    {
                        // Box::fracPos(int...) (Box.hpp:163-167): the product first, then the quotient
                        *box++ = extent.xmin + i * (extent.xmax - extent.xmin) / nx;
                        *box++ = extent.ymin + j * (extent.ymax - extent.ymin) / ny;
                        *box++ = extent.zmin + k * (extent.zmax - extent.zmin) / nz;
                        *box++ = extent.xmin + (i + 1) * (extent.xmax - extent.xmin) / nx;
                        *box++ = extent.ymin + (j + 1) * (extent.ymax - extent.ymin) / ny;
                        *box++ = extent.zmin + (k + 1) * (extent.zmax - extent.zmin) / nz;
                    }
            for (int64_t c = 0; c != count; ++c) readNode(first + static_cast<int>(c), file, properties);
        }
        else
        {
            Array row;
            if (!file.readRow(row)) throw std::runtime_error("Reached end of file in adaptive mesh data before all nodes were read");
            _link[node] = static_cast<int32_t>(properties.size());
            properties.push_back(std::move(row));
            _sites.push_back(boxOf(node).center());
        }
    }

    void AdaptiveMeshSnapshot::load(const MeshImportOptions& o)
    {
        _holdsNumber = o.holdsNumber;
        _extent = o.extent;
        // column roles in the reference's order: AdaptiveMeshMedium.cpp:21-36 (the density before the mass) then ImportedMedium.cpp:20-22;
        // default units of Snapshot.cpp:143-197
        std::vector<ColumnSpec> cols;
        int densityIndex = -1, massIndex = -1;
        if (o.hasDensity)
        {
            densityIndex = static_cast<int>(cols.size());
            cols.push_back(o.holdsNumber ? ColumnSpec{"number density", "numbervolumedensity", "1/cm3"}
                                         : ColumnSpec{"mass density", "massvolumedensity", "Msun/pc3"});
        }
        if (o.hasMass)
        {
            massIndex = static_cast<int>(cols.size());
            cols.push_back(o.holdsNumber ? ColumnSpec{"number", "", ""} : ColumnSpec{"mass", "mass", "Msun"});
        }
        if (densityIndex < 0 && massIndex < 0) throw std::runtime_error("adaptive mesh medium without a density or mass column");
        const MassPolicy policy = appendPolicyColumns(o, cols);

        // AdaptiveMeshSnapshot::readAndClose (AdaptiveMeshSnapshot.cpp:192-208)
        _box = {o.extent.xmin, o.extent.ymin, o.extent.zmin, o.extent.xmax, o.extent.ymax, o.extent.zmax};
        _dims.assign(3, 0);
        _link.assign(1, -1);
        _sites.clear();
        std::vector<Array> properties;
        {
            ColumnTextFile file(o.path, cols, "adaptive mesh cells");
            readNode(0, file, properties);
            Array dummy;
            if (file.readRow(dummy)) throw std::runtime_error("Superfluous lines in adaptive mesh data after all nodes were read");
        }

        // Snapshot::calculateDensityAndMass (Snapshot.cpp:325-384)
        const size_t numCells = properties.size();
        std::vector<double> volume(numCells);
        for (int node = 0; node != numNodes(); ++node)
            if (_dims[3 * static_cast<size_t>(node)] == 0) volume[_link[node]] = boxOf(node).volume();
        _rho.assign(numCells, 0.);
        const double maxT = policy.maxTemperature;  // (0: no cutoff)
        double totalEffectiveMass = 0.;
        for (size_t m = 0; m != numCells; ++m)
        {
            const Array& prop = properties[m];
            double originalDensity = 0.;
            double originalMass = 0.;
            if (maxT && prop[policy.temperatureIndex] > maxT)
            {
                // (ignored: above the temperature cutoff)
            }
            else
            {
                const double V = volume[m];
                originalDensity = std::max(0., densityIndex >= 0 ? prop[densityIndex] : prop[massIndex] / V);
                originalMass = std::max(0., massIndex >= 0 ? prop[massIndex] : prop[densityIndex] * V);
            }
            const double effectiveDensity = originalDensity * (policy.useMetallicity ? prop[policy.metallicityIndex] : 1.) * o.massFraction;
            const double metallicMass = originalMass * (policy.useMetallicity ? prop[policy.metallicityIndex] : 1.);
            const double effectiveMass = metallicMass * o.massFraction;
            _rho[m] = effectiveDensity;
            totalEffectiveMass += effectiveMass;
        }
        _mass = totalEffectiveMass;

        // ---- optional: the same evaluation on the MI355X (include/pmc.h pmc_sampler_create_mesh)
        if (_sampler.api.createMesh && numCells) _sampler.attach(tables());
    }

    pmc_adaptive_mesh AdaptiveMeshSnapshot::tables() const
    {
        pmc_adaptive_mesh mesh{};
        mesh.num_nodes = numNodes();
        mesh.num_cells = numCells();
        mesh.node_box = _box.data();
        mesh.node_dims = _dims.data();
        mesh.node_link = _link.data();
        mesh.cell_density = _rho.data();
        return mesh;
    }

    // AdaptiveMeshSnapshot::Node::leaf and ::child (AdaptiveMeshSnapshot.cpp:108-148) with Box::cellIndices (Box.hpp:171-176)
    int AdaptiveMeshSnapshot::cellIndex(Vec3 r) const
    {
        if (_link.empty() || !boxContains(&_box[0], r)) return -1;
        size_t node = 0;
        while (_dims[3 * node] != 0)
        {
            const double* b = &_box[6 * node];
            const int nx = _dims[3 * node], ny = _dims[3 * node + 1], nz = _dims[3 * node + 2];
            // estimate the child node indices; this may be off by one due to rounding errors
            int i = std::max(0, std::min(nx - 1, static_cast<int>(nx * (r.x - b[0]) / (b[3] - b[0]))));
            int j = std::max(0, std::min(ny - 1, static_cast<int>(ny * (r.y - b[1]) / (b[4] - b[1]))));
            int k = std::max(0, std::min(nz - 1, static_cast<int>(nz * (r.z - b[2]) / (b[5] - b[2]))));
            const size_t first = static_cast<size_t>(_link[node]);
            size_t child = first + (static_cast<size_t>(k) * ny + j) * nx + i;
            const double* c = &_box[6 * child];
            if (!boxContains(c, r))
            {
                if (r.x < c[0])
                    i--;
                else if (r.x > c[3])
                    i++;
                if (r.y < c[1])
                    j--;
                else if (r.y > c[4])
                    j++;
                if (r.z < c[2])
                    k--;
                else if (r.z > c[5])
                    k++;
                // (the reference reads outside its child list here)
                if (i < 0 || i >= nx || j < 0 || j >= ny || k < 0 || k >= nz) throw std::runtime_error(cannotLocate);
                child = first + (static_cast<size_t>(k) * ny + j) * nx + i;
                if (!boxContains(&_box[6 * child], r)) throw std::runtime_error(cannotLocate);
            }
            node = child;
        }
        return _link[node];
    }

    double AdaptiveMeshSnapshot::density(Vec3 r) const
    {
        const int m = cellIndex(r);
        return m >= 0 ? _rho[m] : 0;
    }
}
