// adaptive_mesh.hpp -- import of a medium given on an adaptive mesh (AMR): the cells of a grid-based hydro code as the leaves of a tree
// whose nodes are subdivided into nx x ny x nz children.  Restates, with the reference's arithmetic and ORDER of operations so that the
// densities come out bit-identical:
//   nonleaf lines "! nx ny nz" among the data rows       SKIRT/core/TextInFile.cpp:478-523
//   recursive construction, children k, j, i (i fastest) SKIRT/core/AdaptiveMeshSnapshot.cpp:29-64,192-208
//   child boxes                                          SKIRT/utils/Box.hpp:163-167 (fracPos with integer fractions)
//   column roles and default units                       SKIRT/core/AdaptiveMeshMedium.cpp:21-36, Snapshot.cpp:143-197
//   densities and masses of the cells                    SKIRT/core/Snapshot.cpp:325-384, ImportedMedium.cpp:47-57
//   density at a position: descent with index correction SKIRT/core/AdaptiveMeshSnapshot.cpp:108-148,276-280, Box.hpp:171-176
// Not restated: the path segment generator and the neighbour lists (an AdaptiveMeshSpatialGrid is not supported), generatePosition,
// velocity / magnetic field / variable-mix columns.
#ifndef SKH_ADAPTIVE_MESH_HPP
#define SKH_ADAPTIVE_MESH_HPP

#include "imported.hpp"

namespace skh
{
    class AdaptiveMeshSnapshot : public ImportedSnapshot
    {
    public:
        // reads the file and computes the cell densities; throws std::runtime_error on malformed input
        void load(const MeshImportOptions& options);
        double density(Vec3 r) const override;  // AdaptiveMeshSnapshot.cpp:276-280
        int cellIndex(Vec3 r) const;            // AdaptiveMeshSnapshot.cpp:311-315: the leaf that holds r, -1 outside the domain
        Box extent() const override { return _extent; }
        // (sitePositions(): the centres of the leaves in file order, AdaptiveMeshSnapshot.cpp:241-244)
        // the tree as arrays, which is what the device gets: node 0 is the root, every parent comes before its children, the children of a
        // node have consecutive ids in the order k, j, i (i fastest)
        int numNodes() const { return static_cast<int>(_link.size()); }
        int numCells() const { return static_cast<int>(_rho.size()); }
        const std::vector<double>& nodeBox() const { return _box; }     // [numNodes][6] xmin, ymin, zmin, xmax, ymax, zmax
        const std::vector<int32_t>& nodeDims() const { return _dims; }  // [numNodes][3] nx, ny, nz; 0, 0, 0 for a leaf
        const std::vector<int32_t>& nodeLink() const { return _link; }  // nonleaf: id of child 0; leaf: cell index
        const std::vector<double>& cellDensity() const { return _rho; } // [numCells] mass or number density as the file implies
        pmc_adaptive_mesh tables() const;

    private:
        Box boxOf(int node) const
        {
            const double* b = &_box[6 * static_cast<size_t>(node)];
            return Box(b[0], b[1], b[2], b[3], b[4], b[5]);
        }
        void readNode(int node, ColumnTextFile& file, std::vector<Array>& properties);
        Box _extent;
        std::vector<double> _box;
        std::vector<int32_t> _dims, _link;
        std::vector<double> _rho;
    };
}

#endif
