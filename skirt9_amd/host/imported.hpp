// imported.hpp -- what the media imported from a file share, whatever the kind of their entities (SKIRT/core/Snapshot.hpp,
// ImportedMedium.cpp:12-57): the import options, the mass policy columns, the device sampler and the snapshot base.  A kind of snapshot
// (particles.hpp, adaptive_mesh.hpp) adds its entities, their density at a position and their extent.
#ifndef SKH_IMPORTED_HPP
#define SKH_IMPORTED_HPP

#include "../../include/pmc.h"
#include "column_file.hpp"
#include "mathutil.hpp"
#include <string>
#include <vector>

namespace skh
{
    struct ImportOptions
    {
        std::string path;            // resolved file path
        bool holdsNumber{false};     // massType Number...: the columns hold numbers of entities, not masses
        double massFraction{1.};
        bool importMetallicity{false};
        bool importTemperature{false};
        double maxTemperature{0.};
        bool isDust{true};           // ImportedMedium.cpp:47-57: the temperature cut and the metallicity apply to dust only
    };
    struct MeshImportOptions : ImportOptions
    {
        Box extent;  // the configured domain (MeshMedium minX ... maxZ)
        // massType (AdaptiveMeshMedium.cpp:21-36): which of the density and the mass column the file has -- the density column first
        bool hasDensity{true}, hasMass{false};
    };

    // Snapshot::setMassDensityPolicy as called by ImportedMedium (dust: Tmax and metallicity apply; otherwise not)
    struct MassPolicy
    {
        int metallicityIndex{-1}, temperatureIndex{-1};  // the columns, where imported
        bool useMetallicity{false};
        double maxTemperature{0.};  // 0: no cutoff
    };
    // appends the optional metallicity and temperature columns, in the reference's order (ImportedMedium.cpp:17-22)
    MassPolicy appendPolicyColumns(const ImportOptions& options, std::vector<ColumnSpec>& columns);

    // entry points of the device sampler (include/pmc.h pmc_sampler_*), handed over at run time so that this library keeps no
    // link-time dependency on the HIP engine
    struct SamplerApi
    {
        int (*createParticles)(const pmc_particles*, int32_t, pmc_sampler**){nullptr};
        int (*createMesh)(const pmc_adaptive_mesh*, int32_t, pmc_sampler**){nullptr};
        int (*density)(pmc_sampler*, const double*, int64_t, double*){nullptr};
        void (*destroy)(pmc_sampler*){nullptr};
        const char* (*lastError)(){nullptr};
        int32_t device{0};
    };

    // the pmc_sampler of one snapshot: attached to its tables, asked, and destroyed with the snapshot
    class DeviceSampler
    {
    public:
        DeviceSampler() {}
        DeviceSampler(const DeviceSampler&) = delete;
        DeviceSampler& operator=(const DeviceSampler&) = delete;
        ~DeviceSampler() { release(); }
        SamplerApi api;
        void attach(const pmc_particles& particles) { release(), check(api.createParticles(&particles, api.device, &_sampler), "create failed"); }
        void attach(const pmc_adaptive_mesh& mesh) { release(), check(api.createMesh(&mesh, api.device, &_sampler), "create failed"); }
        bool isAttached() const { return _sampler != nullptr; }
        void densities(const std::vector<Vec3>& positions, double* out) const;

    private:
        void release();
        void check(int code, const char* otherwise) const;  // throws "device density sampler: ..." for a code other than 0
        pmc_sampler* _sampler{nullptr};
    };

    // what an imported medium asks of its snapshot (SKIRT/core/Snapshot.hpp): ImportedMedium in model.hpp is written against this
    class ImportedSnapshot
    {
    public:
        virtual ~ImportedSnapshot() {}
        virtual double density(Vec3 r) const = 0;
        virtual Box extent() const = 0;  // Snapshot::extent()
        // density(r) for many positions: on the MI355X if a device sampler is attached (bit-identical results), otherwise on the host cores
        void densities(const std::vector<Vec3>& positions, std::vector<double>& out) const;
        void useDeviceSampler(const SamplerApi& api) { _sampler.api = api; }
        bool onDevice() const { return _sampler.isAttached(); }
        double mass() const { return _mass; }
        bool holdsNumber() const { return _holdsNumber; }
        // the positions of ALL imported entities in file order, also those that carry no mass (SiteListInterface of ImportedMedium,
        // ImportedMedium.cpp:268-278: the sites of a Voronoi grid with the ImportedSites policy)
        const std::vector<Vec3>& sitePositions() const { return _sites; }

    protected:
        double _mass{0};
        bool _holdsNumber{false};
        std::vector<Vec3> _sites;
        DeviceSampler _sampler;
    };
}

#endif
