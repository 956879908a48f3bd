// simulation.hpp -- the MonteCarloSimulation of the host layer: ski file -> objects -> pmc_scene -> output files.
//
// Counterpart of SKIRT/core/MonteCarloSimulation (setupSimulation / runSimulation, MonteCarloSimulation.cpp:20-100)
// for the primary-emission path.  The photon loop itself is NOT here: the caller hands scene() to an engine
// (the HIP library behind include/pmc.h) and passes the resulting detector arrays to write().
#ifndef SKH_SIMULATION_HPP
#define SKH_SIMULATION_HPP

#include "model.hpp"
#include <cstdint>
#include <functional>
#include <mutex>

namespace skh
{
    struct Reader;  // attribute access for the readers of the ski file (ski_reader.cpp)

    class Simulation
    {
    public:
        // parse the ski file and construct the item tree (XmlHierarchyCreator::readFile)
        static std::unique_ptr<Simulation> fromFile(const std::string& path);
        static std::unique_ptr<Simulation> fromString(const std::string& text, const std::string& prefix,
                                                      const std::string& inputPath = ".");

        // Simulation::setupSimulation: builds grids, densities, tables; consumes the parent random stream
        // exactly as the reference does with one thread.  If treeTopologyFile is non-empty the octree is rebuilt
        // from that TreeSpatialGridTopologyProbe file instead of by density sampling (no random draws for the tree).
        void setup();

        const pmc_scene& scene() const { return _scene; }
        // what the scene's layout has no room for (pmc_create_ext): the phase function of every medium component, the velocity of every source
        const pmc_scene_ext& sceneExt() const { return _sceneExt; }
        uint64_t numPackets() const { return _numPackets; }
        int seed() const { return _seed; }
        // number of uniform deviates drawn from the parent stream during setup (the photon loop of the
        // single-thread reference continues the same stream from here)
        unsigned long long setupDraws() const { return _random.draws(); }
        const std::string& prefix() const { return _prefix; }

        int numInstruments() const { return static_cast<int>(_instruments.size()); }
        const InstrumentModel& instrument(int i) const { return _instruments[i]; }
        int64_t frameSize() const { return _frameSize; }
        const pmc_frame_layout& layout(int i) const { return _layouts[i]; }

        // FluxRecorder::calibrateAndWrite for every instrument (FluxRecorder.cpp:484-846); frames holds the raw
        // detector arrays in the pmc_frame_layout order and is calibrated IN PLACE.  Returns the files written.
        // writeStatistics = false: the flux files only (a segment whose statistics arrays are incomplete: the engine's list pool ran out)
        std::vector<std::string> write(double* frames, const std::string& outdir, bool writeStatistics = true) const;

        // Radiation field (RadiationFieldOptions::storeRadiationField): number of doubles of the table rf[m * nbins + ell]
        // that pmc_download_radiation_field fills (0 if not stored), and the RadiationFieldProbe / PerCellForm output
        // files "<prefix>_<probe>_J.dat" (RadiationFieldProbe.cpp:27-78, PerCellForm.cpp:14-32) written from it
        int64_t radiationFieldSize() const;
        std::vector<std::string> writeRadiationField(const double* rf, const std::string& outdir) const;

        // Probe maps (DensityProbe, OpacityProbe; ParallelProjectionForm, PerCellForm): probes.cpp.  A projected map is one FITS file: the
        // pixels are sums over sub-sample rays of line integrals through the grid, which the caller's integrator computes (the engine's
        // pmc_integrate_rays, handed over at run time: this library does not link the engine)
        struct ProbeMapInfo
        {
            std::string fileName;  // <prefix>_<probeName>_<projectedFileid>.fits
            int nx{0}, ny{0}, sampling{1}, numValues{1};
            int64_t numRays{0};    // nx * ny * sampling^2
            bool afterSetup{true};
            bool averaged{false};  // a weighted average along the rays (TemperatureProbe) instead of an integral
        };
        // sums[i * numValues + v] = sum over the path of ray i of ds * cellValues[v * numCells + m]; nonzero: failure
        typedef int (*IntegrateFn)(void* user, int64_t numRays, const double* origins, const double* directions, int32_t numValues,
                                   const double* cellValues, double* sums);
        int numProbeMaps() const;
        ProbeMapInfo probeMapInfo(int map) const;
        // the rays of a map, [numRays][3] each, ordered by pixel (j, i) and sub-sample (is, js) (ParallelProjectionForm.cpp:67-88)
        void probeMapRays(int map, double* origins, double* directions) const;
        // its cell values [numValues][numCells] in internal units (the projected unit factor is applied to the sums)
        void probeMapValues(int map, double* cellValues) const;

        // Dust temperatures from the stored radiation field (temperature.cpp): the tables of EquilibriumDustEmissionCalculator::precalculate
        // (EquilibriumDustEmissionCalculator.cpp:18-93) per dust component, in the layout of pmc_dust_heating (include/pmc.h) together with the
        // cell factors 1 / (4 pi V) and the mass densities; built at the first request (a thousand Planck integrals per component) and valid
        // while the simulation lives.  Only for a panchromatic simulation that stores the radiation field and has dust.
        struct DustHeating
        {
            std::vector<int> components;  // the dust components h, in order
            Array lambda, width, temperature, sigma, planckabs, cellFactor, massDensity;
            pmc_dust_heating flat{};
        };
        bool hasDustHeating() const;
        const DustHeating& dustHeating() const;
        // out[h][m] for the dust components in order, then the mass-weighted mean (MediumSystem::indicativeTemperature,
        // MediumSystem.cpp:1384-1427): [H + 1][numCells], from the table rf[m * nbins + ell]
        void dustTemperatures(const double* rf, double* out) const { dustTemperatures(dustHeating().flat, rf, out); }
        static void dustTemperatures(const pmc_dust_heating& tables, const double* rf, double* out);

        // TemperatureProbe and DustAbsorptionPerCellProbe need the radiation field: what the caller hands to writeProbes next to the integrator.
        // temperatures (the engine's pmc_dust_temperatures, from the table on the device) or, without it, rf (the table on the host, from
        // which the host computes them); rf also serves DustAbsorptionPerCellProbe; weighted: the engine's pmc_integrate_weighted_rays
        typedef int (*WeightedFn)(void* user, int64_t numRays, const double* origins, const double* directions, int32_t numValues,
                                  const double* cellWeights, const double* cellValues, double* sums);
        typedef int (*TemperatureFn)(void* user, const pmc_dust_heating* tables, double* out);
        // the point sampler of the cut forms (the engine's pmc_sample_cells): cells[p] = SpatialGrid::cellIndex(positions[p]), values[v * numPoints + p] =
        // cellValues[v * numCells + cells[p]] or 0 outside the grid; cells may be null
        typedef int (*SampleFn)(void* user, int64_t numPoints, const double* positions, int32_t numValues, const double* cellValues, double* values,
                                int32_t* cells);
        struct ProbeEngine
        {
            IntegrateFn integrate{nullptr};
            WeightedFn weighted{nullptr};
            TemperatureFn temperatures{nullptr};
            void* user{nullptr};
            const double* rf{nullptr};
            SampleFn sample{nullptr};  // ConvergenceCutsProbe (user as for the others)
        };
        // writes the probe files; when: 0 the probes with probeAfter Setup, 1 those with Run, -1 all.  The per-cell files need no
        // integrator, which may be null when no projected map is written
        std::vector<std::string> writeProbes(const ProbeEngine& engine, const std::string& outdir, int when = -1) const;
        // whether a probe written with `when` reads the radiation field (a TemperatureProbe or DustAbsorptionPerCellProbe that writes a file)
        bool probesNeedRadiationField(int when = -1) const;

        // human-readable summary (grid size, tables, ...) for logs and tests
        std::string summary() const;

        // model objects, exposed for tests
        const SpatialGrid& grid() const { return *_grid; }
        const Medium& medium() const { return *_medium; }
        // MediumSystem::dimension (MediumSystem.cpp:403-408): the largest dimension of the medium components, at least 1
        int dimension() const
        {
            int result = 1;
            for (const auto& part : _media) result = std::max(result, part->dimension());
            return result;
        }
        const Array& numberDensity(size_t h = 0) const { return _density[h]; }
        const SourceModel& source(int h = 0) const { return _sources[h]; }
        int numSources() const { return static_cast<int>(_sources.size()); }
        // Configuration::hasMovingSources (Configuration.cpp:79-81): some source has a velocity (never in an oligochromatic simulation)
        bool hasMovingSources() const
        {
            for (const SourceModel& source : _sources)
                if (source.velocity.kind != PMC_VELOCITY_NONE) return true;
            return false;
        }

        // optional overrides applied before setup()
        void setNumPackets(uint64_t n) { _numPackets = n; }
        // evaluate the densities of the imported media on the GPU during setup (include/pmc.h pmc_sampler_*): each call takes the create
        // function of its kind of medium from `api` and the entry points that the kinds share; ignored for other media
        void setParticleSampler(const SamplerApi& api) { setSampler(api, api.createParticles, _samplerApi.createMesh); }
        void setMeshSampler(const SamplerApi& api) { setSampler(api, _samplerApi.createParticles, api.createMesh); }
        // medium component h as an imported medium; throws for a component of another kind
        const ImportedMedium& importedMedium(int h) const
        {
            if (h < 0 || h >= static_cast<int>(_media.size())) throw std::runtime_error("no such medium component");
            const ImportedMedium* medium = dynamic_cast<const ImportedMedium*>(_media[h].get());
            if (!medium) throw std::runtime_error("medium component " + std::to_string(h) + " is a " + _media[h]->type() + ", not an imported medium");
            return *medium;
        }
        void setTreeTopology(std::vector<char> topology) { _topology = std::move(topology); }

    private:
        Simulation() {}
        struct ProbeModel;
        struct SourceTables;
        struct WavelengthRange
        {
            double min, max;
        };
        struct SimulationWavelengths
        {
            WavelengthRange range;             // with the margins for kinematics and redshift
            std::vector<double> wavelengths;   // the characteristic wavelengths of the simulation, ascending
        };

        // ski_reader.cpp: the systems of the ski file in document order; what reads a single element without the state of the simulation
        // is a free function there
        void parse(const XmlElement& root);
        void readUnits(const XmlElement& sim, Reader& rd);
        void readMode(const XmlElement& sim, Reader& rd);
        void readRandom(const XmlElement& sim, const Reader& rd);
        void readCosmology(const XmlElement& sim, const Reader& rd);
        void readSourceSystem(const XmlElement& sim, const Reader& rd);
        const XmlElement& readMediumSystem(const XmlElement& sim, const Reader& rd);
        void readRadiationFieldOptions(const XmlElement& mediumSystem, const Reader& rd);
        void readInstrumentSystem(const XmlElement& sim, const Reader& rd);
        void readProbeSystem(const XmlElement& sim, const Reader& rd);
        static ProbeModel readDustAbsorptionProbe(const XmlElement& probe, const Reader& rd);
        static ProbeModel readFormProbe(const XmlElement& probe, const Reader& rd);
        static ProbeModel readConvergenceCutsProbe(const XmlElement& probe, const Reader& rd);
        static ProbeModel readConvergenceInfoProbe(const XmlElement& probe, const Reader& rd);
        static std::string readRadiationFieldProbe(const XmlElement& probe, const Reader& rd);

        // simulation.cpp: the stages of setup(), in order
        void chooseWavelengthGrids();
        SimulationWavelengths simulationWavelengths() const;
        void setupMedia(const SimulationWavelengths& simulation);
        void setupGrid();
        void sampleDensities();
        void flattenScene();
        static SourceTables buildSourceTables(SourceModel& source, WavelengthRange sourceRange, const WavelengthGrid* oligoGrid, pmc_source& flat);
        void setLaunchWeights();
        void flattenSources();
        // and what they share
        const WavelengthGrid* defaultWavelengthGrid() const { return _oligo ? _oligoGrid.get() : _defaultGrid.get(); }
        const WavelengthGrid* gridInEffect(const WavelengthGrid* own) const;
        WavelengthRange sourceWavelengthRange() const;
        void flattenGrid();
        void flattenMedia();
        pmc_instrument flattenInstrument(const InstrumentModel& instrument) const;
        void flattenRadiationField();
        static void flattenSourceGeometry(const SourceModel& source, pmc_source& flat);

        std::string _prefix;
        std::string _inputPath{"."};
        void setSampler(const SamplerApi& api, decltype(SamplerApi::createParticles) createParticles, decltype(SamplerApi::createMesh) createMesh)
        {
            _samplerApi = api, _samplerApi.createParticles = createParticles, _samplerApi.createMesh = createMesh;
        }
        SamplerApi _samplerApi;
        OutputUnits _units;
        int _seed{0};
        // cosmology (Configuration.cpp:52-55): redshift of the model and the two distances of an observer at that redshift
        double _modelRedshift{0}, _cosmoAngularDiameterDistance{0}, _cosmoLuminosityDistance{0};
        Random _random;
        bool _oligo{false};
        uint64_t _numPackets{0};
        // source system
        double _ssMinWavelength{0.09e-6}, _ssMaxWavelength{100e-6}, _sourceBias{0.5};
        Array _oligoWavelengths;
        std::vector<SourceModel> _sources;
        // medium system
        pmc_options _options{};
        int _numDensitySamples{100};
        bool _hasMedium{true};                              // Configuration::hasMedium(): false in the NoMedium simulation modes
        std::unique_ptr<XmlElement> _standInMediumSystem;   // (those modes: the empty one-cell medium system the engine runs with)
        std::vector<std::unique_ptr<Medium>> _media;   // the medium components, in ski order (MediumSystem::_media)
        CompositeMedium _composite;                    // all of them as the grid setup sees them: one dust distribution, the electrons apart
        Medium* _medium{nullptr};                      // the only component if it is dust, or the composite
        std::unique_ptr<SpatialGrid> _grid;
        std::vector<char> _topology;
        std::vector<Array> _density;                   // [component][cell] number densities
        std::vector<pmc_medium> _sceneMedia;
        // radiation field
        bool _storeRadiationField{false};
        std::unique_ptr<WavelengthGrid> _rfGridOwn;       // radiationFieldWLG as configured (panchromatic)
        const WavelengthGrid* _rfGrid{nullptr};           // Configuration::radiationFieldWLG()
        std::vector<std::string> _rfProbeNames;           // RadiationFieldProbe items with a PerCellForm
        mutable std::mutex _heatingLock;
        mutable std::unique_ptr<DustHeating> _heating;
        // DensityProbe, OpacityProbe, TemperatureProbe and DustAbsorptionPerCellProbe items
        struct ProbeModel
        {
            std::string type, name, aggregation;  // aggregation: System | Type | Component
            bool afterSetup{true};
            bool projected{false};                // ParallelProjectionForm (else PerCellForm)
            double inclination{0}, azimuth{0}, roll{0}, fieldOfViewX{0}, fieldOfViewY{0}, centerX{0}, centerY{0};
            int numPixelsX{250}, numPixelsY{250}, numSampling{1};
            double wavelength{0.55e-6};               // ConvergenceInfoProbe (SpecialtyWavelengthProbe.hpp)
            std::unique_ptr<WavelengthGrid> ownGrid;  // OpacityProbe::wavelengthGrid (panchromatic only)
            const WavelengthGrid* grid{nullptr};      // Configuration::wavelengthGrid(ownGrid), set by setup()
        };
        std::vector<ProbeModel> _probes;
        struct ProbeQuantity;
        std::vector<ProbeQuantity> probeQuantities(const ProbeModel& probe) const;
        double probeCellValue(const ProbeQuantity& quantity, int value, int m) const;
        // the medium components of a material type, in order: the dust components, or the electron components
        std::vector<int> componentsOfType(bool electrons) const;
        // probes.cpp: what the writers of one writeProbes call share (ProbeOutput), a writer per kind of probe and per form
        struct ProbeOutput;
        struct CutPlane;
        typedef std::function<void(const std::vector<Vec3>& positions, Array& values)> CutValuesFn;
        void writeConvergenceInfo(const ProbeModel& probe, ProbeOutput& out) const;
        void writeConvergenceCuts(const ProbeModel& probe, ProbeOutput& out) const;
        void writeDustAbsorption(const ProbeModel& probe, ProbeOutput& out) const;
        const double* probeTemperatures(const ProbeModel& probe, const ProbeQuantity& q, ProbeOutput& out) const;
        void writePerCell(const ProbeModel& probe, const ProbeQuantity& q, ProbeOutput& out) const;
        void writeProjection(const ProbeModel& probe, const ProbeQuantity& q, ProbeOutput& out) const;
        void writePlanarCut(const std::string& path, const CutPlane& plane, const std::string& quantity, const CutValuesFn& valuesAt, ProbeOutput& out) const;
        // output.cpp: the text file of a PerCellForm; fill computes the values of cell m, in output units
        typedef std::function<void(int m, double* row)> CellRowFn;
        void writePerCellTable(const std::string& path, const std::string& title, const std::string& quantity, const std::string& unit,
                               const Array& outWavelengths, const CellRowFn& fill) const;
        // instruments
        std::unique_ptr<WavelengthGrid> _defaultGrid;     // as configured in the ski (panchromatic)
        std::unique_ptr<WavelengthGrid> _oligoGrid;       // OligoWavelengthGrid
        std::vector<InstrumentModel> _instruments;
        // derived tables referenced by the scene
        // per source: wavelength sampling tables and luminosity; flattened sources and the history index boundaries
        struct SourceTables
        {
            Array oligoWeight, sedLambda, sedp, sedP;
            double luminosity{0};
        };
        std::vector<SourceTables> _sourceTables;
        std::vector<pmc_source> _sceneSources;
        std::vector<uint64_t> _sourceFirst;
        std::vector<pmc_instrument> _pmcInstruments;
        std::vector<pmc_frame_layout> _layouts;
        int64_t _frameSize{0};
        pmc_scene _scene{};
        pmc_scene_ext _sceneExt{};
    };

    // the refusal of a ski file: "ski: <what> is not supported on the MI355X primary-emission path"
    [[noreturn]] void unsupported(const std::string& what);

    // FITS primary image (BITPIX -32) + ASCII table of the third axis, byte-compatible with what the reference
    // produces through CFITSIO (FITSInOut.cpp:127-215)
    struct FitsObserverInfo
    {
        double inclination, azimuth, roll, redshift, luminosityDistance, angularDiameterDistance;
        std::string distanceUnits;
    };
    void writeFitsCube(const std::string& filepath, const double* data, const std::string& dataUnits, int nx, int ny,
                       double incx, double incy, double xc, double yc, const std::string& xyUnits, const Array& z,
                       const std::string& zUnits, const FitsObserverInfo* obsInfo);
}

#endif
