// simulation.cpp -- construction, setup and scene flattening (see simulation.hpp); the ski file is read in ski_reader.cpp.  Citations: SKIRT 9 tree.
//
// setup() is a sequence of stages: chooseWavelengthGrids | simulationWavelengths | setupMedia | setupGrid | sampleDensities | flattenScene |
// buildSourceTables per source | setLaunchWeights | flattenSources.  Only setupGrid and sampleDensities draw from the random stream, in that order.

#include "simulation.hpp"
#include "../../include/pmc_layout.h"
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>

namespace skh
{
    // ================================================================ construction

    std::unique_ptr<Simulation> Simulation::fromFile(const std::string& path)
    {
        std::ifstream in(path, std::ios::binary);
        if (!in) throw std::runtime_error("Cannot open ski file " + path);
        std::stringstream ss;
        ss << in.rdbuf();
        // output prefix = file name without directory and extension (StringUtils::filenameBase)
        std::string base = path;
        size_t slash = base.find_last_of('/');
        if (slash != std::string::npos) base = base.substr(slash + 1);
        size_t dot = base.find_last_of('.');
        if (dot != std::string::npos) base = base.substr(0, dot);
        // input files named in the ski are looked up in the ski file's directory (the reference: FilePaths::input, i.e.
        // the -i directory or the working directory; SKH_INPUT_PATH overrides)
        std::string dir = slash != std::string::npos ? path.substr(0, slash) : std::string(".");
        if (const char* env = getenv("SKH_INPUT_PATH")) dir = env;
        return fromString(ss.str(), base, dir);
    }

    std::unique_ptr<Simulation> Simulation::fromString(const std::string& text, const std::string& prefix, const std::string& inputPath)
    {
        XmlParser parser(text);
        auto root = parser.parseDocument();
        std::unique_ptr<Simulation> sim(new Simulation());
        sim->_prefix = prefix;
        sim->_inputPath = inputPath;
        sim->parse(*root);
        return sim;
    }

    // ================================================================ setup

    void Simulation::setup()
    {
        _random.setSeed(_seed);
        chooseWavelengthGrids();
        setupMedia(simulationWavelengths());
        setupGrid();
        sampleDensities();
        flattenScene();
        // (the arrays of the tables move with them: the addresses that the flattened source holds stay valid)
        _sourceTables.clear();
        _sceneSources.assign(_sources.size(), pmc_source());
        for (size_t hs = 0; hs != _sources.size(); ++hs)
            _sourceTables.push_back(buildSourceTables(_sources[hs], sourceWavelengthRange(), _oligoGrid.get(), _sceneSources[hs]));
        setLaunchWeights();
        flattenSources();
    }

    // Configuration::wavelengthGrid (Configuration.cpp:666-671): the grid in effect for an instrument or probe that may have one of its own
    const WavelengthGrid* Simulation::gridInEffect(const WavelengthGrid* own) const
    {
        const WavelengthGrid* grid = (own && !_oligo) ? own : defaultWavelengthGrid();
        if (!grid) throw std::runtime_error("Cannot find a wavelength grid for instrument or probe");
        return grid;
    }

    // Configuration: wavelength regime (Configuration.cpp:58-73), the grid in effect of every instrument and every OpacityProbe, and observer
    // sharing (DistantInstrument::determineSameObserverAsPreceding, DistantInstrument.cpp:55-63)
    void Simulation::chooseWavelengthGrids()
    {
        if (_oligo)
        {
            _oligoGrid = std::make_unique<WavelengthGrid>();
            _oligoGrid->setWavelengthBins(_oligoWavelengths, 1e-3, true);  // OligoWavelengthGrid.cpp:20-26
        }
        if (_storeRadiationField) _rfGrid = _oligo ? _oligoGrid.get() : _rfGridOwn.get();
        for (size_t i = 0; i < _instruments.size(); ++i)
        {
            InstrumentModel& ins = _instruments[i];
            ins.grid = gridInEffect(ins.ownGrid.get());
            if (i > 0)
            {
                const InstrumentModel& o = _instruments[i - 1];
                ins.sameObserverAsPreceding = ins.distance == o.distance && ins.inclination == o.inclination
                                              && ins.azimuth == o.azimuth && ins.roll == o.roll;
            }
        }
        for (auto& probe : _probes)
            if (probe.type == "OpacityProbe" && _hasMedium) probe.grid = gridInEffect(probe.ownGrid.get());
    }

    Simulation::WavelengthRange Simulation::sourceWavelengthRange() const
    {
        if (_oligo) return {_oligoGrid->rangeMin(), _oligoGrid->rangeMax()};
        return {_ssMinWavelength, _ssMaxWavelength};
    }

    // Configuration::simulationWavelengthRange / simulationWavelengths (Configuration.cpp:566-661)
    Simulation::SimulationWavelengths Simulation::simulationWavelengths() const
    {
        double rangeMin = sourceWavelengthRange().min, rangeMax = sourceWavelengthRange().max;
        auto extend = [&](double lo, double hi) {
            if (lo < rangeMin) rangeMin = lo;
            if (hi > rangeMax) rangeMax = hi;
        };
        // (a wide margin for kinematics, Configuration.cpp:573, before the grids are added)
        if (hasMovingSources())
        {
            rangeMin /= (1. + 1. / 3.);
            rangeMax *= (1. + 1. / 3.);
        }
        std::set<double> wavelengths;
        auto addGrid = [&](const WavelengthGrid* g) {
            extend(g->rangeMin(), g->rangeMax());
            for (double w : g->lambdav) wavelengths.insert(w);
        };
        auto addWavelength = [&](double w) {
            extend(w, w);
            wavelengths.insert(w);
        };
        if (defaultWavelengthGrid()) addGrid(defaultWavelengthGrid());
        if (_rfGrid && !_oligo) addGrid(_rfGrid);  // Configuration.cpp:576-579,644
        for (auto& ins : _instruments)
            if (ins.ownGrid) addGrid(ins.ownGrid.get());
        // an OpacityProbe's own grid is a MaterialWavelengthRangeInterface item (OpacityProbe.cpp:18-33, Configuration.cpp:594-596, 657-659)
        for (auto& probe : _probes)
            if (probe.ownGrid) addGrid(probe.ownGrid.get());
        // ... and so is a ConvergenceInfoProbe, with the single wavelength it looks at (SpecialtyWavelengthProbe.cpp: Range(wavelength, wavelength))
        for (auto& probe : _probes)
            if (probe.type == "ConvergenceInfoProbe") addWavelength(probe.wavelength);
        // MaterialWavelengthRangeInterface items: the normalisation wavelength and the tree policy wavelength
        for (auto& part : _media)
            if (part->normalizationWavelength() > 0) addWavelength(part->normalizationWavelength());
        if (auto tree = dynamic_cast<OctreeSpatialGrid*>(_grid.get()))
            if (tree->maxDustOpticalDepth > 0 && tree->policyWavelength > 0) addWavelength(tree->policyWavelength);
        rangeMin /= (1. + 1. / 100.);  // Range::extendWithRedshift
        rangeMax *= (1. + 1. / 100.);
        return {{rangeMin, rangeMax}, std::vector<double>(wavelengths.begin(), wavelengths.end())};
    }

    // material mixes, medium normalisation
    void Simulation::setupMedia(const SimulationWavelengths& simulation)
    {
        for (auto& part : _media)
        {
            // (ElectronMix.cpp:36, 116: below the Compton limit the cross section and the phase function are Compton's)
            if (part->mix->isElectrons() && simulation.range.min < ElectronMix::comptonWavelength)
                unsupported("ElectronMix with a source or instrument wavelength below 10 nm (Compton scattering)");
            part->mix->setup(simulation.range.min, simulation.range.max, simulation.wavelengths);
            if (auto imported = dynamic_cast<ImportedMedium*>(part.get())) imported->imported().useDeviceSampler(_samplerApi);
            part->setup();
        }
    }

    // the spatial grid; the construction of a tree or of Voronoi sites draws from the random stream
    void Simulation::setupGrid()
    {
        if (auto cart = dynamic_cast<CartesianSpatialGrid*>(_grid.get()))
            cart->setup();
        else if (auto tree = dynamic_cast<OctreeSpatialGrid*>(_grid.get()))
        {
            if (!_topology.empty())
                tree->setupFromTopology(_topology);
            else
                tree->setup(*_medium, _numDensitySamples, _random);
        }
        else if (auto voro = dynamic_cast<VoronoiSpatialGrid*>(_grid.get()))
            voro->setup(_random, *_medium);
    }

    // MediumSystem::setupSelfAfter density sampling (MediumSystem.cpp:80-106,308-321)
    // (the sample positions of a cell are drawn once and serve every component: PropertySampler::prepareForCell, :80-96)
    void Simulation::sampleDensities()
    {
        int numCells = _grid->numCells();
        const size_t H = _media.size();
        _density.assign(H, Array(numCells, 0.));
        if (_numDensitySamples == 1)
        {
            for (size_t h = 0; h != H; ++h)
                for (int m = 0; m != numCells; ++m) _density[h][m] = _media[h]->numberDensity(_grid->centralPositionInCell(m));
            return;
        }
        // positions from the random stream in cell order, densities on all host cores, sums in sample order; the batch size decides the
        // call sizes of a device sampler
        const int batchCells = std::max(1, (1 << 22) / _numDensitySamples);
        std::vector<Vec3> pos;
        std::vector<double> samples;
        for (int m0 = 0; m0 < numCells; m0 += batchCells)
        {
            const int m1 = std::min(numCells, m0 + batchCells);
            pos.clear();
            for (int m = m0; m != m1; ++m)
                for (int n = 0; n != _numDensitySamples; ++n) pos.push_back(_grid->randomPositionInCell(m, _random));
            for (size_t h = 0; h != H; ++h)
            {
                _media[h]->numberDensities(pos, samples);
                size_t at = 0;
                for (int m = m0; m != m1; ++m)
                {
                    double sum = 0.;
                    for (int n = 0; n != _numDensitySamples; ++n) sum += samples[at++];
                    _density[h][m] = sum / _numDensitySamples;
                }
            }
        }
    }

    // ================================================================ sources: luminosity and wavelength sampling tables

    namespace
    {
        // BlackBodySED (BlackBodySED.cpp:12-39): the Planck function up to a constant factor
        struct Planck
        {
            double f1, f2;
            double operator()(double lambda) const { return f2 / pow(lambda, 5) / (exp(f1 / lambda) - 1.0); }
        };

        bool isTabulated(const SourceModel& source) { return source.sedType != "BlackBodySED"; }

        // NR::cdf<NR::interpolateLogLog>(xv, pv, Pv, inxv, inpv, range) (NR.hpp:494-520): the tabulated function restricted to
        // a range, its end points interpolated, and the normalised cumulative distribution
        double cdfInterpolateLogLog(Array& xv, Array& pv, Array& Pv, const Array& inxv, const Array& inpv, double lo, double hi)
        {
            size_t minRight = std::upper_bound(inxv.begin(), inxv.end(), lo) - inxv.begin();
            size_t maxRight = std::lower_bound(inxv.begin(), inxv.end(), hi) - inxv.begin();
            size_t n = 1 + maxRight - minRight;
            xv.assign(n + 1, 0.);
            size_t i = 0;
            xv[i++] = lo;
            for (size_t j = minRight; j < maxRight;) xv[i++] = inxv[j++];
            xv[i++] = hi;
            pv.assign(n + 1, 0.);
            pv[0] = minRight == 0 ? 0. : tab::logLog(xv[0], inxv[minRight - 1], inxv[minRight], inpv[minRight - 1], inpv[minRight]);
            for (size_t q = 1; q < n; ++q) pv[q] = inpv[minRight + q - 1];
            pv[n] = maxRight == inxv.size()
                        ? 0.
                        : tab::logLog(xv[n], inxv[maxRight - 1], inxv[maxRight], inpv[maxRight - 1], inpv[maxRight]);
            return tab::cumulative(true, xv, pv, Pv);
        }

        // the SED of the source on [lo, hi] with its cumulative distribution; returns the integral over the range
        double sedCdf(const SourceModel& source, const Planck& planck, Array& lambdav, Array& pv, Array& Pv, double lo, double hi)
        {
            if (isTabulated(source)) return cdfInterpolateLogLog(lambdav, pv, Pv, source.sedInLambda, source.sedInP, lo, hi);
            size_t n = std::max(static_cast<size_t>(100), static_cast<size_t>(1000. * log10(hi / lo)));
            tab::logGrid(lambdav, lo, hi, static_cast<int>(n));
            pv.resize(n + 1);
            for (size_t i = 0; i <= n; ++i) pv[i] = planck(lambdav[i]);
            return tab::cumulative(true, lambdav, pv, Pv);
        }

        // the normalised SED at a wavelength: of a tabulated one, whose table has been divided by Ltot, NR::value<NR::interpolateLogLog> (NR.hpp:372-378)
        double specificLuminosity(const SourceModel& source, const Planck& planck, double Ltot, double lambda)
        {
            if (!isTabulated(source)) return planck(lambda) / Ltot;
            int i = tab::bracketOrMiss(source.sedInLambda, lambda);
            if (i < 0 || lambda < source.sedInLambda.front()) return 0.;
            return tab::logLog(lambda, source.sedInLambda[i], source.sedInLambda[i + 1], source.sedInP[i], source.sedInP[i + 1]);
        }

        // IntegratedLuminosityNormalization::luminosityForSED (IntegratedLuminosityNormalization.cpp:12-31) and its specific counterpart
        double sourceLuminosity(const SourceModel& source, const Planck& planck, double Ltot)
        {
            if (source.normType == "SpecificLuminosityNormalization")
            {
                double LlambdaSED = specificLuminosity(source, planck, Ltot, source.normWavelength);
                if (LlambdaSED <= 0) throw std::runtime_error("The normalization wavelength is outside of the SED's wavelength range");
                return source.specificLuminosity / LlambdaSED;
            }
            if (source.normRange == "Source") return source.integratedLuminosity;
            double lo = source.normRange == "Custom" ? source.normMinWavelength : 1e-10;
            double hi = source.normRange == "Custom" ? source.normMaxWavelength : 1;
            if (lo >= hi) throw std::runtime_error("the normalization wavelength range is empty");
            Array a, b, cc;
            double L = sedCdf(source, planck, a, b, cc, lo, hi) / (isTabulated(source) ? 1. : Ltot);
            if (L <= 0) throw std::runtime_error("the normalization luminosity is zero");
            return source.integratedLuminosity / L;
        }
    }

    // the tables of one source, which `flat` refers to, for the source system's wavelength range (and oligochromatic grid, if that is the regime);
    // normalises the table of a tabulated SED in place
    Simulation::SourceTables Simulation::buildSourceTables(SourceModel& source, WavelengthRange sourceRange, const WavelengthGrid* oligoGrid,
                                                           pmc_source& flat)
    {
        SourceTables tables;
        flattenSourceGeometry(source, flat);
        // BlackBodySED (BlackBodySED.cpp:12-39) over the normalisation range = source range
        const double h = constants::h, c = constants::c, k = constants::k;
        double f1 = h * c / (k * source.temperature);
        double f2 = 2.0 * h * c * c;
        const Planck planck{f1, f2};
        const bool tabulated = isTabulated(source);
        // SED::normalizationWavelengthRange (SED.cpp:22-28): the source range intersected with the range on which the SED is tabulated
        // (a black body is defined everywhere); it is also the range NormalizedSource hands to its wavelength bias distribution
        // (NormalizedSource.cpp:50-53, DefaultWavelengthDistribution.cpp:13-22, RangeWavelengthDistribution.cpp:12-19)
        double normMin = sourceRange.min, normMax = sourceRange.max;
        if (tabulated)
        {
            normMin = std::max(normMin, source.sedInLambda.front());
            normMax = std::min(normMax, source.sedInLambda.back());
            if (!(normMin < normMax)) throw std::runtime_error("Intrinsic SED wavelength range does not overlap source wavelength range");
        }
        double Ltot = sedCdf(source, planck, tables.sedLambda, tables.sedp, tables.sedP, normMin, normMax);
        if (tabulated)
            for (double& v : source.sedInP) v /= Ltot;  // TabulatedSED.cpp:20-21 (the later integrals use the normalised table)
        tables.luminosity = sourceLuminosity(source, planck, Ltot);

        if (oligoGrid)
        {
            // NormalizedSource::launch with xi = 1 and OligoWavelengthDistribution (NormalizedSource.cpp:26-29,73-110;
            // OligoWavelengthDistribution.cpp:13-41)
            const Array& lam = oligoGrid->lambdav;
            double probability = 1. / oligoGrid->numBins() / oligoGrid->effectiveWidth(0);
            const double xil = 1.;
            tables.oligoWeight.assign(lam.size(), 0.);
            for (size_t i = 0; i < lam.size(); ++i)
            {
                double s = specificLuminosity(source, planck, Ltot, lam[i]);
                if (!s)
                    tables.oligoWeight[i] = 0.;
                else
                {
                    double b = probability;
                    tables.oligoWeight[i] = s / ((1 - xil) * s + xil * b);
                }
            }
            flat.lambda_mode = PMC_LAMBDA_OLIGO;
            flat.num_oligo = static_cast<int32_t>(lam.size());
            flat.oligo_lambda = lam.data();
            flat.oligo_weight = tables.oligoWeight.data();
            return tables;
        }
        flat.lambda_mode = PMC_LAMBDA_TABULATED;
        flat.lambda_bias = source.wavelengthBias;
        flat.num_sed = static_cast<int32_t>(tables.sedLambda.size());
        flat.sed_lambda = tables.sedLambda.data();
        flat.sed_p = tables.sedp.data();
        flat.sed_P = tables.sedP.data();
        flat.sed_kind = tabulated ? PMC_SED_TABULATED : PMC_SED_BLACKBODY;
        flat.sed_f1 = f1;
        flat.sed_f2 = f2;
        flat.sed_ltot = Ltot;
        // bias distribution range: Default = the source's wavelength range, which is the normalization range of its SED; Log/Lin =
        // the configured range intersected with it
        double lo = normMin, hi = normMax;
        if (source.biasDistType != "DefaultWavelengthDistribution")
        {
            lo = std::max(lo, source.biasMin);
            hi = std::min(hi, source.biasMax);
            if (!(lo < hi)) throw std::runtime_error("Wavelength distribution range does not overlap source wavelength range");
        }
        flat.bias_kind = source.biasDistType == "LinWavelengthDistribution" ? PMC_BIAS_LIN : PMC_BIAS_LOG;
        flat.bias_min = lo;
        flat.bias_max = hi;
        return tables;
    }

    // SourceSystem::setupSelfAfter / prepareForLaunch / launch (SourceSystem.cpp:14-40,75-107): normalised luminosities
    // _Lv, launch weights _Wv (composite bias), history index boundaries _Iv, luminosity per packet
    void Simulation::setLaunchWeights()
    {
        const int Ns = static_cast<int>(_sources.size());
        double Lsys = 0.;
        for (const SourceTables& t : _sourceTables) Lsys += t.luminosity;
        if (!(Lsys > 0.)) throw std::runtime_error("The total luminosity of the source system is zero");
        std::vector<double> Lv(Ns), wv(Ns), wLv(Ns), Wv(Ns);
        for (int hs = 0; hs < Ns; ++hs) Lv[hs] = _sourceTables[hs].luminosity;
        for (int hs = 0; hs < Ns; ++hs) Lv[hs] /= Lsys;
        for (int hs = 0; hs < Ns; ++hs) wv[hs] = _sources[hs].sourceWeight;
        double wLsum = 0., wsum = 0.;
        for (int hs = 0; hs < Ns; ++hs)
        {
            wLv[hs] = wv[hs] * Lv[hs];
            wLsum += wLv[hs];
            wsum += wv[hs];
        }
        const double xi = _sourceBias;
        for (int hs = 0; hs < Ns; ++hs) Wv[hs] = (1 - xi) * wLv[hs] / wLsum + xi * wv[hs] / wsum;
        _sourceFirst.assign(Ns + 1, 0);
        double W = 0.;
        for (int hs = 1; hs < Ns; ++hs)
        {
            // track the cumulative normalised weight as a floating point number and limit the index to numPackets
            W += Wv[hs - 1];
            _sourceFirst[hs] = std::min(_numPackets, static_cast<uint64_t>(std::round(W * _numPackets)));
        }
        _sourceFirst[Ns] = _numPackets;
        const double Lpp = Lsys / _numPackets;
        for (int hs = 0; hs < Ns; ++hs) _sceneSources[hs].packet_luminosity = _numPackets ? Lpp * (Lv[hs] / Wv[hs]) : 0.;
    }

    // ================================================================ scene flattening

    // spatial part of one source (PointSource.cpp:32-43, GeometricSource.cpp:66-82 with the geometry's generatePosition)
    void Simulation::flattenSourceGeometry(const SourceModel& source, pmc_source& s)
    {
        if (source.type == "PointSource")
        {
            s.kind = PMC_SOURCE_POINT;
            s.position[0] = source.position.x;
            s.position[1] = source.position.y;
            s.position[2] = source.position.z;
            s.angular_kind = source.angularKind;
            s.angular_axis[0] = source.angularAxis.x, s.angular_axis[1] = source.angularAxis.y, s.angular_axis[2] = source.angularAxis.z;
            s.angular_cos_delta = source.angularCosDelta;
        }
        const Geometry* shape = source.geometry.get();
        if (auto off = dynamic_cast<const OffsetGeometry*>(shape))
        {
            // OffsetGeometryDecorator::generatePosition: the offset travels in the position member
            shape = off->inner();
            s.position[0] = off->offset().x, s.position[1] = off->offset().y, s.position[2] = off->offset().z;
        }
        double flattening = 0.;
        if (auto sph = dynamic_cast<const SpheroidalGeometry*>(shape))
        {
            shape = sph->inner();
            flattening = sph->flattening();
        }
        if (source.type == "PointSource") {}
        else if (auto sersic = dynamic_cast<const SersicGeometry*>(shape))
        {
            s.kind = PMC_SOURCE_SERSIC;
            s.reff = sersic->effectiveRadius();
            s.sersic_n = static_cast<int32_t>(sersic->profile().radii().size());
            s.sersic_s = sersic->profile().radii().data();
            s.sersic_M = sersic->profile().masses().data();
        }
        else if (auto ubox = dynamic_cast<const UniformBoxGeometry*>(shape))
        {
            s.kind = PMC_SOURCE_UNIFORM_BOX;
            const Box& b = ubox->box();
            double v[6] = {b.xmin, b.ymin, b.zmin, b.xmax, b.ymax, b.zmax};
            std::memcpy(s.box, v, sizeof(v));
        }
        else if (auto disk = dynamic_cast<const ExpDiskGeometry*>(shape))
        {
            s.kind = PMC_SOURCE_EXP_DISK;
            disk->parameters(s.box);
        }
        else if (auto plummer = dynamic_cast<const PlummerGeometry*>(shape))
        {
            s.kind = PMC_SOURCE_PLUMMER;
            s.box[0] = plummer->scaleLength();
        }
        if (flattening) s.box[5] = flattening;  // SpheroidalGeometryDecorator of a Sersic or Plummer source: z -> q z
    }

    // everything of the scene but its sources, and the frame layouts
    void Simulation::flattenScene()
    {
        std::memset(&_scene, 0, sizeof(_scene));
        _scene.abi_version = PMC_ABI_VERSION;
        flattenGrid();
        flattenMedia();
        _scene.options = _options;
        _pmcInstruments.clear();
        for (const InstrumentModel& ins : _instruments) _pmcInstruments.push_back(flattenInstrument(ins));
        _scene.num_instruments = static_cast<int32_t>(_pmcInstruments.size());
        _scene.instruments = _pmcInstruments.data();
        flattenRadiationField();
        _layouts.resize(_instruments.size());
        for (size_t i = 0; i < _instruments.size(); ++i) _frameSize = pmc_layout_compute(&_scene, static_cast<int32_t>(i), &_layouts[i]);
    }

    void Simulation::flattenGrid()
    {
        pmc_grid& g = _scene.grid;
        g.xmin = _grid->extent.xmin;
        g.ymin = _grid->extent.ymin;
        g.zmin = _grid->extent.zmin;
        g.xmax = _grid->extent.xmax;
        g.ymax = _grid->extent.ymax;
        g.zmax = _grid->extent.zmax;
        g.eps = 1e-12 * _grid->extent.diagonal();
        g.num_cells = _grid->numCells();
        _grid->fill(g);
    }

    // the medium components, and the scene's extension: their phase functions and the velocities of the sources
    void Simulation::flattenMedia()
    {
        _sceneMedia.assign(_media.size(), pmc_medium());
        for (size_t h = 0; h != _media.size(); ++h)
        {
            pmc_medium& m = _sceneMedia[h];
            const MaterialMix& mix = *_media[h]->mix;
            m.number_density = _density[h].data();
            m.num_lambda = static_cast<int32_t>(mix.lambdaBorder.size());
            m.lambda_border = mix.lambdaBorder.data();
            m.sigma_ext = mix.sigmaExt.data();
            m.sigma_sca = mix.sigmaSca.data();
            m.sigma_abs = mix.sigmaAbs.data();
            m.asymmpar = mix.asymmpar.data();
        }
        _scene.medium = _sceneMedia[0];
        _scene.num_media = static_cast<int32_t>(_media.size());
        _scene.media = _media.size() > 1 ? _sceneMedia.data() : nullptr;
        _sceneExt = pmc_scene_ext{};
        _sceneExt.struct_size = static_cast<int32_t>(sizeof(pmc_scene_ext));
        for (size_t h = 0; h != _media.size(); ++h) _sceneExt.phase_function[h] = _media[h]->mix->phaseFunction();
        static_assert(PMC_EXT_MAX_SOURCES >= 16, "one velocity per source of the largest source system");
        for (size_t i = 0; i != _sources.size(); ++i) _sceneExt.source_velocity[i] = _sources[i].velocity;
    }

    // one instrument (DistantInstrument.cpp:13-51, FrameInstrument.cpp:12-33, FullInstrument.cpp:11-17)
    pmc_instrument Simulation::flattenInstrument(const InstrumentModel& ins) const
    {
        pmc_instrument p{};
        p.costheta = cos(ins.inclination);
        p.sintheta = sin(ins.inclination);
        p.cosphi = cos(ins.azimuth);
        p.sinphi = sin(ins.azimuth);
        p.cosomega = cos(ins.roll);
        p.sinomega = sin(ins.roll);
        // Direction(theta, phi) (Direction.cpp:11-38)
        const double eps = 1e-8;
        double theta = ins.inclination, phi = ins.azimuth;
        if (theta < -eps || theta > M_PI + eps) throw std::runtime_error("Theta should be between 0 and pi.");
        if (theta <= eps)
            p.kobs[0] = 0, p.kobs[1] = 0, p.kobs[2] = 1;
        else if (theta >= M_PI - eps)
            p.kobs[0] = 0, p.kobs[1] = 0, p.kobs[2] = -1;
        else
        {
            double sintheta = sin(theta);
            p.kobs[0] = sintheta * cos(phi);
            p.kobs[1] = sintheta * sin(phi);
            p.kobs[2] = cos(theta);
        }
        p.nxp = ins.numPixelsX;
        p.nyp = ins.numPixelsY;
        p.xpmin = ins.centerX - 0.5 * ins.fieldOfViewX;
        p.xpsiz = ins.fieldOfViewX / ins.numPixelsX;
        p.ypmin = ins.centerY - 0.5 * ins.fieldOfViewY;
        p.ypsiz = ins.fieldOfViewY / ins.numPixelsY;
        p.same_observer_as_preceding = ins.sameObserverAsPreceding;
        p.include_flux_density = ins.type != "FrameInstrument";
        p.include_surface_brightness = ins.type != "SEDInstrument";
        if (ins.type == "SEDInstrument")
        {
            // no frame: one pixel that covers everything, so that the detection code finds bin 0 (FluxRecorder::detect is
            // called with l = 0, SEDInstrument.cpp:19-22)
            p.nxp = p.nyp = 1;
            p.xpmin = p.ypmin = -0.25 * DBL_MAX;
            p.xpsiz = p.ypsiz = 0.5 * DBL_MAX;
        }
        p.aperture_radius2 = ins.radius * ins.radius;
        // (FluxRecorder.cpp:199: without a medium the total flux is all there is to record)
        p.record_components = ins.recordComponents && _hasMedium;
        p.num_scattering_levels = p.record_components ? ins.numScatteringLevels : 0;
        p.record_statistics = ins.recordStatistics;
        p.redshift = ins.redshift;
        p.num_lambda = ins.grid->numBins();
        p.num_border = static_cast<int32_t>(ins.grid->borderv.size());
        p.border = ins.grid->borderv.data();
        p.ellv = ins.grid->ellv.data();
        return p;
    }

    void Simulation::flattenRadiationField()
    {
        _scene.radiation_field = pmc_radiation_field{};
        if (!_storeRadiationField) return;
        pmc_radiation_field& R = _scene.radiation_field;
        R.store = 1;
        R.num_lambda = _rfGrid->numBins();
        R.num_border = static_cast<int32_t>(_rfGrid->borderv.size());
        R.border = _rfGrid->borderv.data();
        R.ellv = _rfGrid->ellv.data();
    }

    // the last stage: the flattened sources, which hold their packet luminosities by now, into the scene
    void Simulation::flattenSources()
    {
        _scene.source = _sceneSources[0];
        if (_sceneSources.size() > 1)
        {
            _scene.num_sources = static_cast<int32_t>(_sceneSources.size());
            _scene.sources = _sceneSources.data();
            _scene.source_first = _sourceFirst.data();
        }
    }

    std::string Simulation::summary() const
    {
        std::ostringstream s;
        s << "simulation " << _prefix << ": " << (_oligo ? "oligochromatic" : "panchromatic") << ", " << _numPackets
          << " packets, seed " << _seed << "\n";
        s << "  grid: " << (_scene.grid.kind == PMC_GRID_CARTESIAN ? "Cartesian" : _scene.grid.kind == PMC_GRID_VORONOI ? "Voronoi" : _scene.grid.kind == PMC_GRID_BINTREE ? "binary tree" : "octree") << " with " << _scene.grid.num_cells
          << " cells";
        if (_scene.grid.kind == PMC_GRID_OCTREE || _scene.grid.kind == PMC_GRID_BINTREE) s << " (" << _scene.grid.num_nodes << " nodes)";
        s << "\n  dust table: " << _scene.medium.num_lambda << " wavelengths; setup draws: " << _random.draws() << "\n";
        s << "  instruments: " << _instruments.size() << "; frame buffer: " << _frameSize << " doubles\n";
        return s.str();
    }
}
