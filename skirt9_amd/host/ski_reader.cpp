// ski_reader.cpp -- Simulation::parse: the elements of a ski file -> model objects (see simulation.hpp).  Citations: SKIRT 9 tree.
//
// What needs no Simulation state is a free function of (element, Reader) that returns a model object; the readers of whole systems, which store
// into members, are Simulation's and run in document order.  Within every reader the checks stand in the order in which a ski file with several
// defects is to name them: moving one changes which refusal such a file gets.

#include "column_file.hpp"
#include "simulation.hpp"
#include "units.hpp"
#include <sstream>

namespace skh
{
    // attribute access with the reference's defaults (ATTRIBUTE_DEFAULT_VALUE in the class headers), and the two facts about the simulation
    // that the reading of a single element depends on
    struct Reader
    {
        std::string unitSystem{"ExtragalacticUnits"};
        bool oligo{false};
        std::string inputPath{"."};

        double quantity(const XmlElement& e, const char* key, const char* qty, const char* fallback = nullptr) const
        {
            if (e.has(key)) return parseQuantity(e.attr(key), qty, unitSystem);
            if (!fallback)
                throw std::runtime_error("ski: <" + e.name + "> lacks the required attribute '" + key + "'");
            return parseQuantity(fallback, qty, unitSystem);
        }
        double number(const XmlElement& e, const char* key, const char* fallback = nullptr) const
        {
            return quantity(e, key, "", fallback);
        }
        int integer(const XmlElement& e, const char* key, int fallback) const
        {
            if (!e.has(key)) return fallback;
            return std::stoi(squeeze(e.attr(key)));
        }
        bool boolean(const XmlElement& e, const char* key, bool fallback) const
        {
            if (!e.has(key)) return fallback;
            std::string v = squeeze(e.attr(key));
            if (v == "true" || v == "True" || v == "1" || v == "yes") return true;
            if (v == "false" || v == "False" || v == "0" || v == "no") return false;
            throw std::runtime_error("ski: invalid boolean '" + v + "' for attribute " + key);
        }
        std::vector<double> list(const XmlElement& e, const char* key, const char* qty, const char* fallback) const
        {
            return parseQuantityList(e.has(key) ? e.attr(key) : std::string(fallback), qty, unitSystem);
        }
        // the file that the element's filename attribute names: looked up in the input directory unless the path is absolute
        std::string inputFile(const XmlElement& e, const std::string& what) const
        {
            std::string filename = e.attr("filename", "");
            if (filename.empty()) throw std::runtime_error("ski: " + what + " lacks a filename");
            return (filename[0] == '/') ? filename : inputPath + "/" + filename;
        }
    };

    void unsupported(const std::string& what)
    {
        throw std::runtime_error("ski: " + what + " is not supported on the MI355X primary-emission path");
    }

    namespace
    {
        // `name` is one of `supported`, else the refusal of `kind + name`
        void requireOneOf(const std::string& name, std::initializer_list<const char*> supported, const std::string& kind)
        {
            for (const char* one : supported)
                if (name == one) return;
            unsupported(kind + name);
        }

        // ---------------------------------------------------------------- geometries and wavelength grids

        std::unique_ptr<Geometry> makeGeometry(const XmlElement& e, const Reader& rd)
        {
            if (e.name == "UniformBoxGeometry")
                return std::make_unique<UniformBoxGeometry>(
                    Box(rd.quantity(e, "minX", "length"), rd.quantity(e, "minY", "length"), rd.quantity(e, "minZ", "length"),
                        rd.quantity(e, "maxX", "length"), rd.quantity(e, "maxY", "length"), rd.quantity(e, "maxZ", "length")));
            if (e.name == "ExpDiskGeometry")
                return std::make_unique<ExpDiskGeometry>(rd.quantity(e, "scaleLength", "length"),
                                                         rd.quantity(e, "scaleHeight", "length"),
                                                         rd.quantity(e, "minRadius", "length", "0"),
                                                         rd.quantity(e, "maxRadius", "length", "0"),
                                                         rd.quantity(e, "maxZ", "length", "0"));
            if (e.name == "SersicGeometry")
                return std::make_unique<SersicGeometry>(rd.quantity(e, "effectiveRadius", "length"), rd.number(e, "index", "1"));
            if (e.name == "PlummerGeometry") return std::make_unique<PlummerGeometry>(rd.quantity(e, "scaleLength", "length"));
            if (e.name == "GaussianGeometry") return std::make_unique<GaussianGeometry>(rd.quantity(e, "dispersion", "length"));
            if (e.name == "OffsetGeometryDecorator")
            {
                const XmlElement* inner = e.item("geometry");
                if (!inner) throw std::runtime_error("ski: OffsetGeometryDecorator lacks a geometry");
                return std::make_unique<OffsetGeometry>(makeGeometry(*inner, rd),
                                                        Vec3{rd.quantity(e, "offsetX", "length", "0"), rd.quantity(e, "offsetY", "length", "0"),
                                                             rd.quantity(e, "offsetZ", "length", "0")});
            }
            if (e.name == "SpheroidalGeometryDecorator")
            {
                const XmlElement* inner = e.item("geometry");
                if (!inner) throw std::runtime_error("ski: SpheroidalGeometryDecorator lacks a geometry");
                requireOneOf(inner->name, {"SersicGeometry", "PlummerGeometry", "ShellGeometry", "GaussianGeometry"}, "SpheroidalGeometryDecorator of ");
                return std::make_unique<SpheroidalGeometry>(makeGeometry(*inner, rd), rd.number(e, "flattening", "1"));
            }
            if (e.name == "ShellGeometry")
                return std::make_unique<ShellGeometry>(rd.quantity(e, "minRadius", "length"), rd.quantity(e, "maxRadius", "length"),
                                                       rd.number(e, "exponent", "2"));
            if (e.name == "TorusGeometry")
                return std::make_unique<TorusGeometry>(rd.number(e, "exponent", "1"), rd.number(e, "index", "1"),
                                                       rd.quantity(e, "openingAngle", "posangle"), rd.quantity(e, "minRadius", "length"),
                                                       rd.quantity(e, "maxRadius", "length"), rd.boolean(e, "reshapeInnerRadius", false),
                                                       rd.quantity(e, "cutoffRadius", "length", "0"));
            if (e.name == "RingGeometry")
                return std::make_unique<RingGeometry>(rd.quantity(e, "ringRadius", "length"), rd.quantity(e, "width", "length"),
                                                      rd.quantity(e, "height", "length"));
            unsupported("geometry " + e.name);
        }

        std::unique_ptr<WavelengthGrid> makeWavelengthGrid(const XmlElement& e, const Reader& rd)
        {
            auto grid = std::make_unique<WavelengthGrid>();
            if (e.name == "LogWavelengthGrid" || e.name == "LinWavelengthGrid")
            {
                // LogWavelengthGrid.cpp:12-24, LinWavelengthGrid.cpp:12-24
                const bool logScale = e.name == "LogWavelengthGrid";
                double lo = rd.quantity(e, "minWavelength", "wavelength");
                double hi = rd.quantity(e, "maxWavelength", "wavelength");
                int n = rd.integer(e, "numWavelengths", 25);
                if (hi <= lo) throw std::runtime_error("the longest wavelength should be larger than the shortest");
                Array lambdav;
                if (logScale)
                    tab::logGrid(lambdav, lo, hi, n - 1);
                else
                    tab::linearGrid(lambdav, lo, hi, n - 1);
                grid->setWavelengthRange(lambdav, logScale);
            }
            else if (e.name == "ListWavelengthGrid")
            {
                Array lambdav = rd.list(e, "wavelengths", "wavelength", "");
                double rhw = rd.number(e, "relativeHalfWidth", "0");
                if (rhw)
                    grid->setWavelengthBins(lambdav, rhw, false);
                else
                    grid->setWavelengthRange(lambdav, rd.boolean(e, "log", true));
            }
            else
                unsupported("wavelength grid " + e.name);
            return grid;
        }

        // ---------------------------------------------------------------- cosmology

        struct ObserverDistances
        {
            double angularDiameter, luminosity;
        };

        // the model sits at redshift z in a flat universe (FlatUniverseCosmology.cpp:18-53): comoving distance
        // c/H0 * integral of dz' / sqrt(Om (1+z')^3 + 1 - Om) by the midpoint rule on max(2000, 10000 z) intervals
        ObserverDistances flatUniverseDistances(double z, double h, double Om)
        {
            const double front = 10. * constants::pc * constants::c / h;
            const int n = std::max(2000, static_cast<int>(z * 10000));
            const double dz = z / n;
            double sum = 0.;
            for (int i = 0; i != n; ++i)
            {
                const double zp1 = (i + 0.5) * dz + 1.;
                sum += 1. / sqrt(Om * zp1 * zp1 * zp1 + (1. - Om));
            }
            const double comoving = front * z * sum / n;
            return {comoving / (1. + z), comoving * (1. + z)};
        }

        // ---------------------------------------------------------------- sources

        // emission direction of a point source
        void readAngularDistribution(const XmlElement& ad, const Reader& rd, SourceModel& source)
        {
            if (ad.name == "IsotropicAngularDistribution")
            {
                source.angularKind = PMC_ANGULAR_ISOTROPIC;
                return;
            }
            requireOneOf(ad.name, {"LaserAngularDistribution", "ConicalAngularDistribution", "NetzerAngularDistribution"}, "angular distribution ");
            source.angularKind = ad.name == "LaserAngularDistribution"     ? PMC_ANGULAR_LASER
                                 : ad.name == "ConicalAngularDistribution" ? PMC_ANGULAR_CONICAL
                                                                           : PMC_ANGULAR_NETZER;
            // AxAngularDistribution.cpp:12-18, Direction.cpp:61-79: the symmetry axis, normalised
            double x = rd.number(ad, "symmetryX", "0"), y = rd.number(ad, "symmetryY", "0"), z = rd.number(ad, "symmetryZ", "1");
            const double norm = std::sqrt(x * x + y * y + z * z);
            if (!(norm > 0.)) throw std::runtime_error("Symmetry axis direction cannot be null vector");
            x /= norm, y /= norm, z /= norm;
            source.angularAxis = Vec3{x, y, z};
            if (ad.name == "ConicalAngularDistribution") source.angularCosDelta = std::cos(rd.quantity(ad, "openingAngle", "posangle", ""));
        }

        void readPointSource(const XmlElement& src, const Reader& rd, SourceModel& source)
        {
            source.position = Vec3{rd.quantity(src, "positionX", "length", "0"), rd.quantity(src, "positionY", "length", "0"),
                                   rd.quantity(src, "positionZ", "length", "0")};
            // SpecialtySource.cpp:31-50: the bulk velocity; none in an oligochromatic simulation
            const double vx = rd.quantity(src, "velocityX", "velocity", "0"), vy = rd.quantity(src, "velocityY", "velocity", "0"),
                         vz = rd.quantity(src, "velocityZ", "velocity", "0");
            if ((vx || vy || vz) && !rd.oligo)
            {
                source.velocity.kind = PMC_VELOCITY_CONSTANT;
                source.velocity.magnitude = 1.;
                source.velocity.vector[0] = vx, source.velocity.vector[1] = vy, source.velocity.vector[2] = vz;
            }
            if (const XmlElement* ad = src.item("angularDistribution")) readAngularDistribution(*ad, rd, source);
            if (const XmlElement* pp = src.item("polarizationProfile"))
                if (pp->name != "NoPolarizationProfile") unsupported("polarization profile " + pp->name);
        }

        // the geometry of a GeometricSource: one that the engine samples, as it is, flattened and/or shifted
        std::unique_ptr<Geometry> readSourceGeometry(const XmlElement& g, const Reader& rd)
        {
            requireOneOf(g.name, {"SersicGeometry", "UniformBoxGeometry", "ExpDiskGeometry", "PlummerGeometry", "SpheroidalGeometryDecorator",
                                  "OffsetGeometryDecorator"}, "source geometry ");
            std::unique_ptr<Geometry> geometry = makeGeometry(g, rd);
            const Geometry* undecorated = geometry.get();
            if (auto off = dynamic_cast<const OffsetGeometry*>(undecorated)) undecorated = off->inner();
            requireOneOf(undecorated->type(), {"SersicGeometry", "UniformBoxGeometry", "ExpDiskGeometry", "PlummerGeometry", "SpheroidalGeometryDecorator"},
                         "source geometry ");
            if (auto sph = dynamic_cast<const SpheroidalGeometry*>(undecorated))
                requireOneOf(sph->inner()->type(), {"SersicGeometry", "PlummerGeometry"}, "source geometry SpheroidalGeometryDecorator of ");
            return geometry;
        }

        // the velocity field of a GeometricSource, `magnitude` times a vector field that may stand about another centre
        pmc_source_velocity readVelocityField(const XmlElement& vd, double magnitude, const Reader& rd)
        {
            pmc_source_velocity v{};
            v.magnitude = magnitude;
            const XmlElement* field = &vd;
            if (field->name == "OffsetVectorFieldDecorator")
            {
                // OffsetVectorFieldDecorator.cpp:16-21: the field about another centre
                v.vector[0] = rd.quantity(*field, "offsetX", "length", "0"), v.vector[1] = rd.quantity(*field, "offsetY", "length", "0"),
                v.vector[2] = rd.quantity(*field, "offsetZ", "length", "0");
                field = field->item("vectorField");
                if (!field) throw std::runtime_error("ski: OffsetVectorFieldDecorator lacks a vectorField");
            }
            if (field->name == "UnidirectionalVectorField")
            {
                // UnidirectionalVectorField.cpp:11-17: the same unit vector everywhere (an offset changes nothing)
                double x = rd.number(*field, "fieldX", "0"), y = rd.number(*field, "fieldY", "0"), z = rd.number(*field, "fieldZ", "1");
                const double norm = std::sqrt(x * x + y * y + z * z);
                if (norm == 0.) throw std::runtime_error("Field direction cannot be null vector");
                x /= norm, y /= norm, z /= norm;
                v.kind = PMC_VELOCITY_CONSTANT;
                v.vector[0] = x, v.vector[1] = y, v.vector[2] = z;
            }
            else if (field->name == "RadialVectorField" || field->name == "CylindricalVectorField")
            {
                v.kind = field->name == "RadialVectorField" ? PMC_VELOCITY_RADIAL : PMC_VELOCITY_CYLINDRICAL;
                v.unity_radius = rd.quantity(*field, "unityRadius", "length", "0");
                v.exponent = rd.number(*field, "exponent", "1");
            }
            else
                unsupported("vector field " + field->name);
            return v;
        }

        void readGeometricSource(const XmlElement& src, const Reader& rd, SourceModel& source)
        {
            const XmlElement* g = src.item("geometry");
            if (!g) throw std::runtime_error("ski: GeometricSource lacks a geometry");
            source.geometry = readSourceGeometry(*g, rd);
            // GeometricSource.cpp:31-41: the velocity field; none in an oligochromatic simulation
            if (const XmlElement* vd = src.item("velocityDistribution"))
                if (const double magnitude = rd.quantity(src, "velocityMagnitude", "velocity", "0"); magnitude && !rd.oligo)
                    source.velocity = readVelocityField(*vd, magnitude, rd);
        }

        void readSed(const XmlElement& sed, const Reader& rd, SourceModel& source)
        {
            source.sedType = sed.name;
            if (sed.name == "BlackBodySED")
            {
                source.temperature = rd.quantity(sed, "temperature", "temperature", "5000 K");
                return;
            }
            if (sed.name == "ListSED")
            {
                // ListSED.cpp:11-18 with the default unit style (per unit of wavelength)
                if (sed.attr("unitStyle", "wavelengthmonluminosity") != "wavelengthmonluminosity")
                    unsupported("ListSED unitStyle " + sed.attr("unitStyle", ""));
                source.sedInLambda = rd.list(sed, "wavelengths", "wavelength", "");
                source.sedInP = rd.list(sed, "specificLuminosities", "wavelengthmonluminosity", "");
                if (source.sedInLambda.size() != source.sedInP.size())
                    throw std::runtime_error("Number of listed luminosities does not match number of listed wavelengths");
            }
            else if (sed.name == "FileSED")
            {
                // FileSED.cpp:11-18
                for (const Array& row : readColumnFile(rd.inputFile(sed, "FileSED"),
                                                       {{"wavelength", "wavelength", "micron"}, {"specific luminosity", "specific", "W/m"}},
                                                       "spectral energy distribution"))
                {
                    source.sedInLambda.push_back(row[0]);
                    source.sedInP.push_back(row[1]);
                }
            }
            else
                unsupported("SED " + sed.name);
            // TabulatedSED::setupSelfBefore (TabulatedSED.cpp:14-21)
            if (source.sedInLambda.size() < 2) throw std::runtime_error("SED must have at least two wavelength/luminosity pairs");
            if (source.sedInLambda.front() > source.sedInLambda.back())
            {
                std::reverse(source.sedInLambda.begin(), source.sedInLambda.end());
                std::reverse(source.sedInP.begin(), source.sedInP.end());
            }
        }

        void readLuminosityNormalization(const XmlElement& norm, const Reader& rd, SourceModel& source)
        {
            source.normType = norm.name;
            if (norm.name == "SpecificLuminosityNormalization")
            {
                // SpecificLuminosityNormalization.cpp:12-21 with Units::fromFluxStyle (Units.cpp:41-51)
                std::string style = norm.attr("unitStyle", "wavelengthmonluminosity");
                requireOneOf(style, {"wavelengthmonluminosity", "neutralmonluminosity", "frequencymonluminosity"},
                             "SpecificLuminosityNormalization unitStyle ");
                source.normWavelength = rd.quantity(norm, "wavelength", "wavelength");
                double L = rd.quantity(norm, "specificLuminosity", style.c_str());
                const double lambda = source.normWavelength;
                if (style == "neutralmonluminosity") L = L / lambda;
                if (style == "frequencymonluminosity") L = L * constants::c / lambda / lambda;
                source.specificLuminosity = L;
            }
            else if (norm.name != "IntegratedLuminosityNormalization")
                unsupported("luminosity normalization " + norm.name);
            source.normRange = norm.attr("wavelengthRange", "Source");
            source.normMinWavelength = rd.quantity(norm, "minWavelength", "wavelength", "0.09 micron");
            source.normMaxWavelength = rd.quantity(norm, "maxWavelength", "wavelength", "100 micron");
            if (norm.name == "IntegratedLuminosityNormalization")
                source.integratedLuminosity = rd.quantity(norm, "integratedLuminosity", "bolluminosity");
        }

        void readWavelengthBiasDistribution(const XmlElement& bd, const Reader& rd, SourceModel& source)
        {
            source.biasDistType = bd.name;
            if (bd.name == "LogWavelengthDistribution" || bd.name == "LinWavelengthDistribution")
            {
                source.biasMin = rd.quantity(bd, "minWavelength", "wavelength", "1 pm");
                source.biasMax = rd.quantity(bd, "maxWavelength", "wavelength", "1 m");
            }
            else if (bd.name != "DefaultWavelengthDistribution")
                unsupported("wavelength bias distribution " + bd.name);
        }

        SourceModel readSource(const XmlElement& src, const Reader& rd)
        {
            SourceModel source;
            source.type = src.name;
            source.sourceWeight = rd.number(src, "sourceWeight", "1");
            source.wavelengthBias = rd.number(src, "wavelengthBias", "0.5");
            if (src.name == "PointSource")
                readPointSource(src, rd, source);
            else if (src.name == "GeometricSource")
                readGeometricSource(src, rd, source);
            else
                unsupported("source " + src.name);
            if (const XmlElement* sed = src.item("sed")) readSed(*sed, rd, source);
            const XmlElement* norm = src.item("normalization");
            if (!norm) throw std::runtime_error("ski: source lacks a luminosity normalization");
            readLuminosityNormalization(*norm, rd, source);
            if (const XmlElement* bd = src.item("wavelengthBiasDistribution")) readWavelengthBiasDistribution(*bd, rd, source);
            return source;
        }

        // ---------------------------------------------------------------- media

        // A simulation without a medium (MonteCarloSimulation.cpp:557; FluxRecorder.cpp:199: the total flux only).  The engine's
        // life cycle is that of a medium system whose one cell holds no matter: the emission peel-off sees optical depth zero, the
        // path of the packet has optical depth zero, and the history ends (MonteCarloSimulation.cpp:705-709).  One density sample
        // at the cell centre: the setup draws no random number, as the reference's setup without a medium draws none.
        const char* const standInMediumSystem =
            "<mediumSystem type=\"MediumSystem\"><MediumSystem>"
            "<photonPacketOptions type=\"PhotonPacketOptions\"><PhotonPacketOptions explicitAbsorption=\"false\" forceScattering=\"true\" "
            "minWeightReduction=\"1e4\" minScattEvents=\"0\" pathLengthBias=\"0.5\"/></photonPacketOptions>"
            "<media type=\"Medium\"><GeometricMedium>"
            "<geometry type=\"Geometry\"><UniformBoxGeometry minX=\"-1 m\" maxX=\"1 m\" minY=\"-1 m\" maxY=\"1 m\" minZ=\"-1 m\" maxZ=\"1 m\"/></geometry>"
            "<materialMix type=\"MaterialMix\"><MeanListDustMix wavelengths=\"1e-6 micron, 1e6 micron\" extinctionCoefficients=\"1 m2/kg, 1 m2/kg\" "
            "albedos=\"0.5, 0.5\" asymmetryParameters=\"0, 0\"/></materialMix>"
            "<normalization type=\"MaterialNormalization\"><NumberMaterialNormalization number=\"0\"/></normalization>"
            "</GeometricMedium></media>"
            "<samplingOptions type=\"SamplingOptions\"><SamplingOptions numDensitySamples=\"1\"/></samplingOptions>"
            "<grid type=\"SpatialGrid\"><CartesianSpatialGrid minX=\"-1 m\" maxX=\"1 m\" minY=\"-1 m\" maxY=\"1 m\" minZ=\"-1 m\" maxZ=\"1 m\">"
            "<meshX type=\"Mesh\"><LinMesh numBins=\"1\"/></meshX><meshY type=\"Mesh\"><LinMesh numBins=\"1\"/></meshY>"
            "<meshZ type=\"Mesh\"><LinMesh numBins=\"1\"/></meshZ></CartesianSpatialGrid></grid>"
            "</MediumSystem></mediumSystem>";

        pmc_options readPhotonPacketOptions(const XmlElement& ms, const Reader& rd)
        {
            pmc_options options{};
            options.force_scattering = 1;
            options.min_weight_reduction = 1e4;
            options.min_scatt_events = 0;
            options.path_length_bias = 0.5;
            options.explicit_absorption = 0;
            if (const XmlElement* po = ms.item("photonPacketOptions"))
            {
                options.explicit_absorption = rd.boolean(*po, "explicitAbsorption", false) ? 1 : 0;
                options.force_scattering = rd.boolean(*po, "forceScattering", true);
                options.min_weight_reduction = rd.number(*po, "minWeightReduction", "1e4");
                options.min_scatt_events = rd.integer(*po, "minScattEvents", 0);
                options.path_length_bias = rd.number(*po, "pathLengthBias", options.force_scattering ? "0.5" : "0");
            }
            return options;
        }

        // the material of a medium component of type `mediumType`
        std::unique_ptr<MaterialMix> readMaterialMix(const XmlElement& mm, const Reader& rd, const std::string& mediumType)
        {
            requireOneOf(mm.name, {"MeanListDustMix", "MeanFileDustMix", "ElectronMix"}, "material mix ");
            if (mm.name == "ElectronMix")
            {
                // ElectronMix.cpp:24-37, 55-70: unpolarized Thomson scattering only.  Thermal dispersion is ignored by the reference in an
                // oligochromatic simulation (:29), and so it is here; the Compton regime is refused once the wavelength range is known (setup)
                if (rd.boolean(mm, "includePolarization", false)) unsupported("ElectronMix with includePolarization");
                if (rd.boolean(mm, "includeThermalDispersion", false) && !rd.oligo)
                    unsupported("ElectronMix with includeThermalDispersion in a panchromatic simulation");
                // (an ionised gas on an adaptive mesh comes as NumberDensity / Number; for particles it stays out)
                if (mediumType != "GeometricMedium" && mediumType != "AdaptiveMeshMedium") unsupported("ElectronMix in a " + mediumType);
                auto electrons = std::make_unique<ElectronMix>();
                electrons->typeName = mm.name;
                return electrons;
            }
            auto mix = std::make_unique<DustMix>();
            mix->typeName = mm.name;
            if (mm.name == "MeanListDustMix")
            {
                mix->inLambda = rd.list(mm, "wavelengths", "wavelength", "");
                mix->inKappaExt = rd.list(mm, "extinctionCoefficients", "masscoefficient", "");
                mix->inAlbedo = rd.list(mm, "albedos", "", "");
                mix->inAsymmpar = rd.list(mm, "asymmetryParameters", "", "");
                return mix;
            }
            // MeanFileDustMix.cpp:11-22: four columns of a text file (wavelength, kappa_ext, albedo, g)
            auto rows = readColumnFile(rd.inputFile(mm, "MeanFileDustMix"), {{"wavelength", "wavelength", "micron"},
                                                                             {"extinction mass coefficient", "masscoefficient", "m2/kg"},
                                                                             {"scattering albedo", "", ""},
                                                                             {"scattering asymmetry parameter", "", ""}},
                                       "optical dust properties");
            for (const Array& row : rows)
            {
                mix->inLambda.push_back(row[0]);
                mix->inKappaExt.push_back(row[1]);
                mix->inAlbedo.push_back(row[2]);
                mix->inAsymmpar.push_back(row[3]);
            }
            return mix;
        }

        std::unique_ptr<Medium> readGeometricMedium(const XmlElement& med, const Reader& rd)
        {
            auto gm = std::make_unique<GeometricMedium>();
            const XmlElement* mg = med.item("geometry");
            if (!mg) throw std::runtime_error("ski: GeometricMedium lacks a geometry");
            gm->geometry = makeGeometry(*mg, rd);
            const XmlElement* mn = med.item("normalization");
            if (!mn) throw std::runtime_error("ski: GeometricMedium lacks a normalization");
            gm->normType = mn->name;
            if (mn->name == "OpticalDepthMaterialNormalization")
            {
                std::string axis = mn->attr("axis", "Z");
                gm->normAxis = axis.empty() ? 'Z' : axis[0];
                gm->normWavelength = rd.quantity(*mn, "wavelength", "wavelength");
                gm->normOpticalDepth = rd.number(*mn, "opticalDepth");
            }
            else if (mn->name == "MassMaterialNormalization")
                gm->normMass = rd.quantity(*mn, "mass", "mass");
            else if (mn->name == "NumberMaterialNormalization")
                gm->normNumber = rd.number(*mn, "number");
            else
                unsupported("material normalization " + mn->name);
            return gm;
        }

        // what the imported media share (ImportedMedium.hpp): the mass policy options, and the refusals of what is not imported
        void readImportOptions(const XmlElement& med, const Reader& rd, ImportOptions& o)
        {
            o.massFraction = rd.number(med, "massFraction", "1");
            o.importMetallicity = rd.boolean(med, "importMetallicity", false);
            o.importTemperature = rd.boolean(med, "importTemperature", false);
            o.maxTemperature = rd.quantity(med, "maxTemperature", "temperature", "0 K");
            if (rd.boolean(med, "importVelocity", false) && !rd.oligo) unsupported("an imported medium with a velocity field");
            if (rd.boolean(med, "importMagneticField", false)) unsupported("an imported medium with a magnetic field");
            if (rd.boolean(med, "importVariableMixParams", false)) unsupported("an imported medium with a variable material mix");
            if (!med.attr("useColumns", "").empty()) unsupported("useColumns (column remapping)");
        }

        // ParticleMedium (ParticleMedium.hpp, ImportedMedium.hpp): a text column file of smoothed particles
        std::unique_ptr<Medium> readParticleMedium(const XmlElement& med, const Reader& rd)
        {
            auto pm = std::make_unique<ParticleMedium>();
            pm->options.path = rd.inputFile(med, "ParticleMedium");
            std::string massType = med.attr("massType", "Mass");
            requireOneOf(massType, {"Mass", "Number"}, "massType ");
            pm->options.holdsNumber = massType == "Number";
            readImportOptions(med, rd, pm->options);
            if (const XmlElement* sk = med.item("smoothingKernel")) pm->kernelType = sk->name;
            return pm;
        }

        // AdaptiveMeshMedium (AdaptiveMeshMedium.hpp, MeshMedium.hpp, ImportedMedium.hpp): a text column file of the cells of an adaptive mesh
        std::unique_ptr<Medium> readAdaptiveMeshMedium(const XmlElement& med, const Reader& rd)
        {
            auto am = std::make_unique<AdaptiveMeshMedium>();
            MeshImportOptions& o = am->options;
            o.path = rd.inputFile(med, "AdaptiveMeshMedium");
            o.extent = Box(rd.quantity(med, "minX", "length"), rd.quantity(med, "minY", "length"), rd.quantity(med, "minZ", "length"),
                           rd.quantity(med, "maxX", "length"), rd.quantity(med, "maxY", "length"), rd.quantity(med, "maxZ", "length"));
            // MeshMedium.cpp:19-21
            if (o.extent.xmax - o.extent.xmin <= 0) throw std::runtime_error("The extent of the domain should be positive in the X direction");
            if (o.extent.ymax - o.extent.ymin <= 0) throw std::runtime_error("The extent of the domain should be positive in the Y direction");
            if (o.extent.zmax - o.extent.zmin <= 0) throw std::runtime_error("The extent of the domain should be positive in the Z direction");
            // AdaptiveMeshMedium.cpp:21-36
            std::string massType = med.attr("massType", "MassDensity");
            requireOneOf(massType, {"MassDensity", "Mass", "MassDensityAndMass", "NumberDensity", "Number", "NumberDensityAndNumber"}, "massType ");
            o.holdsNumber = massType.compare(0, 6, "Number") == 0;
            o.hasDensity = massType != "Mass" && massType != "Number";
            o.hasMass = massType != "MassDensity" && massType != "NumberDensity";
            readImportOptions(med, rd, o);
            return am;
        }

        std::unique_ptr<Medium> readMedium(const XmlElement& med, const Reader& rd)
        {
            requireOneOf(med.name, {"GeometricMedium", "ParticleMedium", "AdaptiveMeshMedium"}, "medium ");
            if (med.item("velocityDistribution") && rd.quantity(med, "velocityMagnitude", "velocity", "0") && !rd.oligo)
                unsupported("a medium with a velocity field");
            if (med.item("magneticFieldDistribution") && rd.quantity(med, "magneticFieldStrength", "magneticfield", "0"))
                unsupported("a medium with a magnetic field");
            const XmlElement* mm = med.item("materialMix");
            if (!mm) throw std::runtime_error("ski: " + med.name + " lacks a material mix");
            std::unique_ptr<MaterialMix> material = readMaterialMix(*mm, rd, med.name);
            std::unique_ptr<Medium> medium = med.name == "GeometricMedium"  ? readGeometricMedium(med, rd)
                                             : med.name == "ParticleMedium" ? readParticleMedium(med, rd)
                                                                            : readAdaptiveMeshMedium(med, rd);
            medium->mix = std::move(material);
            return medium;
        }

        // ---------------------------------------------------------------- spatial grids

        // TabulatedMesh::setupSelfBefore (TabulatedMesh.cpp:12-33) on ListMesh::getMeshBorderPoints: the normalised border points
        std::vector<double> readListMeshPoints(const XmlElement& mesh)
        {
            std::vector<double> points;
            std::string text = mesh.attr("points", "");
            for (char& ch : text)
                if (ch == ',') ch = ' ';
            std::istringstream in(text);
            for (double v; in >> v;) points.push_back(v);
            std::sort(points.begin(), points.end());
            points.erase(std::unique(points.begin(), points.end()), points.end());
            if (points.size() < 1) throw std::runtime_error("The mesh data file has no points");
            if (points.front() < 0.) throw std::runtime_error("The mesh data file has negative points");
            if (points.front() != 0.) points.insert(points.begin(), 0.);
            if (points.size() < 2 || points.back() == 0.) throw std::runtime_error("The mesh data file has no positive points");
            const double last = points.back();
            for (double& v : points) v /= last;
            return points;
        }

        // the mesh of one axis of a Cartesian grid (property meshX, meshY or meshZ) into `spec`; returns its number of bins
        int readAxisMesh(const XmlElement& grid, const char* property, const Reader& rd, CartesianSpatialGrid::MeshSpec& spec)
        {
            const XmlElement* mesh = grid.item(property);
            if (!mesh) return 100;  // Mesh default numBins
            if (mesh->name == "ListMesh")
            {
                spec.type = mesh->name;
                spec.points = readListMeshPoints(*mesh);
                return static_cast<int>(spec.points.size()) - 1;
            }
            requireOneOf(mesh->name, {"LinMesh", "PowMesh", "SymPowMesh", "LogMesh", "SymLogMesh"}, "mesh ");
            spec.type = mesh->name;
            spec.ratio = rd.number(*mesh, "ratio", "1");
            spec.centralBinFraction = rd.number(*mesh, "centralBinFraction", "1e-3");
            return rd.integer(*mesh, "numBins", 100);
        }

        std::unique_ptr<SpatialGrid> readCartesianGrid(const XmlElement& ge, const Reader& rd)
        {
            auto grid = std::make_unique<CartesianSpatialGrid>();
            grid->nx = readAxisMesh(ge, "meshX", rd, grid->meshSpec[0]);
            grid->ny = readAxisMesh(ge, "meshY", rd, grid->meshSpec[1]);
            grid->nz = readAxisMesh(ge, "meshZ", rd, grid->meshSpec[2]);
            // (the engine stages the three border arrays in LDS: 160 KB hold about 20 000 borders; the cell index is an int32)
            if (grid->nx + grid->ny + grid->nz > 20000 || double(grid->nx) * grid->ny * grid->nz >= 2147483648.)
                unsupported("a Cartesian grid with more than 20000 bins on its three axes together, or 2^31 cells");
            return grid;
        }

        std::unique_ptr<SpatialGrid> readTreeGrid(const XmlElement& ge, const Reader& rd)
        {
            const std::string treeType = ge.attr("treeType", "OctTree");
            requireOneOf(treeType, {"OctTree", "BinTree"}, "treeType ");
            auto grid = std::make_unique<OctreeSpatialGrid>();
            grid->binary = treeType == "BinTree";
            if (const XmlElement* pol = ge.item("policy"))
            {
                if (pol->name != "DensityTreePolicy") unsupported("tree policy " + pol->name);
                grid->minLevel = rd.integer(*pol, "minLevel", 3);
                grid->maxLevel = rd.integer(*pol, "maxLevel", 7);
                grid->maxDustFraction = rd.number(*pol, "maxDustFraction", "1e-6");
                grid->maxDustOpticalDepth = rd.number(*pol, "maxDustOpticalDepth", "0");
                grid->policyWavelength = rd.quantity(*pol, "wavelength", "wavelength", "0.55 micron");
                grid->maxDustDensityDispersion = rd.number(*pol, "maxDustDensityDispersion", "0");
                grid->maxElectronFraction = rd.number(*pol, "maxElectronFraction", "1e-6");
            }
            return grid;
        }

        // VoronoiMeshSpatialGrid.hpp: policies Uniform (random sites), CentralPeak, DustDensity, File (sites from a column text file),
        // ImportedSites (the positions of an imported medium's entities)
        std::unique_ptr<SpatialGrid> readVoronoiGrid(const XmlElement& ge, const Reader& rd)
        {
            auto grid = std::make_unique<VoronoiSpatialGrid>();
            grid->policy = ge.attr("policy", "DustDensity");
            requireOneOf(grid->policy, {"Uniform", "File", "DustDensity", "CentralPeak", "ImportedSites"}, "Voronoi site policy ");
            grid->numSites = rd.integer(ge, "numSites", 500);
            if (grid->policy == "File") grid->sitesPath = rd.inputFile(ge, "VoronoiMeshSpatialGrid");
            grid->relaxSites = rd.boolean(ge, "relaxSites", false);
            return grid;
        }

        std::unique_ptr<SpatialGrid> readSpatialGrid(const XmlElement& ge, const Reader& rd)
        {
            Box extent(rd.quantity(ge, "minX", "length"), rd.quantity(ge, "minY", "length"), rd.quantity(ge, "minZ", "length"),
                       rd.quantity(ge, "maxX", "length"), rd.quantity(ge, "maxY", "length"), rd.quantity(ge, "maxZ", "length"));
            std::unique_ptr<SpatialGrid> grid;
            if (ge.name == "CartesianSpatialGrid")
                grid = readCartesianGrid(ge, rd);
            else if (ge.name == "PolicyTreeSpatialGrid")
                grid = readTreeGrid(ge, rd);
            else if (ge.name == "VoronoiMeshSpatialGrid")
                grid = readVoronoiGrid(ge, rd);
            else
                unsupported("spatial grid " + ge.name);
            grid->extent = extent;
            return grid;
        }

        // ---------------------------------------------------------------- instruments

        // `redshift` and `atRedshift`: the model's, and the distances of an observer there (an instrument without a distance of its own)
        InstrumentModel readInstrument(const XmlElement& ie, const Reader& rd, double redshift, const ObserverDistances& atRedshift)
        {
            InstrumentModel ins;
            ins.type = ie.name;
            requireOneOf(ie.name, {"FrameInstrument", "FullInstrument", "SEDInstrument"}, "instrument ");
            // SEDInstrument (SEDInstrument.cpp:11-22, ApertureInstrument.cpp:11-43): the flux density only, optionally within
            // an aperture radius around the line of sight
            if (ie.name == "SEDInstrument") ins.radius = rd.quantity(ie, "radius", "length", "0");
            ins.name = ie.attr("instrumentName");
            ins.inclination = rd.quantity(ie, "inclination", "posangle", "0 deg");
            ins.azimuth = rd.quantity(ie, "azimuth", "posangle", "0 deg");
            ins.roll = rd.quantity(ie, "roll", "posangle", "0 deg");
            if (ie.name != "SEDInstrument")
            {
                ins.fieldOfViewX = rd.quantity(ie, "fieldOfViewX", "length");
                ins.fieldOfViewY = rd.quantity(ie, "fieldOfViewY", "length");
            }
            ins.centerX = rd.quantity(ie, "centerX", "length", "0");
            ins.centerY = rd.quantity(ie, "centerY", "length", "0");
            ins.numPixelsX = rd.integer(ie, "numPixelsX", 250);
            ins.numPixelsY = rd.integer(ie, "numPixelsY", 250);
            ins.recordComponents = rd.boolean(ie, "recordComponents", false);
            ins.numScatteringLevels = rd.integer(ie, "numScatteringLevels", 0);
            ins.recordPolarization = rd.boolean(ie, "recordPolarization", false);
            ins.recordStatistics = rd.boolean(ie, "recordStatistics", false);
            if (ins.recordPolarization) unsupported("recordPolarization");
            // DistantInstrument.cpp:24-36: a distance puts the instrument in the model's rest frame; distance zero means the
            // observer frame of a model at redshift z > 0 (distances from the cosmology, wavelengths shifted by 1 + z)
            ins.distance = rd.quantity(ie, "distance", "distance", "0");
            if (ins.distance > 0.)
                ins.luminosityDistance = ins.angularDiameterDistance = ins.distance;
            else if (redshift > 0.)
            {
                ins.redshift = redshift;
                ins.luminosityDistance = atRedshift.luminosity;
                ins.angularDiameterDistance = atRedshift.angularDiameter;
            }
            else
                throw std::runtime_error("Instrument distance and model redshift are both zero");
            if (const XmlElement* wg = ie.item("wavelengthGrid")) ins.ownGrid = makeWavelengthGrid(*wg, rd);
            return ins;
        }
    }

    // ================================================================ probes (one reader per kind; the model of a probe is Simulation's own)

    // DustAbsorptionPerCellProbe.hpp: no form, always after the run
    Simulation::ProbeModel Simulation::readDustAbsorptionProbe(const XmlElement& pe, const Reader& rd)
    {
        if (rd.boolean(pe, "writeWavelengthGrid", false)) unsupported("DustAbsorptionPerCellProbe writeWavelengthGrid");
        ProbeModel probe;
        probe.type = pe.name;
        probe.name = pe.attr("probeName", "");
        probe.afterSetup = false;
        return probe;
    }

    // DensityProbe, OpacityProbe, TemperatureProbe: a quantity of the medium with a PerCellForm or a ParallelProjectionForm
    Simulation::ProbeModel Simulation::readFormProbe(const XmlElement& pe, const Reader& rd)
    {
        const bool temperatureProbe = pe.name == "TemperatureProbe";
        ProbeModel probe;
        probe.type = pe.name;
        probe.name = pe.attr("probeName", "");
        // (SpatialGridFormProbe.hpp:23: the default form is DefaultCutsForm)
        const XmlElement* form = pe.item("form");
        const std::string formName = form ? form->name : std::string("DefaultCutsForm");
        requireOneOf(formName, {"PerCellForm", "ParallelProjectionForm"}, temperatureProbe ? "TemperatureProbe form " : "probe form ");
        // (SpatialGridWhenFormProbe.hpp:31: Setup unless the probe is a temperature probe; a temperature probe before the
        // secondary emission phase only warns, TemperatureProbe.cpp:49-54, and one after it needs that phase)
        const std::string after = pe.attr("probeAfter", temperatureProbe ? "Run" : "Setup");
        if (temperatureProbe ? after != "Run" : (after != "Setup" && after != "Run")) unsupported(pe.name + " probeAfter " + after);
        probe.afterSetup = after == "Setup";
        probe.aggregation = pe.attr("aggregation", "Type");
        if (probe.aggregation == "Fragment") unsupported(pe.name + " aggregation Fragment");
        if (probe.aggregation != "Type" && probe.aggregation != "Component" && !(probe.aggregation == "System" && pe.name == "OpacityProbe"))
            throw std::runtime_error("ski: invalid aggregation '" + probe.aggregation + "' for " + pe.name);
        probe.projected = formName == "ParallelProjectionForm";
        if (probe.projected)
        {
            // ParallelProjectionForm.hpp:40-92
            probe.inclination = rd.quantity(*form, "inclination", "posangle", "0 deg");
            probe.azimuth = rd.quantity(*form, "azimuth", "posangle", "0 deg");
            probe.roll = rd.quantity(*form, "roll", "posangle", "0 deg");
            probe.fieldOfViewX = rd.quantity(*form, "fieldOfViewX", "length");
            probe.fieldOfViewY = rd.quantity(*form, "fieldOfViewY", "length");
            probe.centerX = rd.quantity(*form, "centerX", "length", "0");
            probe.centerY = rd.quantity(*form, "centerY", "length", "0");
            probe.numPixelsX = rd.integer(*form, "numPixelsX", 250);
            probe.numPixelsY = rd.integer(*form, "numPixelsY", 250);
            probe.numSampling = rd.integer(*form, "numSampling", 1);
            if (!(probe.fieldOfViewX > 0.) || !(probe.fieldOfViewY > 0.) || probe.numPixelsX < 1 || probe.numPixelsX > 10000
                || probe.numPixelsY < 1 || probe.numPixelsY > 10000 || probe.numSampling < 1 || probe.numSampling > 9)
                throw std::runtime_error("ski: ParallelProjectionForm of probe " + probe.name + ": value out of range");
        }
        if (const XmlElement* wg = pe.item("wavelengthGrid"))
        {
            if (pe.name != "OpacityProbe") throw std::runtime_error("ski: " + pe.name + " has no wavelengthGrid");
            if (rd.oligo) unsupported("OpacityProbe wavelengthGrid in an oligochromatic simulation");
            probe.ownGrid = makeWavelengthGrid(*wg, rd);
        }
        return probe;
    }

    // ConvergenceCutsProbe (ConvergenceCutsProbe.hpp, SpecialtyWhenProbe.hpp:25-31): a name and probeAfter; its form is the hard-coded
    // DefaultCutsForm
    Simulation::ProbeModel Simulation::readConvergenceCutsProbe(const XmlElement& pe, const Reader&)
    {
        ProbeModel probe;
        probe.type = pe.name;
        probe.name = pe.attr("probeName", "");
        const std::string after = pe.attr("probeAfter", "Setup");
        if (after == "Primary" || after == "Secondary") unsupported(pe.name + " probeAfter " + after);
        if (after != "Setup" && after != "Run") throw std::runtime_error("ski: invalid probeAfter '" + after + "' for " + pe.name);
        probe.afterSetup = after == "Setup";
        return probe;
    }

    // ConvergenceInfoProbe (ConvergenceInfoProbe.hpp, SpecialtyWavelengthProbe.hpp:27-31): the same with the wavelength of its optical depths
    Simulation::ProbeModel Simulation::readConvergenceInfoProbe(const XmlElement& pe, const Reader& rd)
    {
        ProbeModel probe = readConvergenceCutsProbe(pe, rd);
        probe.wavelength = rd.quantity(pe, "wavelength", "wavelength", "0.55 micron");
        if (!(probe.wavelength >= 1e-12 && probe.wavelength <= 1.))
            throw std::runtime_error("ski: wavelength of probe " + probe.name + " out of range [1 pm, 1 m]");
        return probe;
    }

    // RadiationFieldProbe with a PerCellForm: its name
    std::string Simulation::readRadiationFieldProbe(const XmlElement& pe, const Reader& rd)
    {
        const XmlElement* form = pe.item("form");
        if (!form || form->name != "PerCellForm") unsupported("probe form " + (form ? form->name : std::string("(none)")));
        if (rd.boolean(pe, "writeWavelengthGrid", false)) unsupported("RadiationFieldProbe writeWavelengthGrid");
        std::string after = pe.attr("probeAfter", "Run");
        requireOneOf(after, {"Run", "Primary"}, "RadiationFieldProbe probeAfter ");
        return pe.attr("probeName", "");
    }

    // ================================================================ the systems, in document order

    void Simulation::parse(const XmlElement& root)
    {
        if (root.name != "skirt-simulation-hierarchy" || root.attr("type", "") != "MonteCarloSimulation")
            throw std::runtime_error("ski: the root element is not a skirt-simulation-hierarchy of type MonteCarloSimulation");
        if (root.children.empty() || root.children[0]->name != "MonteCarloSimulation")
            throw std::runtime_error("ski: missing MonteCarloSimulation element");
        const XmlElement& sim = *root.children[0];

        Reader rd;
        rd.inputPath = _inputPath;
        readUnits(sim, rd);  // first: they determine the default unit of unit-less attribute values
        readMode(sim, rd);
        readRandom(sim, rd);
        readCosmology(sim, rd);
        readSourceSystem(sim, rd);
        const XmlElement& mediumSystem = readMediumSystem(sim, rd);
        const XmlElement* grid = mediumSystem.item("grid");
        if (!grid) throw std::runtime_error("ski: MediumSystem lacks a spatial grid");
        _grid = readSpatialGrid(*grid, rd);
        readInstrumentSystem(sim, rd);
        readProbeSystem(sim, rd);
    }

    void Simulation::readUnits(const XmlElement& sim, Reader& rd)
    {
        const XmlElement* u = sim.item("units");
        if (!u) return;
        if (!unitTable().hasSystem(u->name)) unsupported("unit system " + u->name);
        _units.system = rd.unitSystem = u->name;
        _units.wavelengthStyle = u->attr("wavelengthOutputStyle", "Wavelength");
        _units.fluxStyle = u->attr("fluxOutputStyle", "Frequency");
        if (_units.wavelengthStyle != "Wavelength") unsupported("wavelengthOutputStyle " + _units.wavelengthStyle);
        requireOneOf(_units.fluxStyle, {"Frequency", "Wavelength", "Neutral"}, "fluxOutputStyle ");
    }

    // the simulation mode (Reader::oligo, _hasMedium) and the number of packets
    void Simulation::readMode(const XmlElement& sim, Reader& rd)
    {
        std::string mode = sim.attr("simulationMode", "ExtinctionOnly");
        requireOneOf(mode, {"OligoExtinctionOnly", "ExtinctionOnly", "OligoNoMedium", "NoMedium"}, "simulationMode ");
        // (the modes without a medium: Configuration::hasMedium() is false, the medium system of the ski file -- if any -- is not
        // relevant, and the photon life cycle ends with the emission peel-off, MonteCarloSimulation.cpp:557)
        _oligo = rd.oligo = mode == "OligoExtinctionOnly" || mode == "OligoNoMedium";
        _hasMedium = mode == "OligoExtinctionOnly" || mode == "ExtinctionOnly";
        if (rd.boolean(sim, "iteratePrimaryEmission", false)) unsupported("iteratePrimaryEmission");
        _numPackets = static_cast<uint64_t>(rd.number(sim, "numPackets", "1e6"));  // Configuration.cpp:50
    }

    void Simulation::readRandom(const XmlElement& sim, const Reader& rd)
    {
        const XmlElement* r = sim.item("random");
        if (!r) return;
        if (r->name != "Random") unsupported("random generator " + r->name);
        _seed = rd.integer(*r, "seed", 0);
    }

    void Simulation::readCosmology(const XmlElement& sim, const Reader& rd)
    {
        const XmlElement* c = sim.item("cosmology");
        if (!c) return;
        requireOneOf(c->name, {"FlatUniverseCosmology", "LocalUniverseCosmology"}, "cosmology ");
        if (c->name != "FlatUniverseCosmology") return;
        const double z = rd.number(*c, "redshift", "1");
        const double h = rd.number(*c, "reducedHubbleConstant", "0.675");
        const double Om = rd.number(*c, "matterDensityFraction", "0.310");
        if (!(z > 0.)) unsupported("FlatUniverseCosmology with redshift zero");
        const ObserverDistances distances = flatUniverseDistances(z, h, Om);
        _modelRedshift = z;
        _cosmoAngularDiameterDistance = distances.angularDiameter;
        _cosmoLuminosityDistance = distances.luminosity;
    }

    // SourceSystem.hpp properties
    void Simulation::readSourceSystem(const XmlElement& sim, const Reader& rd)
    {
        const XmlElement* ss = sim.item("sourceSystem");
        if (!ss) throw std::runtime_error("ski: missing sourceSystem");
        _ssMinWavelength = rd.quantity(*ss, "minWavelength", "wavelength", "0.09 micron");
        _ssMaxWavelength = rd.quantity(*ss, "maxWavelength", "wavelength", "100 micron");
        _oligoWavelengths = rd.list(*ss, "wavelengths", "wavelength", "0.55 micron");
        _sourceBias = rd.number(*ss, "sourceBias", "0.5");
        auto sources = ss->items("sources");
        if (sources.empty() || sources.size() > 16) unsupported("a source system with " + std::to_string(sources.size()) + " sources");
        for (const XmlElement* src : sources) _sources.push_back(readSource(*src, rd));
    }

    // RadiationFieldOptions (Configuration.cpp:244-250,476-482): the field is stored on the oligochromatic grid, or on the configured
    // radiationFieldWLG; storing it requires forced scattering (the reference switches it on with a warning)
    void Simulation::readRadiationFieldOptions(const XmlElement& ms, const Reader& rd)
    {
        const XmlElement* rf = ms.item("radiationFieldOptions");
        if (!rf || !rd.boolean(*rf, "storeRadiationField", false)) return;
        _storeRadiationField = true;
        if (!_options.force_scattering) unsupported("storeRadiationField without forceScattering");
        if (rd.oligo) return;
        const XmlElement* wg = rf->item("radiationFieldWLG");
        if (!wg) throw std::runtime_error("ski: RadiationFieldOptions lacks a radiationFieldWLG");
        _rfGridOwn = makeWavelengthGrid(*wg, rd);
    }

    // the options and the components; returns the medium system in effect (the stand-in of a simulation without a medium), which also holds the grid
    const XmlElement& Simulation::readMediumSystem(const XmlElement& sim, const Reader& rd)
    {
        const XmlElement* ms = _hasMedium ? sim.item("mediumSystem") : nullptr;
        if (_hasMedium && !ms)
            throw std::runtime_error("ski: simulationMode " + sim.attr("simulationMode", "ExtinctionOnly") + " needs a medium system");
        if (!ms)
        {
            _standInMediumSystem = XmlParser(standInMediumSystem).parseDocument();
            ms = _standInMediumSystem->children.front().get();
        }
        _options = readPhotonPacketOptions(*ms, rd);
        readRadiationFieldOptions(*ms, rd);
        if (const XmlElement* so = ms->item("samplingOptions")) _numDensitySamples = rd.integer(*so, "numDensitySamples", 100);
        auto media = ms->items("media");
        if (media.empty()) unsupported("a medium system without media");
        if (media.size() > PMC_MAX_MEDIA) unsupported("a medium system with more than " + std::to_string(PMC_MAX_MEDIA) + " media");
        // (a moving source: every emission peel-off packet has its own wavelength -- the engine keeps one cross section per observer, for one
        // component; and the radiation field would need the packet's wavelength per path, which its log does not take)
        if (hasMovingSources() && media.size() > 1) unsupported("a moving source together with more than one medium component");
        if (hasMovingSources() && _storeRadiationField) unsupported("a moving source together with storeRadiationField");
        // (several components: every one a dust medium with spatially constant cross sections --
        // Configuration::hasMultipleConstantSectionMedia, MediumSystem.cpp:874-887)
        for (const XmlElement* med : media) _media.push_back(readMedium(*med, rd));
        bool anyElectrons = false;
        for (auto& part : _media)
        {
            (part->mix->isElectrons() ? _composite.electrons : _composite.parts).push_back(part.get());
            anyElectrons |= part->mix->isElectrons();
        }
        _medium = _media.size() == 1 && !anyElectrons ? _media[0].get() : &_composite;
        return *ms;
    }

    void Simulation::readInstrumentSystem(const XmlElement& sim, const Reader& rd)
    {
        const XmlElement* is = sim.item("instrumentSystem");
        if (!is) throw std::runtime_error("ski: missing instrumentSystem");
        if (const XmlElement* dg = is->item("defaultWavelengthGrid")) _defaultGrid = makeWavelengthGrid(*dg, rd);
        const ObserverDistances atRedshift{_cosmoAngularDiameterDistance, _cosmoLuminosityDistance};
        for (const XmlElement* ie : is->items("instruments")) _instruments.push_back(readInstrument(*ie, rd, _modelRedshift, atRedshift));
        if (_instruments.empty()) unsupported("a simulation without instruments");
    }

    // the radiation field per cell (RadiationFieldProbe + PerCellForm); densities, opacities and dust temperatures per cell and in parallel
    // projection (DensityProbe, OpacityProbe, TemperatureProbe + PerCellForm, ParallelProjectionForm) and the absorbed luminosity per cell
    // (DustAbsorptionPerCellProbe) and the true and gridded density in the coordinate planes (ConvergenceCutsProbe), the
    // convergence information file (ConvergenceInfoProbe): probes.cpp; nothing else is
    // on this path
    void Simulation::readProbeSystem(const XmlElement& sim, const Reader& rd)
    {
        const XmlElement* ps = sim.item("probeSystem");
        if (!ps) return;
        for (const XmlElement* pe : ps->items("probes"))
        {
            if (pe->name == "TemperatureProbe" || pe->name == "DustAbsorptionPerCellProbe")
            {
                // without a panchromatic radiation field the reference writes nothing for these (TemperatureProbe.cpp:45); here the
                // probe is refused instead
                if (rd.oligo) unsupported(pe->name + " in an oligochromatic simulation");
                if (!_storeRadiationField) unsupported(pe->name + " in a simulation that does not store the radiation field");
            }
            if (pe->name == "DustAbsorptionPerCellProbe")
                _probes.push_back(readDustAbsorptionProbe(*pe, rd));
            else if (pe->name == "DensityProbe" || pe->name == "OpacityProbe" || pe->name == "TemperatureProbe")
                _probes.push_back(readFormProbe(*pe, rd));
            else if (pe->name == "ConvergenceCutsProbe")
                _probes.push_back(readConvergenceCutsProbe(*pe, rd));
            else if (pe->name == "ConvergenceInfoProbe")
                _probes.push_back(readConvergenceInfoProbe(*pe, rd));
            else if (pe->name == "RadiationFieldProbe")
                _rfProbeNames.push_back(readRadiationFieldProbe(*pe, rd));
            else
                unsupported("probe " + pe->name);
        }
    }
}
