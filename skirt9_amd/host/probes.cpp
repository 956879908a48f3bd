// probes.cpp -- the density, opacity and temperature probes of the spatial grid, per cell and in parallel projection:
//   <prefix>_<probe>_<fileid>.dat            PerCellForm (PerCellForm.cpp:14-38)
//   <prefix>_<probe>_<projectedFileid>.fits  ParallelProjectionForm (ParallelProjectionForm.cpp:18-116)
// restating DensityProbe::probe (DensityProbe.cpp:14-100), OpacityProbe::probe (OpacityProbe.cpp:37-168) and the ProbeFormBridge between a
// probe and its form (ProbeFormBridge.cpp:37-57, 114-136, 548-584, 628-650, 707-725) for the aggregations System, Type and Component.
// The line integrals of a projected map -- ProbeFormBridge::valuesAlongPath -- are not computed here: the caller's integrator walks the
// rays (the engine's pmc_integrate_rays); this file makes the rays and the cell values, averages the sub-samples and writes the files.
// TemperatureProbe (TemperatureProbe.cpp:31-114, dust only) is the one averaged quantity: its cell values are the dust temperatures of
// temperature.cpp -- from the engine's pmc_dust_temperatures or from the host's restatement --, its maps are density-weighted averages along the
// rays (ProbeFormBridge.cpp:61-82, 652-676; the engine's pmc_integrate_weighted_rays returns the raw sums, the division is done here).
// DustAbsorptionPerCellProbe (DustAbsorptionPerCellProbe.cpp:25-63) is a text file from the same radiation field table.

#include "simulation.hpp"
#include "units.hpp"
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <fstream>

namespace skh
{
    // one ProbeFormBridge::writeQuantity call: a scalar (density) or compound (opacity per wavelength) quantity accumulated along paths
    struct Simulation::ProbeQuantity
    {
        enum Kind { MassDensity, NumberDensity, Opacity, Temperature } kind{MassDensity};
        int temperatureRow{0};  // Temperature: the row of the table [H + 1][numCells] of Simulation::dustTemperatures; the weights are the mass density of `components`
        std::string fileid, projectedFileid, quantity, projectedQuantity, description, projectedDescription;
        std::vector<int> components;  // the medium components summed, in order
        bool compound{false};
        Array wave;  // opacity: wavelengths in internal units, in output order
        Array axis;  // ... in output units (the third axis of the FITS file)
        int numValues() const { return compound ? static_cast<int>(axis.size()) : 1; }
    };

    std::vector<int> Simulation::componentsOfType(bool electrons) const
    {
        std::vector<int> components;
        for (int h = 0; h != static_cast<int>(_media.size()); ++h)
            if (_media[h]->mix->isElectrons() == electrons) components.push_back(h);
        return components;
    }

    std::vector<Simulation::ProbeQuantity> Simulation::probeQuantities(const ProbeModel& probe) const
    {
        std::vector<ProbeQuantity> result;
        if (!_hasMedium) return result;  // DensityProbe.cpp:16, OpacityProbe.cpp:39
        const int numMedia = static_cast<int>(_media.size());
        const std::vector<int> dust = componentsOfType(false), electrons = componentsOfType(true);
        std::vector<int> all;
        for (int h = 0; h != numMedia; ++h) all.push_back(h);
        if (probe.type == "DustAbsorptionPerCellProbe") return result;  // (a file of its own kind: writeDustAbsorption)
        if (probe.type == "TemperatureProbe")
        {
            // TemperatureProbe.cpp:45-79: dust only, and only with a panchromatic radiation field (the electron components of this path
            // keep no temperature: hasTemperature, :16-27)
            if (!hasDustHeating()) return result;
            auto add = [&](const std::string& id, const std::vector<int>& components, int row) {
                ProbeQuantity q;
                q.kind = ProbeQuantity::Temperature;
                q.fileid = q.projectedFileid = id + "_T";
                q.quantity = q.projectedQuantity = "temperature";
                q.description = "indicative temperature";
                q.projectedDescription = "density-weighted indicative temperature";
                q.components = components;
                q.temperatureRow = row;
                result.push_back(q);
            };
            if (probe.aggregation == "Type")
                add("dust", dust, static_cast<int>(dust.size()));
            else
                for (size_t b = 0; b != dust.size(); ++b) add(std::to_string(dust[b]), {dust[b]}, static_cast<int>(b));
            return result;
        }
        if (probe.type == "DensityProbe")
        {
            auto add = [&](const std::string& id, bool mass, const std::vector<int>& components) {
                ProbeQuantity q;
                q.kind = mass ? ProbeQuantity::MassDensity : ProbeQuantity::NumberDensity;
                q.fileid = id + (mass ? "_rho" : "_n");
                q.projectedFileid = id + (mass ? "_Sigma" : "_N");
                q.quantity = mass ? "massvolumedensity" : "numbervolumedensity";
                q.projectedQuantity = mass ? "masssurfacedensity" : "numbersurfacedensity";
                q.description = mass ? "mass density" : "number density";
                q.projectedDescription = mass ? "mass surface density" : "column density";
                q.components = components;
                result.push_back(q);
            };
            if (probe.aggregation == "Type")
            {
                if (!dust.empty()) add("dust", true, dust);
                if (!electrons.empty()) add("elec", false, electrons);
            }
            else
                for (int h = 0; h != numMedia; ++h) add(std::to_string(h), !_media[h]->mix->isElectrons(), {h});
        }
        else
        {
            // the wavelengths in output order (OpacityProbe.cpp:44-54; Units::rwavelength, Units.cpp:124-133)
            const WavelengthGrid& wlg = *probe.grid;
            const int numWaves = wlg.numBins();
            const bool reverse = _units.wavelengthStyle != "Wavelength";
            Array wave(numWaves), axis(numWaves);
            for (int i = 0; i != numWaves; ++i)
            {
                const int ell = reverse ? numWaves - 1 - i : i;
                wave[i] = wlg.wavelength(ell);
                axis[i] = _units.owavelength(wlg.wavelength(ell));
            }
            auto add = [&](const std::string& id, const std::vector<int>& components) {
                ProbeQuantity q;
                q.kind = ProbeQuantity::Opacity;
                q.fileid = id + "k";
                q.projectedFileid = id + "tau";
                q.quantity = "opacity";
                q.projectedQuantity = "dimensionless";
                q.description = "opacity";
                q.projectedDescription = "optical depth";
                q.components = components;
                q.compound = true;
                q.wave = wave;
                q.axis = axis;
                result.push_back(q);
            };
            if (probe.aggregation == "System")
                add("", all);
            else if (probe.aggregation == "Type")
            {
                if (!dust.empty()) add("dust_", dust);
                if (!electrons.empty()) add("elec_", electrons);
            }
            else
                for (int h = 0; h != numMedia; ++h) add(std::to_string(h) + "_", {h});
        }
        return result;
    }

    // the value of cell m in internal units: MediumSystem::dustMassDensity / electronNumberDensity / massDensity / numberDensity
    // (MediumSystem.cpp:513-550) and opacityExt over a set of components (:591-624; DustMix.cpp:363-367, ElectronMix.cpp:143-146)
    double Simulation::probeCellValue(const ProbeQuantity& q, int value, int m) const
    {
        double result = 0.;
        for (int h : q.components)
        {
            const double n = _density[h][m];
            const MaterialMix& mix = *_media[h]->mix;
            if (q.kind == ProbeQuantity::MassDensity || q.kind == ProbeQuantity::Temperature)  // (a temperature's weight: MediumSystem.cpp:513-518, 547-550)
                result += n * mix.mass();
            else if (q.kind == ProbeQuantity::NumberDensity)
                result += n;
            else if (mix.isElectrons())
                result += n * mix.sectionSca(q.wave[value]);
            else
                result += n > 0. ? n * mix.sectionExt(q.wave[value]) : 0.;
        }
        return result;
    }

    int Simulation::numProbeMaps() const
    {
        int count = 0;
        for (const ProbeModel& probe : _probes)
            if (probe.projected) count += static_cast<int>(probeQuantities(probe).size());
        return count;
    }

    namespace
    {
        [[noreturn]] void noSuchMap(int map) { throw std::runtime_error("probe map index " + std::to_string(map) + " out of range"); }
    }

    Simulation::ProbeMapInfo Simulation::probeMapInfo(int map) const
    {
        int at = 0;
        for (const ProbeModel& probe : _probes)
        {
            if (!probe.projected) continue;
            for (const ProbeQuantity& q : probeQuantities(probe))
                if (at++ == map)
                {
                    ProbeMapInfo info;
                    info.fileName = _prefix + "_" + probe.name + (q.projectedFileid.empty() ? "" : "_" + q.projectedFileid) + ".fits";
                    info.nx = probe.numPixelsX;
                    info.ny = probe.numPixelsY;
                    info.sampling = probe.numSampling;
                    info.numValues = q.numValues();
                    info.numRays = int64_t(info.nx) * info.ny * info.sampling * info.sampling;
                    info.afterSetup = probe.afterSetup;
                    info.averaged = q.kind == ProbeQuantity::Temperature;
                    return info;
                }
        }
        noSuchMap(map);
    }

    namespace
    {
        // the rays of the rows [j0, j1) of a projection, ordered by pixel (j, i) and sub-sample (is, js): ParallelProjectionForm.cpp:22-51, 67-88
        // with the reference's expressions in their order
        template<typename Probe> void projectionRays(const Probe& form, int j0, int j1, double* origins, double* directions)
        {
            const int Nxp = form.numPixelsX;
            const double xpmin = form.centerX - 0.5 * form.fieldOfViewX;
            const double xpsiz = form.fieldOfViewX / form.numPixelsX;
            const double ypmin = form.centerY - 0.5 * form.fieldOfViewY;
            const double ypsiz = form.fieldOfViewY / form.numPixelsY;
            const int Nsampling = form.numSampling;
            const double costheta = cos(form.inclination);
            const double sintheta = sin(form.inclination);
            const double cosphi = cos(form.azimuth);
            const double sinphi = sin(form.azimuth);
            const double cosomega = cos(form.roll);
            const double sinomega = sin(form.roll);
            // k_z: the direction from observer to model, not normalised again (Direction(..., false))
            const double kzx = -cosphi * sintheta, kzy = -sinphi * sintheta, kzz = -costheta;
            const double zp = 10. * (form.fieldOfViewX + form.fieldOfViewY);
            size_t at = 0;
            for (int j = j0; j != j1; ++j)
                for (int i = 0; i != Nxp; ++i)
                    for (int is = 0; is < Nsampling; ++is)
                        for (int js = 0; js < Nsampling; ++js)
                        {
                            double xp = xpmin + (i + (is + 1.0) / (Nsampling + 1.0)) * xpsiz;
                            double yp = ypmin + (j + (js + 1.0) / (Nsampling + 1.0)) * ypsiz;
                            double xpp = sinomega * xp - cosomega * yp;
                            double ypp = cosomega * xp + sinomega * yp;
                            double zpp = zp;
                            double x = cosphi * costheta * xpp - sinphi * ypp + cosphi * sintheta * zpp;
                            double y = sinphi * costheta * xpp + cosphi * ypp + sinphi * sintheta * zpp;
                            double z = -sintheta * xpp + costheta * zpp;
                            origins[at] = x, origins[at + 1] = y, origins[at + 2] = z;
                            directions[at] = kzx, directions[at + 1] = kzy, directions[at + 2] = kzz;
                            at += 3;
                        }
        }
    }

    void Simulation::probeMapRays(int map, double* origins, double* directions) const
    {
        int at = 0;
        for (const ProbeModel& probe : _probes)
        {
            if (!probe.projected) continue;
            const int count = static_cast<int>(probeQuantities(probe).size());
            if (map < at + count)
            {
                projectionRays(probe, 0, probe.numPixelsY, origins, directions);
                return;
            }
            at += count;
        }
        noSuchMap(map);
    }

    void Simulation::probeMapValues(int map, double* cellValues) const
    {
        int at = 0;
        for (const ProbeModel& probe : _probes)
        {
            if (!probe.projected) continue;
            for (const ProbeQuantity& q : probeQuantities(probe))
                if (at++ == map)
                {
                    const int numCells = _grid->numCells();
                    for (int v = 0; v != q.numValues(); ++v)
                        for (int m = 0; m != numCells; ++m) cellValues[size_t(v) * numCells + m] = probeCellValue(q, v, m);
                    return;
                }
        }
        noSuchMap(map);
    }

    bool Simulation::probesNeedRadiationField(int when) const
    {
        // (MediumSystem::hasDust: without dust neither probe writes a file)
        if (!_hasMedium || !_storeRadiationField || componentsOfType(false).empty()) return false;
        for (const ProbeModel& probe : _probes)
        {
            if (when >= 0 && (when == 0) != probe.afterSetup) continue;
            if (probe.type == "DustAbsorptionPerCellProbe" || (probe.type == "TemperatureProbe" && hasDustHeating())) return true;
        }
        return false;
    }

    // what the writers of one writeProbes call share
    struct Simulation::ProbeOutput
    {
        const ProbeEngine& engine;
        std::string base;                  // <outdir>/<prefix>_
        std::vector<std::string> files;    // written so far
        std::vector<double> temperatures;  // [H + 1][numCells], once a probe has asked for them (Simulation::probeTemperatures)
    };

    // ConvergenceInfoProbe::probe (ConvergenceInfoProbe.cpp:17-175): <prefix>_<probe>_convergence.dat.  Per material type present the input
    // mass against the gridded mass, the input optical depth along the coordinate axes (Medium::opticalDepthX/Y/Z) against the gridded one --
    // two rays per axis from (eps, eps, eps), eps = 1e-15 diagonals of the grid, through the caller's integrator with the opacity of that type
    // as the cell value: MediumSystem::getExtinctionOpticalDepth(path, lambda, type), MediumSystem.cpp:1264-1275 --, then the statistics of the
    // cells' diagonal optical depths.  Line formats: writeValues, StringUtils::toString 'g' with 6 digits, the percentage 'f' with 2
    void Simulation::writeConvergenceInfo(const ProbeModel& probe, ProbeOutput& output) const
    {
        const ProbeEngine& engine = output.engine;
        if (!engine.integrate)
            throw std::runtime_error("probe " + probe.name + " (ConvergenceInfoProbe) needs an integrator for its gridded optical depths");
        const int numMedia = static_cast<int>(_media.size());
        const int numCells = _grid->numCells();
        const double lambda = probe.wavelength;
        auto number = [](double value, char format, int precision) {
            char buf[40];
            snprintf(buf, sizeof(buf), format == 'f' ? "%1.*f" : "%1.*g", precision, value);
            return std::string(buf);
        };
        const std::string path = output.base + probe.name + "_convergence.dat";
        std::ofstream out(path);
        if (!out) throw std::runtime_error("Could not open output file " + path);
        auto line = [&](const std::string& text) { out << text << std::endl; };
        auto writeValues = [&](double t, double g, double factor, const std::string& unit) {
            std::string tail;
            if (!unit.empty()) tail += " " + unit;
            line("  Input:   " + number(t * factor, 'g', 6) + tail);
            if (t > 0) tail += " (" + number(100. * (g - t) / t, 'f', 2) + " %)";
            line("  Gridded: " + number(g * factor, 'g', 6) + tail);
        };
        const std::string atWavelength = number(_units.owavelength(lambda), 'g', 6) + " " + _units.uwavelength();
        line("Spatial grid convergence information");
        line("------------------------------------");
        std::vector<int> all;
        for (int h = 0; h != numMedia; ++h) all.push_back(h);
        for (int kind = 0; kind != 2; ++kind)
        {
            const std::vector<int> components = componentsOfType(kind == 1);
            if (components.empty()) continue;  // MediumSystem::hasDust / hasElectrons
            line("");
            line(std::string("------ ") + (kind ? "Electrons" : "Dust") + " ------");
            double mass_t = 0., mass_g = 0.;
            for (int h : components)
            {
                mass_t += _media[h]->totalMass();
                for (int m = 0; m != numCells; ++m) mass_g += _density[h][m] * _media[h]->mix->mass() * _grid->volume(m);
            }
            line("");
            line("Total mass");
            writeValues(mass_t, mass_g, _units.out("mass", 1.), _units.unit("mass"));
            double tau_t[3] = {0., 0., 0.};
            for (int h : components)
                for (int axis = 0; axis != 3; ++axis) tau_t[axis] += _media[h]->opticalDepth(axis, lambda);
            // the six rays of griddedOpticalDepth: per axis along it and against it
            ProbeQuantity q;
            q.kind = ProbeQuantity::Opacity;
            q.components = components;
            q.wave = Array{lambda};
            std::vector<double> opacity(numCells);
            for (int m = 0; m != numCells; ++m) opacity[m] = probeCellValue(q, 0, m);
            const double eps = 1e-15 * _grid->extent.diagonal();
            double origins[18], directions[18], sums[6] = {0., 0., 0., 0., 0., 0.};
            for (int ray = 0; ray != 6; ++ray)
                for (int a = 0; a != 3; ++a)
                {
                    origins[3 * ray + a] = eps;
                    directions[3 * ray + a] = a == ray / 2 ? (ray % 2 ? -1. : 1.) : (ray % 2 ? -0. : 0.);
                }
            if (engine.integrate(engine.user, 6, origins, directions, 1, opacity.data(), sums) != 0)
                throw std::runtime_error("probe " + probe.name + ": the ray integrator failed");
            const char* axisName[3] = {"X", "Y", "Z"};
            for (int axis = 0; axis != 3; ++axis)
            {
                double tau_g = sums[2 * axis];
                tau_g += sums[2 * axis + 1];
                line("");
                line("Optical depth at " + atWavelength + " along full " + axisName[axis] + "-axis");
                writeValues(tau_t[axis], tau_g, 1., "");
            }
        }
        // writeOpticalDepthStatistics (ConvergenceInfoProbe.cpp:107-145)
        {
            ProbeQuantity q;
            q.kind = ProbeQuantity::Opacity;
            q.components = all;
            q.wave = Array{lambda};
            Array tauV(numCells);
            for (int m = 0; m != numCells; ++m) tauV[m] = _grid->diagonal(m) * probeCellValue(q, 0, m);
            double sum = 0., taumin = tauV[0], taumax = tauV[0];
            for (double tau : tauV)
            {
                sum += tau;
                taumin = std::min(taumin, tau);
                taumax = std::max(taumax, tau);
            }
            const double tauavg = sum / numCells;
            const int numBins = 500;
            std::vector<int> countV(numBins + 1);
            for (double tau : tauV)
            {
                int index = std::max(0, std::min(numBins, static_cast<int>((tau - taumin) / (taumax - taumin) * numBins)));
                countV[index]++;
            }
            int count = 0;
            int index = 0;
            for (; index < numBins; index++)
            {
                count += countV[index];
                if (count > 0.9 * numCells) break;
            }
            const double tau90 = taumin + index * (taumax - taumin) / numBins;
            line("");
            line("------ Cell statistics ------");
            line("");
            line("Optical depth of cell diagonal at " + atWavelength);
            line("  Largest: " + number(taumax, 'g', 6));
            line("  Average: " + number(tauavg, 'g', 6));
            line("  90% <  : " + number(tau90, 'g', 6));
        }
        line("");
        line("------------------------------------");
        output.files.push_back(path);
    }

    // a coordinate plane through the origin: the axes that run (xy: i along x, j along y; xz: x, z; yz: y, z) and its name in file names
    struct Simulation::CutPlane
    {
        bool xd, yd, zd;
        const char* name;
    };

    // PlanarCutsForm::writePlanarCut (PlanarCutsForm.cpp:32-103) as DefaultCutsForm calls it (DefaultCutsForm.cpp:20-34): the grid's bounding
    // box in 1024 x 1024 pixels of a coordinate plane, the values that `valuesAt` gives at the pixel centres -- in output units of `quantity`,
    // [j][i] -- and the axes of the FITS file
    void Simulation::writePlanarCut(const std::string& path, const CutPlane& plane, const std::string& quantity, const CutValuesFn& valuesAt,
                                    ProbeOutput& output) const
    {
        constexpr int Np = 1024, Ni = Np, Nj = Np;
        const Box box = _grid->extent;
        // PlanarCutsForm.cpp:36-44
        const double xpsize = (box.xmax - box.xmin) / Np;
        const double ypsize = (box.ymax - box.ymin) / Np;
        const double zpsize = (box.zmax - box.zmin) / Np;
        const double xbase = box.xmin + 0.5 * xpsize;
        const double ybase = box.ymin + 0.5 * ypsize;
        const double zbase = box.zmin + 0.5 * zpsize;
        const Vec3 center = box.center();
        const double xp = 0., yp = 0., zp = 0.;
        std::vector<Vec3> positions(size_t(Ni) * Nj);
        for (int j = 0; j != Nj; ++j)
        {
            const double z = plane.zd ? (zbase + j * zpsize) : zp;
            for (int i = 0; i != Ni; ++i)
            {
                const double x = plane.xd ? (xbase + i * xpsize) : xp;
                const double y = plane.yd ? (ybase + (plane.zd ? i : j) * ypsize) : yp;
                positions[size_t(j) * Ni + i] = Vec3{x, y, z};
            }
        }
        Array vvv(positions.size(), 0.);
        valuesAt(positions, vvv);
        writeFitsCube(path, vvv.data(), _units.unit(quantity), Ni, Nj, _units.out("length", plane.xd ? xpsize : ypsize),
                      _units.out("length", plane.zd ? zpsize : ypsize), _units.out("length", plane.xd ? center.x : center.y),
                      _units.out("length", plane.zd ? center.z : center.y), _units.unit("length"), Array(), std::string("1"), nullptr);
        output.files.push_back(path);
    }

    // ConvergenceCutsProbe::probe (ConvergenceCutsProbe.cpp:23-60) with its hard-coded DefaultCutsForm: per material type the true density (an
    // InputScalar quantity: the media's own density at the position, times the unit factor) and the gridded density (a GridScalarAccumulated
    // quantity: ProbeFormBridge::valuesAtPosition, the value of the cell at cellIndex(position) times the unit factor, 0 outside) on every
    // coordinate plane of the model's dimension.  The true density is evaluated here (Medium::massDensities / numberDensities: all host cores,
    // or the device sampler of an imported medium); the gridded one by the caller's point sampler, with the unit factor multiplied into the
    // cell values beforehand (valuesInCell: one rounding)
    void Simulation::writeConvergenceCuts(const ProbeModel& probe, ProbeOutput& output) const
    {
        const ProbeEngine& engine = output.engine;
        if (!engine.sample)
            throw std::runtime_error("probe " + probe.name + " (ConvergenceCutsProbe) needs a sampler: hand over the engine's pmc_sample_cells");
        const int numCells = _grid->numCells();
        const int dim = dimension();
        std::vector<CutPlane> planes{{true, true, false, "xy"}};
        if (dim >= 2) planes.push_back({true, false, true, "xz"});
        if (dim == 3) planes.push_back({false, true, true, "yz"});
        std::vector<double> flat, one, cellValues(numCells);
        for (int kind = 0; kind != 2; ++kind)
        {
            const bool mass = kind == 0;
            const std::vector<int> components = componentsOfType(!mass);
            if (components.empty()) continue;  // MediumSystem::hasDust / hasElectrons
            const std::string quantity = mass ? "massvolumedensity" : "numbervolumedensity";
            const double unitFactor = _units.out(quantity, 1.);
            ProbeQuantity q;
            q.kind = mass ? ProbeQuantity::MassDensity : ProbeQuantity::NumberDensity;
            q.components = components;
            for (int m = 0; m != numCells; ++m) cellValues[m] = probeCellValue(q, 0, m) * unitFactor;
            // MediumSystem::dustMassDensity(Position) / electronNumberDensity(Position) (MediumSystem.cpp:456-470): the sum over the components in
            // order, then the unit factor
            const CutValuesFn trueDensity = [&](const std::vector<Vec3>& positions, Array& vvv) {
                for (int h : components)
                {
                    if (mass)
                        _media[h]->massDensities(positions, one);
                    else
                        _media[h]->numberDensities(positions, one);
                    for (size_t p = 0; p != vvv.size(); ++p) vvv[p] += one[p];
                }
                for (double& v : vvv) v *= unitFactor;
            };
            const CutValuesFn griddedDensity = [&](const std::vector<Vec3>& positions, Array& vvv) {
                flat.resize(3 * positions.size());
                for (size_t p = 0; p != positions.size(); ++p)
                    flat[3 * p] = positions[p].x, flat[3 * p + 1] = positions[p].y, flat[3 * p + 2] = positions[p].z;
                if (engine.sample(engine.user, static_cast<int64_t>(positions.size()), flat.data(), 1, cellValues.data(), vvv.data(), nullptr) != 0)
                    throw std::runtime_error("probe " + probe.name + ": the point sampler failed");
            };
            for (int gridded = 0; gridded != 2; ++gridded)
                for (const CutPlane& plane : planes)
                    writePlanarCut(output.base + probe.name + "_" + (mass ? "dust" : "elec") + (gridded ? "_g_" : "_t_") + plane.name + ".fits", plane,
                                   quantity, gridded ? griddedDensity : trueDensity, output);
        }
    }

    // DustAbsorptionPerCellProbe.cpp:25-63: <prefix>_<probe>_Labs.dat, the spectral luminosity that the dust of every cell absorbs
    void Simulation::writeDustAbsorption(const ProbeModel& probe, ProbeOutput& output) const
    {
        const std::vector<int> dust = componentsOfType(false);
        if (!_hasMedium || !_storeRadiationField || dust.empty()) return;  // MediumSystem::hasDust
        const double* rf = output.engine.rf;
        if (!rf) throw std::runtime_error("probe " + probe.name + " needs the radiation field table");
        const WavelengthGrid& wlg = *_rfGrid;
        const int nbins = wlg.numBins();
        const bool reverse = _units.wavelengthStyle != "Wavelength";
        std::vector<int> order(nbins);
        Array outWavelengths(nbins);
        for (int i = 0; i != nbins; ++i)
        {
            order[i] = reverse ? nbins - 1 - i : i;
            outWavelengths[i] = _units.owavelength(wlg.wavelength(order[i]));
        }
        output.files.push_back(output.base + probe.name + "_Labs.dat");
        writePerCellTable(output.files.back(), "Spectral luminosity absorbed by dust per spatial cell", _units.smonluminosity() + "^abs",
                          _units.umonluminosity(), outWavelengths, [&](int m, double* row) {
                              // MediumSystem::meanIntensity (MediumSystem.cpp:1370-1380) and the factor 4 pi V back again
                              const double Jfactor = 1. / (4. * M_PI * _grid->volume(m));
                              const double factor = 4. * M_PI * _grid->volume(m);
                              for (int i = 0; i != nbins; ++i)
                              {
                                  const int ell = order[i];
                                  const double lambda = wlg.wavelength(ell);
                                  const double J = rf[size_t(m) * nbins + ell] * Jfactor / wlg.effectiveWidth(ell);
                                  // MediumSystem::opacityAbs(lambda, m, Dust) (MediumSystem.cpp:599-605; DustMix.cpp:347-351)
                                  double opacity = 0.;
                                  for (int h : dust)
                                  {
                                      const double n = _density[h][m];
                                      opacity += n > 0. ? n * _media[h]->mix->sectionAbs(lambda) : 0.;
                                  }
                                  row[i] = _units.omonluminosity(lambda, J * factor * opacity);
                              }
                          });
    }

    // the row of a temperature quantity in the dust temperatures [H + 1][numCells] (null: another quantity), which are computed when the first
    // probe asks for them: by the engine from the table on the device, else by the host from the caller's copy of it
    const double* Simulation::probeTemperatures(const ProbeModel& probe, const ProbeQuantity& q, ProbeOutput& output) const
    {
        if (q.kind != ProbeQuantity::Temperature) return nullptr;
        const ProbeEngine& engine = output.engine;
        const size_t numCells = size_t(_grid->numCells());
        if (output.temperatures.empty())
        {
            const DustHeating& tables = dustHeating();
            output.temperatures.assign(size_t(tables.flat.num_components + 1) * numCells, 0.);
            if (engine.temperatures)
            {
                if (engine.temperatures(engine.user, &tables.flat, output.temperatures.data()) != 0)
                    throw std::runtime_error("probe " + probe.name + ": the computation of the dust temperatures failed");
            }
            else if (engine.rf)
                dustTemperatures(engine.rf, output.temperatures.data());
            else
                throw std::runtime_error("probe " + probe.name + " needs the radiation field: hand over the table or the engine that holds it");
        }
        return output.temperatures.data() + size_t(q.temperatureRow) * numCells;
    }

    // PerCellForm.cpp:14-38: the values of every cell times the unit factor (ProbeFormBridge::valuesInCell)
    void Simulation::writePerCell(const ProbeModel& probe, const ProbeQuantity& q, ProbeOutput& output) const
    {
        const double* temperature = probeTemperatures(probe, q, output);
        const double unitFactor = _units.out(q.quantity, 1.);
        const int numValues = q.numValues();
        std::string title = q.description + " per spatial cell";
        title[0] = static_cast<char>(std::toupper(static_cast<unsigned char>(title[0])));
        output.files.push_back(output.base + probe.name + (q.fileid.empty() ? "" : "_" + q.fileid) + ".dat");
        writePerCellTable(output.files.back(), title, q.description, _units.unit(q.quantity), q.compound ? q.axis : Array(), [&](int m, double* row) {
            for (int v = 0; v != numValues; ++v) row[v] = (temperature ? temperature[m] : probeCellValue(q, v, m)) * unitFactor;
        });
    }

    // ParallelProjectionForm.cpp:18-116: the rays of the map through the caller's integrator in batches of rows, the sums (of an averaged
    // quantity the weighted sums over the sums of the weights) in output units, averaged over the sub-samples of a pixel
    void Simulation::writeProjection(const ProbeModel& probe, const ProbeQuantity& q, ProbeOutput& output) const
    {
        const ProbeEngine& engine = output.engine;
        const double* temperature = probeTemperatures(probe, q, output);
        const bool averaged = temperature != nullptr;
        if (averaged ? !engine.weighted : !engine.integrate)
            throw std::runtime_error("probe " + probe.name + " is a projected map: it needs an integrator");
        const int numCells = _grid->numCells(), numValues = q.numValues();
        const int Nxp = probe.numPixelsX, Nyp = probe.numPixelsY, Ns = probe.numSampling;
        const int Nsampling2 = Ns * Ns;
        const double projectedUnitFactor = _units.out(q.projectedQuantity, 1.);
        // (an averaged quantity: the weights of the cells -- probeCellValue of a temperature is its weight -- next to the values)
        std::vector<double> cellValues(size_t(numValues) * numCells);
        for (int v = 0; v != numValues; ++v)
            for (int m = 0; m != numCells; ++m) cellValues[size_t(v) * numCells + m] = probeCellValue(q, v, m);
        Array vvv(size_t(numValues) * Nyp * Nxp, 0.);
        // (rows in batches of about a million rays: the rays of a 10000 x 10000 map with 81 samples would not fit in memory at once)
        const int raysPerRow = Nxp * Nsampling2;
        const int rowsPerBatch = std::max(1, (1 << 20) / raysPerRow);
        const int sumsPerRay = averaged ? 2 : numValues;
        std::vector<double> origins, directions, sums;
        for (int j0 = 0; j0 < Nyp; j0 += rowsPerBatch)
        {
            const int j1 = std::min(Nyp, j0 + rowsPerBatch);
            const size_t numRays = size_t(j1 - j0) * raysPerRow;
            origins.resize(3 * numRays);
            directions.resize(3 * numRays);
            sums.assign(numRays * sumsPerRay, 0.);
            projectionRays(probe, j0, j1, origins.data(), directions.data());
            const int rc = averaged ? engine.weighted(engine.user, static_cast<int64_t>(numRays), origins.data(), directions.data(), 1,
                                                      cellValues.data(), temperature, sums.data())
                                    : engine.integrate(engine.user, static_cast<int64_t>(numRays), origins.data(), directions.data(), numValues,
                                                       cellValues.data(), sums.data());
            if (rc != 0) throw std::runtime_error("probe " + probe.name + ": the ray integrator failed");
            size_t ray = 0;
            for (int j = j0; j != j1; ++j)
                for (int i = 0; i != Nxp; ++i)
                    for (int s = 0; s != Nsampling2; ++s, ++ray)
                        for (int p = 0; p != numValues; ++p)
                        {
                            double value;
                            if (averaged)
                            {
                                // valuesAlongPath, GridScalarAveraged: if (totalWeight) value *= unit factor / totalWeight
                                const double totalWeight = sums[ray * 2];
                                value = sums[ray * 2 + 1];
                                if (totalWeight) value *= projectedUnitFactor / totalWeight;
                            }
                            else
                                // valuesAlongPath: the sum times the projected unit factor
                                value = sums[ray * numValues + p] * projectedUnitFactor;
                            // ... then the share of the sub-sample
                            vvv[(size_t(p) * Nyp + j) * Nxp + i] += value / Nsampling2;
                        }
        }
        const double xpsiz = probe.fieldOfViewX / probe.numPixelsX, ypsiz = probe.fieldOfViewY / probe.numPixelsY;
        const std::string path = output.base + probe.name + (q.projectedFileid.empty() ? "" : "_" + q.projectedFileid) + ".fits";
        writeFitsCube(path, vvv.data(), _units.unit(q.projectedQuantity), Nxp, Nyp, _units.out("length", xpsiz), _units.out("length", ypsiz),
                      _units.out("length", probe.centerX), _units.out("length", probe.centerY), _units.unit("length"),
                      q.compound ? q.axis : Array(), q.compound ? _units.uwavelength() : std::string("1"), nullptr);
        output.files.push_back(path);
    }

    std::vector<std::string> Simulation::writeProbes(const ProbeEngine& engine, const std::string& outdir, int when) const
    {
        ProbeOutput output{engine, outdir, {}, {}};
        if (!output.base.empty() && output.base.back() != '/') output.base += '/';
        output.base += _prefix + "_";
        for (const ProbeModel& probe : _probes)
        {
            if (when >= 0 && (when == 0) != probe.afterSetup) continue;
            if (probe.type == "ConvergenceInfoProbe")
            {
                if (_hasMedium) writeConvergenceInfo(probe, output);  // ConvergenceInfoProbe.cpp:152
            }
            else if (probe.type == "ConvergenceCutsProbe")
            {
                if (_hasMedium) writeConvergenceCuts(probe, output);  // ConvergenceCutsProbe.cpp:25
            }
            else if (probe.type == "DustAbsorptionPerCellProbe")
                writeDustAbsorption(probe, output);
            else
                for (const ProbeQuantity& q : probeQuantities(probe))
                    if (probe.projected)
                        writeProjection(probe, q, output);
                    else
                        writePerCell(probe, q, output);
        }
        return output.files;
    }
}


