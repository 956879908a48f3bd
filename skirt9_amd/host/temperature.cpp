// temperature.cpp -- dust temperatures from the stored radiation field: the tables of EquilibriumDustEmissionCalculator::precalculate
// (EquilibriumDustEmissionCalculator.cpp:18-93) and the CPU restatement of the energy balance per cell that the engine's
// pmc_dust_temperatures computes on the GPU: MediumSystem::meanIntensity (MediumSystem.cpp:1370-1380),
// EquilibriumDustEmissionCalculator::equilibriumTemperature (:120-130), MediumSystem::indicativeTemperature (MediumSystem.cpp:1384-1427).

#include "simulation.hpp"
#include <cmath>

namespace skh
{
    bool Simulation::hasDustHeating() const
    {
        // Configuration::hasPanRadiationField and MediumSystem::hasDust (TemperatureProbe.cpp:45)
        if (!_hasMedium || !_storeRadiationField || _oligo || !_rfGrid || !_grid) return false;
        for (const auto& part : _media)
            if (!part->mix->isElectrons()) return true;
        return false;
    }

    const Simulation::DustHeating& Simulation::dustHeating() const
    {
        std::lock_guard<std::mutex> guard(_heatingLock);
        if (_heating) return *_heating;
        if (!hasDustHeating())
            throw std::runtime_error("dust temperatures need a panchromatic simulation that stores the radiation field and has a dust component");
        auto tables = std::make_unique<DustHeating>();
        DustHeating& D = *tables;
        const int numMedia = static_cast<int>(_media.size());
        for (int h = 0; h != numMedia; ++h)
            if (!_media[h]->mix->isElectrons()) D.components.push_back(h);
        const int H = static_cast<int>(D.components.size());

        // the radiation field grid (:26-35)
        const int n = _rfGrid->numBins();
        D.lambda.resize(n);
        D.width.resize(n);
        for (int k = 0; k != n; ++k)
        {
            D.lambda[k] = _rfGrid->wavelength(k);
            D.width[k] = _rfGrid->effectiveWidth(k);
        }
        // (the CMB source term stays zero: includeHeatingByCMB belongs to the dust emission options, :39-45)

        // NR::buildPowerLawGrid(_Tv, 0., 5000., 1000, 500.) (NR.hpp:221-235)
        {
            const int bins = 1000;
            const double xmin = 0., xmax = 5000., ratio = 500.;
            D.temperature.resize(bins + 1);
            const double range = xmax - xmin;
            const double q = pow(ratio, 1. / (bins - 1));
            const double qn = pow(q, bins);
            for (int i = 0; i <= bins; ++i) D.temperature[i] = xmin + (1. - pow(q, i)) / (1. - qn) * range;
        }
        const size_t numT = D.temperature.size();

        D.sigma.assign(size_t(H) * n, 0.);
        D.planckabs.assign(size_t(H) * numT, 0.);
        for (int b = 0; b != H; ++b)
        {
            const auto& mix = static_cast<const DustMix&>(*_media[D.components[b]]->mix);
            Array lambdav, sigmaabsv;
            mix.heatingSamples(lambdav, sigmaabsv);
            // NR::resample<NR::interpolateLogLog> (:60; NR.hpp:373-378, 411-417): zero outside the mix's own grid
            for (int k = 0; k != n; ++k)
            {
                const double x = D.lambda[k];
                const int i = tab::bracketOrMiss(lambdav, x);
                D.sigma[size_t(b) * n + k] = (i < 0 || x < lambdav.front()) ? 0. : tab::logLog(x, lambdav[i], lambdav[i + 1], sigmaabsv[i], sigmaabsv[i + 1]);
            }
            // the Planck-integrated absorption on the temperature grid (:71-91; PlanckFunction.cpp:12-27)
            const size_t numLambda = lambdav.size();
            double* planckabsv = D.planckabs.data() + size_t(b) * numT;
            const Array& Tv = D.temperature;
            parallelFor(numT, [&](size_t begin, size_t end) {
                for (size_t p = begin; p != end; ++p)
                {
                    if (!p) continue;  // (the value at T = 0 stays zero)
                    const double f1 = constants::h * constants::c / (constants::k * Tv[p]);
                    const double f2 = 2.0 * constants::h * constants::c * constants::c;
                    double planckabs = 0.;
                    for (size_t j = 1; j != numLambda; ++j)  // (the first wavelength only bounds the first bin)
                    {
                        const double lambda = lambdav[j];
                        const double dlambda = lambdav[j] - lambdav[j - 1];
                        const double B = f2 / pow(lambda, 5) / (exp(f1 / lambda) - 1.0);
                        planckabs += sigmaabsv[j] * B * dlambda;
                    }
                    planckabsv[p] = planckabs;
                }
            });
        }

        // per cell: 1 / (4 pi V) (MediumSystem.cpp:1374) and the mass densities n * mu (:547-550)
        const int numCells = _grid->numCells();
        D.cellFactor.resize(numCells);
        for (int m = 0; m != numCells; ++m) D.cellFactor[m] = 1. / (4. * M_PI * _grid->volume(m));
        D.massDensity.resize(size_t(H) * numCells);
        for (int b = 0; b != H; ++b)
        {
            const int h = D.components[b];
            const double mass = _media[h]->mix->mass();
            for (int m = 0; m != numCells; ++m) D.massDensity[size_t(b) * numCells + m] = _density[h][m] * mass;
        }

        D.flat.num_components = H;
        D.flat.num_lambda = n;
        D.flat.num_temperatures = static_cast<int32_t>(numT);
        D.flat.num_cells = numCells;
        D.flat.width = D.width.data();
        D.flat.sigma = D.sigma.data();
        D.flat.planckabs = D.planckabs.data();
        D.flat.temperature = D.temperature.data();
        D.flat.cell_factor = D.cellFactor.data();
        D.flat.mass_density = D.massDensity.data();
        _heating = std::move(tables);
        return *_heating;
    }

    void Simulation::dustTemperatures(const pmc_dust_heating& T, const double* rf, double* out)
    {
        const int H = T.num_components, n = T.num_lambda, numT = T.num_temperatures;
        const size_t numCells = static_cast<size_t>(T.num_cells);
        if (H < 1 || n < 1 || numT < 2) throw std::runtime_error("dust temperatures: empty tables");
        // NR::clampedValue<NR::interpolateLinLin>(x, xv, yv) (NR.hpp:168-173, 328-331, 394-401)
        const auto clampedLinLin = [numT](double x, const double* xv, const double* yv) {
            int i;
            if (x == xv[numT - 1])
                i = numT - 2;
            else
            {
                int jl = -1, ju = numT;
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
            if (i >= numT - 1) return yv[numT - 1];
            return tab::linLin(x, xv[i], xv[i + 1], yv[i], yv[i + 1]);
        };
        parallelFor(numCells, [&](size_t begin, size_t end) {
            std::vector<double> Jv(n);
            for (size_t m = begin; m != end; ++m)
            {
                // MediumSystem::meanIntensity
                const double factor = T.cell_factor[m];
                for (int ell = 0; ell != n; ++ell) Jv[ell] = rf[m * n + ell] * factor / T.width[ell];
                double sumRhoT = 0., sumRho = 0.;
                for (int b = 0; b != H; ++b)
                {
                    const double rho = T.mass_density[size_t(b) * numCells + m];
                    double temperature = 0.;
                    if (rho > 0.)
                    {
                        // (_rfsigmaabsvv[b] * (Jv + _Bcmbv) * _rfdlambdav).sum(): the sum of a valarray expression runs from its last element
                        // down to its first (libstdc++ _Expr::sum)
                        const double* sigma = T.sigma + size_t(b) * n;
                        double inputabs = sigma[n - 1] * Jv[n - 1] * T.width[n - 1];
                        for (int ell = n - 2; ell >= 0; --ell) inputabs += sigma[ell] * Jv[ell] * T.width[ell];
                        if (inputabs > 0.) temperature = clampedLinLin(inputabs, T.planckabs + size_t(b) * numT, T.temperature);
                        sumRhoT += rho * temperature;
                        sumRho += rho;
                    }
                    out[size_t(b) * numCells + m] = temperature;
                }
                out[size_t(H) * numCells + m] = sumRho > 0. ? sumRhoT / sumRho : 0.;
            }
        });
    }
}
