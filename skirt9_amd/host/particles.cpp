// particles.cpp -- see particles.hpp
#include "particles.hpp"
#include <limits>
#include <stdexcept>

namespace skh
{
    // ================================================================ smoothing kernels

    namespace
    {
        // CubicSplineSmoothingKernel.cpp:40-50
        class CubicSplineSmoothingKernel : public SmoothingKernel
        {
        public:
            std::string type() const override { return "CubicSplineSmoothingKernel"; }
            double density(double u) const override
            {
                if (!(u >= 0.0 && u < 1.0)) return 0.0;
                const double norm = 8.0 / M_PI;
                const double rest = 1.0 - u;
                if (u < 0.5) return norm * (1.0 - 6.0 * u * u * rest);  // inner half: 1 - 6 u^2 (1 - u)
                return norm * 2.0 * rest * rest * rest;                 // outer half: 2 (1 - u)^3
            }
        };
        // ScaledGaussianSmoothingKernel.cpp:16-47
        class ScaledGaussianSmoothingKernel : public SmoothingKernel
        {
        public:
            std::string type() const override { return "ScaledGaussianSmoothingKernel"; }
            double density(double u) const override
            {
                // front factor and exponent of the Gaussian truncated at the smoothing length
                static const double front = 2.56810060330949540082, exponent = -5.85836755024609305208;
                if (!(u >= 0. && u <= 1.)) return 0.;
                return front * exp(exponent * u * u);
            }
        };
        // UniformSmoothingKernel.cpp:13-17
        class UniformSmoothingKernel : public SmoothingKernel
        {
        public:
            std::string type() const override { return "UniformSmoothingKernel"; }
            double density(double u) const override
            {
                return (u >= 0.0 && u <= 1.0) ? 0.75 / M_PI : 0.0;
            }
        };
    }

    std::unique_ptr<SmoothingKernel> SmoothingKernel::create(const std::string& type)
    {
        if (type == "CubicSplineSmoothingKernel") return std::make_unique<CubicSplineSmoothingKernel>();
        if (type == "ScaledGaussianSmoothingKernel") return std::make_unique<ScaledGaussianSmoothingKernel>();
        if (type == "UniformSmoothingKernel") return std::make_unique<UniformSmoothingKernel>();
        throw std::runtime_error("smoothing kernel " + type + " is not supported on the MI355X path");
    }

    // ================================================================ block search grid (BoxSearch.cpp:14-127)

    namespace
    {
        // Separators of one axis that put about the same number of entity centres into every slab: a histogram of the
        // centres with 100 bins per slab, then a separator at the upper edge of the bin in which the running count passes
        // the next multiple of (entities / slabs) -- at most one separator per bin; separators that are never reached stay
        // zero, the outermost ones are infinite.
        Array balancedSeparators(const Array& centres, int slabs, double lower, double upper)
        {
            if (lower == upper)
            {
                // a degenerate extent is widened by a relative 1e-12
                const double margin = 1e-12 * (lower ? std::abs(lower) : 1.);
                lower -= margin;
                upper += margin;
            }
            const int bins = slabs * 100;
            const double width = (upper - lower) / bins;
            std::vector<int> histogram(bins);
            for (double centre : centres) histogram[static_cast<int>((centre - lower) / width)] += 1;

            const double quota = static_cast<double>(centres.size()) / slabs;
            const double infinite = std::numeric_limits<double>::infinity();
            Array separators(slabs + 1, 0.);
            separators.front() = -infinite;
            separators.back() = infinite;
            int running = 0, next = 1;
            for (int bin = 0; bin < bins && next < slabs; ++bin)
            {
                running += histogram[bin];
                if (running > quota * next) separators[next++] = lower + (bin + 1) * width;
            }
            return separators;
        }

        // does the sphere (centre c, radius r) reach into the box?  The squared radius minus the squared distance from
        // the centre to the box, accumulated axis by axis (Box.cpp:91-109)
        bool sphereReachesBox(const Box& box, double cx, double cy, double cz, double r)
        {
            auto outside = [](double c, double low, double high) { return c < low ? c - low : c > high ? c - high : 0.; };
            const double ex = outside(cx, box.xmin, box.xmax);
            const double ey = outside(cy, box.ymin, box.ymax);
            const double ez = outside(cz, box.zmin, box.zmax);
            double remaining = r * r;
            remaining -= ex * ex;
            remaining -= ey * ey;
            remaining -= ez * ez;
            return remaining >= 0.;
        }
    }

    template<class Bounds, class Intersects> void BoxSearch::loadEntities(int numEntities, Bounds bounds, Intersects intersects)
    {
        _listv.clear();
        _extent = Box();
        _numBlocks = 0;
        if (numEntities <= 0) return;

        // bounding boxes, their union, and their centres per axis
        std::vector<Box> boxes(numEntities);
        Array midX(numEntities), midY(numEntities), midZ(numEntities);
        for (int m = 0; m != numEntities; ++m)
        {
            const Box box = bounds(m);
            boxes[m] = box;
            midX[m] = 0.5 * (box.xmin + box.xmax);
            midY[m] = 0.5 * (box.ymin + box.ymax);
            midZ[m] = 0.5 * (box.zmin + box.zmax);
            if (m == 0) _extent = box;
            _extent = Box(std::min(_extent.xmin, box.xmin), std::min(_extent.ymin, box.ymin), std::min(_extent.zmin, box.zmin),
                          std::max(_extent.xmax, box.xmax), std::max(_extent.ymax, box.ymax), std::max(_extent.zmax, box.zmax));
        }
        _numBlocks = std::max(10, static_cast<int>(std::cbrt(numEntities)));
        _xgrid = balancedSeparators(midX, _numBlocks, _extent.xmin, _extent.xmax);
        _ygrid = balancedSeparators(midY, _numBlocks, _extent.ymin, _extent.ymax);
        _zgrid = balancedSeparators(midZ, _numBlocks, _extent.zmin, _extent.zmax);

        // every entity is listed in the blocks its bounding box overlaps and it actually intersects; entities are visited in
        // index order, so every list is ascending
        _listv.resize(static_cast<size_t>(_numBlocks) * _numBlocks * _numBlocks);
        struct Span
        {
            int first, last;
        };
        auto span = [](const Array& separators, double low, double high) {
            return Span{tab::bracketClipped(separators, low), tab::bracketClipped(separators, high)};
        };
        for (int m = 0; m != numEntities; ++m)
        {
            const Box& box = boxes[m];
            const Span sx = span(_xgrid, box.xmin, box.xmax), sy = span(_ygrid, box.ymin, box.ymax), sz = span(_zgrid, box.zmin, box.zmax);
            for (int i = sx.first; i <= sx.last; ++i)
                for (int j = sy.first; j <= sy.last; ++j)
                    for (int k = sz.first; k <= sz.last; ++k)
                    {
                        const Box block(_xgrid[i], _ygrid[j], _zgrid[k], _xgrid[i + 1], _ygrid[j + 1], _zgrid[k + 1]);
                        if (intersects(m, block)) _listv[blockIndex(i, j, k)].push_back(m);
                    }
        }
    }

    const std::vector<int>& BoxSearch::entitiesFor(Vec3 r) const
    {
        if (!_numBlocks) return _empty;
        int i = tab::bracketClipped(_xgrid, r.x);
        int j = tab::bracketClipped(_ygrid, r.y);
        int k = tab::bracketClipped(_zgrid, r.z);
        return _listv[blockIndex(i, j, k)];
    }

    void BoxSearch::flatten(std::vector<int64_t>& start, std::vector<int32_t>& list) const
    {
        start.assign(_listv.size() + 1, 0);
        list.clear();
        for (size_t b = 0; b != _listv.size(); ++b)
        {
            start[b] = static_cast<int64_t>(list.size());
            list.insert(list.end(), _listv[b].begin(), _listv[b].end());
        }
        start[_listv.size()] = static_cast<int64_t>(list.size());
    }

    size_t BoxSearch::numReferences() const
    {
        size_t n = 0;
        for (const auto& l : _listv) n += l.size();
        return n;
    }

    // ================================================================ ParticleSnapshot

    void ParticleSnapshot::load(const ImportOptions& o, std::unique_ptr<SmoothingKernel> kernel)
    {
        _kernel = std::move(kernel);
        _holdsNumber = o.holdsNumber;
        // column roles in the reference's order: ParticleMedium.cpp:19-30 then ImportedMedium.cpp:17-18
        std::vector<ColumnSpec> cols = {{"position x", "length", "pc"}, {"position y", "length", "pc"}, {"position z", "length", "pc"},
                                        {"size h", "length", "pc"}};
        const int massIndex = 4;
        cols.push_back(o.holdsNumber ? ColumnSpec{"number", "", ""} : ColumnSpec{"mass", "mass", "Msun"});
        const MassPolicy policy = appendPolicyColumns(o, cols);

        std::vector<Array> rows = readColumnFile(o.path, cols, "smoothed particles");
        // ParticleSnapshot::readAndClose (ParticleSnapshot.cpp:79-151)
        _pv.clear();
        _pv.reserve(rows.size());
        _sites.clear();
        _sites.reserve(rows.size());
        double sumImported = 0, sumMetallic = 0, sumEffective = 0;
        for (const Array& prop : rows)
        {
            _sites.push_back(Vec3{prop[0], prop[1], prop[2]});  // (every imported row: ParticleSnapshot::position(m), ParticleSnapshot.cpp:286-289)
            if (policy.maxTemperature && prop[policy.temperatureIndex] > policy.maxTemperature) continue;
            if (prop[massIndex] == 0.) continue;
            double imported = prop[massIndex];
            double metallic = imported * (policy.useMetallicity ? prop[policy.metallicityIndex] : 1.);
            double effective = metallic * o.massFraction;
            _pv.push_back(Particle{prop[0], prop[1], prop[2], prop[3], effective});
            sumImported += imported;
            sumMetallic += metallic;
            sumEffective += effective;
        }
        if (sumImported < 0 || sumMetallic < 0 || sumEffective < 0)
        {
            _pv.clear();
            sumEffective = 0;
        }
        _mass = sumEffective;
        _search.loadEntities(
            static_cast<int>(_pv.size()),
            [this](int m) {
                const Particle& p = _pv[m];
                return Box(p.x - p.h, p.y - p.h, p.z - p.h, p.x + p.h, p.y + p.h, p.z + p.h);
            },
            [this](int m, const Box& box) { return sphereReachesBox(box, _pv[m].x, _pv[m].y, _pv[m].z, _pv[m].h); });

        // ---- optional: the same evaluation on the MI355X (include/pmc.h pmc_sampler_*)
        if (_sampler.api.createParticles && !_pv.empty())
        {
            pmc_particles P{};
            if (_kernel->type() == "CubicSplineSmoothingKernel")
                P.kernel = PMC_KERNEL_CUBIC_SPLINE;
            else if (_kernel->type() == "UniformSmoothingKernel")
                P.kernel = PMC_KERNEL_UNIFORM;
            else
                throw std::runtime_error("device density sampler: " + _kernel->type()
                                         + " evaluates a transcendental function and would not be bit-identical; use the host");
            std::vector<double> table(5 * _pv.size());
            for (size_t m = 0; m != _pv.size(); ++m)
            {
                table[5 * m] = _pv[m].x, table[5 * m + 1] = _pv[m].y, table[5 * m + 2] = _pv[m].z, table[5 * m + 3] = _pv[m].h;
                table[5 * m + 4] = _pv[m].density();
            }
            std::vector<int64_t> start;
            std::vector<int32_t> list;
            _search.flatten(start, list);
            P.num_particles = static_cast<int64_t>(_pv.size());
            P.particle = table.data();
            P.num_blocks = _search.numBlocks();
            P.xgrid = _search.xgrid().data(), P.ygrid = _search.ygrid().data(), P.zgrid = _search.zgrid().data();
            P.block_start = start.data();
            P.block_list = list.data();
            _sampler.attach(P);
        }
    }

    double ParticleSnapshot::density(Vec3 r) const
    {
        double sum = 0.;
        for (int m : _search.entitiesFor(r))
        {
            const Particle& p = _pv[m];
            const double dx = r.x - p.x, dy = r.y - p.y, dz = r.z - p.z;
            double u = sqrt(dx * dx + dy * dy + dz * dz) / p.h;
            sum += _kernel->density(u) * p.density();
        }
        return sum > 0. ? sum : 0.;
    }
}
