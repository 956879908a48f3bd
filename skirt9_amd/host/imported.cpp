// imported.cpp -- see imported.hpp
#include "imported.hpp"
#include <atomic>
#include <limits>
#include <stdexcept>

namespace skh
{
    MassPolicy appendPolicyColumns(const ImportOptions& o, std::vector<ColumnSpec>& columns)
    {
        MassPolicy policy;
        if (o.importMetallicity)
        {
            policy.metallicityIndex = static_cast<int>(columns.size());
            columns.push_back({"metallicity", "", ""});
        }
        if (o.importTemperature)
        {
            policy.temperatureIndex = static_cast<int>(columns.size());
            columns.push_back({"temperature", "temperature", "K"});
        }
        policy.useMetallicity = o.isDust && o.importMetallicity;
        if (o.isDust && o.importTemperature && o.maxTemperature > 0) policy.maxTemperature = o.maxTemperature;
        return policy;
    }

    void DeviceSampler::release()
    {
        if (_sampler && api.destroy) api.destroy(_sampler);
        _sampler = nullptr;
    }

    void DeviceSampler::check(int code, const char* otherwise) const
    {
        if (code != 0) throw std::runtime_error(std::string("device density sampler: ") + (api.lastError ? api.lastError() : otherwise));
    }

    void DeviceSampler::densities(const std::vector<Vec3>& positions, double* out) const
    {
        static_assert(sizeof(Vec3) == 3 * sizeof(double), "Vec3 must be three packed doubles");
        check(api.density(_sampler, reinterpret_cast<const double*>(positions.data()), static_cast<int64_t>(positions.size()), out), "failed");
    }

    void ImportedSnapshot::densities(const std::vector<Vec3>& positions, std::vector<double>& out) const
    {
        out.resize(positions.size());
        if (positions.empty()) return;
        if (_sampler.isAttached()) return _sampler.densities(positions, out.data());
        // (an exception must not leave a worker thread: the lowest failing position is reported afterwards, as the device sampler does)
        const size_t none = std::numeric_limits<size_t>::max();
        std::atomic<size_t> failed{none};
        parallelFor(positions.size(), [&](size_t b, size_t e) {
            for (size_t i = b; i != e; ++i)
            {
                try
                {
                    out[i] = density(positions[i]);
                }
                catch (const std::runtime_error&)
                {
                    size_t seen = failed.load();
                    while (i < seen && !failed.compare_exchange_weak(seen, i)) {}
                    return;
                }
            }
        });
        if (failed.load() == none) return;
        try
        {
            density(positions[failed.load()]);
        }
        catch (const std::runtime_error& error)
        {
            throw std::runtime_error(std::string(error.what()) + " (position " + std::to_string(failed.load()) + ")");
        }
    }
}
