// column_file.cpp -- see column_file.hpp
#include "column_file.hpp"
#include "units.hpp"
#include <cstring>
#include <fstream>
#include <limits>
#include <regex>
#include <sstream>
#include <stdexcept>

namespace skh
{
    namespace
    {
        std::string squeezeText(const std::string& text)
        {
            std::string out;
            bool haveSpace = true;
            for (char c : text)
            {
                if (c == ' ' || c == '\t' || c == '\n' || c == '\r')
                {
                    if (!haveSpace)
                    {
                        out.push_back(' ');
                        haveSpace = true;
                    }
                }
                else
                {
                    out.push_back(c);
                    haveSpace = false;
                }
            }
            if (haveSpace && !out.empty()) out.pop_back();
            return out;
        }
    }

    struct ColumnTextFile::State
    {
        std::ifstream in;
        std::vector<UnitFactor> conv;
    };

    ColumnTextFile::~ColumnTextFile() {}

    ColumnTextFile::ColumnTextFile(const std::string& path, const std::vector<ColumnSpec>& columns, const std::string& description)
        : _state(std::make_unique<State>())
    {
        std::ifstream& in = _state->in;
        in.open(path);
        if (!in) throw std::runtime_error("Could not open the " + description + " text file " + path);
        // ---- header: "# column N: description (unit)" lines (TextInFile.cpp:16-47,87-101); other '#' lines are comments
        struct FileColumn
        {
            std::string title, unit;
        };
        std::vector<FileColumn> fileCols;
        static const std::regex syntax("#\\s*column\\s*(\\d*)\\s*:\\s*([^()]*)\\(\\s*([a-zA-Z0-9/]*)\\s*\\)\\s*", std::regex::icase);
        while (true)
        {
            while (true)
            {
                int ch = in.peek();
                if (ch != ' ' && ch != '\t' && ch != '\n' && ch != '\r') break;
                in.get();
            }
            if (in.peek() != '#') break;
            std::string line;
            std::getline(in, line);
            std::smatch matches;
            if (std::regex_match(line, matches, syntax) && matches.size() == 4)
            {
                std::string index = matches[1].str();
                fileCols.push_back(FileColumn{squeezeText(matches[2].str()), matches[3].str()});
                if (!index.empty() && std::stoul(index) != fileCols.size())
                    throw std::runtime_error("Incorrect column index in file header for column " + std::to_string(fileCols.size()));
            }
        }
        // ---- logical columns in file order (TextInFile::addColumn without column remapping, :214-262)
        const size_t ncol = columns.size();
        std::vector<UnitFactor>& conv = _state->conv;
        conv.resize(ncol);
        for (size_t c = 0; c != ncol; ++c)
        {
            std::string unit = columns[c].defaultUnit;
            if (!fileCols.empty())
            {
                if (c + 1 > fileCols.size()) throw std::runtime_error("No column info in file header for column " + std::to_string(c + 1));
                unit = fileCols[c].unit;
            }
            if (columns[c].quantity == "specific")
            {
                // an arbitrarily scaled value per unit of wavelength (TextInFile.cpp:232-245): the unit must be one of the
                // per-wavelength styles, and NO conversion factor is applied (waveExponent 0); the per-frequency, neutral
                // and per-energy styles would need the wavelength column and are not supported here
                if (!unitTable().has("wavelengthmonluminosity", unit))
                    throw std::runtime_error("Invalid or unsupported units (" + unit + ") for specific quantity in column "
                                             + std::to_string(c + 1) + " (only per-wavelength units are supported)");
                conv[c] = UnitFactor{1., 1., 0.};
            }
            else if (columns[c].quantity.empty())
            {
                if (!unit.empty() && unit != "1")
                    throw std::runtime_error("Invalid units (" + unit + ") for dimensionless quantity in column " + std::to_string(c + 1));
                conv[c] = UnitFactor{1., 1., 0.};
            }
            else
            {
                if (!unitTable().has(columns[c].quantity, unit))
                    throw std::runtime_error("Invalid units (" + unit + ") for quantity '" + columns[c].quantity + "' in column "
                                             + std::to_string(c + 1));
                conv[c] = unitTable().factorOf(columns[c].quantity, unit);
            }
        }
    }

    // TextInFile::readRow (:286-330): value = factor * value^power
    bool ColumnTextFile::readRow(Array& row)
    {
        const std::vector<UnitFactor>& conv = _state->conv;
        const size_t ncol = conv.size();
        std::string line;
        while (std::getline(_state->in, line))
        {
            auto pos = line.find_first_not_of(" \t\r");
            if (pos == std::string::npos || line[pos] == '#') continue;
            row.assign(ncol, 0.);
            const char* p = line.c_str() + pos;
            for (size_t c = 0; c != ncol; ++c)
            {
                while (*p == ' ' || *p == '\t') ++p;
                if (!*p || *p == '\r') throw std::runtime_error("One or more required value(s) on text line are missing");
                char* end = nullptr;
                double value = strtod(p, &end);
                if (end == p)
                {
                    if (strncasecmp(p, "nan", 3) != 0)
                        throw std::runtime_error(std::string("Input text is not formatted as a floating point number: ") + p);
                    value = std::numeric_limits<double>::quiet_NaN();
                    end = const_cast<char*>(p) + 3;
                }
                p = end;
                if (conv[c].power != 1.) value = pow(value, conv[c].power);
                value *= conv[c].factor;
                row[c] = value;
            }
            return true;
        }
        return false;
    }

    // TextInFile::readNonLeaf (TextInFile.cpp:478-523)
    bool ColumnTextFile::readNonLeaf(int& nx, int& ny, int& nz)
    {
        std::ifstream& in = _state->in;
        std::string line;
        while (true)
        {
            const int c = in.peek();
            if (c == '#')
                std::getline(in, line);
            else if (c == '!')
            {
                in.get();
                std::getline(in, line);
                std::stringstream linestream(line);
                linestream >> nx >> ny >> nz;
                if (linestream.fail()) throw std::runtime_error("Nonleaf subdivision specifiers are missing or not formatted as integers");
                return true;
            }
            else if (c == ' ' || c == '\t' || c == '\n' || c == '\r')
                in.get();
            else
                return false;
        }
    }

    std::vector<Array> readColumnFile(const std::string& path, const std::vector<ColumnSpec>& columns, const std::string& description)
    {
        ColumnTextFile file(path, columns, description);
        std::vector<Array> rows;
        Array row;
        while (file.readRow(row)) rows.push_back(row);
        return rows;
    }
}
