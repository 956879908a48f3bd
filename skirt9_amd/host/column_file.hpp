// column_file.hpp -- column text file with an optional unit header (SKIRT/core/TextInFile.cpp:16-47,57-110,214-330,478-523): what the
// imported media, file SEDs, file dust mixes and Voronoi site lists are read from.  "# column N: description (unit)" header lines are
// optional; without them every column carries the default unit its role declares.  Not restated: column remapping, .scol binary files.
#ifndef SKH_COLUMN_FILE_HPP
#define SKH_COLUMN_FILE_HPP

#include "mathutil.hpp"
#include <memory>
#include <string>
#include <vector>

namespace skh
{
    struct ColumnSpec
    {
        std::string description, quantity, defaultUnit;
    };
    // the open file: the header is read at construction, then the rows one at a time.  An adaptive mesh file mixes data rows with
    // "! nx ny nz" lines of nonleaf nodes (TextInFile::readNonLeaf, TextInFile.cpp:478-523).  `description` names the contents in the
    // message for a file that cannot be opened
    class ColumnTextFile
    {
    public:
        ColumnTextFile(const std::string& path, const std::vector<ColumnSpec>& columns, const std::string& description);
        ~ColumnTextFile();
        bool readRow(Array& row);                   // the next data row in internal units; false at the end of the file
        bool readNonLeaf(int& nx, int& ny, int& nz);  // true, and the three numbers, if the next line that holds anything starts with '!'
    private:
        struct State;
        std::unique_ptr<State> _state;
    };
    std::vector<Array> readColumnFile(const std::string& path, const std::vector<ColumnSpec>& columns, const std::string& description);
}

#endif
