// Stand-alone check of the host model layer's reading and setup (skirt9_amd/host/ski_reader.cpp, simulation.cpp and what they call): one ski
// file through skh_load (Simulation::fromFile), skh_setup and skh_scene_save.  Compiled TOGETHER WITH the host sources, so that all of them
// run under the sanitizers -- the throw paths of the readers included, where a half-built model is abandoned:
//   g++ -std=c++17 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all tools/ski_read_check.cpp
//       skirt9_amd/host/[every .cpp but main.cpp] -pthread -o ski_read_check
// (tests/test_ski_read_check.py does that).
//   ski_read_check FILE.ski SCENE-FILE
// prints "ok <fnv1a-64 of the scene file's bytes>" and leaves the scene file, or "refused: <text>"; exit status 0 in both cases.
#include "../include/skirt_host.h"
#include <cstdio>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 3)
    {
        std::fprintf(stderr, "usage: ski_read_check FILE.ski SCENE-FILE\n");
        return 2;
    }
    skh_simulation* sim = skh_load(argv[1]);
    if (!sim || skh_setup(sim) != 0 || skh_scene_save(sim, argv[2]) != 0)
    {
        std::printf("refused: %s\n", skh_last_error());
        skh_free(sim);
        return 0;
    }
    skh_free(sim);
    std::FILE* in = std::fopen(argv[2], "rb");
    if (!in)
    {
        std::fprintf(stderr, "cannot read back %s\n", argv[2]);
        return 1;
    }
    unsigned long long h = 14695981039346656037ull;
    std::vector<unsigned char> block(1 << 20);
    for (size_t n; (n = std::fread(block.data(), 1, block.size(), in)) > 0;)
        for (size_t i = 0; i < n; ++i) h = (h ^ block[i]) * 1099511628211ull;
    std::fclose(in);
    std::printf("ok %016llx\n", h);
    return 0;
}
